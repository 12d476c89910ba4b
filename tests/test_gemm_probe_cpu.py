"""The test-only GEMM probe library (csrc/apa_gemm_probe.hip): built by build() beside the product library,
its descriptor layout agrees with the ctypes mirror in tests/_gemm_probe.py, and the product library does not
carry it.  Also: the GPU case table reaches every kernel kind, ring / wide tile height, layout, output type, split
form, reduce form and twin form the dispatcher has (each case asserts its traced path on the GPU)."""
import ctypes
import os
import subprocess

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp


def test_probe_library_is_built_and_matches_the_ctypes_mirror():
    assert os.path.exists(gp.PROBE_PATH), 'build() did not produce libapa_gemm_probe.so'
    assert os.path.dirname(gp.PROBE_PATH) == os.path.dirname(cof.LIB_PATH)
    lib = gp.load_probe()      # asserts version and struct size
    assert lib.apa_probe_gemm_struct_size() == ctypes.sizeof(gp.ProbeGemm) == 8 * len(gp.ProbeGemm._fields_)
    for name in gp.PROBE_SYMBOLS:
        assert hasattr(lib, name), name
    # host-only helpers
    assert lib.apa_probe_gemm_ws_bytes(100, 16, 1) == 0
    assert lib.apa_probe_gemm_ws_bytes(100, 16, 3) == 3 * 100 * 16 * 4
    assert lib.apa_probe_sgemm_ws_bytes(32, 393, 8) == 8 * 32 * 393 * 4
    assert lib.apa_probe_gemm_pick_splits(6272, 16, 768) == 6
    assert lib.apa_probe_gemm_pick_splits(6272, 768, 2048) == 1


def test_product_library_does_not_carry_the_probe():
    prod = cof.load_library()
    for name in gp.PROBE_SYMBOLS:
        assert not hasattr(prod, name), 'libapa_hip.so exports ' + name
    out = subprocess.run(['nm', '-D', '--defined-only', cof.LIB_PATH], capture_output=True, text=True, check=True)
    assert 'apa_probe' not in out.stdout


def test_gpu_case_table_covers_every_path():
    from tests import test_gemm_paths_gpu as t
    reached = set()
    for c in t.CASES + t.TWIN_CASES:
        e = c['expect']
        kind = e['kind']
        reached.add(('kind', kind))
        if 'mt' in e:
            reached.add((kind + '_mt', e['mt']))
        a_kc, b_kc = c.get('a_kc', True), c.get('b_kc', False)
        reached.add((kind + '_layout', a_kc, b_kc))
        reached.add((kind + '_out', c.get('tc', 0)))
        reached.add((kind + '_split', e['split'] > 1))
        reached.add((kind + '_drop', 'a{}'.format(c['drop_a']) if c.get('drop_a') else
                     'c' if c.get('drop_c') else 'none'))
        reached.add(('reduce', e['reduce']))
        reached.add(('twin', e['twin']))
    reached.add(('reduce', 'tail'))     # test_reduce_tail_colsum_is_m1_colsum_bit_for_bit
    need = {('kind', k) for k in ('generic', 'bf16', 'wide', 'ring', 'glds64', 'glds128')}
    need |= {('ring_mt', m) for m in range(4, 9)} | {('wide_mt', m) for m in range(4, 8)}
    need |= {('ring_layout', True, b) for b in (True, False)}
    need |= {(k + '_layout', a, b) for k in ('glds64', 'glds128', 'generic') for a in (True, False)
             for b in (True, False)}
    need |= {(k + '_out', tc) for k in ('generic', 'bf16', 'wide', 'ring', 'glds64', 'glds128') for tc in (0, 1)}
    need |= {(k + '_split', s) for k in ('generic', 'bf16', 'glds64', 'glds128') for s in (False, True)}
    need |= {('reduce', r) for r in ('none', 'vec', 'scalar', 'tail')} | {('twin', w) for w in ('none', 'fused', 'serial')}
    # output dropout on every kind that accepts it (the A-operand masks make a product ineligible for the bf16 path)
    need |= {(k + '_drop', 'c') for k in ('generic', 'bf16', 'wide', 'ring', 'glds64', 'glds128')}
    need |= {('generic_drop', m) for m in ('a1', 'a2')}
    missing = need - reached
    assert not missing, sorted(missing, key=str)
    names = [c['name'] for c in t.CASES + t.TWIN_CASES]
    assert len(names) == len(set(names))


# ------------------------------------------------------------------------------------------ M == 1 dispatch trace
def test_m1_probe_symbols_and_plan():
    from tests import _m1_probe as mp
    lib = mp.load_m1_probe()           # asserts the trace struct size
    assert lib.apa_probe_m1_trace_size() == ctypes.sizeof(mp.M1Trace) == 4 * len(mp.M1Trace._fields_)
    for name in mp.M1_SYMBOLS:
        assert hasattr(lib, name), name
    prod = cof.load_library()
    for name in mp.M1_SYMBOLS:
        assert not hasattr(prod, name), 'libapa_hip.so exports ' + name
    # hand-checked plans: S = round(512 / N) clamped to [1, min(P / 4, 256)], ppb = ceil(P / S)
    assert mp.plan(32, 196, 2048, 2048, 393)[:3] == (16, 13, 512)      # cfg 002
    assert mp.plan(33, 225, 2048, 2048, 393)[:3] == (16, 15, 528)
    assert mp.plan(170, 196, 2048, 2048, 51)[:2] == (3, 66)
    assert mp.plan(342, 196, 1024, 1024, 51)[:2] == (1, 196)
    assert mp.plan(6, 49, 1024, 1024, 51)[:2] == (12, 5)                # clamped to P / 4
    assert mp.plan(1, 4, 2048, 2048, 51)[:2] == (1, 4)                  # P < 8: one split


def test_m1_support_has_no_unreachable_instances():
    """The dispatch asks for the streaming kernels first and m1_logits2 before the small-K kernels: the per-pixel
    (vec) family has instances for no streaming C, and every C the small-K kernels accept is an m1_logits2 C."""
    from tests import _m1_probe as mp
    F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
    for dt in (F32, BF16):
        for C in range(8, 8193, 8):
            for K in (1, 51, 393, 736):
                sup = mp.support(8, C, K, dt)
                assert not (sup & mp.SUP_VEC and sup & mp.SUP_STREAM), (dt, C, K)
                assert not (sup & mp.SUP_SMALL) or sup & mp.SUP_LOGITS2, (dt, C, K)
    # and the vec instances that remain serve exactly these C's
    for dt, Cs in ((F32, (256, 512)), (BF16, (512, 1024))):
        vec = [C for C in range(8, 8193, 8) if mp.support(8, C, 51, dt) & mp.SUP_VEC]
        assert vec == list(Cs), (dt, vec)


def test_m1_gpu_case_table_covers_every_reachable_trace_value():
    from tests import test_m1_paths_gpu as t
    reached = set()
    for c in t.CASES:
        e = dict(c['expect'])
        pool = e.get('pool_fwd')
        if pool:
            reached.add(('pool', pool, c['dt'], e.get('fwd_w'), e.get('fwd_pix')))
            if c['relu_in']:
                reached.add(('relu_input', c['dt'], e.get('fwd_w')))
        for k in ('S', 'cw', 'logits', 'head', 'gemv', 'reduce', 'keep_bits', 'rng_bump', 'cat_fwd'):
            if k in e:
                reached.add((k, e[k]))
        if e.get('logits') in ('xent', 'xent_probs'):
            reached.add(('nv4', e['logits'], e.get('logits_nv4')))
        if 'logits_nsub' in e:
            reached.add(('nsub', e['logits_nsub']))
        if e.get('head') in ('tiles', 'rows'):
            reached.add((e['head'], e.get('head_ug')))
        if e.get('head') == 'small':
            reached.add(('small', e.get('head_mv')))
        if e.get('gemv'):
            reached.add(('gemv_dt', e['gemv'], c['dt']))
        for m in c['mis']:
            reached.add(('misaligned', m))
        if c['rng'] != 'hash':
            reached.add(('rng', c['rng']))
        reached.add(('entry', c['entry']))
    F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
    need = {('pool', 'stream', F32, 1, 1), ('pool', 'stream', F32, 2, 1), ('pool', 'stream', F32, 4, 2),
            ('pool', 'stream', BF16, 1, 2),
            ('pool', 'vec', F32, 1, None), ('pool', 'vec', F32, 2, None), ('pool', 'vec', BF16, 1, None),
            ('pool', 'vec', BF16, 2, None), ('pool', 'generic', F32, None, None), ('pool', 'generic', BF16, None, None),
            ('relu_input', F32, 1), ('relu_input', F32, 2), ('relu_input', F32, 4), ('relu_input', BF16, 1)}
    need |= {('S', 1), ('S', 3), ('S', 16), ('cw', 256), ('cw', 128), ('cw', 64)}
    need |= {('logits', v) for v in ('xent', 'xent_probs', 'logits2', 'sgemm')}
    need |= {('nv4', 'xent', v) for v in (1, 2, 4)} | {('nv4', 'xent_probs', v) for v in (1, 2, 4)}
    need |= {('nsub', 1), ('nsub', 4)}
    need |= {('tiles', u) for u in (1, 2, 4, 7)} | {('rows', u) for u in (1, 2, 4, 7, 13)}
    need |= {('small', m) for m in (4, 8, 13, 26)} | {('head', 'sgemm')}
    need |= {('gemv_dt', g, d) for g in ('bwd2', 'bwd2_rank1', 'bwd') for d in (F32, BF16)}
    need |= {('reduce', 'colsum'), ('reduce', 'bwd_reduce'), ('keep_bits', 1), ('rng_bump', 1)}
    need |= {('cat_fwd', 1), ('cat_fwd', 16), ('rng', 'device'), ('rng', 'external')}
    need |= {('misaligned', m) for m in ('zsave', 'G', 'Wt')} | {('entry', e) for e in ('sep', 'step', 'eval')}
    missing = need - reached
    assert not missing, sorted(missing, key=str)
    names = [c['name'] for c in t.CASES]
    assert len(names) == len(set(names))


# ------------------------------------------------------------------------------------------ pose-head dispatch trace
def test_pose_probe_symbols_and_plan():
    from tests import _pose_probe as pp
    lib = pp.load_pose_probe()         # asserts the trace struct size
    assert lib.apa_probe_pose_trace_size() == ctypes.sizeof(pp.PoseTrace) == 4 * len(pp.PoseTrace._fields_)
    for name in pp.POSE_SYMBOLS:
        assert hasattr(lib, name), name
    prod = cof.load_library()
    for name in pp.POSE_SYMBOLS:
        assert not hasattr(prod, name), 'libapa_hip.so exports ' + name
    # the carve of the benchmark shape, by hand: dPpre [6272][768] bf16 first, 256-byte aligned regions, the bf16
    # copy of W1 (2048 x 768 x 2 bytes) in front of the loss partials; the total is what the product reports
    pl = pp.plan(32, 196, 2048, 768, 16, cof.APA_DTYPE_BF16)
    assert (pl['R'], pl['nchunks'], pl['off_dppre']) == (6272, 784, 0)
    assert pl['off_partial'] == 6272 * 768 * 2
    assert pl['off_lpart'] - pl['off_w1b'] == 2048 * 768 * 2
    assert all(pl[k] % 256 == 0 for k in pp.PLAN_FIELDS[2:])
    assert pl['total'] == prod.apa_pose_head_workspace_bytes(32, 196, 2048, 768, 16, cof.APA_DTYPE_BF16)


def test_pose_gpu_case_table_covers_every_reachable_trace_value():
    from tests import test_pose_paths_gpu as t
    F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
    reached = set()
    for c in t.CASES + t.MIS_CASES:
        e, dt, R, J, Cp = c['expect'], c['dt'], c['N'] * c['P'], c['J'], c['Cp']
        sep = c['entry'] == 'sep'
        form = e.get('form_t')
        if e.get('pl') == 'fast' or 'pl_ks' in e:
            reached.add(('pl_fast', e['pl_ks'], 'w2t' if e.get('pl_w2t') else 'fused' if e.get('pl_fused') else 'plain'))
            if sep and R % 64 != 0 and J < 16:
                reached.add(('pl_fast_ragged_jlt16', e['pl_ks']))
        if e.get('pl') == 'gemm':
            reached.add(('pl_gemm', 'f32' if dt == F32 else 'ppre8' if c['mis'].get('Ppre') == 4 else
                         'j20' if J == 20 else 'cp384' if Cp == 384 else 'bf16'))
        rows = e.get('rows')
        if rows == 'mfma' and 'wpb' in e:
            reached.add(('mfma', e['wpb'], e['ngrp']))
            if 'G' in e and form:
                reached.add(('mfma_g', e['G'], form))
                if R % 32 != 0:
                    reached.add(('mfma_ragged32',))
                if e['G'] == 2 and 1 <= R % 64 <= 31:
                    reached.add(('mfma_g2_second_group_empty',))
        if rows == 'mfma' and e.get('wa'):
            reached.add(('mfma_wa',))
        if rows == 'valu':
            if sep and not c['mis']:
                reached.add(('valu', dt, e['rpb'], form, R >= 4065))
                reached.add(('valu_j', dt, 16 if J == 16 else 'lt16'))
                if (Cp // 2) % 64 != 0:
                    reached.add(('valu_idle_threads', dt))
            if e.get('wa'):
                reached.add(('valu_wa', dt))
        if rows == 'dppre':
            reached.add(('dppre', dt, e['jm']))
            reached.add(('dppre_form', form))
            reached.add(('dppre_dw2', e.get('dw2')))
            if J == 32 or 17 <= J <= 31:
                reached.add(('dppre_j', 32 if J == 32 else 'mid'))
            if Cp == 2048:
                reached.add(('dppre_cp2048', dt))
            if R % 8 != 0:
                reached.add(('dppre_ragged8',))
        for k in ('colsum', 'w1_fwd', 'w1_bwd', 'dx_beta'):
            if k in e:
                reached.add((k, e[k]))
        if c['reuse']:
            reached.add(('w1_bwd', 'reused'))
        if sep:
            reached.add(('dx_beta', int(bool(c['beta']))))
        for m, off in c['mis'].items():
            reached.add(('misaligned', m, off, rows))
        reached.add(('entry', c['entry'], dt, c['images'], c['train']))
        if (c['N'], c['P'], c['C'], Cp) in ((32, 196, 2048, 768), (33, 225, 2048, 768)) and sep:
            reached.add(('shipped', c['N'], dt, J))
    need = {('pl_fast', ks, f) for ks in (8, 16, 24, 32) for f in ('plain', 'fused', 'w2t')}
    need |= {('pl_fast_ragged_jlt16', ks) for ks in (8, 16, 24, 32)}
    need |= {('pl_gemm', w) for w in ('f32', 'cp384', 'j20', 'ppre8')}
    need |= {('mfma', w, g) for w, g in ((4, 1), (3, 2), (4, 2), (2, 5), (3, 4), (2, 7), (4, 4))}
    need |= {('mfma_g', G, f) for G in (1, 2) for f in ('plain', 'rank1')}
    need |= {('mfma_ragged32',), ('mfma_g2_second_group_empty',), ('mfma_wa',), ('valu_wa', BF16)}
    # 32 rows per block on each side of the 64 KB limit, per (dtype, form); 16 rows at small R too
    need |= {('valu', dt, rpb, f, True) for dt in (F32, BF16) for rpb in (16, 32) for f in ('plain', 'ext', 'rank1')}
    need |= {('valu', dt, 16, f, False) for dt, f in ((F32, 'rank1'), (BF16, 'plain'), (BF16, 'ext'), (BF16, 'rank1'))}
    need |= {('valu_j', dt, j) for dt in (F32, BF16) for j in (16, 'lt16')}
    need |= {('valu_idle_threads', F32), ('valu_idle_threads', BF16)}
    need |= {('dppre', dt, jm) for dt in (F32, BF16) for jm in (16, 32)}
    need |= {('dppre_form', f) for f in ('plain', 'ext', 'rank1')} | {('dppre_dw2', 'gemm'), ('dppre_dw2', 'memset')}
    need |= {('dppre_j', 32), ('dppre_j', 'mid'), ('dppre_cp2048', F32), ('dppre_cp2048', BF16), ('dppre_ragged8',)}
    need |= {('colsum', 'tail'), ('colsum', 'own'), ('dx_beta', 0), ('dx_beta', 1)}
    need |= {('w1_fwd', w) for w in ('bf16_copy', 'f32', 'shadow')}
    need |= {('w1_bwd', w) for w in ('bf16_copy', 'f32', 'reused', 'shadow')}
    need |= {('misaligned', 'Ppre', 4, 'valu'), ('misaligned', 'Ppre', 2, 'dppre'), ('misaligned', 'Ppre', 1, 'dppre'),
             ('misaligned', 'W2', 1, 'dppre'), ('misaligned', 'dPl', 1, 'valu'), ('misaligned', 'W1', 1, 'mfma')}
    need |= {('entry', 'step', BF16, (), False), ('entry', 'step', BF16, ('w1', 'w2t'), True),
             ('entry', 'step', BF16, ('w2t',), False), ('entry', 'step', F32, (), False),
             ('entry', 'sep', F32, (), False), ('entry', 'sep', BF16, (), False)}
    need |= {('shipped', 32, dt, j) for dt in (F32, BF16) for j in (16, 13)} | {('shipped', 33, BF16, 16)}
    missing = need - reached
    assert not missing, sorted(missing, key=str)
    names = [c['name'] for c in t.CASES + t.MIS_CASES]
    assert len(names) == len(set(names))


def test_pose_head_launches_no_instance_outside_the_case_table():
    """Part A of apa_dense.hip launches pose_pl_kernel<8|16|24|32, FUSED, W2T>, pose_bwd_rows_mfma_kernel<R1, WA> in
    the three forms (false, false), (true, false), (true, true), pose_bwd_rows_kernel<T, R1, EXT, RPB, WA> and
    pose_dppre_kernel<T, JM, R1> -- each arm is a `need` entry of the coverage test above.  The fp32 WA form of the
    rows kernel had no caller (the fused outputs need bf16 features: pose_step_fast_ok) and is gone."""
    import re
    src = open(os.path.join(os.path.dirname(cof.LIB_PATH), '..', 'csrc', 'apa_dense.hip')).read()
    part_a = src[:src.index('// B. Per-class bottom-up maps')]
    arms = re.findall(r'APA_ROWS\((float|bf16_t), (true|false), (true|false), (true|false)\);', part_a)
    assert sorted(arms) == sorted([('float', 'true', 'false', 'false'), ('float', 'false', 'true', 'false'),
                                   ('float', 'false', 'false', 'false'), ('bf16_t', 'true', 'false', 'true'),
                                   ('bf16_t', 'true', 'false', 'false'), ('bf16_t', 'false', 'true', 'false'),
                                   ('bf16_t', 'false', 'false', 'false')]), arms
    assert re.findall(r'APA_ROWSM\((true|false), (true|false)\);', part_a) == [('true', 'true'), ('true', 'false'),
                                                                                 ('false', 'false')]
    assert re.findall(r'case (\d+): APA_PL\((\d+)\)', part_a) == [('8', '8'), ('16', '16'), ('24', '24')]
    assert 'default: APA_PL(32)' in part_a
    assert re.findall(r'APA_DPPRE\((float|bf16_t), (16|32)\)', part_a) == [
        ('float', '16'), ('float', '32'), ('bf16_t', '16'), ('bf16_t', '32')]
