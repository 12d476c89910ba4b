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
    """apa_pose_head.hip launches pose_pl_kernel<8|16|24|32, FUSED, W2T>, pose_bwd_rows_mfma_kernel<R1, WA> in
    the three forms (false, false), (true, false), (true, true), pose_bwd_rows_kernel<T, R1, EXT, RPB, WA> and
    pose_dppre_kernel<T, JM, R1> -- each arm is a `need` entry of the coverage test above.  The fp32 WA form of the
    rows kernel had no caller (the fused outputs need bf16 features: pose_step_fast_ok) and is gone."""
    import re
    part_a = open(os.path.join(os.path.dirname(cof.LIB_PATH), '..', 'csrc', 'apa_pose_head.hip')).read()
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


# ------------------------------------------------------------------------------------------ per-class maps dispatch trace
def test_pc_probe_symbols_and_plan():
    from tests import _pc_probe as pc
    lib = pc.load_pc_probe()           # asserts the trace struct size
    assert lib.apa_probe_pc_trace_size() == ctypes.sizeof(pc.PcTrace) == 4 * (len(pc._INTS) + 6 * len(pc.GEMMS))
    for name in pc.PC_SYMBOLS:
        assert hasattr(lib, name), name
    prod = cof.load_library()
    for name in pc.PC_SYMBOLS:
        assert not hasattr(prod, name), 'libapa_hip.so exports ' + name
    # the carve of the HMDB-51 shape, by hand: Kp = 64; padded Wa, Wt (fp32-sized slots), ba, Z [R][64] f32, dT, dZ
    # [R][64] bf16; then the fused part: WcatT, Wcat2 (128 x 2048 bf16 each), bcat (128 f32), [dT | dZ] [R][128] bf16,
    # 32 dW split partials [2048][128] f32, one keep bit per feature element, two partial rows of 64 per 32-row block,
    # and the 256-byte tag; the total is what the product reports
    N, P, C, K = 32, 196, 2048, 51
    R = N * P
    pl = pc.plan(N, P, C, C, K, cof.APA_DTYPE_BF16)
    assert (pl['R'], pl['Kp'], pl['off_wap']) == (R, 64, 0)
    assert pl['off_wtp'] == C * 64 * 4 and pl['off_bap'] == 2 * C * 64 * 4 and pl['off_z'] == pl['off_bap'] + 256
    assert pl['off_dt'] - pl['off_z'] == R * 64 * 4 and pl['off_dz'] - pl['off_dt'] == R * 64 * 2
    assert pl['off_pdbt'] - pl['off_dz'] == R * 64 * 2 and pl['off_pdba'] - pl['off_pdbt'] == K * 4
    assert pl['off_bits'] - pl['off_xd'] == R * C * 2
    assert pl['WcatT'] == pl['off_fused'] and pl['Wcat2'] - pl['WcatT'] == 128 * C * 2
    assert pl['bcat'] - pl['Wcat2'] == C * 128 * 2 and pl['dTdZ'] - pl['bcat'] == 512
    assert pl['partial'] - pl['dTdZ'] == R * 128 * 2 and pl['maskbits'] - pl['partial'] == 32 * C * 128 * 4
    assert pl['lpart'] - pl['maskbits'] == R * C // 8 and pl['bits_tag'] - pl['lpart'] == (R // 32) * 2 * 64 * 4
    assert pl['fused_end'] - pl['bits_tag'] == 256 and pl['fused_end'] == pl['total']
    assert all(pl[k] % 256 == 0 for k in pc.PLAN_FIELDS[2:] if k not in ('off_pdba',))
    assert pl['total'] == prod.apa_attn_pool_workspace_bytes(N, P, C, C, K, K, 0)
    # 64 channel units in 5 ranges of 13, 13, 13, 13, 12; 49 row blocks; 16 channel tiles x 14 row splits of 448 rows
    assert pc.geometry(R, C) == dict(upb=13, dx_splits=5, rbs=49, dw_S=14, dw_rows=448, dw_ctiles=16)
    assert pc.support(N, P, C, C, 64, cof.APA_DTYPE_BF16, 0) == (True, True)
    assert pc.support(N, P, C, C, 65, cof.APA_DTYPE_BF16, 0)[0] is False
    assert pc.support(N, 25, C, C, K, cof.APA_DTYPE_BF16, 0) == (True, False)
    assert pc.support(N, P, C, C, K, cof.APA_DTYPE_BF16, 2) == (True, False)
    assert pc.support(N, P, 8448, 8448, K, cof.APA_DTYPE_BF16, 0)[0] is False
    assert pc.support(N, P, C, C, K, cof.APA_DTYPE_F32, 0)[0] is False


def _pc_reached():
    from tests import test_pc_paths_gpu as t
    reached = set()
    for c in t.CASES + t.MIS_CASES:
        e = t.expected(c)
        lit = dict(c['expect'])
        if 'topdown_t' in lit:
            lit['topdown'] = lit.pop('topdown_t')
        for k, v in lit.items():
            assert e.get(k, v) == v, (c['name'], k, v, e.get(k))
        e.update(lit)
        N, P, C, K, R = c['N'], c['P'], c['C'], c['K'], c['N'] * c['P']
        fused = e['path_fwd'] == 'fused'
        train = bool(c['train'] and c['entry'] != 'eval')
        reached.add(('path', e['path_fwd'], c['dt']))
        reached.add(('entry', e['path_fwd'], c['entry'], train))
        reached.add(('act', e['path_fwd'], c['dt'], c['act']))
        reached.add(('rng', e['path_fwd'], c['rng'], train))
        reached.add(('wimg', e['path_fwd'], c['wimg'], train, c['entry']))
        reached.add(('keep', c['keep'], train))
        for k in ('logits', 'xent', 'fwd_act', 'bwd_act', 'dx', 'dw', 'tail', 'wa_to'):
            if k in e:
                reached.add((k, e['path_fwd'], e[k]))
        if c['topdown']:
            reached.add(('topdown', e['path_fwd'], c['dt']))
        if c['Ca'] is not None:
            reached.add(('xatt', c['dt'], 'same_width' if c['Ca'] == C else 'other_width', train))
        for m, off in c['mis'].items():
            reached.add(('misaligned', m, off, e['path_fwd'], e.get('dx')))
        if fused:
            reached.add(('fused_K', K))
            reached.add(('fused_C', C))
            reached.add(('fused_P', P))
            reached.add(('zt', e['zt_train'], e['zt_fold']))
            reached.add(('prep_fwd', e['prep_fwd']))
            if 'prep_bwd' in e:
                reached.add(('prep_bwd', e['prep_bwd']))
            reached.add(('tag', c['pre'], c['rng']))
            if 'next_bits' in e:
                reached.add(('next_bits', e['next_bits'], e['dx']))
            if R % 32 and R % 128:
                reached.add(('fused_ragged',))
            if R < 32:
                reached.add(('fused_R_lt_32',))
            if R < 64:
                reached.add(('fused_R_lt_64',))
            for k in ('upb', 'dx_splits', 'dw_S'):
                if k in lit:
                    reached.add((k, lit[k]))
            if e.get('dx') == 'fused':
                reached.add(('dx_train', train))
                reached.add(('dx_xent', e['xent'] == 'dx'))
                if (R + 127) // 128 >= 2 and P == 33:
                    reached.add(('dx_block_of_5_images',))
            if 'dw' in e:
                reached.add(('dw_train', train))
            if e.get('tail') == 'dw_tail':
                reached.add(('dw_tail', e['rng_bump'], e['aux'], e['next_bits']))
        else:
            reached.add(('generic_K', c['dt'], K))
            reached.add(('generic', c['dt'], e['cat'], e['fast'], train))
            reached.add(('pad_fwd', e['pad_segs_fwd'], e['pad_drop_fwd']))
            reached.add(('t_drop_a', e['t_drop_a']))
            if 'pad_segs_bwd' in e:
                reached.add(('pad_bwd', e['pad_segs_bwd'], e['pad_drop_bwd']))
                reached.add(('reuse_fwd', e['reuse_fwd']))
                reached.add(('dw_drop_a', e['dw_drop_a']))
                reached.add(('dx_form', e['dx'], e.get('mid_bits'), e.get('dx_drop_c'), e.get('wa_to')))
                reached.add(('colsum', e['rng_bump'], e['aux']))
            if 'ps' in lit:
                reached.add(('ps', lit['ps']))
            if c['wide'] is not None:
                reached.add(('wide', c['wide'], e['dx']))
            if C % 8:
                reached.add(('generic_C_mod_8', c['dt']))
            if (N, P, C) == (32, 196, 2048):
                reached.add(('shipped', K, c['entry']))
            if K <= 64 and c['dt'] == cof.APA_DTYPE_BF16:
                reached.add(('neighbour', 'c8448' if C > 8192 else 'c_mod_256' if C % 256 else 'xatt' if
                             c['Ca'] == C else 'ca' if c['Ca'] is not None else 'x_misaligned' if c['mis'].get('X')
                             else 'rng_external' if c['rng'] == 'external' else '?'))
            if K == 65 and C % 256 == 0 and c['Ca'] is None and not c['mis']:
                reached.add(('neighbour', 'k65'))
        if (N, P, C, K) == (32, 196, 2048, 51):
            reached.add(('shipped', K, c['entry']))
    return reached, t


def test_pc_gpu_case_table_covers_every_reachable_trace_value():
    F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
    reached, t = _pc_reached()
    need = {('path', 'fused', BF16), ('path', 'generic', BF16), ('path', 'generic', F32)}
    need |= {('entry', p, en, tr) for p in ('fused', 'generic') for en, tr in
             (('sep', False), ('sep', True), ('step', False), ('step', True), ('eval', False))}
    need |= {('act', 'fused', BF16, a) for a in ('id', 'relu', 'softmax')}
    need |= {('act', 'generic', dt, a) for dt in (F32, BF16) for a in ('id', 'relu', 'softmax')}
    need |= {('rng', 'fused', 'value', True), ('rng', 'fused', 'device', True), ('rng', 'generic', 'device', True),
             ('rng', 'generic', 'external', True)}
    need |= {('wimg', 'fused', True, False, 'sep'), ('wimg', 'fused', True, True, 'sep'),
             ('wimg', 'fused', True, True, 'step'), ('wimg', 'generic', True, True, 'sep'),
             ('wimg', 'generic', True, False, 'sep')}
    need |= {('keep', 0.5, True), ('keep', 0.7, True)}
    # fused path: the shapes and edges
    need |= {('fused_K', k) for k in (2, 3, 4, 21, 51, 63, 64)}   # (K = 1 has M == 1: the M == 1 path serves it)
    need |= {('fused_C', ch) for ch in (256, 768, 2048, 4096, 8192)}
    need |= {('fused_P', p) for p in (25, 32, 33, 36, 49, 196, 225)}
    need |= {('fused_ragged',), ('fused_R_lt_32',), ('fused_R_lt_64',), ('dx_block_of_5_images',)}
    need |= {('upb', 1), ('upb', 13), ('upb', 16), ('dx_splits', 5), ('dw_S', 1)}
    # every launched instance: pc_fwd_zt_dma_kernel<TRAIN, FOLD>, pc_bwd_dx_kernel<TRAIN>, pc_bwd_dw_kernel<TRAIN>
    need |= {('zt', tr, fo) for tr in (0, 1) for fo in (0, 1)}
    need |= {('dx_train', tr) for tr in (False, True)} | {('dw_train', tr) for tr in (False, True)}
    need |= {('dx_xent', x) for x in (False, True)}
    need |= {('prep_fwd', p) for p in ('none', 'weights', 'bits', 'both')}
    need |= {('prep_bwd', p) for p in ('none', 'weights', 'bits', 'both')}
    need |= {('tag', p, 'value') for p in ('fresh', 'believed', 'jump', 'foreign')} | {('tag', 'believed', 'device')}
    need |= {('next_bits', 1, 'fused'), ('next_bits', 1, 'mid_gemm'), ('next_bits', 0, 'fused')}
    need |= {('logits', 'fused', v) for v in ('finish', 'dx', 'fwd_act')}
    need |= {('xent', 'fused', v) for v in ('none', 'fwd_act', 'dx', 'own')}
    need |= {('fwd_act', 'fused', v) for v in ('folded', 'bf16')} | {('bwd_act', 'fused', v) for v in ('folded', 'bf16')}
    need |= {('dx', 'fused', v) for v in ('fused', 'mid_gemm', 'plain_gemm')}
    # the three kinds of tail block of pc_dw_reduce_kernel: column sums (+ counter bump, + loss mean), next step's bits
    need |= {('dw_tail', 0, 0, 0), ('dw_tail', 1, 0, 0), ('dw_tail', 0, 1, 0), ('dw_tail', 0, 1, 1), ('dw_tail', 1, 1, 1)}
    need |= {('topdown', 'fused', BF16), ('topdown', 'generic', F32)}
    # neighbours of the fused path
    need |= {('neighbour', w) for w in ('k65', 'c8448', 'c_mod_256', 'xatt', 'ca', 'x_misaligned', 'rng_external')}
    # generic path
    need |= {('generic_K', BF16, k) for k in (2, 65, 130, 393, 1000, 1024, 1025)}
    need |= {('generic_K', F32, k) for k in (2, 51, 65, 393, 1025)}
    need |= {('generic', BF16, 1, 1, tr) for tr in (False, True)} | {('generic', BF16, 0, 1, tr) for tr in (False, True)}
    need |= {('generic', BF16, 0, 0, True), ('generic', F32, 0, 0, False), ('generic', F32, 0, 0, True)}
    need |= {('pad_fwd', 3, 1), ('pad_fwd', 3, 0), ('pad_fwd', 2, 0), ('pad_fwd', 0, 1), ('pad_fwd', 0, 0)}
    need |= {('pad_bwd', 2, 1), ('pad_bwd', 2, 0), ('pad_bwd', 0, 1), ('pad_bwd', 0, 0)}
    need |= {('reuse_fwd', 0), ('reuse_fwd', 1), ('t_drop_a', 0), ('t_drop_a', 1), ('dw_drop_a', 0), ('dw_drop_a', 2)}
    need |= {('dx_form', 'wide', 1, None, None), ('dx_form', 'two', None, 0, 'dx_beta1'),
             ('dx_form', 'two', None, 1, 'dx_beta1'), ('dx_form', 'two', None, 0, 'dxatt'),
             ('dx_form', 'two', None, 1, 'dxatt')}
    need |= {('wide', True, 'wide'), ('wide', True, 'two'), ('wide', False, 'two')}
    need |= {('xent', 'generic', v) for v in ('none', 'bwd_act', 'own')}
    need |= {('fwd_act', 'generic', v) for v in ('f32', 'bf16')} | {('bwd_act', 'generic', v) for v in ('f32', 'bf16')}
    need |= {('colsum', 0, 0), ('colsum', 1, 0), ('colsum', 0, 1)}
    need |= {('ps', 1), ('ps', 2), ('ps', 8)}
    need |= {('xatt', BF16, 'same_width', True), ('xatt', BF16, 'other_width', False),
             ('xatt', BF16, 'other_width', True), ('xatt', F32, 'other_width', True)}
    need |= {('generic_C_mod_8', BF16)}
    need |= {('misaligned', 'X', 1, 'generic', 'two'), ('misaligned', 'dX', 4, 'generic', 'two')}
    need |= {('shipped', 51, 'step'), ('shipped', 51, 'eval'), ('shipped', 393, 'step'), ('shipped', 393, 'sep')}
    missing = need - reached
    assert not missing, sorted(missing, key=str)
    names = [c['name'] for c in t.CASES + t.MIS_CASES]
    assert len(names) == len(set(names))


def test_per_class_launches_no_instance_outside_the_case_table():
    """apa_pc.hip and apa_pc_fused.hip launch pc_fwd_zt_dma_kernel<TRAIN, FOLD> (four arms),
    pc_bwd_dx_kernel<TRAIN>, pc_bwd_dw_kernel<TRAIN>, pc_fwd_act_kernel / pc_bwd_act_kernel for float and bf16_t, and the
    untemplated pc_prep / pc_pad / pc_logits_finish / pc_dw_reduce kernels -- each arm is a `need` entry of the coverage
    test above.  pc_fused_forward's own `C % ZB_KT` refusal had no caller behind pc_fused_supported (C % 256 == 0) and
    is gone.  The general (non-"small form") arm of pc_fill_bits / the forward kernel's slow arm stays: its callers are
    the maps of more than 2^33 elements (a 16 GB bf16 feature map: R > 2^20 rows at C = 8192), which the device
    holds but no test allocates."""
    import re
    here = os.path.join(os.path.dirname(cof.LIB_PATH), '..', 'csrc')
    fused = open(os.path.join(here, 'apa_pc_fused.hip')).read()
    part_b = open(os.path.join(here, 'apa_pc.hip')).read()
    assert re.findall(r'APA_ZT\((true|false), (true|false)\);', fused) == [
        ('true', 'true'), ('false', 'true'), ('true', 'false'), ('false', 'false')]
    assert re.findall(r'APA_DX\((true|false)\);', fused) == ['true', 'false']
    assert re.findall(r'APA_DW\((true|false)\);', fused) == ['true', 'false']
    assert 'C % ZB_KT != 0' not in fused
    assert sorted(re.findall(r'hipLaunchKernelGGL\(\(?(pc_\w+)', fused)) == sorted(
        ['pc_prep_kernel', 'pc_logits_finish_kernel', 'pc_fwd_zt_dma_kernel', 'pc_bwd_dx_kernel', 'pc_bwd_dw_kernel',
         'pc_dw_reduce_kernel'])
    launches = re.findall(r'hipLaunchKernelGGL\(\(?(pc_\w+?)(?:<(\w+)>)?[,)]', part_b)
    assert sorted(launches) == sorted(
        [('pc_pad_kernel', ''), ('pc_fwd_act_kernel', 'bf16_t'), ('pc_fwd_act_kernel', 'float'),
         ('pc_bwd_act_kernel', 'bf16_t'), ('pc_bwd_act_kernel', 'float')]), launches   # one site per (kernel, type)
    # the table reaches both element types of both activation kernels, on both paths where they exist
    reached, _ = _pc_reached()
    for need in (('fwd_act', 'fused', 'bf16'), ('fwd_act', 'generic', 'bf16'), ('fwd_act', 'generic', 'f32'),
                 ('bwd_act', 'fused', 'bf16'), ('bwd_act', 'generic', 'bf16'), ('bwd_act', 'generic', 'f32')):
        assert need in reached, need
