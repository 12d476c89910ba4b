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
