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
