"""The reach table of the FP8 case table (tests/_fp8_cases.py; run on the GPU by tests/test_fp8_instances_gpu.py), with
no GPU: every template instance (NV, TRAIN, GATHER) of the two FP8 streaming kernels, both lane occupancies of each NV,
every class of chunk-loop trip count per NV, both kinds of split, and both head routes behind the wide instances have a
case -- computed from the dispatch's own functions through the probe library (apa_probe_m1f_instance,
apa_probe_m1_plan, apa_probe_m1_support) and the kernels' own chunk formulas, so deleting or narrowing a case fails
here.  And the relu cases' gate condition, from the inputs alone."""
import pytest

from tests import _fp8_cases as fc
from tests import _m1_probe as mp
from tests import test_m1_paths_gpu as m1p


def test_the_probe_names_the_launchers_instance():
    """apa_probe_m1f_instance is m1f_vectors_per_lane behind m1f_supported: 0 where the family refuses C, else the
    64-lane rows of 16-code vectors rounded up to 1 / 2 / 4 / 8; the documented limits of each instance."""
    for C in (0, 8, 24, 8208, 16384):
        assert mp.fp8_instance(C) == 0, C
    for C in range(16, 8193, 16):
        rows = (C // 16 + 63) // 64
        assert mp.fp8_instance(C) == (1 if rows <= 1 else 2 if rows <= 2 else 4 if rows <= 4 else 8), C
    for nv in (1, 2, 4, 8):
        assert mp.fp8_instance(fc.NARROW[nv]) == nv == mp.fp8_instance(fc.WIDE[nv])
        assert (fc.NARROW[nv] // 16) % 64 == 1 or nv == 1       # one vector in the last lane row
        assert mp.fp8_instance(fc.WIDE[nv] + 16) != nv


def test_case_table_reaches_every_key():
    table = fc.reach_table()
    missing = fc.REQUIRED - set(table)
    assert not missing, sorted(missing, key=str)
    names = [c['name'] for c in fc.CASES]
    assert len(names) == len(set(names))
    # 16 instances per pass; no case above 7e7 feature elements or at the benchmark's N = 512, P = 196
    assert len({k for k in table if k[0] == 'instance'}) == 16
    for c in fc.CASES:
        assert c['N'] * c['P'] * c['C'] <= 7e7 and (c['N'], c['P']) != (512, 196), c['name']
        if c['gathered']:
            idx = fc.index_of(c).tolist()
            assert len(idx) == c['N'] and fc.T - 1 in idx and len(set(idx)) < len(idx) and idx != sorted(idx)
            assert min(idx) >= 0 and max(idx) < fc.T
    # the steady state of the chunk loop (a second outer trip) is reached with every PIX
    for nv in (1, 2, 4, 8):
        assert max(max(fc.trip_counts(c)[0]) for c in fc.CASES if mp.fp8_instance(c['C']) == nv) >= 4
    # the head routes behind the pass, by the library's own predicates
    assert {fc.routes(c) for c in fc.CASES if c['C'] in fc.NARROW.values()} == {('sgemm', 'sgemm')}
    wide = {(mp.fp8_instance(c['C']), c['K']): fc.routes(c) for c in fc.CASES if c['C'] >= 4096 and c['C'] % 128 == 0}
    assert wide[(4, 393)] == ('logits2', 'rows') and wide[(4, 20)] == ('logits2', 'tiles')
    assert wide[(8, 20)] == ('logits2', 'rows') and wide[(8, 393)] == ('logits2', 'tiles')


@pytest.mark.parametrize('drop', [c['name'] for c in fc.CASES])
def test_no_case_is_redundant_for_the_reach_table(drop):
    """every case carries at least one key alone: the table is the smallest of its kind, and losing any case is noticed"""
    rest = [c for c in fc.CASES if c['name'] != drop]
    assert fc.REQUIRED - set(fc.reach_table(rest)), drop


@pytest.mark.parametrize('c', [c for c in fc.CASES if c['act'] == 'relu'], ids=lambda c: c['name'])
def test_relu_cases_meet_the_gate_condition(c):
    """In the float64 reference alone: at most 3 % of the N P gates within their bound of zero, 10 % to 90 % of the
    unit-magnitude images' gates open.  A pixel's pre-activation does not depend on its batch position or on the dropout
    mask, so the figures follow from the source images (a gathered case: its T cache images) and the index."""
    inp = fc.inputs(c, 'cpu', batch=False)
    n_img = inp['X'].shape[0]
    mc = dict(fc.model_case(c), N=n_img, train=False)
    ref, amb = m1p._forward_ref(mc, inp, None)
    src = inp['src']
    excl, opn = fc.gate_condition(c, inp, ref['att'].ref[src], amb[src])
    assert opn is not None and excl <= 0.03
