"""Average precision / mAP / accuracy on the device (csrc/apa_metrics.hip) without a GPU: the float64 restatement of
the ranking rule (tests/_map_reference.py) against the product's host routine, the C ABI and every refusal -- made
before any HIP call -- and the argument checks of eval_utils.DeviceEvaluation."""
import os
import re

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd import deploy, eval_utils
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _map_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
FAKE = 0x10000                       # a 16-byte aligned non-null address: nothing is dereferenced


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('T,K', [(1, 1), (2, 3), (3, 2), (63, 5), (64, 5), (65, 5), (257, 40), (1025, 5), (4097, 3),
                                 (16384, 2)])
def test_restatement_equals_compute_map_on_tie_free_scores(T, K):
    scores = mr.tie_free_scores(T, K, seed=T + K)
    labels = np.random.default_rng(T).integers(0, K, size=T)
    ref = mr.map_reference(scores, labels=labels)
    m, aps = eval_utils.compute_map(scores, labels)
    tol_ap, tol_map = mr.bounds(T, K)
    assert len(aps) == len(ref['aps']) == int((ref['npos'] > 0).sum())
    worst = max(abs(a - b) for a, b in zip(aps, ref['aps']))
    print('T=%d K=%d: largest |restatement - compute_map| = %.3g (bound %.3g)' % (T, K, worst, tol_ap))
    assert worst <= tol_ap
    assert abs(m - ref['mAP']) <= tol_map
    assert ref['accuracy'] == eval_utils.accuracy(scores, labels)
    assert np.array_equal(ref['npos'], np.bincount(labels, minlength=K))


def test_restatement_differs_from_compute_map_under_ties():
    """why tied cases are compared with the restatement, never with compute_map: numpy's default argsort is unstable,
    the rule is not"""
    rng = np.random.default_rng(11)
    T, K = 2000, 6
    scores = (np.floor(rng.random((T, K)) * 8) / 8).astype(np.float32)            # 8 levels
    labels = rng.integers(0, K, size=T)
    ref = mr.map_reference(scores, labels=labels)
    _, aps = eval_utils.compute_map(scores, labels)
    diff = max(abs(a - b) for a, b in zip(aps, ref['aps']))
    print('largest |restatement - compute_map| on 8-level scores: %.3g' % diff)
    assert diff > 1e-6
    # the rule itself, on a column small enough to rank by hand: ties by descending index, -0.0 == +0.0, NaN last
    col = np.array([0.5, -0.0, 0.5, 0.0, np.nan, np.inf, -np.inf, 0.5], dtype=np.float32)
    assert mr.ranking(col).tolist() == [5, 7, 2, 0, 3, 1, 6, 4]


def test_restatement_on_multi_hot_targets_is_calc_pr_ovr_noref():
    rng = np.random.default_rng(5)
    T, K = 300, 7
    scores = mr.tie_free_scores(T, K, seed=9)
    targets = (rng.random((T, K)) < 0.3).astype(np.float32) * rng.integers(1, 4, size=(T, K))
    targets[:, 4] = 0
    ref = mr.map_reference(scores, targets=targets)
    assert ref['npos'][4] == 0 and ref['ap'][4] == 0.0 and np.isnan(ref['accuracy'])
    for k in range(K):
        if k != 4:
            assert abs(ref['ap'][k] - eval_utils.calc_pr_ovr_noref(targets[:, k], scores[:, k])[3]) <= T * mr.EPS
    assert abs(ref['mAP'] - np.mean([ref['ap'][k] for k in range(K) if k != 4])) <= (T + K) * mr.EPS


# ------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_entry_points_and_the_rule():
    header = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    defs = dict(re.findall(r'#define\s+(APA_[A-Z0-9_]+)\s+(\d+)u?\b', header))
    assert int(defs['APA_VERSION']) >= 312
    assert int(defs['APA_AP_MAX_SAMPLES']) == cof.APA_AP_MAX_SAMPLES == 16384
    lib = cof.load_library()
    assert lib.apa_version() >= 312
    for name in ('apa_average_precision_workspace_bytes', 'apa_average_precision'):
        assert re.search(r'\b%s\s*\(' % name, header), name + ' is not declared in include/apa.h'
        assert name in cof.exported_symbols() and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(cof._SIGNATURES[name][1])
    assert 'DESCENDING sample' in header and "kind='stable'" in header
    assert 'DESCENDING sample index' in eval_utils.__doc__
    assert callable(cof.average_precision) and callable(cof.average_precision_workspace_bytes)
    assert callable(deploy.FusedHeadEval.new_evaluation)


def _ap(lib, T=100, K=5, labels=FAKE, targets=None, ws=FAKE, ws_bytes=1 << 40, null=None):
    ptrs = dict(scores=FAKE, ap=FAKE, npos=FAKE, summary=FAKE, status=FAKE)
    if null:
        ptrs[null] = None
    rc = lib.apa_average_precision(ptrs['scores'], labels, targets, T, K, ptrs['ap'], ptrs['npos'], ptrs['summary'],
                                   ptrs['status'], ws, ws_bytes, None)
    return rc, lib.apa_last_error().decode()


@pytest.mark.parametrize('field', ['scores', 'ap', 'npos', 'summary', 'status'])
def test_null_required_pointer(field):
    rc, msg = _ap(cof.load_library(), null=field)
    assert rc == INVALID and 'null' in msg


def test_refusals_come_before_any_hip_call():
    lib = cof.load_library()
    rc, msg = _ap(lib, labels=FAKE, targets=FAKE)
    assert rc == INVALID and 'exactly one of labels / targets' in msg and 'both' in msg
    rc, msg = _ap(lib, labels=None, targets=None)
    assert rc == INVALID and 'exactly one of labels / targets' in msg and 'neither' in msg
    for kw in (dict(T=0), dict(K=0), dict(T=-4), dict(K=-1)):
        rc, msg = _ap(lib, **kw)
        assert rc == INVALID and 'non-positive' in msg, (kw, msg)
    for T in (16385, 1 << 20):
        rc, msg = _ap(lib, T=T)
        assert rc == UNSUPPORTED and 'APA_AP_MAX_SAMPLES' in msg and str(T) in msg, msg
        assert lib.apa_status_string(rc) == b'APA_ERR_UNSUPPORTED'
    # the last accepted call stops at the workspace check, with labels and with targets
    for T, K in ((1, 1), (100, 5), (7000, 393), (9600, 600), (16384, 3)):
        need = lib.apa_average_precision_workspace_bytes(T, K)
        assert need > 0
        for kw in (dict(), dict(labels=None, targets=FAKE)):
            rc, msg = _ap(lib, T=T, K=K, ws_bytes=need - 1, **kw)
            assert rc == WORKSPACE and 'workspace' in msg, (T, K, msg)
            rc, msg = _ap(lib, T=T, K=K, ws=None, ws_bytes=need, **kw)
            assert rc == WORKSPACE
    # ... and, with room, at the alignment of the workspace
    rc, msg = _ap(lib, ws=FAKE + 8)
    assert rc == INVALID and 'aligned' in msg


def test_workspace_query():
    q = cof.load_library().apa_average_precision_workspace_bytes
    for T, K in ((1, 1), (1024, 7), (1025, 7), (7000, 393), (16384, 600)):
        tpad = max(1024, 1 << (T - 1).bit_length())
        assert q(T, K) >= K * tpad * 8                           # one 64-bit key per class and padded sample
        assert q(T, K) < K * tpad * 8 + (1 << 16)
        assert cof.average_precision_workspace_bytes(T, K) == q(T, K)
    for bad in ((0, 5), (5, 0), (-1, 5), (16385, 5)):
        assert q(*bad) == 0, bad


def test_wrapper_argument_checks():
    s = torch.zeros(4, 3)
    with pytest.raises(cof.ApaError, match='exactly one'):
        cof.average_precision(s)
    with pytest.raises(cof.ApaError, match='exactly one'):
        cof.average_precision(s, labels=torch.zeros(4, dtype=torch.int64), targets=torch.zeros(4, 3))
    with pytest.raises(cof.ApaError, match=r'labels \[T\]'):
        cof.average_precision(s, labels=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(cof.ApaError, match=r'targets \[T,K\]'):
        cof.average_precision(s, targets=torch.zeros(4, 2))
    with pytest.raises(cof.ApaError, match=r'scores \[T,K\]'):
        cof.average_precision(torch.zeros(4), labels=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(cof.ApaError, match='GPU memory'):        # no CPU fallback
        cof.average_precision(s, labels=torch.zeros(4, dtype=torch.int64))
    assert cof.average_precision_result_bytes(393) == 393 * 12 + 32


# ------------------------------------------------------------------------------------------ DeviceEvaluation
def test_device_evaluation_argument_checks():
    ev = eval_utils.DeviceEvaluation(8, 3, 'cpu')
    assert len(ev) == 0
    with pytest.raises(ValueError, match='nothing was accumulated'):
        ev.result()
    ev.update(torch.rand(5, 3), torch.tensor([0, 1, 2, 0, 1]))
    ev.update(torch.rand(2, 3).double(), torch.tensor([[0], [1]]))               # cast on copy; [n,1] labels as Evaluation
    assert len(ev) == 7
    with pytest.raises(ValueError, match='overflow the capacity of 8'):
        ev.update(torch.rand(2, 3), torch.tensor([0, 1]))
    assert len(ev) == 7                                                          # a refused batch leaves the cursor
    with pytest.raises(ValueError, match=r'labels \[n\]'):
        ev.update(torch.rand(1, 3), torch.zeros(1, 3))
    with pytest.raises(ValueError, match=r'scores \[n,3\]'):
        ev.update(torch.rand(1, 4), torch.tensor([0]))
    with pytest.raises(cof.ApaError, match='GPU memory'):                        # the metric has no CPU fallback
        ev.result()
    ev.reset()
    assert len(ev) == 0
    ml = eval_utils.DeviceEvaluation(4, 3, 'cpu', multi_label=True)
    with pytest.raises(ValueError, match=r'targets \[n,K\]'):
        ml.update(torch.rand(2, 3), torch.tensor([0, 1]))
    ml.update(torch.rand(2, 3), torch.tensor([[0, 1, 1], [1, 0, 0]]))            # any dtype -> float32 on copy
    assert len(ml) == 2 and ml._truth.dtype == torch.float32
    for bad in (dict(capacity=0, num_classes=3), dict(capacity=4, num_classes=0)):
        with pytest.raises(ValueError, match='positive'):
            eval_utils.DeviceEvaluation(device='cpu', **bad)
    with pytest.raises(ValueError, match='16384'):
        eval_utils.DeviceEvaluation(16385, 3, 'cpu')
    # eval_utils.Evaluation is untouched: single labels, host metric
    old = eval_utils.Evaluation()
    old.update(torch.tensor([[0.9, 0.1], [0.2, 0.8]]), torch.tensor([0, 1]))
    assert old.result()['mAP'] == 1.0
