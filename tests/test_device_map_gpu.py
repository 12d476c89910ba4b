"""Average precision / mAP / accuracy on the device (csrc/apa_metrics.hip: apa_average_precision, three launches)
against the product's host routines (eval_utils.compute_map / calc_pr_ovr_noref / accuracy) on tie-free scores and
against the float64 restatement of the ranking rule (tests/_map_reference.py) under ties.

Bounds (tests/_map_reference.bounds): the terms of an AP are non-negative and sum to at most 1, so any fixed summation
order and the host's sequential one differ by at most T * 2^-52 per class, the means by (T + K) * 2^-52.  (The kernel
adds an AP's terms in the host's own order; each test prints what it measured, on an MI355X 0 per class.)  Counts and
the accuracy are exact.  Shapes: the sort kernel pads a class to max(1024, next power of two) keys, 16 per
thread -- T = 1 .. 65 run one wave, 1025 two, 4097 eight, 16384 the full 1024-thread block with 128 KiB of LDS."""
import functools

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd import config as apa_config, deploy, eval_utils, nets_factory
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _map_reference as mr

pytestmark = pytest.mark.gpu

P = 'USE_POSE_PRELOGITS_BASED_ATTENTION'


def device_map(gpu, scores, labels=None, targets=None):
    """the raw call on numpy inputs -> (ap, npos, summary, status) as numpy"""
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(gpu)
    lab = None if labels is None else torch.from_numpy(np.asarray(labels, dtype=np.int64)).to(gpu)
    tgt = None if targets is None else torch.from_numpy(np.ascontiguousarray(targets, dtype=np.float32)).to(gpu)
    out = cof.average_precision(s, labels=lab, targets=tgt)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def tie_free_case(T, K):
    scores = mr.tie_free_scores(T, K, seed=100 * T + K)
    labels = np.random.default_rng(T + 7 * K).integers(0, K, size=T)
    m, aps = eval_utils.compute_map(scores, labels)
    return scores, labels, m, aps, eval_utils.accuracy(scores, labels)


def check_against(ap, npos, summary, status, ref_ap, ref_npos, ref_map, ref_acc, T, K, what):
    tol_ap, tol_map = mr.bounds(T, K)
    assert status.tolist() == [0, 0], what
    assert np.array_equal(npos, ref_npos), what
    err = float(np.abs(ap - ref_ap).max())
    print('%s: T=%d K=%d  max |ap - ref| = %.3g (bound %.3g)  |mAP - ref| = %.3g (bound %.3g)'
          % (what, T, K, err, tol_ap, abs(summary[0] - ref_map), tol_map))
    assert err <= tol_ap, what
    assert np.all(ap[ref_npos == 0] == 0.0), what
    assert abs(summary[0] - ref_map) <= tol_map, what
    assert summary[2] == float((ref_npos > 0).sum()), what
    if ref_acc is None:
        assert np.isnan(summary[1]), what
    else:
        assert summary[1] == ref_acc, what                       # bit-equal: an integer count over T


SHAPES = [(T, K) for T in (1, 2, 3, 63, 64, 65, 1025, 4097) for K in (1, 5)] + [(257, 393), (16384, 3)]


@pytest.mark.parametrize('T,K', SHAPES)
def test_tie_free_scores_match_compute_map(gpu, T, K):
    scores, labels, m, aps, acc = tie_free_case(T, K)
    ref_npos = np.bincount(labels, minlength=K).astype(np.int32)
    ref_ap = np.zeros(K)
    ref_ap[ref_npos > 0] = aps                                   # compute_map lists the classes with positives, in order
    out = device_map(gpu, scores, labels=labels)
    check_against(*out, ref_ap, ref_npos, m, acc, T, K, 'tie-free')


def tied_columns(T, rng):
    q8 = (np.floor(rng.random(T) * 8) / 8 - 0.5).astype(np.float32)               # 8 levels, some negative
    const = np.full(T, 0.25, dtype=np.float32)
    zeros = np.where(rng.random(T) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros[::7] = rng.standard_normal(len(zeros[::7])).astype(np.float32)
    infs = rng.standard_normal(T).astype(np.float32)
    infs[rng.random(T) < 0.2] = np.inf
    infs[rng.random(T) < 0.2] = -np.inf
    return np.stack([q8, const, zeros, infs, q8[::-1].copy()], axis=1)


@pytest.mark.parametrize('T', [65, 1500])
def test_tied_scores_match_the_restatement(gpu, T):
    rng = np.random.default_rng(T)
    scores = tied_columns(T, rng)
    K = scores.shape[1]
    assert np.signbit(scores[:, 2]).any() and (scores[:, 2] == 0).sum() > T // 2
    labels = rng.integers(0, K, size=T)
    ref = mr.map_reference(scores, labels=labels)
    out = device_map(gpu, scores, labels=labels)
    check_against(*out, ref['ap'], ref['npos'], ref['mAP'], ref['accuracy'], T, K, 'tied columns')


def test_row_maximum_attained_twice(gpu):
    rng = np.random.default_rng(3)
    T, K = 200, 6
    scores = (np.floor(rng.random((T, K)) * 8) / 8).astype(np.float32)
    a, b = rng.integers(0, K, size=T), rng.integers(0, K, size=T)
    rows = np.arange(T)
    scores[rows, a] = 2.0
    scores[rows, b] = 2.0                                        # the row's maximum, twice where a != b
    labels = np.where(rng.random(T) < 0.5, np.minimum(a, b), np.maximum(a, b))
    assert (a != b).sum() > T // 2
    ref = mr.map_reference(scores, labels=labels)
    assert 0.3 < ref['accuracy'] < 0.9                           # the first maximum wins, as np.argmax: not all, not none
    out = device_map(gpu, scores, labels=labels)
    check_against(*out, ref['ap'], ref['npos'], ref['mAP'], ref['accuracy'], T, K, 'double maxima')


def test_edge_classes(gpu):
    T, K = 90, 6
    scores = mr.tie_free_scores(T, K, seed=1)
    # every sample positive for class 2 (so no other class has one): AP == 1.0 exactly, the mean is over one class
    ap, npos, summary, status = device_map(gpu, scores, labels=np.full(T, 2))
    assert npos.tolist() == [0, 0, T, 0, 0, 0] and ap.tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert summary[0] == 1.0 and summary[2] == 1.0 and status.tolist() == [0, 0]
    # class 4's single positive ranks last: AP = 1 / T; classes 2 and 5 have no positive and are left out of the mean
    labels = np.random.default_rng(2).choice([0, 1, 3], size=T)
    last = int(np.argmin(scores[:, 4]))
    labels[last] = 4
    ref = mr.map_reference(scores, labels=labels)
    out = device_map(gpu, scores, labels=labels)
    check_against(*out, ref['ap'], ref['npos'], ref['mAP'], ref['accuracy'], T, K, 'edge classes')
    ap, npos, summary, _ = out
    assert npos[2] == 0 and npos[5] == 0 and npos[4] == 1 and ap[4] == 1.0 / T
    assert summary[2] == 4.0 and abs(summary[0] - ap[[0, 1, 3, 4]].mean()) <= (T + K) * mr.EPS
    # the same three kinds in one multi-hot call; no class has a positive at all: mAP is NaN
    targets = np.zeros((T, K), dtype=np.float32)
    targets[:, 0] = 1
    targets[int(np.argmin(scores[:, 1])), 1] = 3.0
    ap, npos, summary, _ = device_map(gpu, scores, targets=targets)
    assert npos.tolist() == [T, 1, 0, 0, 0, 0] and ap[0] == 1.0 and ap[1] == 1.0 / T and not ap[2:].any()
    ap, npos, summary, _ = device_map(gpu, scores, targets=np.zeros((T, K), dtype=np.float32))
    assert not npos.any() and not ap.any() and np.isnan(summary[0]) and summary[2] == 0.0


def test_multi_hot_targets_match_calc_pr_ovr_noref(gpu):
    rng = np.random.default_rng(5)
    T, K = 300, 7
    scores = mr.tie_free_scores(T, K, seed=9)
    targets = (rng.random((T, K)) < 0.3).astype(np.float32) * rng.integers(1, 4, size=(T, K))
    targets[rng.random((T, K)) < 0.05] = -1.0                    # not positive: the rule is > 0
    targets[:, 4] = 0
    ref_npos = (targets > 0).sum(0).astype(np.int32)
    ref_ap = np.array([eval_utils.calc_pr_ovr_noref(targets[:, k], scores[:, k])[3] if ref_npos[k] else 0.0
                       for k in range(K)])
    out = device_map(gpu, scores, targets=targets)
    check_against(*out, ref_ap, ref_npos, float(ref_ap[ref_npos > 0].mean()), None, T, K, 'multi-hot')
    assert out[1][4] == 0 and 0.2 * T < out[1][0] < 0.4 * T


def test_status_counts_and_the_python_layer_raises(gpu):
    T, K = 70, 4
    scores = mr.tie_free_scores(T, K, seed=4)
    labels = np.random.default_rng(4).integers(0, K, size=T)
    bad_scores = scores.copy()
    bad_scores[13, 2] = np.nan
    bad_labels = labels.copy()
    bad_labels[40] = K
    ap, npos, summary, status = device_map(gpu, bad_scores, labels=bad_labels)
    assert status.tolist() == [1, 1]
    assert int(npos.sum()) == T - 1                              # a label outside [0,K) matches no class
    # the NaN ranks last: the other classes' APs are those of the clean scores
    clean = mr.map_reference(scores, labels=bad_labels)
    assert np.abs(ap[[0, 1, 3]] - clean['ap'][[0, 1, 3]]).max() <= T * mr.EPS
    nan_ref = mr.map_reference(bad_scores, labels=bad_labels)
    assert abs(ap[2] - nan_ref['ap'][2]) <= T * mr.EPS
    for s, l, text in ((bad_scores, labels, '1 NaN scores, 0 labels'), (scores, bad_labels, '0 NaN scores, 1 labels')):
        ev = eval_utils.DeviceEvaluation(T, K, gpu)
        ev.update(torch.from_numpy(s).to(gpu), torch.from_numpy(l).to(gpu))
        with pytest.raises(ValueError, match=text):
            ev.result()
    ev = eval_utils.DeviceEvaluation(T, K, gpu)
    ev.update(torch.from_numpy(scores).to(gpu), torch.from_numpy(labels).to(gpu))
    assert ev.result()['mAP'] > 0


def test_two_calls_give_the_same_bits(gpu):
    scores, labels, _, _, _ = tie_free_case(4097, 5)
    s, lab = torch.from_numpy(scores).to(gpu), torch.from_numpy(labels).to(gpu)
    first = [t.clone() for t in cof.average_precision(s, labels=lab)]
    second = cof.average_precision(s, labels=lab)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    tied = torch.from_numpy(tied_columns(1500, np.random.default_rng(0))).to(gpu)
    lab = torch.from_numpy(np.random.default_rng(1).integers(0, 5, size=1500)).to(gpu)
    first = [t.clone() for t in cof.average_precision(tied, labels=lab)]
    for a, b in zip(first, cof.average_precision(tied, labels=lab)):
        assert torch.equal(a, b)


def _stream(ev, scores, labels, batches):
    at = 0
    for n in batches:
        ev.update(scores[at:at + n], labels[at:at + n])
        at += n
    assert at == len(scores) == len(ev)
    return ev.result()


def test_streaming_equals_evaluation_and_reset_leaks_nothing(gpu):
    K, batches = 5, (5, 32, 1, 32, 5)
    T = sum(batches)
    ev = eval_utils.DeviceEvaluation(128, K, gpu)
    tol_ap, tol_map = mr.bounds(T, K)
    for seed, bs in ((1, batches), (2, batches[:3])):            # the second pass is shorter: stale rows stay behind it
        n = sum(bs)
        scores = torch.from_numpy(mr.tie_free_scores(n, K, seed=seed)).to(gpu)
        labels = torch.from_numpy(np.random.default_rng(seed).integers(0, K, size=n)).to(gpu)
        old = eval_utils.Evaluation()
        old.update(scores, labels)
        ref = old.result()
        got = _stream(ev, scores, labels, bs)
        assert got['accuracy'] == ref['accuracy']
        assert len(got['aps']) == len(ref['aps']) and abs(got['mAP'] - ref['mAP']) <= tol_map
        assert max(abs(a - b) for a, b in zip(got['aps'], ref['aps'])) <= tol_ap
        assert got['npos'].tolist() == np.bincount(labels.cpu().numpy(), minlength=K).tolist()
        assert got['ap_per_class'].shape == (K,) and got['ap_per_class'].dtype == np.float64
        ev.reset()
        assert len(ev) == 0
    with pytest.raises(ValueError, match='overflow'):
        ev.update(torch.zeros(129, K, device=gpu), torch.zeros(129, dtype=torch.int64, device=gpu))


def test_through_fused_head_eval(gpu):
    apa_config.reset_cfg()
    K = 7
    for loss_fn, multi in (('softmax-xentropy', False), ('multi-label', True)):
        cfg = apa_config.cfg_from_dict({'NET': {P: True, P + '_SINGLE_LAYER_ATT': True},
                                        'TRAIN': {'LOSS_FN_ACTION': loss_fn}})
        fn = nets_factory.get_network_fn('resnet_v1_101', K, 16, cfg, is_training=False, device=gpu, in_channels=32)
        with torch.no_grad():                                    # weights large enough for scores that differ
            fn.head.td_weights.normal_(0.0, 0.5, generator=torch.Generator(device=gpu).manual_seed(1))
        ev = deploy.FusedHeadEval(fn, cfg)
        meter = ev.new_evaluation(16)
        assert isinstance(meter, eval_utils.DeviceEvaluation) and meter.multi_label == multi
        assert meter.num_classes == K and meter.capacity == 16 and meter.device == fn.head.td_weights.device
        g = torch.Generator().manual_seed(8)
        kept, truth = [], []
        for _ in range(3):
            x = torch.relu(torch.randn(4, 3, 3, 32, generator=g)).to(gpu)
            lab = (torch.rand(4, K, generator=g) < 0.4).float() if multi else torch.randint(0, K, (4,), generator=g)
            scores, _, _ = ev(x, None if multi else lab.to(gpu))
            meter.update(scores, lab.to(gpu))
            kept.append(scores.clone())                          # (the step's buffer is overwritten by the next batch)
            truth.append(lab)
        scores = torch.cat(kept).cpu().numpy()
        truth = torch.cat(truth).numpy()
        ref = mr.map_reference(scores, targets=truth) if multi else mr.map_reference(scores, labels=truth)
        got = meter.result()
        tol_ap, tol_map = mr.bounds(12, K)
        assert got['npos'].tolist() == ref['npos'].tolist()
        assert np.abs(got['ap_per_class'] - ref['ap']).max() <= tol_ap
        assert abs(got['mAP'] - ref['mAP']) <= tol_map
        assert (np.isnan(got['accuracy']) and multi) or got['accuracy'] == ref['accuracy']
        assert len(got['aps']) == int((ref['npos'] > 0).sum())
    apa_config.reset_cfg()
