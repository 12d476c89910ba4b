"""The multi-head cached step (include/apa_multihead.h) without a GPU: the header's constants and symbols against the
module's, every refusal in its documented order with the named argument (NULL pointers and dummy addresses: nothing is
ever queued), the workspace plan, and the float64 reference of tests/_multihead_reference.py held against an fp32
emulation of the kernels' arithmetic and against seeded value errors."""
import ctypes
import os
import re

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from attentionalpoolingaction_amd.custom_ops import multihead as mh
from tests import _m1_probe as mp
from tests import _multihead_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, UNSUP, WS = -1, -2, -3
D = 256          # a dummy, 256-byte aligned address: every refusal comes before anything is queued


def _header():
    return open(os.path.join(ROOT, 'include', 'apa_multihead.h')).read()


def test_header_constants_and_symbols_are_the_modules():
    text = _header()
    assert int(re.search(r'#define APA_HEADS_MAX (\d+)', text).group(1)) == mh.APA_HEADS_MAX == 4
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(apa_m\w+)\s*\(', code)))
    assert declared == mh.exported_symbols()
    lib = mh.load_library()
    for name in declared:
        assert hasattr(lib, name), name
        assert name not in cof.exported_symbols()          # apa.h's table stays apa.h's
    assert ctypes.sizeof(mh.ApaMultihead) == 40 and ctypes.sizeof(mh.ApaMultiheadSgd) == 72


class _Call(object):
    """one training / evaluation call on dummy addresses; keyword arguments replace single arguments"""

    def __init__(self, train=True):
        self.train = train
        self.fc = cof.ApaFeatureCache(D, 7, 0, None)
        self.heads = mh.ApaMultihead(2, D, D, D, D)
        self.a = dict(cache=ctypes.addressof(self.fc), heads=ctypes.addressof(self.heads), X=D, labels=D, logits=D, att=D,
                      zsave=D, abar=D, loss=D, G=D, dWa=D, dba=D, dWt=D, dbt=D, probs=D, pred=D, fused_probs=D,
                      fused_pred=D, ws=D, ws_bytes=1 << 30, N=3, P=5, C=512, K=5,
                      flags=cof.APA_FLAG_FROZEN_INPUT if train else 0, dtype=cof.APA_DTYPE_F32, scores_kind=0)

    def __call__(self, **kw):
        lib = mh.load_library()
        a = dict(self.a, **kw)
        if self.train:
            rc = lib.apa_multihead_train_step_cached(
                a['cache'], None, a['heads'], a['X'], a['labels'], 1.0, 1.0, a['logits'], a['att'], a['zsave'], a['abar'],
                a['loss'], a['G'], a['dWa'], a['dba'], a['dWt'], a['dbt'], a['ws'], a['ws_bytes'], a['N'], a['P'], a['C'],
                a['K'], a['flags'], 0.5, 1, 2, a['dtype'], None)
        else:
            rc = lib.apa_multihead_eval_step_cached(
                a['cache'], a['heads'], a['scores_kind'], a['X'], a['labels'], a['logits'], a['att'], a['zsave'], a['abar'],
                a['loss'], a['probs'], a['pred'], a['fused_probs'], a['fused_pred'], a['ws'], a['ws_bytes'], a['N'],
                a['P'], a['C'], a['K'], a['flags'], a['dtype'], None)
        return rc, lib.apa_last_error().decode()


@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
def test_refusals_come_in_the_documented_order(train):
    """each refusal with EVERY later rule violated as well: the earlier one must answer"""
    call = _Call(train)
    FR = cof.APA_FLAG_FROZEN_INPUT if train else 0
    bad_heads = mh.ApaMultihead(5, D, D, D, D)
    rules = [
        # (keyword arguments, code, word of apa_last_error)
        (dict(X=D + 4), UNSUP, 'X must be 16-byte aligned'),                                   # 8
        (dict(ws_bytes=16), WS, 'ws_bytes'),                                                    # 7
        (dict(dtype=cof.APA_DTYPE_FP8_E4M3), UNSUP, 'FP8'),                                     # 6
        (dict(flags=FR | cof.APA_FLAG_RNG_EXTERNAL), UNSUP, 'APA_FLAG_RNG_EXTERNAL'),           # 5
    ]
    if train:
        rules.append((dict(flags=cof.APA_FLAG_RNG_EXTERNAL), INVAL, 'APA_FLAG_FROZEN_INPUT'))   # 4 (5 still violated)
    rules += [
        (dict(C=4100), UNSUP, 'C = 4100'),                                                      # 3
        (dict(heads=ctypes.addressof(bad_heads)), INVAL, 'H = 5'),                              # 2
        (dict(cache=None), INVAL, 'cache is NULL'),                                             # 1
    ]
    acc = {}             # the violations accumulate from the last rule back: the newest one must answer
    for kw, code, word in rules:
        acc.update(kw)
        rc, msg = call(**acc)
        assert rc == code and word in msg, (kw, rc, msg)


def test_each_refusal_names_its_argument():
    call = _Call(True)
    FR = cof.APA_FLAG_FROZEN_INPUT
    fc_null_index = cof.ApaFeatureCache(None, 7, 0, None)
    fc_t0 = cof.ApaFeatureCache(D, 0, 0, None)
    fc_odd = cof.ApaFeatureCache(D + 2, 7, 0, None)
    h0 = mh.ApaMultihead(0, D, D, D, D)
    h_null = mh.ApaMultihead(2, D, None, D, D)
    cases = [
        (dict(heads=None), INVAL, 'heads is NULL'),
        (dict(cache=ctypes.addressof(fc_null_index)), INVAL, 'cache->index is NULL'),
        (dict(heads=ctypes.addressof(h_null)), INVAL, 'heads->ba is NULL'),
        (dict(labels=None), INVAL, 'labels is NULL'), (dict(G=None), INVAL, 'G is NULL'),
        (dict(dbt=None), INVAL, 'dbt is NULL'), (dict(ws=None), INVAL, 'ws is NULL'),
        (dict(heads=ctypes.addressof(h0)), INVAL, 'H = 0'),
        (dict(N=0), INVAL, 'non-positive'), (dict(P=0), INVAL, 'non-positive'), (dict(K=0), INVAL, 'non-positive'),
        (dict(cache=ctypes.addressof(fc_t0)), INVAL, 'cache_images=0'),
        (dict(C=510), UNSUP, 'C = 510'),                                   # not whole 16-byte vectors
        (dict(C=516, dtype=cof.APA_DTYPE_BF16), UNSUP, 'C = 516'),         # fp32 serves it, bf16 does not
        (dict(flags=FR | cof.APA_FLAG_SOFTMAX_ATT), UNSUP, 'APA_FLAG_SOFTMAX_ATT'),
        (dict(flags=FR | cof.APA_FLAG_RELU_INPUT), UNSUP, 'APA_FLAG_RELU_INPUT'),
        (dict(flags=FR | cof.APA_FLAG_RNG_DEVICE), UNSUP, 'APA_FLAG_RNG_DEVICE'),
        (dict(dtype=9), INVAL, 'unknown dtype'),
        (dict(ws_bytes=mh.workspace_bytes(2, 3, 5, 512, 5) - 1), WS, 'ws_bytes'),
        (dict(ws=D + 8), UNSUP, 'ws must be 16-byte aligned'), (dict(zsave=D + 4), UNSUP, 'zsave must be'),
        (dict(cache=ctypes.addressof(fc_odd)), UNSUP, 'cache->index must be 4-byte aligned'),
    ]
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    ev = _Call(False)
    for kw, code, word in [(dict(probs=None), INVAL, 'probs is NULL'), (dict(pred=None), INVAL, 'pred is NULL'),
                           (dict(fused_probs=None), INVAL, 'fused_probs is NULL'),
                           (dict(labels=None), INVAL, 'labels is NULL'), (dict(loss=None), INVAL, 'loss is NULL'),
                           (dict(scores_kind=2), INVAL, 'scores_kind'),
                           (dict(scores_kind=1), INVAL, 'sigmoid'),
                           (dict(dtype=cof.APA_DTYPE_FP8_E4M3), UNSUP, 'FP8')]:
        rc, msg = ev(**kw)
        assert rc == code and word in msg, (kw, rc, msg)


def test_sgd_and_epoch_refusals():
    lib = mh.load_library()
    w = (ctypes.c_void_p * 1)(D)
    sz = (ctypes.c_size_t * 1)(8)
    f = (ctypes.c_float * 4)(0, 0, 0, 0)
    A = ctypes.addressof
    assert lib.apa_momentum_sgd_step_heads(5, 1, A(w), A(sz), A(f), D, D, A(f), A(f), 1.0, None) == INVAL
    assert 'H = 5' in lib.apa_last_error().decode()
    assert lib.apa_momentum_sgd_step_heads(2, 0, A(w), A(sz), A(f), D, D, A(f), A(f), 1.0, None) == INVAL
    assert lib.apa_momentum_sgd_step_heads(2, 1, A(w), A(sz), A(f), D, D, None, A(f), 1.0, None) == INVAL
    wn = (ctypes.c_void_p * 1)(None)
    assert lib.apa_momentum_sgd_step_heads(2, 1, A(wn), A(sz), A(f), D, D, A(f), A(f), 1.0, None) == INVAL
    assert 'weights[0] is NULL' in lib.apa_last_error().decode()
    # the epochs: ep / opt / lr / order, then the count rules
    fc = cof.ApaFeatureCache(None, 7, 0, None)
    heads = mh.ApaMultihead(2, D, D, D, D)
    opt = mh.ApaMultiheadSgd(1, A(w), A(sz), A(f), D, D, A(f), A(f), 1.0)
    ep = cof.ApaEpoch(D, 6)
    tail = (D, D, 1.0, 1.0) + (D,) * 10 + (D, 1 << 30, 3, 5, 512, 5, cof.APA_FLAG_FROZEN_INPUT, 0.5, 1, 2, 0, None)

    def train(ep_, opt_, fc_=A(fc), heads_=A(heads), tail_=tail):
        rc = lib.apa_multihead_train_epoch_cached(ep_, opt_, fc_, None, heads_, *tail_)
        return rc, lib.apa_last_error().decode()
    assert train(None, A(opt)) == (INVAL, 'apa_multihead_train_epoch_cached: ep is NULL')
    assert train(A(ep), None)[1].endswith('opt is NULL')
    assert train(A(ep), A(mh.ApaMultiheadSgd(1, A(w), A(sz), A(f), D, D, None, A(f), 1.0)))[1].endswith('opt->lr is NULL')
    assert train(A(cof.ApaEpoch(None, 6)), A(opt))[1].endswith('ep->order is NULL')
    rc, msg = train(A(cof.ApaEpoch(D, 7)), A(opt))
    assert rc == INVAL and 'count = 7' in msg
    rc, msg = train(A(ep), A(opt), tail_=tail[:-5] + (0.5, 1, 2, cof.APA_DTYPE_FP8_E4M3, None))
    assert rc == UNSUP and 'FP8' in msg
    etail = (0, D, None) + (D,) * 4 + (None, D, D, D, D) + (D, 1 << 30, 3, 5, 512, 5, 0, 0, None)
    rc = lib.apa_multihead_eval_epoch_cached(A(cof.ApaEpoch(D, 0)), A(fc), A(heads), *etail)
    assert rc == INVAL and 'count = 0' in lib.apa_last_error().decode()
    rc = lib.apa_multihead_eval_epoch_cached(A(cof.ApaEpoch(D, 7)), A(fc), A(heads), *(etail[:-3] + (0, cof.APA_DTYPE_FP8_E4M3, None)))
    assert rc == UNSUP and 'FP8' in lib.apa_last_error().decode()


@pytest.mark.parametrize('shape', [(1, 1, 1, 512, 1), (4, 32, 196, 2048, 393), (3, 33, 5, 516, 5), (2, 3, 7, 520, 12),
                                   (4, 512, 196, 2048, 393), (1, 1025, 9, 8, 2)])
def test_workspace_bytes_equal_the_plan(shape):
    assert mh.workspace_bytes(*shape) == mh.plan_bytes(*shape) > 0
    H, N, P, C, K = shape
    assert mr.plan(N, P)[2] == N * mr.plan(N, P)[0]


def test_workspace_bytes_of_refused_arguments_are_zero():
    for shape in [(0, 3, 5, 512, 5), (5, 3, 5, 512, 5), (2, 0, 5, 512, 5), (2, 3, 0, 512, 5), (2, 3, 5, 0, 5),
                  (2, 3, 5, 512, 0)]:
        assert mh.workspace_bytes(*shape) == mh.plan_bytes(*shape) == 0


def test_grad_layout_is_the_stacked_outputs_back_to_back():
    offs, total = mh.grad_layout(3, 8, 5)
    assert offs == [0, 24, 27, 147] and total == 162


# ------------------------------------------------------------------------------------------ the float64 reference
def _host_mask(n, keep, seed, offset):
    """apa_dropout_mask restated on the host (csrc/apa_device.h: rng_hash / rng_keep2, apa_internal.h: rng_key)"""
    M64, M32 = (1 << 64) - 1, (1 << 32) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (offset + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    k0, k1 = z & M32, z >> 32
    thresh = int(min(max(keep * 65536.0 + 0.5, 0.0), 65536.0))
    q = torch.arange((n + 1) // 2, dtype=torch.int64)
    x = (q ^ k0) & M32
    x ^= x >> 16
    x = ((x & 0xFFFFFF) * 0xB5297B) & M32
    x ^= x >> 13
    x ^= k1
    x ^= x >> 17
    x = ((x & 0xFFFFFF) * 0x68E31D) & M32
    x ^= x >> 15
    m = torch.stack([(x & 0xFFFF) < thresh, (x >> 16) < thresh], dim=1).reshape(-1)[:n]
    return m.to(torch.uint8)


CPU_CASES = [mr.case('cpu_f32_relu', 3, 3, 5, 64, 5), mr.case('cpu_bf16_id', 2, 3, 9, 72, 7, bf16=True, relu=False)]


@pytest.mark.parametrize('c', CPU_CASES, ids=[c['name'] for c in CPU_CASES])
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'dropout'])
def test_reference_admits_the_fp32_emulation_and_rejects_value_errors(c, train):
    inp = mr.inputs(c)
    assert mr.gate_count(c, inp) == 0
    N, P, C = c['N'], c['P'], c['C']
    mask = _host_mask(N * P * C, mr.KEEP, mr.SEED, mr.OFFSET) if train else None
    if train:
        assert 0.4 < float(mask.float().mean()) < 0.6
    got = mr.emulate_fp32(c, inp, mask)
    got['loss'] = torch.cat([got['loss'][:, None], got.pop('loss_rows')], dim=1)
    mr.check_all(c, inp, got, mask)
    # seeded value errors: one element of one output moved by 1e-3 of the output's scale, a head's rows swapped, a
    # dropped pixel -- each must be rejected
    g = torch.Generator().manual_seed(5)
    for key in ('att', 'zsave', 'abar', 'logits', 'G', 'dWa', 'dWt', 'dbt', 'dba'):
        bad = {k: v.contiguous().clone() for k, v in got.items()}
        flat = bad[key].view(-1)
        i = int(torch.randint(0, flat.numel(), (1,), generator=g))
        flat[i] += 1e-3 * float(bad[key].abs().max())
        with pytest.raises(AssertionError):
            mr.check_all(c, inp, bad, mask)
    bad = {k: v.contiguous().clone() for k, v in got.items()}
    bad['zsave'] = bad['zsave'].flip(0)
    with pytest.raises(AssertionError):
        mr.check_all(c, inp, bad, mask)
    bad = {k: v.contiguous().clone() for k, v in got.items()}
    bad['abar'] = bad['abar'] - got['att'][:, :, 0] / P
    with pytest.raises(AssertionError):
        mr.check_all(c, inp, bad, mask)


def test_fused_scores_reference():
    p = torch.softmax(torch.randn(4, 3, 11, generator=torch.Generator().manual_seed(1)), dim=-1)
    fused = ((p[0] + p[1]) + p[2] + p[3]) / 4
    mp.check(fused, mr.fused_bnd(p), 'fused')
    with pytest.raises(AssertionError):
        mp.check(fused * (1 + 1e-5), mr.fused_bnd(p), 'fused')


def test_gpu_case_table_reaches_every_edge():
    cs = mr.CASES
    assert {c['H'] for c in cs} == {1, 2, 3, 4}
    assert {2048, 512} <= {c['C'] for c in cs} and any(c['C'] % 256 for c in cs)
    for bf in (False, True):          # the wide instance with one vector in its last lane row, per element type
        epv = 8 if bf else 4
        assert any(c['bf16'] == bf and c['C'] > 512 and (c['C'] // epv) % 64 == 1 for c in cs)
        assert any(c['bf16'] == bf and c['C'] == 2048 for c in cs) and any(c['bf16'] == bf and c['C'] == 512 for c in cs)
    assert {1, 5, 196} <= {c['P'] for c in cs} and {1, 3, 33} <= {c['N'] for c in cs} and {1, 5, 393} <= {c['K'] for c in cs}
    assert {c['relu'] for c in cs} == {False, True} and {c['labels_cached'] for c in cs} == {False, True}
