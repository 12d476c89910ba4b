"""A whole clip / multi-label epoch behind one host call, without a GPU: the new header, clip_epoch.py's signature table
and the library agree; the keyed sampler's draw rule against an independent big-integer transcription; every refusal of
the three entry points and of the two deploy methods is made, by name, before any HIP call (dummy pointers: a call that
got past its checks would fault)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import clip_epoch as ce
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests.test_epoch_call_cpu import _Sgd         # an apa_epoch_sgd over host arrays of fake device pointers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
FAKE = 0x10000                       # a 16-byte aligned non-null address: nothing is dereferenced
FROZEN = cof.APA_FLAG_FROZEN_INPUT
UNIFORM, RANDOM = cof.APA_CLIP_FRAMES_UNIFORM, cof.APA_CLIP_FRAMES_RANDOM_SEGMENT
ML, ML2 = cof.ACTION_LOSS_KINDS['multi-label'], cof.ACTION_LOSS_KINDS['multi-label-2']


# ------------------------------------------------------------------------------------------ ABI
def _bare_header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'apa_clip_epoch.h')).read(), flags=re.S)


def test_header_table_and_library_agree():
    bare = _bare_header()
    declared = set(re.findall(r'\b(apa_[a-z0-9_]+)\s*\(', bare))
    assert declared == {'apa_sample_clip_frames_keyed', 'apa_attn_head_train_epoch_cached_clips',
                        'apa_attn_head_eval_epoch_cached_clips'}
    assert declared == set(ce.exported_symbols()) == set(ce._SIGNATURES)          # nothing else is bound
    assert '#include "apa.h"' in bare
    lib = ce.load_library()
    assert lib is cof.load_library()                                            # the same libapa_hip.so
    for name in declared:
        fn = getattr(lib, name)
        assert fn.restype is ce._SIGNATURES[name][0] and list(fn.argtypes) == list(ce._SIGNATURES[name][1]), name
        assert name not in cof.exported_symbols()                               # apa.h's table stays apa.h's
        # one ctypes slot per declared parameter
        m = re.search(r'\b%s\s*\((.*?)\)\s*;' % name, bare, flags=re.S)
        assert len(m.group(1).split(',')) == len(ce._SIGNATURES[name][1]), name
    # the epoch signatures are the *_cached_clips steps' with the descriptors in front
    step = cof._SIGNATURES['apa_attn_head_train_step_cached_clips']      # (cache, ml, clip, hooks, X ...)
    assert ce._SIGNATURES['apa_attn_head_train_epoch_cached_clips'] == (step[0], [ctypes.c_void_p] * 3 + list(step[1]))
    ev = cof._SIGNATURES['apa_attn_head_eval_step_cached_clips']         # (cache, clip, kind, X ...)
    assert ce._SIGNATURES['apa_attn_head_eval_epoch_cached_clips'] == (ev[0], [ctypes.c_void_p] * 2 + list(ev[1]))
    # the descriptor: field order and types are the ABI
    m = re.search(r'typedef struct apa_clip_epoch \{(.*?)\} apa_clip_epoch;', bare, flags=re.S)
    fields = [f.strip() for f in m.group(1).split(';') if f.strip()]
    assert fields == ['const int32_t* video_first', 'const int32_t* video_frames', 'const int64_t* video_labels',
                      'const float* video_targets', 'int V', 'int mode', 'uint64_t seed, epoch', 'int32_t* index',
                      'int64_t* labels', 'float* targets']
    assert [n for n, _ in ce.ApaClipEpoch._fields_] == ['video_first', 'video_frames', 'video_labels', 'video_targets',
                                                        'V', 'mode', 'seed', 'epoch', 'index', 'labels', 'targets']
    E = ce.ApaClipEpoch
    assert ctypes.sizeof(E) == 80 and (E.V.offset, E.mode.offset, E.seed.offset, E.epoch.offset, E.index.offset,
                                       E.targets.offset) == (32, 36, 40, 48, 56, 72)


# ------------------------------------------------------------------------------------------ the draw rule
M64, M32 = (1 << 64) - 1, (1 << 32) - 1


def _mix64_int(s, o):
    """include/apa.h's mix64 on python integers, transcribed from the header (not from custom_ops_factory)"""
    z = (s + 0x9E3779B97F4A7C15 * (o + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _hash_int(x, k0, k1):
    """include/apa.h's hash on python integers"""
    x ^= k0
    x ^= x >> 16
    x = ((x & 0xFFFFFF) * 0xB5297B) & M32
    x ^= x >> 13
    x ^= k1
    x ^= x >> 17
    x = ((x & 0xFFFFFF) * 0x68E31D) & M32
    return x ^ (x >> 15)


def _draws_int(n, seed, epoch, step):
    """the 24-bit integers u[j] * 2^24 of include/apa_clip_epoch.h"""
    h = _mix64_int(_mix64_int(seed & M64, epoch & M64), step & M64)
    return [_hash_int(j, h & M32, h >> 32) >> 8 for j in range(n)]


@pytest.mark.parametrize('seed,epoch,step', [(0, 0, 0), (7, 3, 2), (2 ** 64 - 1, 2 ** 40 + 5, 2 ** 33), (-1, 1, 0)])
def test_draw_rule_is_the_big_integer_transcription(seed, epoch, step):
    B, F = 37, 25
    u = ce.clip_draws_rule_cpu(B, F, seed, epoch, step)
    assert u.dtype == torch.float32 and tuple(u.shape) == (B * F,) and u.is_contiguous()
    want = _draws_int(B * F, seed, epoch, step)
    assert all(0 <= w < 2 ** 24 for w in want)
    scaled = u.double() * 2.0 ** 24
    assert bool((u >= 0).all()) and bool((u < 1).all())                    # every u in [0, 1)
    assert torch.equal(scaled, scaled.round())                              # u * 2^24 is an integer ...
    assert scaled.long().tolist() == want                                   # ... the transcription's, exactly
    # element j depends on j alone: a shorter call is a prefix
    assert torch.equal(ce.clip_draws_rule_cpu(3, F, seed, epoch, step), u[:3 * F])


def test_draws_differ_between_steps_epochs_and_seeds_and_fill_the_interval():
    base = ce.clip_draws_rule_cpu(8, 25, 11, 5, 3)
    assert torch.equal(base, ce.clip_draws_rule_cpu(8, 25, 11, 5, 3))
    for key in ((11, 5, 4), (11, 6, 3), (12, 5, 3), (5, 11, 3), (11, 3, 5)):
        other = ce.clip_draws_rule_cpu(8, 25, *key)
        assert not torch.equal(base, other) and int((base == other).sum()) <= 1, key
    # 40000 draws: the mean and the occupancy of 16 bins are a uniform sample's (sigma of the mean: 0.0014)
    u = ce.clip_draws_rule_cpu(1600, 25, 1, 2, 3).double()
    assert abs(float(u.mean()) - 0.5) < 0.01
    bins = torch.bincount((u * 16).long(), minlength=16)
    assert int(bins.min()) > 2500 * 0.9 and int(bins.max()) < 2500 * 1.1
    with pytest.raises(cof.ApaError, match='B >= 1'):
        ce.clip_draws_rule_cpu(0, 3, 1, 2, 3)
    with pytest.raises(cof.ApaError, match='integers'):
        ce.clip_draws_rule_cpu(2, 3, 'x', 2, 3)


# ------------------------------------------------------------------------------------------ refusals: the sampler
def _keyed(lib, first=FAKE, frames=FAKE, vlab=None, vtar=None, videos=FAKE, index=FAKE, labels=None, targets=None,
           V=5, B=2, F=3, K=8, mode=RANDOM):
    rc = lib.apa_sample_clip_frames_keyed(first, frames, vlab, vtar, videos, index, labels, targets, None, V, B, F, K,
                                          mode, 1, 2, 3, None)
    return rc, lib.apa_last_error()


def test_keyed_sampler_refusals_are_the_samplers_minus_u():
    lib = ce.load_library()
    fn = b'apa_sample_clip_frames_keyed'
    for kw, word in ((dict(first=None), b'null video_first'), (dict(frames=None), b'null video_first'),
                     (dict(videos=None), b'null video_first'), (dict(index=None), b'null video_first'),
                     (dict(vlab=FAKE), b'video_labels needs labels'), (dict(vtar=FAKE), b'video_targets needs targets'),
                     (dict(V=0), b'non-positive size V=0'), (dict(B=0), b'B=0'), (dict(F=-1), b'frames=-1'),
                     (dict(vtar=FAKE, targets=FAKE, K=0), b'K=0'), (dict(mode=2), b'unknown mode 2'),
                     (dict(B=2 ** 20, F=2 ** 11), b'past 2^31 - 1')):
        rc, err = _keyed(lib, **kw)
        assert rc == INVALID and word in err and fn in err, (kw, rc, err)
        # the same refusal, with the same words behind the name, as apa_sample_clip_frames makes it
        a = dict(dict(first=FAKE, frames=FAKE, vlab=None, vtar=None, videos=FAKE, index=FAKE, labels=None, targets=None,
                      V=5, B=2, F=3, K=8, mode=RANDOM), **kw)
        rc2 = lib.apa_sample_clip_frames(a['first'], a['frames'], a['vlab'], a['vtar'], a['videos'], FAKE, a['index'],
                                         a['labels'], a['targets'], None, a['V'], a['B'], a['F'], a['K'], a['mode'], None)
        assert rc2 == INVALID and lib.apa_last_error().split(b': ', 1)[1] == err.split(b': ', 1)[1], kw
    # python: refused before the library is asked
    cache = cof.FeatureCache(torch.zeros(6, 1, 1, 16))
    with pytest.raises(cof.ApaError, match='set_videos first'):
        ce.sample_clips_keyed(cache, [0], 3)
    cache.set_videos([0, 2], [2, 4])
    with pytest.raises(cof.ApaError, match='GPU memory'):
        ce.sample_clips_keyed(cache, [0], 3)
    with pytest.raises(cof.ApaError, match='mode must be one of'):
        ce.sample_clips_keyed(cache, [0], 3, mode='dense')


# ------------------------------------------------------------------------------------------ refusals: the epoch calls
def _ce(first=FAKE, frames=FAKE, vlab=FAKE, vtar=FAKE, V=7, mode=RANDOM, index=FAKE, labels=FAKE, targets=FAKE):
    return ce.ApaClipEpoch(first, frames, vlab, vtar, V, mode, 3, 4, index, labels, targets)


def _clip(frames=3, w=None, b=None, pooled=FAKE, tatt=None, dw=None, db=None):
    return cof.ApaClipPool(frames, w, b, pooled, tatt, dw, db)


def _ptr(s):
    return None if s is None else ctypes.addressof(s)


def _train(lib, ep='default', opt='default', cep='default', cache='default', ml=None, clip='default', dtype=0, N=6,
           P=9, C=32, K=8, M=1, flags=FROZEN, xatt=FAKE, dX=None, ws_bytes=0, loss=FAKE, order=FAKE, count=6, keep=1.0):
    ep = cof.ApaEpoch(order, count) if ep == 'default' else ep
    sgd = _Sgd() if opt == 'default' else opt
    cep = _ce() if cep == 'default' else cep
    cache = cof.ApaFeatureCache(None, 30, 1, None) if cache == 'default' else cache      # (index, labels_cached: ignored)
    clip = _clip() if clip == 'default' else clip
    rc = lib.apa_attn_head_train_epoch_cached_clips(
        _ptr(ep), None if sgd is None else _ptr(sgd.c), _ptr(cep), _ptr(cache), _ptr(ml), _ptr(clip), None, FAKE, xatt,
        FAKE, FAKE, FAKE, FAKE, None, 1.0, 1.0, FAKE, FAKE, FAKE, FAKE, loss, FAKE, dX, None if xatt == FAKE else FAKE,
        FAKE, FAKE, FAKE, FAKE, FAKE, ws_bytes, N, P, C, C, K, M, flags, keep, 0, 0, dtype, None)
    return rc, lib.apa_last_error()


def _eval(lib, ep='default', cep='default', cache='default', clip='default', dtype=0, N=9, P=9, C=32, K=8, M=1, flags=0,
          xatt=FAKE, ws_bytes=0, kind=0, order=FAKE, count=7, loss=None, probs=FAKE):
    ep = cof.ApaEpoch(order, count) if ep == 'default' else ep
    cep = _ce(mode=UNIFORM) if cep == 'default' else cep
    cache = cof.ApaFeatureCache(None, 30, 0, None) if cache == 'default' else cache
    clip = _clip() if clip == 'default' else clip
    rc = lib.apa_attn_head_eval_epoch_cached_clips(
        _ptr(ep), _ptr(cep), _ptr(cache), _ptr(clip), kind, FAKE, xatt, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE,
        FAKE, loss, probs, FAKE, FAKE, ws_bytes, N, P, C, C, K, M, flags, dtype, None)
    return rc, lib.apa_last_error()


@pytest.mark.parametrize('dtype', [0, 1, 2], ids=['f32', 'bf16', 'fp8'])
def test_train_epoch_refusals_name_their_reason_before_any_hip_call(dtype):
    lib = ce.load_library()
    fn = b'apa_attn_head_train_epoch_cached_clips'
    mlk = lambda kind=ML: cof.ApaMultilabel(kind, None, 10.0)           # (its labels pointer is not read)
    # everything in order -- every served form: the next refusal is the workspace's, nothing was launched
    for kw in (dict(), dict(ml=mlk()), dict(ml=mlk(ML2)), dict(clip=None, N=2, count=6, ml=mlk()),
               dict(clip=None, N=2, count=6), dict(clip=_clip(frames=1), N=2, ml=mlk()),
               dict(clip=_clip(w=FAKE, b=FAKE, tatt=FAKE, dw=FAKE, db=FAKE)), dict(cep=_ce(mode=UNIFORM)),
               dict(cep=_ce(vtar=None, targets=None)), dict(ml=mlk(), cep=_ce(vlab=None, labels=None))):
        rc, err = _train(lib, dtype=dtype, **kw)
        assert rc == WORKSPACE and b'workspace' in err, (kw, rc, err)      # (the clip step's, or the pooling call's)
    # 1. the epoch's own
    for kw, word in ((dict(opt=None), b'null apa_epoch_sgd'), (dict(opt=_Sgd(lr=False)), b'null apa_epoch_sgd / lr'),
                     (dict(ep=None), b'null apa_epoch'), (dict(order=None), b'null apa_epoch'),
                     (dict(cache=None), b'null apa_feature_cache'), (dict(cep=None), b'null apa_clip_epoch'),
                     (dict(N=0), b'N=0 is not a whole'), (dict(N=7), b'N=7 is not a whole, positive number of clips of 3'),
                     (dict(clip=_clip(frames=0)), b'clips of 0 frames'),
                     (dict(count=1), b'count=1'), (dict(count=0), b'count=0'), (dict(count=-2), b'count=-2'),
                     (dict(count=7), b'count=7 is not a whole, positive number of batches of B=2')):
        rc, err = _train(lib, dtype=dtype, **kw)
        assert rc == INVALID and word in err and fn in err, (kw, rc, err)
    # 2. the optimiser's, in front of the sampler's and the step's
    for opt, word in ((_Sgd(nseg=0), b'nseg=0'), (_Sgd(nseg=17), b'nseg=17'), (_Sgd(null_weight=1), b'weights[1] is NULL')):
        rc, err = _train(lib, dtype=dtype, opt=opt, cep=_ce(index=None), M=8)
        assert rc == INVALID and word in err and b'apa_epoch_sgd' in err and fn in err, (word, rc, err)
    # 3. the sampler's, in front of the step's
    for kw, word in ((dict(cep=_ce(index=None)), b'apa_clip_epoch.index'), (dict(cep=_ce(index=FAKE + 2)), b'4-byte aligned'),
                     (dict(cep=_ce(vlab=None)), b'sampled labels'), (dict(cep=_ce(labels=None)), b'sampled labels'),
                     (dict(ml=mlk(), cep=_ce(vtar=None)), b'sampled targets'),
                     (dict(ml=mlk(), cep=_ce(targets=None)), b'sampled targets'),
                     (dict(cep=_ce(first=None)), b'null video_first'), (dict(cep=_ce(frames=None)), b'null video_first'),
                     (dict(cep=_ce(V=0)), b'non-positive size V=0'), (dict(cep=_ce(mode=5)), b'unknown mode 5'),
                     (dict(ml=mlk(7)), b'unknown loss kind 7')):
        rc, err = _train(lib, dtype=dtype, M=8, **kw)
        assert rc == INVALID and word in err and fn in err, (kw, rc, err)
    # 4. what the step refuses about the cache, the form and itself
    for kw, word in ((dict(cache=cof.ApaFeatureCache(None, 0, 0, None)), b'cache_images=0'),
                     (dict(dX=FAKE), b'dX must be NULL'), (dict(flags=0), b'APA_FLAG_FROZEN_INPUT'),
                     (dict(P=0), b'non-positive'), (dict(dtype=3), b'unknown dtype'),
                     (dict(loss=None), b'null clip / labels / loss'),
                     (dict(clip=_clip(pooled=None)), b'apa_clip_pool needs pooled'),
                     (dict(clip=_clip(w=FAKE, b=FAKE, tatt=FAKE)), b'apa_clip_pool needs pooled')):
        rc, err = _train(lib, **dict(dict(dtype=dtype), **kw))
        assert rc == INVALID and word in err and fn in err, (kw, rc, err)
    # the pooling call's own, in its words (a clip step asks for its workspace first; FAKE stands for one)
    rc, err = _train(lib, dtype=dtype, flags=FROZEN | cof.APA_FLAG_TRAIN, keep=0.0, ws_bytes=1 << 20)
    assert rc == INVALID and b'keep_prob' in err, err
    for kw, word in ((dict(M=8), b'per-class maps'), (dict(xatt=FAKE + 0x1000), b'separate attention input'),
                     (dict(flags=FROZEN | cof.APA_FLAG_SOFTMAX_ATT), b'APA_FLAG_SOFTMAX_ATT'),
                     (dict(flags=FROZEN | cof.APA_FLAG_RELU_INPUT), b'APA_FLAG_RELU_INPUT')):
        rc, err = _train(lib, dtype=dtype, **kw)
        assert rc == UNSUPPORTED and word in err and b'feature cache' in err and fn in err, (kw, rc, err)
    rc, err = _train(lib, dtype=dtype, C=24 if dtype == 2 else 30, ws_bytes=1 << 20)
    assert rc == UNSUPPORTED and (b'multiple of 16' if dtype == 2 else b'16-byte vectors') in err, err


@pytest.mark.parametrize('dtype', [0, 1, 2], ids=['f32', 'bf16', 'fp8'])
def test_eval_epoch_refusals_name_their_reason_before_any_hip_call(dtype):
    lib = ce.load_library()
    fn = b'apa_attn_head_eval_epoch_cached_clips'
    for kw in (dict(), dict(kind=cof.APA_SCORES_SIGMOID), dict(count=1), dict(loss=FAKE),
               dict(clip=None, N=3), dict(clip=_clip(frames=1), N=3), dict(clip=_clip(w=FAKE, b=FAKE, tatt=FAKE)),
               dict(cep=_ce(vlab=None, labels=None, vtar=None, targets=None)), dict(cep=_ce(mode=5))):   # (mode: not read)
        rc, err = _eval(lib, dtype=dtype, **kw)
        assert rc == WORKSPACE and b'workspace' in err, (kw, rc, err)
    for kw, word in ((dict(ep=None), b'null apa_epoch'), (dict(order=None), b'null apa_epoch'),
                     (dict(cache=None), b'null apa_feature_cache'), (dict(cep=None), b'null apa_clip_epoch'),
                     (dict(N=0), b'N=0 is not a whole'), (dict(N=10), b'N=10 is not a whole'),
                     (dict(count=0), b'count=0'), (dict(count=-1), b'count=-1'),
                     (dict(count=2 ** 31 - 1), b'past 2^31 - 1'),      # ceil(count / 3) * 3 = 2^31 + 1
                     (dict(cep=_ce(index=None)), b'apa_clip_epoch.index'),
                     (dict(loss=FAKE, cep=_ce(vlab=None)), b'sampled labels'),
                     (dict(loss=FAKE, cep=_ce(labels=None)), b'sampled labels'),
                     (dict(cep=_ce(first=None)), b'null video_first'), (dict(cep=_ce(V=-1)), b'non-positive size V=-1'),
                     (dict(cache=cof.ApaFeatureCache(None, -3, 0, None)), b'cache_images=-3'),
                     (dict(kind=5), b'scores kind'), (dict(probs=None), b'null logits / probs / pred'),
                     (dict(kind=cof.APA_SCORES_SIGMOID, loss=FAKE), b'sigmoid scores take no labels'),
                     (dict(clip=_clip(pooled=None)), b'apa_clip_pool needs pooled'),
                     (dict(clip=_clip(w=FAKE)), b'apa_clip_pool needs pooled'), (dict(K=0), b'non-positive')):
        rc, err = _eval(lib, dtype=dtype, **kw)
        assert rc == INVALID and word in err and fn in err, (kw, rc, err)
    for kw, word in ((dict(M=8), b'per-class maps'), (dict(xatt=FAKE + 0x1000), b'separate attention input'),
                     (dict(flags=cof.APA_FLAG_SOFTMAX_ATT), b'APA_FLAG_SOFTMAX_ATT')):
        rc, err = _eval(lib, dtype=dtype, **kw)
        assert rc == UNSUPPORTED and word in err and b'feature cache' in err and fn in err, (kw, rc, err)


def test_bound_epochs_refuse_on_the_host():
    V, K = 4, 5
    cache = cof.FeatureCache(torch.zeros(9, 3, 3, 32))
    w = [torch.zeros(32, 1), torch.zeros(1), torch.zeros(32, K), torch.zeros(K)]
    flat = torch.zeros(sum(t.numel() for t in w))
    args = (w[0], w[1], w[2], w[3], tuple(torch.zeros_like(t) for t in w), w, [0.0] * 4, flat, flat.clone())
    with pytest.raises(cof.ApaError, match='set_videos first'):
        ce.ClipTrainEpoch(cache, 2, 3, *args, steps=2)
    cache.set_videos([0, 1, 3, 6], [1, 2, 3, 3], labels=torch.zeros(V, dtype=torch.int64), targets=torch.zeros(V, K))
    with pytest.raises(cof.ApaError, match='GPU memory'):
        ce.ClipTrainEpoch(cache, 2, 3, *args, steps=2)
    with pytest.raises(cof.ApaError, match='GPU memory'):
        ce.ClipEvalEpoch(cache, 2, 3, *w, capacity=4)
    with pytest.raises(cof.ApaError, match='action_loss must be one of'):
        ce.ClipTrainEpoch(cache, 2, 3, *args, steps=2, action_loss='l2')
    with pytest.raises(cof.ApaError, match='scores must be'):
        ce.ClipEvalEpoch(cache, 2, 3, *w, capacity=4, scores='tanh')


# ------------------------------------------------------------------------------------------ deploy
def _head(name, device='cpu', **train):
    from tests import _ref_fixture as rf
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_%s.npz' % name))
    fx.meta = dict(fx.meta, train_cfg=dict(fx.meta['train_cfg'], **train))
    return rf.build_head(fx, device=device)


def _video_cache(C, K, labels=True, targets=True):
    cache = cof.FeatureCache(torch.zeros(12, 3, 3, C))
    cache.set_videos([0, 3, 6, 9], [3, 3, 3, 3], labels=torch.zeros(4, dtype=torch.int64) if labels else None,
                     targets=torch.zeros(4, K) if targets else None)
    return cache


def test_deploy_train_video_epoch_refusals_name_their_reason():
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from tests import _ref_fixture as rf
    order = torch.arange(4, dtype=torch.int32)
    try:
        name = 'vstep_temporal_att_train'
        network_fn, cfg = _head(name)
        K = int(network_fn.head.num_classes)
        cache = _video_cache(32, K)
        fused = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
        with pytest.raises(ValueError, match='make_optimizer\\(\\) first'):
            fused.train_video_epoch(cache, 2, 3, order)
        assert fused.video_epoch_unsupported_reason(cache) == ''
        fused.make_optimizer(0.01)
        with pytest.raises(ValueError, match='FeatureCache without videos'):
            fused.train_video_epoch(cof.FeatureCache(torch.zeros(12, 3, 3, 32)), 2, 3, order)
        with pytest.raises(ValueError, match='FeatureCache without video labels'):
            fused.train_video_epoch(_video_cache(32, K, labels=False), 2, 3, order)
        with pytest.raises(ValueError, match='not a whole number of batches of 3'):
            fused.train_video_epoch(cache, 3, 3, order)
        with pytest.raises(ValueError, match='one learning rate per step'):
            fused.train_video_epoch(cache, 2, 3, order, lr=[0.1])
        step0 = network_fn.head._step
        with pytest.raises(cof.ApaError, match='GPU memory'):          # no CPU fallback
            fused.train_video_epoch(cache, 2, 3, order)
        assert network_fn.head._step == step0
        fused.loss_scale = 0.5
        with pytest.raises(ValueError, match='more than one clone'):
            fused.train_video_epoch(cache, 2, 3, order)
        with pytest.raises(ValueError, match='frozen_features=False'):
            f = deploy.FusedHeadStep(network_fn, cfg, frozen_features=False)
            f.make_optimizer(0.01)
            f.train_video_epoch(cache, 2, 3, order)
        for train, word in ((dict(OPTIMIZER='adam'), "TRAIN.OPTIMIZER 'adam'"), (dict(ITER_SIZE=2), 'TRAIN.ITER_SIZE 2'),
                            (dict(CLIP_GRADIENTS=1.0), 'TRAIN.CLIP_GRADIENTS > 0')):
            net, c = _head(name, **train)
            f = deploy.FusedHeadStep(net, c, frozen_features=True)
            f.make_optimizer(0.01)
            with pytest.raises(ValueError, match='train_video_epoch: a clip epoch call is not served with '
                               + re.escape(word)):
                f.train_video_epoch(cache, 2, 3, order)
        # a sigmoid loss is served, and needs the targets
        netm, cfgm = _head('mlstep_clip_temporal_ml')
        fm = deploy.FusedHeadStep(netm, cfgm, frozen_features=True)
        fm.make_optimizer(0.01)
        Km = int(netm.head.num_classes)
        assert fm.video_epoch_unsupported_reason(_video_cache(32, Km, labels=False)) == ''
        with pytest.raises(ValueError, match='FeatureCache without video targets'):
            fm.train_video_epoch(_video_cache(32, Km, targets=False), 2, 3, order)
        # per-class maps and the cfg 003 form
        netp, cfgp = _head('vstep_perclass_temporal_train')
        fp = deploy.FusedHeadStep(netp, cfgp, frozen_features=True)
        fp.make_optimizer(0.01)
        with pytest.raises(ValueError, match='not served with per-class attention maps'):
            fp.train_video_epoch(_video_cache(int(netp.head.in_channels), int(netp.head.num_classes)), 2, 3, order)
        fx3 = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_train.npz'))
        net3, cfg3 = rf.build_head(fx3, device='cpu', in_channels=2048)
        f3 = deploy.FusedHeadStep(net3, cfg3, frozen_features=True)
        f3.make_optimizer(0.01)
        with pytest.raises(ValueError, match='not served with attention from pose_pre_logits'):
            f3.train_video_epoch(cache, 2, 3, order)
    finally:
        apa_config.reset_cfg()


def test_deploy_evaluate_videos_refusals_name_their_reason():
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from tests import _ref_fixture as rf
    try:
        net, cfg = _head('vstep_temporal_att_train')
        net.head.is_training = False
        K = int(net.head.num_classes)
        cache = _video_cache(32, K)
        ev = deploy.FusedHeadEval(net, cfg)
        with pytest.raises(ValueError, match='FeatureCache without videos'):
            ev.evaluate_videos(cof.FeatureCache(torch.zeros(12, 3, 3, 32)), 2, 3)
        with pytest.raises(ValueError, match='FeatureCache without video labels'):
            ev.evaluate_videos(_video_cache(32, K, labels=False), 2, 3)
        with pytest.raises(ValueError, match='batch_videos >= 1'):
            ev.evaluate_videos(cache, 0, 3)
        with pytest.raises(cof.ApaError, match='int32 vector'):
            ev.evaluate_videos(cache, 2, 3, order=torch.arange(4))
        meter = ev.new_evaluation(4)
        with pytest.raises(cof.ApaError, match='GPU memory'):          # no CPU fallback; the meter was not advanced
            ev.evaluate_videos(cache, 2, 3, meter=meter)
        assert len(meter) == 0
        ev.multi_label = True
        with pytest.raises(ValueError, match='FeatureCache without video targets'):
            ev.evaluate_videos(_video_cache(32, K, targets=False), 2, 3)
        fx3 = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_eval.npz'))
        net3, cfg3 = rf.build_head(fx3, device='cpu', in_channels=2048)
        with pytest.raises(ValueError, match='not served with attention from pose_pre_logits'):
            deploy.FusedHeadEval(net3, cfg3).evaluate_videos(cache, 2, 3)
    finally:
        apa_config.reset_cfg()
