"""Clips and the multi-label losses from a resident frame cache, without a GPU: the header, the ctypes table and the
library agree on the three new names; every refusal of the new entry points is made, by name, before any HIP call; the
numpy restatement of the frame rule against the literal rule; FeatureCache.set_videos / sample_clips / video_epoch host
validation; the refusals HeadTrainStep and the deploy layer keep."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _clip_sampler_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
NEW = ('apa_attn_head_train_step_cached_clips', 'apa_attn_head_eval_step_cached_clips', 'apa_sample_clip_frames')
FAKE = 0x10000                       # a 16-byte aligned non-null address: nothing is dereferenced
FROZEN = cof.APA_FLAG_FROZEN_INPUT


# ------------------------------------------------------------------------------------------ ABI
def test_header_table_and_library_agree_on_the_new_names():
    header = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(apa_[a-z0-9_]+)\s*\(', bare))
    lib = cof.load_library()
    for name in NEW:
        assert name in declared and name in cof.exported_symbols() and hasattr(lib, name), name
    defs = dict(re.findall(r'#define\s+(APA_[A-Z0-9_]+)\s+(\d+)', header))
    assert int(defs['APA_VERSION']) >= 313 and lib.apa_version() >= 313
    assert int(defs['APA_CLIP_FRAMES_UNIFORM']) == cof.APA_CLIP_FRAMES_UNIFORM == ref.UNIFORM == 0
    assert int(defs['APA_CLIP_FRAMES_RANDOM_SEGMENT']) == cof.APA_CLIP_FRAMES_RANDOM_SEGMENT == ref.RANDOM_SEGMENT == 1
    sig, vp = cof._SIGNATURES, ctypes.c_void_p
    # (cache, ml, clip) in front of the cached step's (hooks, ...); (cache) in front of the clip evaluation step's
    t, c = sig['apa_attn_head_train_step_cached_clips'], sig['apa_attn_head_train_step_cached']
    assert t == (c[0], [vp, vp, vp] + list(c[1][1:]))
    assert sig['apa_attn_head_eval_step_cached_clips'] == sig['apa_attn_head_eval_step_cached']
    # every parameter the header declares has a slot in the table
    for name in NEW:
        m = re.search(r'\b%s\s*\((.*?)\)\s*;' % name, bare, flags=re.S)
        assert len(m.group(1).split(',')) == len(sig[name][1]), name


# ------------------------------------------------------------------------------------------ refusals
def _desc(index=FAKE, T=7, labels_cached=0, status=None):
    return cof.ApaFeatureCache(index, T, labels_cached, status)


def _clip(frames=2, w=None, b=None, pooled=FAKE, tatt=None, dw=None, db=None):
    c = cof.ApaClipPool()
    c.frames, c.w, c.b, c.pooled, c.tatt, c.dw, c.db = frames, w, b, pooled, tatt, dw, db
    return c


def _ml(kind=None, labels=FAKE):
    m = cof.ApaMultilabel()
    m.kind = cof.ACTION_LOSS_KINDS['multi-label'] if kind is None else kind
    m.labels, m.pos_weight = labels, 10.0
    return m


def _ptr(s):
    return None if s is None else ctypes.addressof(s)


def _train(lib, cache, ml=None, clip=None, dtype=0, N=4, P=9, C=32, K=8, M=1, flags=FROZEN, xatt=FAKE, dX=None,
           ws_bytes=0, labels=FAKE):
    rc = lib.apa_attn_head_train_step_cached_clips(
        _ptr(cache), _ptr(ml), _ptr(clip), None, FAKE, xatt, FAKE, FAKE, FAKE, FAKE, labels, 1.0, 1.0, FAKE, FAKE, FAKE,
        FAKE, FAKE, FAKE, dX, None if xatt == FAKE else FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ws_bytes, N, P, C, C, K, M,
        flags, 1.0, 0, 0, dtype, None)
    return rc, lib.apa_last_error().decode()


def _plain_cached(lib, cache, dtype=0, N=4, P=9, C=32, K=8, M=1, flags=FROZEN, xatt=FAKE, dX=None, ws_bytes=0,
                  labels=FAKE):
    rc = lib.apa_attn_head_train_step_cached(
        _ptr(cache), None, FAKE, xatt, FAKE, FAKE, FAKE, FAKE, labels, 1.0, 1.0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, dX,
        None if xatt == FAKE else FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ws_bytes, N, P, C, C, K, M, flags, 1.0, 0, 0,
        dtype, None)
    return rc, lib.apa_last_error().decode()


def _eval(lib, cache, clip, kind=0, dtype=0, N=4, P=9, C=32, K=8, M=1, flags=0, xatt=FAKE, ws_bytes=0, labels=None,
          loss=None, fn='apa_attn_head_eval_step_cached_clips'):
    rc = getattr(lib, fn)(_ptr(cache), _ptr(clip), kind, FAKE, xatt, FAKE, FAKE, FAKE, FAKE, labels, FAKE, FAKE, FAKE,
                          FAKE, loss, FAKE, FAKE, FAKE, ws_bytes, N, P, C, C, K, M, flags, dtype, None)
    return rc, lib.apa_last_error().decode()


@pytest.mark.parametrize('dtype', [0, 1, 2], ids=['f32', 'bf16', 'fp8'])
def test_cached_clip_refusals_name_their_reason_before_any_hip_call(dtype):
    """(dummy pointers: a call that got past its checks would fault -- an accepted call stops at the workspace check,
    still in front of the first launch)"""
    lib = cof.load_library()
    ok, other = _desc(), FAKE + 0x1000
    TRAIN = 'apa_attn_head_train_step_cached_clips'
    forms = ((None, _clip()), (_ml(), None), (_ml(), _clip()),
             (None, _clip(w=FAKE, b=FAKE, tatt=FAKE, dw=FAKE, db=FAKE)))
    for ml, clip in forms:
        # everything in order: the workspace is asked for next, with the clip step's size on clips
        rc, err = _train(lib, ok, ml, clip, dtype)
        assert rc == WORKSPACE and 'workspace' in err, err
        if clip is not None:
            need = lib.apa_clip_step_workspace_bytes(4, 2, 9, 32, 32, 8, 1, FROZEN)
            assert TRAIN in err and 'apa_clip_step_workspace_bytes' in err and '< %d' % need in err, err
            assert need > lib.apa_attn_pool_workspace_bytes(4, 9, 32, 32, 8, 1, FROZEN)
        else:
            assert '< %d)' % lib.apa_attn_pool_workspace_bytes(4, 9, 32, 32, 8, 1, FROZEN) in err, err
        # the descriptor and the forms a cache cannot have: the cached step's sentences under the new name
        for cache, word in ((None, 'null apa_feature_cache'), (_desc(index=None), 'null apa_feature_cache'),
                            (_desc(T=0), 'cache_images=0'), (_desc(index=FAKE + 2), '4-byte aligned')):
            rc, err = _train(lib, cache, ml, clip, dtype)
            assert rc == INVALID and word in err and TRAIN in err, (word, rc, err)
        for kw, word in ((dict(M=8), 'per-class maps'), (dict(xatt=other), 'separate attention input'),
                         (dict(flags=cof.APA_FLAG_SOFTMAX_ATT | FROZEN), 'APA_FLAG_SOFTMAX_ATT'),
                         (dict(flags=cof.APA_FLAG_RELU_INPUT | FROZEN), 'APA_FLAG_RELU_INPUT')):
            rc, err = _train(lib, ok, ml, clip, dtype, **kw)
            assert rc == UNSUPPORTED and word in err and 'a feature cache does not serve' in err, (kw, rc, err)
        rc, err = _train(lib, ok, ml, clip, dtype, dX=FAKE)
        assert rc == INVALID and 'dX must be NULL' in err
        rc, err = _train(lib, ok, ml, clip, dtype, flags=0)
        assert rc == INVALID and 'APA_FLAG_FROZEN_INPUT' in err
        # labels are per clip / per row: never through the frame index -- after the descriptor, before the clip
        rc, err = _train(lib, _desc(labels_cached=1), ml, clip, dtype)
        assert rc == INVALID and 'labels_cached' in err and 'sampler' in err, err
        rc, err = _train(lib, _desc(labels_cached=1, T=0), ml, clip, dtype)
        assert rc == INVALID and 'cache_images=0' in err, err
        rc, err = _train(lib, _desc(labels_cached=1), ml, clip, dtype, N=5)
        assert rc == INVALID and 'labels_cached' in err, err
    # the clip's and the loss's own refusals: the plain entry points' sentences
    rc, err = _train(lib, ok, None, _clip(frames=3), dtype)
    assert rc == INVALID and 'N=4 is not a whole number of clips of 3 frames' in err, err
    rc, err = _train(lib, ok, _ml(), _clip(frames=0), dtype)
    assert rc == INVALID and 'not a whole number of clips' in err, err
    rc, err = _train(lib, ok, None, _clip(pooled=None), dtype)
    assert rc == INVALID and 'apa_clip_pool needs pooled' in err, err
    rc, err = _train(lib, ok, None, _clip(w=FAKE), dtype)
    assert rc == INVALID and 'with w also b, tatt, dw and db' in err, err
    rc, err = _train(lib, ok, None, _clip(), dtype, labels=None)
    assert rc == INVALID and 'null clip / labels' in err, err
    rc, err = _train(lib, ok, _ml(), _clip(), dtype, labels=None)        # a sigmoid loss does not read `labels`
    assert rc == WORKSPACE, err
    rc, err = _train(lib, ok, _ml(kind=77), None, dtype)
    assert rc == INVALID and 'unknown loss kind 77' in err, err
    rc, err = _train(lib, ok, _ml(labels=None), _clip(), dtype)
    assert rc == INVALID and 'null apa_multilabel / labels' in err, err
    rc, err = _train(lib, ok, None, _clip(), dtype, N=0)
    assert rc == INVALID and 'non-positive' in err, err
    if dtype == 2:          # FP8 keeps its own limits (on clips behind the clip step's workspace check, as ever)
        rc, err = _train(lib, ok, None, _clip(), dtype, C=24, ws_bytes=1 << 20)
        assert rc == UNSUPPORTED and 'multiple of 16' in err and 'APA_DTYPE_FP8_E4M3' in err, err

    # ---- the evaluation step
    EV = 'apa_attn_head_eval_step_cached_clips'
    for clip in (_clip(), _clip(w=FAKE, b=FAKE, tatt=FAKE)):
        for kind in (cof.APA_SCORES_SOFTMAX, cof.APA_SCORES_SIGMOID):
            rc, err = _eval(lib, ok, clip, kind, dtype)
            assert rc == WORKSPACE and 'workspace' in err, err
        rc, err = _eval(lib, None, clip, 0, dtype)
        assert rc == INVALID and 'null apa_feature_cache' in err and EV in err, err
        rc, err = _eval(lib, ok, clip, 0, dtype, M=8)
        assert rc == UNSUPPORTED and 'per-class maps' in err and EV in err, err
        rc, err = _eval(lib, ok, clip, 5, dtype)
        assert rc == INVALID and 'unknown scores kind 5' in err, err
        rc, err = _eval(lib, ok, clip, 0, dtype, N=5)
        assert rc == INVALID and 'N=5 is not a whole number of clips of 2 frames' in err, err
        rc, err = _eval(lib, ok, clip, 0, dtype, labels=FAKE)
        assert rc == INVALID and 'labels and loss must be given together' in err, err
        rc, err = _eval(lib, ok, clip, cof.APA_SCORES_SIGMOID, dtype, labels=FAKE, loss=FAKE)
        assert rc == INVALID and 'sigmoid scores take no labels' in err, err
        rc, err = _eval(lib, _desc(labels_cached=1), clip, 0, dtype)
        assert rc == INVALID and 'labels_cached' in err, err
    rc, err = _eval(lib, ok, _clip(pooled=None), 0, dtype)
    assert rc == INVALID and 'apa_clip_pool needs pooled' in err, err
    rc, err = _eval(lib, ok, _clip(w=FAKE), 0, dtype)
    assert rc == INVALID and 'with w also b and tatt' in err, err
    # the old entry point refuses a clip as it always did
    rc, err = _eval(lib, ok, _clip(), 0, dtype, fn='apa_attn_head_eval_step_cached')
    assert rc == UNSUPPORTED and 'a feature cache does not serve clips' in err, err


@pytest.mark.parametrize('dtype', [0, 2], ids=['f32', 'fp8'])
def test_without_ml_and_clip_the_new_entry_answers_what_the_cached_step_answers(dtype):
    """ml == clip == NULL: status and message of apa_attn_head_train_step_cached, byte for byte, defect by defect"""
    lib = cof.load_library()
    other = FAKE + 0x1000
    cases = [(_desc(), {}), (None, {}), (_desc(index=None), {}), (_desc(T=0), {}), (_desc(index=FAKE + 2), {}),
             (_desc(), dict(M=8)), (_desc(), dict(xatt=other)), (_desc(), dict(dX=FAKE)), (_desc(), dict(flags=0)),
             (_desc(), dict(flags=cof.APA_FLAG_SOFTMAX_ATT | cof.APA_FLAG_RELU_INPUT | FROZEN)),
             (_desc(), dict(N=0)), (_desc(), dict(C=24)), (_desc(), dict(labels=None)),
             (_desc(labels_cached=1, status=FAKE), {}), (_desc(), dict(dX=FAKE, flags=cof.APA_FLAG_SOFTMAX_ATT | FROZEN)),
             (_desc(), dict(ws_bytes=64))]
    for cache, kw in cases:
        got = _train(lib, cache, None, None, dtype, **kw)
        want = _plain_cached(lib, cache, dtype, **kw)
        assert got == want and got[0] != 0 and '_cached_clips' not in got[1], (kw, got, want)
    # and the evaluation entry without a clip is the cached evaluation step
    for kw in ({}, dict(M=8), dict(kind=5), dict(kind=cof.APA_SCORES_SIGMOID), dict(labels=FAKE)):
        got = _eval(lib, _desc(), None, dtype=dtype, **kw)
        want = _eval(lib, _desc(), None, dtype=dtype, fn='apa_attn_head_eval_step_cached', **kw)
        assert got == want and got[0] != 0 and '_cached_clips' not in got[1], (kw, got, want)


def test_sampler_refusals():
    lib = cof.load_library()

    def call(first=FAKE, count=FAKE, vlab=None, vtar=None, videos=FAKE, u=None, index=FAKE, labels=None, targets=None,
             status=None, V=3, B=2, F=4, K=0, mode=0):
        rc = lib.apa_sample_clip_frames(first, count, vlab, vtar, videos, u, index, labels, targets, status, V, B, F, K,
                                        mode, None)
        return rc, lib.apa_last_error().decode()

    for kw in (dict(first=None), dict(count=None), dict(videos=None), dict(index=None)):
        rc, err = call(**kw)
        assert rc == INVALID and 'null video_first / video_frames / videos / index' in err, (kw, err)
    rc, err = call(vlab=FAKE)
    assert rc == INVALID and 'video_labels needs labels' in err
    rc, err = call(vtar=FAKE, K=5)
    assert rc == INVALID and 'video_targets needs targets' in err
    for kw in (dict(V=0), dict(B=0), dict(F=0), dict(B=-1), dict(vtar=FAKE, targets=FAKE, K=0)):
        rc, err = call(**kw)
        assert rc == INVALID and 'non-positive size' in err, (kw, err)
    rc, err = call(mode=2)
    assert rc == INVALID and 'unknown mode 2' in err
    rc, err = call(mode=cof.APA_CLIP_FRAMES_RANDOM_SEGMENT)
    assert rc == INVALID and 'needs the uniform draws' in err
    rc, err = call(B=1 << 20, F=1 << 11)
    assert rc == INVALID and 'past 2^31' in err
    rc, err = call(B=65536, F=32768, mode=1, u=FAKE)
    assert rc == INVALID and 'past 2^31' in err


# ------------------------------------------------------------------------------------------ the frame rule
NS, FS = (1, 2, 3, 7, 25, 40, 400), (1, 3, 25)


def _literal_uniform(n, F):
    """_get_frame_sublist's uniform arm in Python integers: num_consec_frames = 1, start_frame = 0, floor division"""
    step = max((n - 1) // F, 1)
    return [min(0 + step * i, n - 1) for i in range(F)]


@pytest.mark.parametrize('F', FS)
@pytest.mark.parametrize('n', NS)
def test_uniform_arm_is_the_literal_rule(n, F):
    got = ref.frames_uniform(n, F)
    assert got.dtype == np.int32 and got.tolist() == _literal_uniform(n, F)
    assert got.min() >= 0 and got.max() <= n - 1
    assert np.all(np.diff(got) >= 0)                           # frames never run backwards
    if n - 1 >= F:                                              # a video long enough: F distinct, evenly spaced frames
        assert len(set(got.tolist())) == F and set(np.diff(got).tolist()) <= {(n - 1) // F}


@pytest.mark.parametrize('F', FS)
@pytest.mark.parametrize('n', NS)
def test_random_draws_fall_in_their_segment(n, F):
    lo, hi = ref.segments(n, F)
    for u in (np.float32(0.0), np.nextafter(np.float32(1.0), np.float32(0.0)), np.float32(0.5)):
        got = ref.frames_random(n, F, np.full(F, u, dtype=np.float32))
        assert got.dtype == np.int32 and got.min() >= 0 and got.max() <= n - 1, (n, F, u, got)
        for i in range(F):
            if hi[i] > lo[i] and lo[i] >= 0:        # the reference's interval [lo, hi)
                assert lo[i] <= got[i] < hi[i], (n, F, u, i, got[i], lo[i], hi[i])
            else:                                   # n = 1: the reference's [-1, 0) -- the only frame there is
                assert got[i] == min(max(lo[i], 0), n - 1)
        if u == 0.0:
            assert got.tolist() == np.clip(lo, 0, n - 1).tolist()
        if u > 0.9:                                 # the last frame of each segment, never the next segment's first
            assert got.tolist() == np.clip(np.where(hi > lo, hi - 1, lo), 0, n - 1).tolist()


def test_sample_restatement_clamps_and_copies():
    first = np.array([0, 1, 3], dtype=np.int32)
    count = np.array([1, 2, 7], dtype=np.int32)
    lab = np.array([4, 5, 6], dtype=np.int64)
    tar = np.arange(15, dtype=np.float32).reshape(3, 5)
    idx, labels, targets, bad = ref.sample(first, count, [2, 2, 9, -1], 3, ref.UNIFORM, None, lab, tar)
    assert idx.tolist() == [3, 5, 7, 3, 5, 7, 3, 5, 7, 0, 0, 0] and bad == 2
    assert labels.tolist() == [6, 6, 6, 4] and np.array_equal(targets, tar[[2, 2, 2, 0]])


# ------------------------------------------------------------------------------------------ FeatureCache on the CPU
def _cache(T=12):
    return cof.FeatureCache(torch.zeros(T, 2, 3, 16))


def test_set_videos_sample_clips_video_epoch_host_validation():
    cache = _cache()
    with pytest.raises(cof.ApaError, match='set_videos first'):
        cache.sample_clips([0], 2)
    with pytest.raises(cof.ApaError, match='set_videos first'):
        list(cache.video_epoch(2, seed=1))
    for first, count in (([0, 5], [5, 0]), ([0, 5], [5, 8]), ([-1, 5], [5, 7]), ([0], [1, 2]), ([], []),
                         ([0.0, 5.0], [5, 7])):
        with pytest.raises(cof.ApaError):
            cache.set_videos(first, count)
    with pytest.raises(cof.ApaError, match='labels int64'):
        cache.set_videos([0, 5], [5, 7], labels=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(cof.ApaError, match='labels int64'):
        cache.set_videos([0, 5], [5, 7], labels=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(cof.ApaError, match='targets float32'):
        cache.set_videos([0, 5], [5, 7], targets=torch.zeros(3, 4))
    with pytest.raises(cof.ApaError, match='targets float32'):
        cache.set_videos([0, 5], [5, 7], targets=torch.zeros(2, 4, dtype=torch.float64))
    assert cache.video_first is None                            # nothing half-set by a refused call
    cache.set_videos([0, 5], torch.tensor([5, 7]), labels=torch.tensor([3, 1]), targets=torch.zeros(2, 4))
    assert cache.V == 2 and cache.video_first.dtype == torch.int32 and cache.video_frames.tolist() == [5, 7]
    with pytest.raises(cof.ApaError, match='mode'):
        cache.sample_clips([0, 1], 2, mode='caffe')
    with pytest.raises(cof.ApaError, match='frames >= 1'):
        cache.sample_clips([0, 1], 0)
    with pytest.raises(cof.ApaError, match='1-D integer index'):
        cache.sample_clips([], 2)
    with pytest.raises(cof.ApaError, match='u float32'):
        cache.sample_clips([0, 1], 2, mode='random-segment', u=torch.zeros(3))
    with pytest.raises(cof.ApaError, match='out must be a CachedClips'):
        cache.sample_clips([0, 1], 2, out=cof.CachedClips(cache, 2, 3))
    with pytest.raises(cof.ApaError, match='out must be a CachedClips'):
        cache.sample_clips([0, 1], 2, out=cache.select([0, 1, 2, 3]))
    with pytest.raises(cof.ApaError, match='GPU memory'):      # no CPU fallback
        cache.sample_clips([0, 1], 2)
    clips = cof.CachedClips(cache, 3, 4)
    assert isinstance(clips, cof.CachedBatch) and clips.shape == (12, 2, 3, 16) and clips.frames == 4
    assert clips.index.dtype == torch.int32 and clips.index.numel() == 12
    assert clips.labels.dtype == torch.int64 and tuple(clips.labels.shape) == (3,)
    assert clips.targets.dtype == torch.float32 and tuple(clips.targets.shape) == (3, 4)
    # video_epoch: epoch's contract over the V videos
    cache.set_videos(list(range(0, 12, 2)) , [2] * 6)
    for drop_last in (True, False):
        batches = list(cache.video_epoch(4, seed=5, drop_last=drop_last))
        again = list(cache.video_epoch(4, seed=5, drop_last=drop_last))
        assert all(b.dtype == torch.int32 for b in batches)
        assert [b.numel() for b in batches] == ([4] if drop_last else [4, 2])
        assert all(torch.equal(a, b) for a, b in zip(batches, again))
        ids = torch.cat(batches).tolist()
        assert len(set(ids)) == len(ids) and set(ids) <= set(range(6))
    assert torch.cat(list(cache.video_epoch(4, seed=0, shuffle=False, drop_last=False))).tolist() == list(range(6))
    with pytest.raises(cof.ApaError):
        list(cache.video_epoch(0, seed=1))
    assert cof.CachedClips(cache, 2, 2).labels is None and cof.CachedClips(cache, 2, 2).targets is None


def test_head_train_step_refusals_that_remain():
    cache = _cache()
    cache.set_videos([0, 5], [5, 7], labels=torch.tensor([3, 1]), targets=torch.zeros(2, 4))
    clips = cof.CachedClips(cache, 2, 2)
    Wa, ba, Wt, bt = torch.zeros(16, 1), torch.zeros(1), torch.zeros(16, 4), torch.zeros(4)
    g = (None, None, torch.zeros(16, 1), torch.zeros(1), torch.zeros(16, 4), torch.zeros(4))
    with pytest.raises(cof.ApaError, match='need labels'):
        cof.HeadTrainStep(clips, clips, Wa, ba, Wt, bt, None, g, frames=2)
    with pytest.raises(cof.ApaError, match='need labels'):
        cof.HeadTrainStep(clips, clips, Wa, ba, Wt, bt, None, g, action_loss='multi-label')
    with pytest.raises(cof.ApaError, match='class-agnostic'):
        cof.HeadTrainStep(clips, clips, Wa, ba, Wt, bt, clips.labels, g, frames=2, weight_images=True)
    with pytest.raises(cof.ApaError, match='class-agnostic'):           # per-class maps
        cof.HeadTrainStep(clips, clips, torch.zeros(16, 4), torch.zeros(4), Wt, bt, clips.labels, g, frames=2)
    with pytest.raises(cof.ApaError, match='frozen'):                    # a cache has no gradient
        cof.HeadTrainStep(clips, clips, Wa, ba, Wt, bt, clips.labels, (torch.zeros(4, 6, 16),) + g[1:], frames=2)
    with pytest.raises(cof.ApaError, match='same object'):
        cof.HeadTrainStep(clips, cache.select([0, 1, 2, 3]), Wa, ba, Wt, bt, clips.labels, g, frames=2)
    with pytest.raises(cof.ApaError, match='GPU memory'):                # well-formed: only the device is missing
        cof.HeadTrainStep(clips, clips, Wa, ba, Wt, bt, clips.labels, g, frames=2)
    with pytest.raises(cof.ApaError, match='no per-class maps'):
        cof.HeadEvalStep(clips, clips, torch.zeros(16, 4), torch.zeros(4), Wt, bt, frames=2)


def test_deploy_refusals_that_remain():
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from tests import _ref_fixture as rf
    try:
        fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_train_c2048_libmask.npz'))
        network_fn, cfg = rf.build_head(fx, device='cpu')
        cache = cof.FeatureCache(torch.zeros(8, 3, 3, 2048))
        cache.set_videos([0, 4], [4, 4])                                 # no labels, no targets
        clips = cof.CachedClips(cache, 2, 2)
        with pytest.raises(ValueError, match='frozen_features=False'):
            deploy.FusedHeadStep(network_fn, cfg, frozen_features=False)(clips, None)
        with pytest.raises(ValueError, match='needs a CachedClips with labels'):
            deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)(clips, None)
        cfg.TRAIN.LOSS_FN_ACTION = 'multi-label'
        with pytest.raises(ValueError, match='needs a CachedClips with targets'):
            deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)(clips, None)
        with pytest.raises(ValueError, match=r'needs labels_action \[N,K\]'):
            deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)(cache.select([0, 1]), None)
        fx3 = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_train.npz'))
        net3, cfg3 = rf.build_head(fx3, device='cpu', in_channels=2048)
        with pytest.raises(ValueError, match='a CachedBatch is not served with attention from pose_pre_logits'):
            deploy.FusedHeadStep(net3, cfg3, frozen_features=True)(clips, None, None, None)
        fxe = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_eval.npz'))
        net3e, cfg3e = rf.build_head(fxe, device='cpu', in_channels=2048)
        with pytest.raises(ValueError, match='a CachedBatch is not served with attention from pose_pre_logits'):
            deploy.FusedHeadEval(net3e, cfg3e)(clips)
    finally:
        apa_config.reset_cfg()
