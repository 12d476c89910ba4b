"""Every path of the M == 1 attentional pooling (csrc/apa_m1*.hip) against a float64 reference, stage by stage.

Each case runs the product's entry points through the test-only probe library (tests/_m1_probe.py), asserts the
traced dispatch (kernel family and instance, plan, finalize width, logits / backward-head / GEMV / reduce form,
keep bits, RNG bump, concat kernels) and then compares, elementwise under the bound documented in
tests/_m1_probe.py:
  * the forward (att, zsave, abar, logits, zext) with a float64 forward from X, Wa, ba, Wt, bt and the library's
    own dropout mask (apa_dropout_mask, or the caller's packed mask under APA_FLAG_RNG_EXTERNAL);
  * the backward (dX, dXatt, dWa, dba, dWt, dbt, dXext) with a float64 backward from the kernel's OWN att, zsave,
    abar, zext and G, so that no forward error is carried into it;
  * the one-call steps' loss, G, probs and pred with float64 from the kernel's own logits, and every output of the
    one-call train / eval step with the separate entry points bit for bit (apa_capi.hip: same kernels, same
    reduction trees).
Every output and the workspace sit inside NaN-guarded allocations: valid outputs must be finite and no guard may
move.  Every case runs twice and must repeat bit for bit.
"""
import ctypes

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests._m1_probe import Bnd, contract

pytestmark = pytest.mark.gpu

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
KEEP = 0.5


def case(name, N, P, C, K, *, dt=F32, act='id', train=False, Ca=None, rank1=False, relu_in=False, rng='hash',
         entry='sep', J=0, mis=(), keep=KEEP, **expect):
    return dict(name=name, N=N, P=P, C=C, K=K, dt=dt, act=act, train=train, Ca=Ca, rank1=rank1, relu_in=relu_in,
                rng=rng, entry=entry, J=J, mis=tuple(mis), keep=keep, expect=expect)


# Expected traces are read off the dispatch conditions (apa_m1.hip m1_call_fill / m1_forward / m1_backward, the
# launchers of apa_m1_stream.hip / apa_m1_vec.hip / apa_m1_generic.hip, apa_m1_small.hip); S / ppb / nblk are checked against m1_plan for every case.
CASES = [
    # ---- streaming kernels: fp32 C 1024 / 2048 / 4096 (VW 1 / 2 / 4, PIX 1 / 1 / 2), bf16 C 2048 (VW 1, PIX 2)
    # S = 1: 196 one-pixel chunks per block; logits2 with 4 sub-chunks (N >= 128); head tiles UG 1
    case('stream_f32_c1024_S1_softmax_train', 342, 196, 1024, 51, act='softmax', train=True,
         pool_fwd='stream', fwd_w=1, fwd_pix=1, pool_bwd='stream', bwd_w=1, bwd_pix=1, S=1, ppb=196, cw=256,
         logits='logits2', logits_nsub=4, head='tiles', head_ug=1, reduce='colsum', keep_bits=0),
    # S = 3, P = 196 (not a multiple of S): blocks of 65 / 65 / 66 pixels -- an odd chunk count under the
    # two-slot register ring; head tiles UG 2
    case('stream_f32_c2048_S3_relu_eval', 170, 196, 2048, 100, act='relu',
         pool_fwd='stream', fwd_w=2, fwd_pix=1, S=3, ppb=66, cw=256, logits='logits2', logits_nsub=4,
         head='tiles', head_ug=2, reduce='colsum'),
    # S = 16, P = 225: 14 / 15 pixels per block in chunks of 2 -- a partial last chunk; head rows UG 13 (K = 600);
    # RELU_INPUT on the VW 4 instance; finalize width 128
    case('stream_f32_c4096_S16_softmax_train_relu_input', 32, 225, 4096, 600, act='softmax', train=True,
         relu_in=True, pool_fwd='stream', fwd_w=4, fwd_pix=2, pool_bwd='stream', bwd_w=4, bwd_pix=2, S=16, ppb=15,
         cw=128, relu_input=1, logits='logits2', logits_nsub=1, head='rows', head_ug=13),
    # bf16 through the one-call step: keep-bits backward form, 13-pixel blocks = 7 chunks of 2, the last partial
    case('stream_bf16_c2048_S16_softmax_step', 32, 196, 2048, 393, dt=BF16, act='softmax', train=True, entry='step',
         pool_fwd='stream', fwd_w=1, fwd_pix=2, pool_bwd='stream', bwd_w=1, bwd_pix=2, S=16, ppb=13, cw=64,
         keep_bits=1, logits='xent', logits_nv4=4, head='rows', head_ug=7, reduce='colsum'),
    case('stream_bf16_c2048_S16_id_train_sep', 32, 196, 2048, 51, dt=BF16, train=True,
         pool_fwd='stream', fwd_pix=2, bwd_pix=2, S=16, keep_bits=0, logits='logits2', head='rows', head_ug=1),
    # RELU_INPUT on every other streaming instance
    case('relu_input_f32_c1024_relu_train', 6, 49, 1024, 51, act='relu', train=True, relu_in=True,
         pool_fwd='stream', fwd_w=1, S=12, ppb=5, relu_input=1, head='rows', head_ug=1),
    case('relu_input_f32_c2048_softmax_eval', 6, 49, 2048, 51, act='softmax', relu_in=True,
         pool_fwd='stream', fwd_w=2, relu_input=1),
    case('relu_input_bf16_c2048_id_train', 6, 49, 2048, 51, dt=BF16, train=True, relu_in=True,
         pool_fwd='stream', fwd_w=1, fwd_pix=2, relu_input=1),
    # separate attention input on the streaming kernels (fp32 / bf16, full dXatt / rank-1)
    case('stream_sep_f32_c2048_softmax_train', 4, 196, 2048, 100, act='softmax', train=True, Ca=768,
         pool_fwd='stream', fused=0, head='rows', head_ug=2, gemv='bwd2', reduce='colsum'),
    case('stream_sep_bf16_c2048_rank1_relu', 4, 196, 2048, 200, dt=BF16, act='relu', Ca=512, rank1=True,
         pool_fwd='stream', fused=0, head='rows', head_ug=4, gemv='bwd2_rank1'),
    # ---- per-pixel vec kernels: fp32 C 256 / 512 (VEC 1 / 2), bf16 C 512 / 1024 (VEC 1 / 2)
    case('vec_f32_c256_softmax_train', 5, 36, 256, 51, act='softmax', train=True,
         pool_fwd='vec', fwd_w=1, pool_bwd='vec', bwd_w=1, head='small', head_mv=4, reduce='colsum'),
    case('vec_f32_c512_relu_k200', 40, 25, 512, 200, act='relu',
         pool_fwd='vec', fwd_w=2, pool_bwd='vec', bwd_w=2, head='small', head_mv=8),
    case('vec_bf16_c512_sep_train', 3, 64, 512, 10, dt=BF16, train=True, Ca=200,
         pool_fwd='vec', fwd_w=1, pool_bwd='vec', bwd_w=1, head='rows', head_ug=1, gemv='bwd2'),
    case('vec_bf16_c1024_softmax_train', 12, 49, 1024, 393, dt=BF16, act='softmax', train=True,
         pool_fwd='vec', fwd_w=2, pool_bwd='vec', bwd_w=2, head='small', head_mv=13),
    # ---- generic run-time-loop kernels
    case('generic_f32_c96_k3', 3, 20, 96, 3, pool_fwd='generic', pool_bwd='generic', logits='sgemm',
         head='sgemm', reduce='bwd_reduce'),
    case('generic_f32_c832_softmax_train', 4, 30, 832, 51, act='softmax', train=True,
         pool_fwd='generic', logits='logits2', head='sgemm', reduce='bwd_reduce'),
    case('generic_f32_c1000_relu', 5, 16, 1000, 51, act='relu', pool_fwd='generic', logits='sgemm', head='sgemm'),
    case('generic_f32_c2064_sep_ca1280_train', 3, 49, 2064, 51, train=True, Ca=1280,
         pool_fwd='generic', logits='sgemm', head='sgemm', gemv='bwd', reduce='bwd_reduce'),
    case('generic_bf16_c4096_softmax', 8, 36, 4096, 51, dt=BF16, act='softmax',
         pool_fwd='generic', pool_bwd='generic', head='rows', head_ug=1),
    case('generic_external_mask_f32_c2048', 4, 49, 2048, 51, train=True, rng='external',
         pool_fwd='generic', pool_bwd='generic', head='rows'),
    # ---- logits + cross-entropy (one-call steps): NV4 1 / 2 / 4, with probabilities in the eval step
    case('xent_k51_step', 40, 49, 2048, 51, train=True, entry='step', logits='xent', logits_nv4=1,
         head='tiles', head_ug=1),
    case('xent_k200_step', 40, 49, 2048, 200, act='softmax', entry='step', logits='xent', logits_nv4=2,
         head='tiles', head_ug=4),
    case('xent_k512_step', 48, 16, 2048, 512, train=True, entry='step', logits='xent', logits_nv4=4,
         head='rows', head_ug=13),
    case('xent_k393_tiles_step', 36, 49, 2048, 393, act='relu', train=True, entry='step', logits='xent',
         logits_nv4=4, head='tiles', head_ug=7),
    case('xent_probs_k51_eval', 8, 49, 2048, 51, entry='eval', logits='xent_probs', logits_nv4=1),
    case('xent_probs_k200_eval', 8, 49, 1024, 200, act='softmax', entry='eval', logits='xent_probs', logits_nv4=2),
    # ---- the small backward products
    case('small_f32_c128_k1', 4, 16, 128, 1, pool_fwd='generic', head='small', head_mv=4, reduce='colsum'),
    case('small_f32_c256_k2', 4, 16, 256, 2, act='relu', pool_fwd='vec', head='small', head_mv=4),
    case('small_f32_c384_k3', 4, 16, 384, 3, act='softmax', pool_fwd='generic', head='small', head_mv=4),
    case('small_f32_c512_k600_mv26', 6, 25, 512, 600, act='softmax', pool_fwd='vec', head='small', head_mv=26),
    case('head_sgemm_k800_rng_device', 6, 49, 1024, 800, train=True, rng='device', logits='logits2',
         head='sgemm', reduce='bwd_reduce', rng_bump=1),
    # ---- 16-byte alignment of caller buffers
    case('misaligned_zsave', 4, 49, 2048, 51, train=True, mis=('zsave',), logits='sgemm', head='sgemm',
         reduce='bwd_reduce'),
    case('misaligned_G', 4, 49, 1024, 51, act='softmax', mis=('G',), logits='logits2', head='sgemm',
         reduce='bwd_reduce'),
    case('misaligned_Wt', 4, 49, 1024, 51, mis=('Wt',), logits='logits2', head='sgemm', reduce='bwd_reduce'),
    case('misaligned_G_step', 4, 49, 2048, 51, train=True, entry='step', mis=('G',), logits='logits2',
         head='sgemm', reduce='bwd_reduce'),
    # ---- attention-side GEMV backward
    case('gemv_bwd2_rank1_f32', 4, 49, 1024, 51, act='softmax', Ca=200, rank1=True, gemv='bwd2_rank1'),
    case('gemv_bwd_f32_ca2048', 3, 49, 1024, 51, act='relu', train=True, Ca=2048, gemv='bwd'),
    case('gemv_bwd_bf16_ca2560', 3, 49, 2048, 51, dt=BF16, act='softmax', Ca=2560, gemv='bwd'),
    # ---- device-side dropout counter: read by both passes, advanced once by the backward's last launch
    case('rng_device_step', 8, 49, 2048, 51, act='softmax', train=True, rng='device', entry='step',
         rng_bump=1, reduce='colsum'),
    case('rng_device_sep_bf16', 8, 49, 2048, 51, dt=BF16, train=True, rng='device', rng_bump=1),
    # ---- ..._WITH_POSE_FEAT concat (apa_m1_cat.hip)
    case('cat_j1_train', 4, 49, 2048, 51, train=True, J=1, cat_fwd=1, cat_bwd=1),
    case('cat_j16_softmax_train', 4, 49, 1024, 100, act='softmax', train=True, J=16, cat_fwd=16, cat_bwd=16),
    # ---- shipped shapes (cfg 002: N = 32 x 14x14x2048 fp32, K = 393, keep 0.2) and ragged neighbours
    case('cfg002_train_step', 32, 196, 2048, 393, train=True, keep=0.2, entry='step',
         pool_fwd='stream', fwd_w=2, fwd_pix=1, S=16, ppb=13, cw=64, logits='xent', logits_nv4=4, head='rows',
         head_ug=7, reduce='colsum'),
    case('cfg002_eval_step', 32, 196, 2048, 393, entry='eval', pool_fwd='stream', logits='xent_probs',
         logits_nv4=4),
    case('cfg002_ragged_train_step', 33, 225, 2048, 393, train=True, keep=0.2, entry='step',
         S=16, ppb=15, cw=64, logits='xent', head='tiles', head_ug=7),
    case('cfg002_ragged_eval_step', 33, 225, 2048, 393, entry='eval', logits='xent_probs'),
]


# ------------------------------------------------------------------------------------------ inputs
def _inputs(c, dev):
    g = torch.Generator(device=dev).manual_seed(sum(map(ord, c['name'])))
    N, P, C, K, J = c['N'], c['P'], c['C'], c['K'], c['J']
    Ca = c['Ca'] or C
    tdt = torch.bfloat16 if c['dt'] == BF16 else torch.float32

    def u(*shape):
        return torch.rand(shape, generator=g, device=dev) * 1.25 - 0.25

    rows = 0.25 + 1.5 * torch.rand((N, P, 1), generator=g, device=dev)   # a per-pixel scale
    X = (u(N, P, C) * rows).to(tdt)
    Xatt = X if c['Ca'] is None else (u(N, P, Ca) * rows).to(tdt)
    # positive-mean attention weights: Z = Xatt . Wa follows the per-pixel scale (0.14 s Wscale on average), so
    # relu gates both ways around the mean pixel (ba) and softmax is peaked, without cancellation in the sum
    wscale = {'id': 4.0, 'relu': 4.0, 'softmax': 8.0}[c['act']]
    Wa = u(Ca) * (wscale / Ca)
    ba = -(Xatt.float().mean(dim=(0, 1)) @ Wa).reshape(1) if c['act'] == 'relu' else u(1) * 0.1
    Wt = u(C + J, K) / C ** 0.5
    bt = u(K) * 0.1
    G = u(N, K) / N
    labels = torch.randint(0, K, (N,), generator=g, device=dev)
    Xext = (u(N, P, J) * rows).contiguous() if J else None
    return dict(X=X, Xatt=Xatt, Wa=Wa, ba=ba, Wt=Wt, bt=bt, G=G, labels=labels, Xext=Xext)


def _flags(c):
    f = {'id': 0, 'relu': cof.APA_FLAG_RELU_ATT, 'softmax': cof.APA_FLAG_SOFTMAX_ATT}[c['act']]
    if c['train']:
        f |= cof.APA_FLAG_TRAIN
    if c['relu_in']:
        f |= cof.APA_FLAG_RELU_INPUT
    return f


class _Run:
    """The buffers of one case (NaN-guarded outputs and workspace) and the calls that fill them."""

    def __init__(self, c, inp, dev, lib):
        self.c, self.inp, self.dev, self.lib = c, inp, dev, lib
        N, P, C, K, J = c['N'], c['P'], c['C'], c['K'], c['J']
        Ca = c['Ca'] or C
        tdt = inp['X'].dtype
        self.N, self.P, self.C, self.Ca, self.K, self.J = N, P, C, Ca, K, J
        fused = c['Ca'] is None
        off = {k: (1 if k in c['mis'] else 0) for k in ('zsave', 'G', 'Wt')}
        Gd = gp.Guarded
        self.Wt = Gd(C + J, K, K, torch.float32, dev, off=off['Wt'], data=inp['Wt'])
        self.out = {
            'logits': Gd(N, K, K, torch.float32, dev), 'att': Gd(N, P, P, torch.float32, dev),
            'zsave': Gd(N, C, C, torch.float32, dev, off=off['zsave']), 'abar': Gd(1, N, N, torch.float32, dev),
            'G': Gd(N, K, K, torch.float32, dev, off=off['G']),
            'dX': Gd(N * P, C, C, tdt, dev), 'dWa': Gd(1, Ca, Ca, torch.float32, dev),
            'dba': Gd(1, 1, 1, torch.float32, dev), 'dWt': Gd(C + J, K, K, torch.float32, dev),
            'dbt': Gd(1, K, K, torch.float32, dev),
        }
        if not fused:
            self.out['dXatt'] = (Gd(1, N * P, N * P, torch.float32, dev) if c['rank1'] else
                                 Gd(N * P, Ca, Ca, tdt, dev))
        if c['entry'] == 'step':
            self.out['loss'] = Gd(1, N + 1, N + 1, torch.float32, dev)
        if c['entry'] == 'eval':
            self.out['probs'] = Gd(N, K, K, torch.float32, dev)
            self.pred = torch.full((N,), -1, dtype=torch.int64, device=dev)
        if J:
            self.out['zext'] = Gd(N, J, J, torch.float32, dev)
            self.out['dXext'] = Gd(N * P, J, J, torch.float32, dev)
        flags = _flags(c)
        if c['rank1']:
            flags |= cof.APA_FLAG_DXATT_RANK1
        self.flags = flags
        ws_bytes = int(lib.apa_attn_pool_workspace_bytes(N, P, C, Ca, K, 1, flags))
        self.ws_bytes = ws_bytes
        self.ws = Gd(1, (ws_bytes + 3) // 4, (ws_bytes + 3) // 4, torch.float32, dev)
        self.counter = torch.tensor([5], dtype=torch.int64, device=dev) if c['rng'] == 'device' else None
        self.mask = None
        if c['train']:
            if c['rng'] == 'external':
                g = torch.Generator(device=dev).manual_seed(99)
                self.mask = (torch.rand(N * P * (C + J), generator=g, device=dev) < c['keep']).to(torch.uint8)
                self.packed = cof.pack_keep_mask(self.mask)
            else:
                self.mask = cof.dropout_mask((N * P * (C + J),), c['keep'], 1234, 5 if c['rng'] == 'device' else 7)
        if c['entry'] == 'sep':
            self.out['G'].view.copy_(inp['G'])
        for b in list(self.out.values()) + [self.ws]:
            b.snapshot()

    def key(self):
        c = self.c
        if c['rng'] == 'external':
            return self.packed.bits.data_ptr(), 0, self.flags | cof.APA_FLAG_RNG_EXTERNAL
        if c['rng'] == 'device':
            return 1234, self.counter.data_ptr(), self.flags | cof.APA_FLAG_RNG_DEVICE
        return 1234, 7, self.flags

    def p(self, k):
        return self.out[k].ptr if k in self.out else None

    def run(self):
        """-> merged trace of the calls."""
        c, lib, inp = self.c, self.lib, self.inp
        N, P, C, Ca, K = self.N, self.P, self.C, self.Ca, self.K
        X = inp['X'].data_ptr()
        Xatt = X if c['Ca'] is None else inp['Xatt'].data_ptr()
        Wa, ba, bt = inp['Wa'].data_ptr(), inp['ba'].data_ptr(), inp['bt'].data_ptr()
        Wt = self.Wt.ptr
        seed, offset, flags = self.key()
        st = gp.stream_ptr()
        dt = c['dt']
        t1, t2 = mp.M1Trace(), mp.M1Trace()
        tr = ctypes.byref
        if c['entry'] == 'step':
            rc = lib.apa_probe_m1_train_step_ex(
                tr(t1), None, X, Xatt, Wa, ba, Wt, bt, inp['labels'].data_ptr(), 1.0, 1.0, self.p('logits'),
                self.p('att'), self.p('zsave'), self.p('abar'), self.p('loss'), self.p('G'), self.p('dX'),
                self.p('dXatt'), self.p('dWa'), self.p('dba'), self.p('dWt'), self.p('dbt'), self.ws.ptr,
                self.ws_bytes, N, P, C, Ca, K, 1, flags, c['keep'], seed, offset, dt, st)
            assert rc == 0, lib.apa_last_error()
            return mp.merge(t1)
        if c['entry'] == 'eval':
            rc = lib.apa_probe_m1_eval_step(
                tr(t1), X, Xatt, Wa, ba, Wt, bt, None, self.p('logits'), self.p('att'), self.p('zsave'),
                self.p('abar'), None, self.p('probs'), self.pred.data_ptr(), self.ws.ptr, self.ws_bytes,
                N, P, C, Ca, K, 1, flags, dt, st)
            assert rc == 0, lib.apa_last_error()
            return mp.merge(t1)
        if c['J']:
            cat = cof.ApaConcatFeat(inp['Xext'].data_ptr(), c['J'], self.p('zext'), self.p('dXext'))
            rc = lib.apa_probe_m1_fwd_cat(
                tr(t1), ctypes.addressof(cat), None, X, Xatt, Wa, ba, Wt, bt, self.p('logits'), self.p('att'),
                self.p('zsave'), self.p('abar'), None, self.ws.ptr, self.ws_bytes, N, P, C, Ca, K, 1, flags,
                c['keep'], seed, offset, dt, st)
            assert rc == 0, lib.apa_last_error()
            rc = lib.apa_probe_m1_bwd_cat(
                tr(t2), ctypes.addressof(cat), None, X, Xatt, Wa, ba, Wt, bt, self.p('att'), self.p('zsave'),
                self.p('abar'), self.p('G'), self.p('dX'), self.p('dXatt'), self.p('dWa'), self.p('dba'),
                self.p('dWt'), self.p('dbt'), self.ws.ptr, self.ws_bytes, N, P, C, Ca, K, 1, flags, c['keep'],
                seed, offset, dt, st)
            assert rc == 0, lib.apa_last_error()
            return mp.merge(t1, t2)
        rc = lib.apa_probe_m1_fwd_ex(
            tr(t1), None, X, Xatt, Wa, ba, Wt, bt, self.p('logits'), self.p('att'), self.p('zsave'), self.p('abar'),
            None, self.ws.ptr, self.ws_bytes, N, P, C, Ca, K, 1, flags, c['keep'], seed, offset, dt, st)
        assert rc == 0, lib.apa_last_error()
        rc = lib.apa_probe_m1_bwd_ex(
            tr(t2), None, X, Xatt, Wa, ba, Wt, bt, self.p('att'), self.p('zsave'), self.p('abar'), self.p('G'),
            self.p('dX'), self.p('dXatt'), self.p('dWa'), self.p('dba'), self.p('dWt'), self.p('dbt'), self.ws.ptr,
            self.ws_bytes, N, P, C, Ca, K, 1, flags, c['keep'], seed, offset, dt, st)
        assert rc == 0, lib.apa_last_error()
        return mp.merge(t1, t2)

    def restore(self):
        for b in list(self.out.values()) + [self.ws]:
            b.restore()
        if self.counter is not None:
            self.counter.fill_(5)

    def check_guards(self):
        for k, b in self.out.items():
            b.check_guards(k)
        self.ws.check_guards('workspace')

    def bits(self):
        d = {k: b.bits() for k, b in self.out.items()}
        if hasattr(self, 'pred'):
            d['pred'] = self.pred.clone()
        return d


# ------------------------------------------------------------------------------------------ references
def _forward_ref(c, inp, keepmask):
    """Bnd att, zsave, abar, logits (+ zext), and the relu-ambiguous pixels, from the inputs alone.  The contractions
    over the channels and over the pixels are taken as Ca and P additions long; a case may state the kernel's own
    longest chains instead (c['chains']: 'dot' for a pixel's channel contraction, 'pool' for the pooled sums over the
    pixels, 'logits' for the logits' channel contraction -- tests/_fp8_cases.py derives them), never longer ones."""
    N, P, C, K, J = c['N'], c['P'], c['C'], c['K'], c['J']
    X = inp['X'].double()
    if c['relu_in']:
        X = X.clamp_min(0)
    Xa = X if c['Ca'] is None else inp['Xatt'].double()
    Ca = Xa.shape[-1]
    chains = c.get('chains') or {}
    Ldot, Lpool, Llog = min(chains.get('dot', Ca), Ca), min(chains.get('pool', P), P), min(chains.get('logits', C), C)
    zl =contract('npc,c->np', Bnd(Xa), Bnd(inp['Wa'].double()), Ldot) + Bnd(inp['ba'].double().expand(N, P))
    amb = None
    if c['act'] == 'softmax':
        A = mp.softmax_p(zl)
    elif c['act'] == 'relu':
        A = Bnd(zl.ref.clamp_min(0), zl.err)
        amb = zl.ref.abs() <= zl.err
    else:
        A = zl
    Xt, Xe = _dropped(c, inp, X, keepmask)
    zs = contract('np,npc->nc', A, Xt, Lpool).scale(1.0 / P)
    ones = Bnd(torch.ones(P, dtype=torch.float64, device=X.device))
    ab = contract('np,p->n', A, ones, Lpool).scale(1.0 / P)
    Wt = inp['Wt'].double()
    lg = contract('nc,ck->nk', zs, Bnd(Wt[:C]), Llog) + Bnd(ab.ref[:, None], ab.err[:, None]).mul(
        Bnd(inp['bt'].double()[None, :]))
    ze = None
    if J:
        ze = contract('np,npj->nj', A, Xe, P).scale(1.0 / P)
        lg = lg + contract('nj,jk->nk', ze, Bnd(Wt[C:]), J)
    return dict(att=A, zsave=zs, abar=ab, logits=lg.rounded(), zext=ze), amb


def _dropped(c, inp, X, keepmask):
    """Bnd X * mask / keep (fp32 scaling: one rounding) and the same for the concat channels."""
    N, P, C, J = c['N'], c['P'], c['C'], c['J']
    Xe = inp['Xext'].double() if J else None
    if not c['train']:
        return Bnd(X), (Bnd(Xe) if J else None)
    inv = float(torch.tensor(1.0 / c['keep'], dtype=torch.float32))
    m = keepmask.double()
    Xt = Bnd(X * m[:N * P * C].view(N, P, C) * inv).rounded()
    Xet = Bnd(Xe * m[N * P * C:].view(N, P, J) * inv).rounded() if J else None
    return Xt, Xet


def _backward_ref(c, inp, got, keepmask):
    """Bnd dX, dXatt, dWa, dba, dWt, dbt (+ dXext) from the kernel's own att, zsave, abar, zext and G (every
    backward kernel reads `att`, so a relu gate is att > 0 exactly).  c['chains']['dot']: as in _forward_ref."""
    N, P, C, K, J = c['N'], c['P'], c['C'], c['K'], c['J']
    X = inp['X'].double()
    Xr = X.clamp_min(0) if c['relu_in'] else X
    Xa = Xr if c['Ca'] is None else inp['Xatt'].double()
    Ca = Xa.shape[-1]
    A = Bnd(got['att'].double().reshape(N, P))
    G = Bnd(got['G'].double().reshape(N, K))
    zs = Bnd(got['zsave'].double().reshape(N, C))
    ab = Bnd(got['abar'].double().reshape(N))
    Wt = inp['Wt'].double()
    Wa = Bnd(inp['Wa'].double())
    Xt, Xe = _dropped(c, inp, Xr, keepmask)
    out = {}
    dz = contract('nk,ck->nc', G, Bnd(Wt[:C]), K)
    out['dWt'] = contract('nc,nk->ck', zs, G, N)
    out['dbt'] = contract('n,nk->k', ab, G, N)
    sn = contract('nk,k->n', G, Bnd(inp['bt'].double()), K)
    dA = contract('npc,nc->np', Xt, dz, min((c.get('chains') or {}).get('dot', C), C)) + \
        Bnd(sn.ref[:, None].expand(N, P), sn.err[:, None].expand(N, P))
    if J:
        ze = Bnd(got['zext'].double().reshape(N, J))
        out['dWt_ext'] = contract('nj,nk->jk', ze, G, N)
        dze = contract('nk,jk->nj', G, Bnd(Wt[C:]), K)
        dA = dA + contract('npj,nj->np', Xe, dze, J)
    dA = dA.scale(1.0 / P).rounded()
    if c['act'] == 'softmax':
        s = contract('np,np->n', A, dA, P)
        dZ = A.mul(Bnd(dA.ref - s.ref[:, None], dA.err + s.err[:, None]).rounded())
    elif c['act'] == 'relu':
        gate = (A.ref > 0).double()
        dZ = Bnd(dA.ref * gate, dA.err * gate)
    else:
        dZ = dA
    # dWa / dba: per-block partial sums (a block's pixels) then a column sum over the blocks -- the longest chain
    # of fp32 additions any element sees is (pixels per block + blocks), not N P
    S, ppb, nblk, _ = mp.plan(N, P, C, Ca, K)
    if c['Ca'] is None:
        Lw = ppb + nblk
    else:                                  # apa_m1.hip m1_backward: the GEMV's own block count
        nb = min(max((N * P + 15) // 16, 1), 1024, nblk)
        Lw = (N * P + nb - 1) // nb + nb
    out['dWa'] = contract('np,npc->c', dZ, Bnd(Xa), Lw)
    ones = Bnd(torch.ones(N, P, dtype=torch.float64, device=X.device))
    dba = contract('np,np->', dZ, ones, Lw)
    out['dba'] = Bnd(dba.ref.reshape(1), dba.err.reshape(1))
    Apx = Bnd(A.ref[:, :, None] / P)
    dXp = Apx.mul(Bnd(dz.ref[:, None, :], dz.err[:, None, :]))
    if c['train']:
        inv = float(torch.tensor(1.0 / c['keep'], dtype=torch.float32))
        m = keepmask.double()
        dXp = dXp.mul(Bnd(m[:N * P * C].view(N, P, C) * inv))
    if c['Ca'] is None:
        dX = dXp + Bnd(dZ.ref[:, :, None], dZ.err[:, :, None]).mul(Bnd(Wa.ref[None, None, :]))
        dX = dX.rounded()
    else:
        dX = dXp
        if c['rank1']:
            out['dXatt'] = dZ
        else:
            out['dXatt'] = Bnd(dZ.ref[:, :, None], dZ.err[:, :, None]).mul(Bnd(Wa.ref[None, None, :]))
    if c['relu_in']:
        pos = (X > 0).double()
        dX = Bnd(dX.ref * pos, dX.err * pos)
    out['dX'] = dX
    if J:
        dXe = Apx.mul(Bnd(dze.ref[:, None, :], dze.err[:, None, :]))
        if c['train']:
            dXe = dXe.mul(Bnd(keepmask.double()[N * P * C:].view(N, P, J) * inv))
        out['dXext'] = dXe
    return out


def _check_forward(c, got, ref, amb):
    mp.check(got['att'], ref['att'], 'att', ambiguous=amb)
    for k in ('zsave', 'abar', 'logits'):
        mp.check(got[k], ref[k], k)
    if c['J']:
        mp.check(got['zext'], ref['zext'], 'zext')


def _check_backward(c, got, ref):
    C, K, J = c['C'], c['K'], c['J']
    bf = c['dt'] == BF16
    mp.check(got['dX'], ref['dX'], 'dX', bf16=bf)
    if c['Ca'] is not None:
        mp.check(got['dXatt'], ref['dXatt'], 'dXatt', bf16=bf and not c['rank1'])
    # dWa = sum_p dZ Xatt and dba = sum_p dZ cancel where sum_p dZ = 0 (softmax) or the rows of G sum to zero (the cross-entropy G
    # of the one-call step): its bound, carried from dA's C-long contraction, is then not small against the result
    # and only the elementwise bound is asserted
    cancels = c['act'] == 'softmax' or c['entry'] == 'step'
    mp.check(got['dWa'], ref['dWa'], 'dWa', zero_ref=cancels)
    mp.check(got['dba'], ref['dba'], 'dba', zero_ref=cancels)
    dWt = got['dWt'].reshape(C + J, K)
    mp.check(dWt[:C], ref['dWt'], 'dWt')
    if J:
        mp.check(dWt[C:], ref['dWt_ext'], 'dWt (concat rows)')
        mp.check(got['dXext'], ref['dXext'], 'dXext')
    mp.check(got['dbt'], ref['dbt'], 'dbt')


def _check_loss(c, got, inp):
    """loss / G (train step) or probs / pred (eval step) from the kernel's own logits."""
    N, K = c['N'], c['K']
    lg = got['logits'].double().reshape(N, K)
    p = torch.softmax(lg, dim=1)
    tol = mp.C_ACC * (K + 16) * mp.EPS32
    if c['entry'] == 'eval':
        mp.check(got['probs'], Bnd(p, tol * p), 'probs')
        assert torch.equal(got['pred'], lg.argmax(dim=1)), 'pred'
        return
    lab = inp['labels']
    onehot = torch.nn.functional.one_hot(lab, K).double()
    mp.check(got['G'], Bnd((p - onehot) / N, tol * (p + onehot) / N), 'G')
    lse = torch.logsumexp(lg, dim=1)
    per = lse - lg.gather(1, lab[:, None])[:, 0]
    mag = lse.abs() + lg.abs().amax(dim=1)
    loss = got['loss'].double().reshape(N + 1)
    mp.check(loss[1:], Bnd(per, tol * mag), 'loss per example')
    mp.check(loss[:1], Bnd(per.mean().reshape(1), (tol * mag).mean().reshape(1) + tol * per.abs().mean()),
             'loss')


def _separate_equivalent(c, r, lib):
    """The one-call step's outputs from the separate entry points (fwd, softmax_xent, bwd), as bits."""
    c2 = dict(c, entry='sep')
    s = _Run(c2, r.inp, r.dev, lib)
    s.restore()
    if c['entry'] == 'step':
        seed, offset, flags = s.key()
        st = gp.stream_ptr()
        N, P, C, Ca, K = s.N, s.P, s.C, s.Ca, s.K
        X = r.inp['X'].data_ptr()
        Xatt = X if c['Ca'] is None else r.inp['Xatt'].data_ptr()
        args = (X, Xatt, r.inp['Wa'].data_ptr(), r.inp['ba'].data_ptr(), s.Wt.ptr, r.inp['bt'].data_ptr())
        assert lib.apa_attn_pool_fwd_ex(None, *args, s.p('logits'), s.p('att'), s.p('zsave'), s.p('abar'), None,
                                        s.ws.ptr, s.ws_bytes, N, P, C, Ca, K, 1, flags, c['keep'], seed, offset,
                                        c['dt'], st) == 0, lib.apa_last_error()
        loss = gp.Guarded(1, N + 1, N + 1, torch.float32, r.dev)
        assert lib.apa_softmax_xent_fwd_bwd(s.p('logits'), r.inp['labels'].data_ptr(), loss.ptr, s.p('G'), None,
                                            None, N, K, 1.0, 1.0, st) == 0, lib.apa_last_error()
        assert lib.apa_attn_pool_bwd_ex(None, *args, s.p('att'), s.p('zsave'), s.p('abar'), s.p('G'), s.p('dX'),
                                        s.p('dXatt'), s.p('dWa'), s.p('dba'), s.p('dWt'), s.p('dbt'), s.ws.ptr,
                                        s.ws_bytes, N, P, C, Ca, K, 1, flags, c['keep'], seed, offset, c['dt'],
                                        st) == 0, lib.apa_last_error()
        out = s.bits()
        out['loss'] = loss.bits()
        return out
    seed, offset, flags = s.key()
    st = gp.stream_ptr()
    N, P, C, Ca, K = s.N, s.P, s.C, s.Ca, s.K
    X = r.inp['X'].data_ptr()
    Xatt = X if c['Ca'] is None else r.inp['Xatt'].data_ptr()
    assert lib.apa_attn_pool_fwd_ex(None, X, Xatt, r.inp['Wa'].data_ptr(), r.inp['ba'].data_ptr(), s.Wt.ptr,
                                    r.inp['bt'].data_ptr(), s.p('logits'), s.p('att'), s.p('zsave'), s.p('abar'),
                                    None, s.ws.ptr, s.ws_bytes, N, P, C, Ca, K, 1, flags, 1.0, seed, offset,
                                    c['dt'], st) == 0, lib.apa_last_error()
    probs = gp.Guarded(N, K, K, torch.float32, r.dev)
    pred = torch.full((N,), -1, dtype=torch.int64, device=r.dev)
    loss = gp.Guarded(1, N + 1, N + 1, torch.float32, r.dev)   # (probs / pred do not depend on the labels)
    assert lib.apa_softmax_xent_fwd_bwd(s.p('logits'), r.inp['labels'].data_ptr(), loss.ptr, None, probs.ptr,
                                        pred.data_ptr(), N, K, 1.0, 1.0, st) == 0, lib.apa_last_error()
    out = s.bits()
    out['probs'], out['pred'] = probs.bits(), pred
    return out


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_m1_path(gpu, c):
    lib = mp.load_m1_probe()
    torch.manual_seed(0)
    inp = _inputs(c, gpu)
    r = _Run(c, inp, gpu, lib)
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    # the traced path
    S, ppb, nblk, _ = mp.plan(c['N'], c['P'], c['C'], c['Ca'] or c['C'], c['K'])
    exp = dict(c['expect'], S=c['expect'].get('S', S), ppb=c['expect'].get('ppb', ppb), nblk=nblk)
    exp.setdefault('fused', int(c['Ca'] is None))
    exp.setdefault('relu_input', int(c['relu_in']))
    exp.setdefault('rng_bump', 0)
    exp.setdefault('cat_fwd', c['J'])
    if c['entry'] != 'eval':
        exp.setdefault('cat_bwd', c['J'])
        exp.setdefault('reduce', 'colsum' if exp.get('head') in ('tiles', 'rows', 'small', None) else 'bwd_reduce')
        exp.setdefault('gemv', 'none' if c['Ca'] is None else exp.get('gemv'))
    else:
        for k in ('pool_bwd', 'head', 'gemv', 'reduce'):
            exp.setdefault(k, 'none')
    bad = {k: (trace[k], v) for k, v in exp.items() if v is not None and trace[k] != v}
    assert not bad, 'trace mismatch (got, expected): {} in {}'.format(bad, trace)
    assert (S, ppb) == (trace['S'], trace['ppb'])
    if c['rng'] == 'device':
        assert int(r.counter) == 6, 'the dropout counter must advance exactly once per step'

    got = {k: b.view.clone() for k, b in r.out.items()}
    if c['entry'] == 'eval':
        got['pred'] = r.pred.clone()
    keepmask = r.mask
    with torch.no_grad():
        fref, amb = _forward_ref(c, inp, keepmask)
        if amb is not None:
            assert int(amb.sum()) <= max(2, amb.numel() // 100), 'too many relu gates at zero: {}'.format(
                int(amb.sum()))
        _check_forward(c, got, fref, amb)
        if c['entry'] != 'eval':
            bref = _backward_ref(c, inp, got, keepmask)
            _check_backward(c, got, bref)
        if c['entry'] != 'sep':
            _check_loss(c, got, inp)
        del fref

    # repeats bit for bit
    first = r.bits()
    r.restore()
    trace2 = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    assert trace2 == trace
    second = r.bits()
    for k in first:
        assert torch.equal(first[k], second[k]), '{} differs between two identical calls'.format(k)
    # the one-call steps equal the separate entry points bit for bit (apa.h: same kernels, same reduction trees)
    if c['entry'] in ('step', 'eval'):
        sep = _separate_equivalent(c, r, lib)
        torch.cuda.synchronize()
        keys = first if c['entry'] == 'step' else ('logits', 'att', 'zsave', 'abar', 'probs', 'pred')
        for k in keys:
            assert torch.equal(first[k], sep[k]), '{}: one-call step differs from the separate calls'.format(k)


# ------------------------------------------------------------------------------------------ refusals
APA_ERR_UNSUPPORTED = -2    # include/apa.h

# (case, extra flags of the refused calls, which calls are refused, apa_last_error text)
REFUSALS = [
    # 257 fp32 vectors per attention row: one more than the register-resident GEMV, the only one with a rank-1 form
    (case('refused_rank1_ca1028', 2, 16, 256, 3, Ca=1028, rank1=True), 0, ('bwd',),
     'attn_pool M=1: APA_FLAG_DXATT_RANK1: Ca=1028 not served by the register-resident GEMV'),
    # a per-pixel (vec) C: the relu-on-load instances exist in the streaming family only
    (case('refused_relu_input_c512', 2, 16, 512, 3), cof.APA_FLAG_RELU_INPUT, ('fwd', 'bwd'),
     'attn_pool M=1: APA_FLAG_RELU_INPUT needs Xatt == X and C in {1024,2048,4096} (f32) / 2048 (bf16)'),
]


@pytest.mark.parametrize('c,extra,refused,text', REFUSALS, ids=[r[0]['name'] for r in REFUSALS])
def test_m1_refused_call_launches_nothing(gpu, c, extra, refused, text):
    """A call the M == 1 path refuses returns APA_ERR_UNSUPPORTED with its message before anything is queued: after
    a synchronize no byte of any output, of the workspace or of their guards has changed.  (The backward calls read
    att / zsave / abar of a served forward call, so a kernel launched in spite of the refusal would write numbers
    over the NaN sentinels.)"""
    lib = mp.load_m1_probe()
    torch.manual_seed(0)
    inp = _inputs(c, gpu)
    r = _Run(c, inp, gpu, lib)
    N, P, C, Ca, K = r.N, r.P, r.C, r.Ca, r.K
    X = inp['X'].data_ptr()
    Xatt = X if c['Ca'] is None else inp['Xatt'].data_ptr()
    args = (None, X, Xatt, inp['Wa'].data_ptr(), inp['ba'].data_ptr(), r.Wt.ptr, inp['bt'].data_ptr())
    st = gp.stream_ptr()

    def fwd(flags):
        return lib.apa_attn_pool_fwd_ex(*args, r.p('logits'), r.p('att'), r.p('zsave'), r.p('abar'), None, r.ws.ptr,
                                        r.ws_bytes, N, P, C, Ca, K, 1, flags, 1.0, 0, 0, c['dt'], st)

    def bwd(flags):
        return lib.apa_attn_pool_bwd_ex(*args, r.p('att'), r.p('zsave'), r.p('abar'), r.p('G'), r.p('dX'),
                                        r.p('dXatt'), r.p('dWa'), r.p('dba'), r.p('dWt'), r.p('dbt'), r.ws.ptr,
                                        r.ws_bytes, N, P, C, Ca, K, 1, flags, 1.0, 0, 0, c['dt'], st)

    assert fwd(r.flags) == 0, lib.apa_last_error()       # the served forward call: real att, zsave, abar
    torch.cuda.synchronize()
    bufs = dict(r.out, workspace=r.ws)
    for b in bufs.values():
        b.snapshot()
    for which in refused:
        rc = (fwd if which == 'fwd' else bwd)(r.flags | extra)
        assert rc == APA_ERR_UNSUPPORTED, (which, rc)
        assert lib.apa_last_error().decode() == text, which
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert torch.equal(b.base.view(gp._INT_VIEW[b.dtype]), b.snap), \
                '{}: the refused {} call changed {}'.format(c['name'], which, k)
