"""Every path of the per-class maps (M == K: csrc/apa_pc.hip and csrc/apa_pc_fused.hip) against float64,
stage by stage.

Each case runs the product's entry points through the test-only probe library (tests/_pc_probe.py), asserts the traced
dispatch (path, preparation launches, forward kernel instance, where the logits were finished and the cross-entropy was
taken, backward activation form, dX / dW forms, reduce tail) and then compares every stage, elementwise under the
bounds derived in tests/_pc_probe.py, with float64 computed from THE TENSORS THAT STAGE'S KERNEL READ:
  * the operand images in the workspace (WcatT / Wcat2 / bcat, or the padded [Wt | Wa] and ba) with the bf16-rounded
    parameters, exactly; the keep-bit map with `cof.dropout_mask` packed LSB-first, exactly (after a tagged step: the
    NEXT step's mask, and the tag says so); the materialised dropout(X), exactly;
  * Z (where the kernel stores it) and T from X, the operand roundings and the mask; att from the kernel's own Z (or,
    behind the folded forward kernel, from the float64 Z under Z's bound); logits from the kernel's own att and T; loss,
    G, probs, pred from the kernel's own logits;
  * dT / dZ (read out of the workspace) from the kernel's own G, att and T -- the relu gate is `att > 0` of that
    tensor --; dbt / dba from the same; dWt, dWa, dX, dXatt from the STORED dT / dZ and the mask;
  * the device-side dropout counter after the call.
Every input, output and the whole workspace sits in a NaN-guarded allocation: outputs finite, no guard element
changed.  Every case runs twice and repeats bit for bit; one-call steps equal the separate entry points bit for bit.
No case, element or stage is skipped or masked.

Inputs (positive-mean recipe, as tests/test_pose_paths_gpu.py): X = relu(U(-0.25, 1)) * rowscale U(0.5, 1.5);
Wa = U(-0.25, 1) / Ca, Wt = U(-0.25, 1) / C; bt = 0.1 N(0, 1); ba = 0.1 N(0, 1), or under relu attention
-median_r (Xatt Wa)[r, k] * U(0.9, 1.1) so that about half of the gates are open (25 % .. 75 % asserted);
G (separate entry points) = U(-0.25, 1) / N; labels (one-call steps) = (n // 2) mod K: two images per class, so that no
column of G = (softmax - onehot) / N sums to zero over the batch -- under the spatial softmax sum_p att = 1 and
dbt[k] = sum_n G[n, k] / P exactly, which labels n mod K cancel to rounding at N = K = 2 (softmax ~ 1 / 2).
"""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests import _pc_probe as pc
from tests._m1_probe import Bnd, C_ACC, EPS32, U_BF16

pytestmark = pytest.mark.gpu

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
TDT = {F32: torch.float32, BF16: torch.bfloat16}
ACT_CODE = {'id': 0, 'relu': 1, 'softmax': 2}
ACT_FLAG = {'id': 0, 'relu': cof.APA_FLAG_RELU_ATT, 'softmax': cof.APA_FLAG_SOFTMAX_ATT}
SEED, OFFSET = 1234, 5
ZB_MAX_C, DX_MAXU, DX_MAXIMG = 8192, 16, 5      # csrc/apa_pc_fused.hip


def case(name, N, P, C, K, *, Ca=None, dt=BF16, act='id', train=False, keep=0.5, entry='sep', rng='value', wimg=False,
         topdown=False, mis=(), pre=None, wide=None, **expect):
    """Ca=None: Xatt is X itself (else a separate [R, Ca] tensor); entry: sep (fwd_ex + bwd_ex, G given) / step
    (apa_attn_head_train_step_ex) / eval (apa_attn_head_eval_step); rng: value / device / external; wimg:
    APA_FLAG_WEIGHT_IMAGES after apa_per_class_weight_images; mis: {buffer: element offset}; pre (tagged steps): what
    happened on the workspace before the step -- fresh / believed (the previous step, offset - 1) / jump (a step three
    offsets back) / foreign (the previous step, then a separate backward call of another offset); wide: does the wide
    bf16 kernel serve the one-product dX (asserted against gemm_bf16_wide_serves on the device)."""
    return dict(name=name, N=N, P=P, C=C, K=K, Ca=Ca, dt=dt, act=act, train=train, keep=keep, entry=entry, rng=rng,
                wimg=wimg, topdown=topdown, mis=dict(mis), pre=pre, wide=wide, expect=expect)


def expected(c):
    """The trace of a case, transcribed from the dispatch conditions of pc_forward / pc_backward (apa_pc.hip) and
    the pc_fused_* host functions (apa_pc_fused.hip) -- not read back from a run."""
    N, P, C, K, dt, act = c['N'], c['P'], c['C'], c['K'], c['dt'], ACT_CODE[c['act']]
    Ca = C if c['Ca'] is None else c['Ca']
    bf, train, entry, wimg = dt == BF16, c['train'] and c['keep'] < 1.0, c['entry'], c['wimg']
    if entry == 'eval':
        train = False
    step = entry == 'step'
    esz = 2 if bf else 4
    x16 = (c['mis'].get('X', 0) * esz) % 16 == 0
    dx16 = (c['mis'].get('dX', 0) * esz) % 16 == 0
    same = c['Ca'] is None
    fused = (bf and same and 1 <= K <= 64 and C % 256 == 0 and C <= ZB_MAX_C and x16 and c['rng'] != 'external')
    Kp = (K + 63) // 64 * 64 if bf else (K + 7) // 8 * 8
    e = {}
    if fused:
        dxs = act != 2 and P >= 32
        fold = act != 2 and not c['topdown'] and P >= 32
        tagged = train and wimg and step
        e.update(path_fwd='fused', zt=1, zt_train=int(train), zt_fold=int(fold), check_tag=int(tagged),
                 topdown=int(c['topdown']))
        e['prep_fwd'] = 'none' if tagged else {(1, 1): 'both', (1, 0): 'weights', (0, 1): 'bits', (0, 0): 'none'}[
            (int(not wimg), int(train))]
        xent_here = step and 4 <= K <= 64
        if fold:
            e['fwd_act'] = 'folded'
            e['logits'] = 'dx' if xent_here and dxs else 'finish'
            e['xent'] = 'dx' if xent_here and dxs else 'own' if step else 'none'
        else:
            e.update(fwd_act='bf16', fwd_act_xe=int(xent_here), logits='fwd_act')
            e['xent'] = 'fwd_act' if xent_here else 'own' if step else 'none'
        if entry == 'eval':
            e['xent'] = 'own'
            return e
        e['path_bwd'] = 'fused'
        e['prep_bwd'] = 'none' if step else {(1, 1): 'both', (1, 0): 'weights', (0, 1): 'bits', (0, 0): 'none'}[
            (int(not wimg), int(train))]
        bump = int(train and c['rng'] == 'device')
        e.update(dw='fused', tail='dw_tail', rng_bump=bump, next_bits=int(train and wimg and step),
                 aux=int(step and e['xent'] != 'own'))
        if dxs:
            e.update(dx='fused', bwd_act='folded', tail_nrows=(N * P + 127) // 128)
        else:
            ps = 1 if act == 2 else None
            e.update(dx='mid_gemm' if train else 'plain_gemm', bwd_act='bf16', ldg=128)
            if ps:
                e.update(ps=1, tail_nrows=N)
        return e
    fast = bf and C % 8 == 0 and x16
    cat = fast and Ca == C
    e.update(path_fwd='generic', cat=int(cat), fast=int(fast), topdown=int(c['topdown']),
             fwd_act='bf16' if bf else 'f32', logits='fwd_act')
    e['pad_segs_fwd'] = 0 if wimg else 3 if fast else 2
    e['pad_drop_fwd'] = int(fast and train)
    e['pad_fwd'] = int(e['pad_segs_fwd'] > 0 or e['pad_drop_fwd'])
    e['t_drop_a'] = int(train and not fast)
    deferred = step and 4 <= K <= 1024
    if entry == 'eval':
        e['xent'] = 'own'
        return e
    reuse = step and fast
    e.update(path_bwd='generic', reuse_fwd=int(reuse), bwd_act='bf16' if bf else 'f32',
             ldg=2 * Kp if cat else Kp, dw='twin_gemm', tail='colsum', rng_bump=int(train and c['rng'] == 'device'),
             xent='bwd_act' if deferred else 'own' if step else 'none', aux=int(deferred),
             dw_drop_a=2 if (train and not fast) else 0)
    e['pad_segs_bwd'] = 0 if (reuse or wimg) else 2
    e['pad_drop_bwd'] = int(fast and train and not reuse)
    e['pad_bwd'] = int(e['pad_segs_bwd'] > 0 or e['pad_drop_bwd'])
    one = cat and same and bool(c['wide']) and dx16
    if one:
        e.update(dx='wide', mid_bits=int(train), g_dx_kind='wide')
    else:
        e.update(dx='two', dx_drop_c=int(train), wa_to='dx_beta1' if same else 'dxatt')
    if not bf or Ca != C:
        e.update(g_z_twin='serial', g_dwt_twin='serial')       # fp32 never shares a launch; Ca != C: shapes differ
    return e


# Literal `expect` values are read off the same conditions by hand for the values the case is in the table for.
CASES = [
    # ---- fused path (bf16, Xatt == X, K <= 64, C % 256 == 0, C <= 8192)
    # the shipped HMDB-51 step: N = 32, 14 x 14 x 2048, K = 51; 64 units in 5 channel ranges of 13, 13, 13, 13, 12
    case('f_ship_k51_train_step', 32, 196, 2048, 51, train=True, entry='step', path_fwd='fused', zt_fold=1, zt_train=1,
         prep_fwd='both', prep_bwd='none', logits='dx', xent='dx', dx='fused', upb=13, dx_splits=5, rbs=49, dw='fused',
         dw_S=14, dw_ctiles=16, tail='dw_tail', aux=1, next_bits=0, check_tag=0),
    case('f_ship_k51_relu_eval_entry', 32, 196, 2048, 51, act='relu', entry='eval', path_fwd='fused', zt_fold=1,
         zt_train=0, prep_fwd='weights', logits='finish', xent='own'),
    # K = 2 (< 4: no in-kernel cross-entropy), C = 256: 8 units, one per block (upb = 1); R = 96 < 128.  (K = 1 cannot
    # reach this family: a call with K = 1 has M == 1 and every entry point hands it to the M == 1 path, apa_capi.hip.)
    case('f_k2_c256_p32_id_eval_sep', 3, 32, 256, 2, path_fwd='fused', zt_fold=1, logits='finish', xent='none',
         dx='fused', upb=1, dx_splits=8, rbs=1, dw_S=2, prep_bwd='weights'),
    # K = 3, C = 768 (6 k tiles: chunk swizzle off), P = 33: R = 264, row block 1 touches DX_MAXIMG = 5 images and the
    # 32-row forward blocks straddle two images at every offset; K < 4: the step's cross-entropy is its own launch
    case('f_k3_c768_p33_relu_train_step', 8, 33, 768, 3, act='relu', train=True, entry='step', zt_fold=1,
         logits='finish', xent='own', dx='fused', aux=0, rbs=3),
    # K = 4: the smallest K whose cross-entropy is taken in the dX kernel; evaluation-mode step (no dropout)
    case('f_k4_c256_p36_relu_step_notrain', 2, 36, 256, 4, act='relu', entry='step', zt_train=0, logits='dx', xent='dx',
         prep_fwd='weights', aux=1, rng_bump=0),
    case('f_k21_c4096_p49_id_train_sep_device_keep07', 3, 49, 4096, 21, train=True, keep=0.7, rng='device',
         prep_fwd='both', prep_bwd='both', zt_train=1, zt_fold=1, logits='finish', dx='fused', rng_bump=1),
    # C = 8192 = ZB_MAX_C; R = 32 < 64: one k tile, the dW splits are limited to 1
    case('f_k63_c8192_p32_id_eval_sep_r32', 1, 32, 8192, 63, zt_fold=1, dx='fused', dw_S=1, dw_ctiles=64, rbs=1),
    # C = 8192, R = 1960: 16 row blocks -> 16 channel ranges of upb = 16 = DX_MAXU units
    case('f_k51_c8192_p196_id_train_sep_upb16', 10, 196, 8192, 51, train=True, dx='fused', upb=16,
         dx_splits=16, rbs=16),
    case('f_k64_c2048_p225_relu_train_sep', 2, 225, 2048, 64, act='relu', train=True, zt_fold=1, dx='fused'),
    # P = 25 < 32: no fold, no fused dX -> pc_fwd_act_kernel / pc_bwd_act_kernel<bf16_t> + the mid-dropout GEMM;
    # R = 100, and R = 25 < 32
    case('f_k51_c2048_p25_id_train_sep', 4, 25, 2048, 51, train=True, zt_fold=0, fwd_act='bf16', logits='fwd_act',
         bwd_act='bf16', dx='mid_gemm', ldg=128, tail='dw_tail'),
    case('f_k51_c2048_p25_relu_step_notrain_r25', 1, 25, 2048, 51, act='relu', entry='step', zt_fold=0, fwd_act_xe=1,
         xent='fwd_act', dx='plain_gemm', aux=1),
    case('f_k51_c2048_p196_softmax_train_step', 2, 196, 2048, 51, act='softmax', train=True, entry='step', zt_fold=0,
         fwd_act_xe=1, xent='fwd_act', bwd_act='bf16', ps=1, dx='mid_gemm', tail_nrows=2, aux=1),
    case('f_k51_c2048_p49_softmax_eval_sep', 3, 49, 2048, 51, act='softmax', zt_fold=0, dx='plain_gemm', ps=1),
    case('f_k2_c256_p25_softmax_step_notrain', 2, 25, 256, 2, act='softmax', entry='step', fwd_act_xe=0, xent='own',
         aux=0),
    # the TopDownAttention copy is requested: the activation pass keeps its own launch
    case('f_k51_c2048_p196_topdown_eval_sep', 2, 196, 2048, 51, topdown=True, zt_fold=0, fwd_act='bf16', topdown_t=1,
         logits='fwd_act', dx='fused'),
    # ---- caller-kept weight images (APA_FLAG_WEIGHT_IMAGES)
    case('f_wimg_eval_sep', 4, 49, 2048, 51, wimg=True, prep_fwd='none', prep_bwd='none'),
    case('f_wimg_train_sep', 4, 49, 2048, 51, wimg=True, train=True, prep_fwd='bits', prep_bwd='bits', check_tag=0),
    # the one-call train step with kept images: no preparation launch; the map is believed iff its tag matches
    case('f_tag_fresh_refused', 4, 49, 2048, 51, wimg=True, train=True, entry='step', pre='fresh', prep_fwd='none',
         check_tag=1, next_bits=1),
    case('f_tag_believed', 4, 49, 2048, 51, wimg=True, train=True, entry='step', pre='believed', check_tag=1,
         next_bits=1, prep_fwd='none', prep_bwd='none'),
    case('f_tag_believed_device_keep07_relu', 4, 49, 2048, 51, wimg=True, train=True, keep=0.7, act='relu',
         entry='step', rng='device', pre='believed', check_tag=1, next_bits=1, rng_bump=1),
    case('f_tag_jump_refused', 4, 49, 2048, 51, wimg=True, train=True, entry='step', pre='jump', check_tag=1),
    case('f_tag_foreign_refused', 4, 49, 2048, 51, wimg=True, train=True, entry='step', pre='foreign', check_tag=1),
    case('f_tag_softmax_believed', 2, 49, 2048, 51, wimg=True, train=True, act='softmax', entry='step',
         pre='believed', check_tag=1, next_bits=1, dx='mid_gemm'),
    # ---- neighbours of the fused path that must take the generic one
    case('g_nb_k65', 2, 49, 2048, 65, train=True, path_fwd='generic', path_bwd='generic', cat=1, fast=1),
    case('g_nb_c8448', 1, 32, 8448, 51, path_fwd='generic', cat=1),
    case('g_nb_c384', 2, 36, 384, 51, train=True, path_fwd='generic', cat=1),
    case('g_nb_xatt_separate_same_width', 2, 36, 256, 51, Ca=256, train=True, path_fwd='generic', cat=1,
         dx='two', wa_to='dxatt'),
    case('g_nb_ca_differs', 2, 36, 256, 51, Ca=128, path_fwd='generic', cat=0, fast=1, wa_to='dxatt',
         g_z_twin='serial'),
    case('g_nb_rng_external', 2, 36, 256, 51, train=True, rng='external', path_fwd='generic', cat=1, pad_drop_fwd=1),
    # ---- generic path, bf16
    # the shipped K = 393 step (N = 32, 14 x 14 x 2048): the wide kernel's one-product dX with the mid-contraction mask;
    # 7 class groups x 32 images: ps = 2
    case('g_ship_k393_train_step', 32, 196, 2048, 393, train=True, entry='step', wide=True, path_fwd='generic', cat=1,
         fast=1, pad_segs_fwd=3, pad_drop_fwd=1, reuse_fwd=1, pad_bwd=0, xent='bwd_act', dx='wide', mid_bits=1, ps=2,
         tail='colsum', tail_nrows=64, aux=1),
    case('g_ship_k393_eval_sep_dx_misaligned', 32, 196, 2048, 393, wide=True, mis={'dX': 4}, dx='two',
         wa_to='dx_beta1', pad_segs_bwd=2),
    case('g_bf16_k130_softmax_train_sep', 3, 49, 256, 130, act='softmax', train=True, ps=1, dx='two', dx_drop_c=1,
         pad_drop_bwd=1),
    case('g_bf16_k2_relu_eval_sep_ps8', 2, 196, 128, 2, act='relu', ps=8, tail_nrows=16),
    # K = 1000: not a multiple of 8; Kp = 1024, 2 Kp / 64 = 32 k tiles: the wide kernel refuses
    case('g_bf16_k1000_train_step', 2, 36, 128, 1000, train=True, entry='step', xent='bwd_act', dx='two'),
    case('g_ship_k1000_eval_sep_wide_refuses', 32, 196, 2048, 1000, wide=False, cat=1, dx='two', wa_to='dx_beta1'),
    case('g_bf16_k1024_relu_step_notrain', 2, 16, 64, 1024, act='relu', entry='step', xent='bwd_act', ps=1),
    # K = 1025: past the deferred cross-entropy
    case('g_bf16_k1025_train_step', 2, 16, 64, 1025, train=True, entry='step', xent='own', aux=0),
    # C % 8 != 0: no DMA operands -- scalar staging, the mask applied by the stagers (drop_a 1 / 2) and on dX (drop_c)
    case('g_bf16_c100_k65_train_sep', 2, 36, 100, 65, train=True, cat=0, fast=0, pad_segs_fwd=2, pad_drop_fwd=0,
         t_drop_a=1, dw_drop_a=2, dx='two', dx_drop_c=1),
    case('g_bf16_ca96_k130_relu_train_step', 3, 25, 256, 130, Ca=96, act='relu', train=True, entry='step', cat=0,
         fast=1, wa_to='dxatt', reuse_fwd=1),
    case('g_bf16_wimg_k65_train_sep', 2, 49, 256, 65, wimg=True, train=True, pad_segs_fwd=0, pad_drop_fwd=1,
         pad_segs_bwd=0, pad_drop_bwd=1),
    case('g_bf16_wimg_k65_eval_sep', 2, 49, 256, 65, wimg=True, pad_fwd=0, pad_bwd=0),
    case('g_bf16_k65_eval_entry', 2, 36, 256, 65, entry='eval', xent='own'),
    # ---- generic path, fp32
    case('g_f32_k2_id_eval_sep', 2, 49, 64, 2, dt=F32, fwd_act='f32', bwd_act='f32', cat=0, fast=0, dx='two'),
    case('g_f32_k51_relu_train_sep_device', 3, 36, 96, 51, dt=F32, act='relu', train=True, keep=0.7, rng='device',
         t_drop_a=1, dw_drop_a=2, dx_drop_c=1, rng_bump=1),
    case('g_f32_k65_softmax_train_step', 2, 49, 64, 65, dt=F32, act='softmax', train=True, entry='step',
         xent='bwd_act', reuse_fwd=0, pad_segs_bwd=2),
    case('g_f32_k393_ca48_train_sep', 2, 25, 64, 393, dt=F32, Ca=48, train=True, wa_to='dxatt'),
    case('g_f32_k1025_eval_entry', 2, 16, 32, 1025, dt=F32, entry='eval', xent='own'),
    case('g_f32_k51_topdown_eval_sep', 2, 36, 64, 51, dt=F32, topdown=True, topdown_t=1),
]

# Buffers at the offsets the dispatcher itself tests for and routes to the scalar-staging forms.
MIS_CASES = [
    # X 2 bytes off 16-byte alignment: a fused-path shape falls to the generic path without cat / fast
    case('mis_x2_k51_train_sep', 2, 36, 256, 51, train=True, mis={'X': 1}, path_fwd='generic', cat=0, fast=0,
         t_drop_a=1, dw_drop_a=2, dx='two', dx_drop_c=1),
    case('mis_x2_k65_relu_train_step', 2, 36, 256, 65, act='relu', train=True, entry='step', mis={'X': 1}, cat=0,
         fast=0, reuse_fwd=0, xent='bwd_act'),
    case('mis_dx8_k65_train_sep', 2, 49, 256, 65, train=True, mis={'dX': 4}, cat=1, dx='two', wa_to='dx_beta1'),
]


# ------------------------------------------------------------------------------------------ figures for the profile
FIGS = []


def _check(c, got, b, stage, **kw):
    """mp.check, after recording max |err| / bound and max bound / max |ref| of the stage."""
    g = got.double().reshape(b.ref.shape)
    tol = mp.tolerance(b, bool(kw.get('bf16')))      # the tolerance mp.check asserts
    nz = tol > 0
    r_err = float(((g - b.ref).abs()[nz] / tol[nz]).max()) if bool(nz.any()) else 0.0
    if bool(((g - b.ref).abs()[~nz] > 0).any()):
        r_err = float('inf')
    r_bnd = float(b.err.max() / b.ref.abs().max()) if float(b.ref.abs().max()) > 0 else 0.0
    FIGS.append((c['name'], stage, r_err, r_bnd))
    print('PC_FIG {} {} err/bound {:.4f} bound/ref {:.3e}'.format(c['name'], stage, r_err, r_bnd))
    mp.check(got, b, '{}: {}'.format(c['name'], stage), **kw)


def _exact(c, got, ref, stage):
    """bit-for-value equality (images, bit maps, exact activations, zero pads)."""
    assert got.shape == ref.shape, '{}: {} shape {} vs {}'.format(c['name'], stage, tuple(got.shape), tuple(ref.shape))
    bad = got != ref
    n = int(bad.sum())
    FIGS.append((c['name'], stage + ' (exact)', 0.0 if n == 0 else float('inf'), 0.0))
    assert n == 0, '{}: {}: {} of {} elements differ (first flat {})'.format(
        c['name'], stage, n, bad.numel(), int(bad.reshape(-1).nonzero()[0]))


def _prod(a, b, L, extra=0.0, scale=1.0, add=None):
    """(a @ b) * scale accumulated in fp32 over L terms (+ addends inside the same chain)."""
    ref, mag = (a @ b) * scale, (a.abs() @ b.abs()) * abs(scale)
    for t in add or ():
        ref, mag = ref + t, mag + t.abs()
    return Bnd(ref, (C_ACC * (L + 8) * EPS32 + extra) * mag)


def _pack(mask):
    """{0,1} uint8 [n] -> bytes, LSB first."""
    w = 1 << torch.arange(8, device=mask.device, dtype=torch.int32)
    return (mask.reshape(-1, 8).to(torch.int32) * w).sum(dim=1).to(torch.uint8)


# ------------------------------------------------------------------------------------------ one case on the device
class _Run:
    def __init__(self, c, dev, lib):
        self.c, self.dev, self.lib = c, dev, lib
        N, P, C, K, dt = c['N'], c['P'], c['C'], c['K'], c['dt']
        Ca = C if c['Ca'] is None else c['Ca']
        R = N * P
        self.R, self.Ca, tdt = R, Ca, TDT[dt]
        self.bf = dt == BF16
        self.train = c['train'] and c['keep'] < 1.0 and c['entry'] != 'eval'
        gen = torch.Generator(device=dev)
        gen.manual_seed(zlib.crc32(c['name'].encode()))
        rnd = lambda *s: torch.rand(*s, generator=gen, device=dev, dtype=torch.float64)
        ro = lambda *s: rnd(*s) * 1.25 - 0.25
        rn = lambda *s: torch.randn(*s, generator=gen, device=dev, dtype=torch.float64) * 0.1
        mis = c['mis']
        self.b = {}

        def buf(name, rows, cols, dtype, data=None):
            g = gp.Guarded(rows, cols, cols, dtype, dev, off=mis.get(name, 0), data=data)
            self.b[name] = g
            return g

        X = (torch.relu(ro(R, C)) * (0.5 + rnd(R, 1))).to(tdt)
        buf('X', R, C, tdt, X)
        Xa = X
        if c['Ca'] is not None:
            Xa = (torch.relu(ro(R, Ca)) * (0.5 + rnd(R, 1))).to(tdt)
            buf('Xatt', R, Ca, tdt, Xa)
        Wa = (ro(Ca, K) / Ca).float()
        if c['act'] == 'relu':
            Wav = Wa.to(torch.bfloat16) if self.bf else Wa
            ba = (-(Xa.double() @ Wav.double()).median(dim=0).values * (0.9 + 0.2 * rnd(K))).float()
        else:
            ba = rn(K).float()
        buf('Wa', Ca, K, torch.float32, Wa)
        buf('ba', 1, K, torch.float32, ba)
        buf('Wt', C, K, torch.float32, (ro(C, K) / C).float())
        buf('bt', 1, K, torch.float32, rn(K).float())
        self.labels = ((torch.arange(N, device=dev) // 2) % K).to(torch.int64)
        self.outs = ['logits', 'att', 'Tsave']
        buf('logits', N, K, torch.float32)
        buf('att', R, K, torch.float32)
        buf('Tsave', R, K, torch.float32)
        if c['topdown']:
            buf('topdown', R, K, tdt)
            self.outs.append('topdown')
        if c['entry'] != 'eval':
            for name, rows, cols, t in (('dX', R, C, tdt), ('dWa', Ca, K, torch.float32), ('dba', 1, K, torch.float32),
                                        ('dWt', C, K, torch.float32), ('dbt', 1, K, torch.float32)):
                buf(name, rows, cols, t)
                self.outs.append(name)
            if c['Ca'] is not None:
                buf('dXatt', R, Ca, tdt)
                self.outs.append('dXatt')
            buf('G', N, K, torch.float32, (ro(N, K) / N).float() if c['entry'] == 'sep' else None)
            if c['entry'] == 'step':
                self.outs.append('G')
        if c['entry'] in ('step', 'eval'):
            buf('loss', 1, N + 1, torch.float32)
            self.outs.append('loss')
        if c['entry'] == 'eval':
            buf('probs', N, K, torch.float32)
            self.outs.append('probs')
            self.pred = torch.full((N,), -1, dtype=torch.int64, device=dev)
        self.plan = pc.plan(N, P, C, Ca, K, dt)
        self.ws_bytes = int(lib.apa_attn_pool_workspace_bytes(N, P, C, Ca, K, K, 0))
        assert self.ws_bytes >= self.plan['total'] and self.plan['R'] == R
        buf('ws', 1, (self.ws_bytes + 3) // 4, torch.float32)
        self.counter = torch.tensor([OFFSET], dtype=torch.int64, device=dev) if c['rng'] == 'device' else None
        self.ext = None
        if c['rng'] == 'external':
            self.ext = cof.pack_keep_mask(cof.dropout_mask((R, C), c['keep'], SEED, OFFSET, device=dev), device=dev)
        self.flags = ACT_FLAG[c['act']] | (cof.APA_FLAG_TRAIN if c['train'] else 0) | \
            (cof.APA_FLAG_WEIGHT_IMAGES if c['wimg'] else 0)
        for g in self.b.values():
            g.snapshot()

    def p(self, name):
        return self.b[name].ptr if name in self.b else None

    def restore(self):
        for g in self.b.values():
            g.restore()
        if self.counter is not None:
            self.counter.fill_(OFFSET)

    def check_guards(self):
        for name, g in self.b.items():
            g.check_guards('{}: {}'.format(self.c['name'], name))

    def raw(self, off, nbytes):
        return self.b['ws'].view.view(-1).view(torch.uint8)[off:off + nbytes]

    def bits(self):
        out = {k: self.b[k].bits() for k in self.outs}
        if self.c['entry'] == 'eval':
            out['pred'] = self.pred.clone()
        return out

    def _ok(self, rc, what):
        assert rc == 0, '{}: {} returned {} ({})'.format(self.c['name'], what, rc, self.lib.apa_last_error().decode())

    def key(self, offset=OFFSET):
        """(seed, offset, flags) as the C ABI takes them."""
        if self.ext is not None:
            return self.ext.bits.data_ptr(), 0, self.flags | cof.APA_FLAG_RNG_EXTERNAL
        if self.counter is not None:
            self.counter.fill_(offset)
            return SEED, self.counter.data_ptr(), self.flags | cof.APA_FLAG_RNG_DEVICE
        return SEED, offset, self.flags

    def dims(self):
        c = self.c
        return c['N'], c['P'], c['C'], self.Ca, c['K'], c['K']

    def head(self):
        p = self.p
        return p('X'), (p('Xatt') if self.c['Ca'] is not None else p('X')), p('Wa'), p('ba'), p('Wt'), p('bt')

    def fwd(self, trace=None, offset=OFFSET):
        seed, off, flags = self.key(offset)
        p, c = self.p, self.c
        self._ok(self.lib.apa_probe_pc_fwd_ex(
            ctypes.addressof(trace) if trace is not None else None, None, *self.head(), p('logits'), p('att'),
            p('Tsave'), None, p('topdown'), p('ws'), self.ws_bytes, *self.dims(), flags, c['keep'], seed, off, c['dt'],
            gp.stream_ptr()), 'fwd')

    def bwd(self, trace=None, offset=OFFSET, keep_counter=False):
        if keep_counter and self.counter is not None:
            seed, off, flags = SEED, self.counter.data_ptr(), self.flags | cof.APA_FLAG_RNG_DEVICE
        else:
            seed, off, flags = self.key(offset)
        p, c = self.p, self.c
        self._ok(self.lib.apa_probe_pc_bwd_ex(
            ctypes.addressof(trace) if trace is not None else None, None, *self.head(), p('att'), p('Tsave'), None,
            p('G'), p('dX'), p('dXatt'), p('dWa'), p('dba'), p('dWt'), p('dbt'), p('ws'), self.ws_bytes, *self.dims(),
            flags, c['keep'], seed, off, c['dt'], gp.stream_ptr()), 'bwd')

    def step(self, trace=None, offset=OFFSET):
        seed, off, flags = self.key(offset)
        p, c = self.p, self.c
        self._ok(self.lib.apa_probe_pc_train_step_ex(
            ctypes.addressof(trace) if trace is not None else None, None, *self.head(), self.labels.data_ptr(), 1.0, 1.0,
            p('logits'), p('att'), p('Tsave'), None, p('loss'), p('G'), p('dX'), p('dXatt'), p('dWa'), p('dba'),
            p('dWt'), p('dbt'), p('ws'), self.ws_bytes, *self.dims(), flags, c['keep'], seed, off, c['dt'],
            gp.stream_ptr()), 'step')

    def weight_images(self, trace=None):
        c = self.c
        p = self.p
        n = ctypes.c_int(0)
        maps = (cof.ApaWeightImage * cof.APA_WIMG_MAX)()
        self._ok(self.lib.apa_probe_pc_weight_images(
            ctypes.addressof(trace) if trace is not None else None, p('Wa'), p('ba'), p('Wt'), p('bt'), p('ws'),
            self.ws_bytes, c['N'], c['P'], c['C'], self.Ca, c['K'], c['dt'], ctypes.addressof(maps), ctypes.byref(n),
            gp.stream_ptr()), 'weight_images')
        return n.value

    def run(self):
        """-> the merged trace of the case's own call(s)."""
        c = self.c
        tw = pc.PcTrace()
        self.nmaps = None
        if c['wimg']:
            self.nmaps = self.weight_images(tw)
            self.tw = tw.as_dict()
        if c['pre'] in ('believed', 'foreign'):
            self.step(offset=OFFSET - 1)
        elif c['pre'] == 'jump':
            self.step(offset=OFFSET - 3)
        if c['pre'] == 'foreign':       # another caller's backward on the same workspace: its own bits, its own tag
            self.b['G'].restore()
            self.b['G'].view.fill_(0.01)
            self.bwd(offset=OFFSET + 40)
        if c['pre']:
            for k in self.outs:         # what the earlier calls wrote must not pass for this call's output
                self.b[k].restore()
        t1, t2 = pc.PcTrace(), pc.PcTrace()
        if c['entry'] == 'step':
            self.step(t1)
            return pc.merge(t1)
        if c['entry'] == 'eval':
            p = self.p
            self._ok(self.lib.apa_probe_pc_eval_step(
                ctypes.addressof(t1), *self.head(), self.labels.data_ptr(), p('logits'), p('att'), p('Tsave'), None,
                p('loss'), p('probs'), self.pred.data_ptr(), p('ws'), self.ws_bytes, *self.dims(), self.flags,
                c['dt'], gp.stream_ptr()), 'eval')
            return pc.merge(t1)
        self.fwd(t1)
        self.bwd(t2, keep_counter=True)
        return pc.merge(t1, t2)


# ------------------------------------------------------------------------------------------ float64 stages
def _check_case(c, r, trace):
    N, P, C, K, R, Ca, bf = c['N'], c['P'], c['C'], c['K'], r.R, r.Ca, r.bf
    dev = r.dev
    pl = r.plan
    Kp = pl['Kp']
    tdt = TDT[c['dt']]
    esz = 2 if bf else 4
    v = lambda name: r.b[name].view.double()
    rnd16 = lambda t: t.to(torch.bfloat16).double() if bf else t.double()   # the operand rule of tests/_gemm_probe.py
    fusedp = trace['path_fwd'] == 'fused'
    train, keep = r.train, c['keep']
    act = c['act']
    has_bwd = c['entry'] != 'eval'
    X = v('X')
    Xa = v('Xatt') if c['Ca'] is not None else X
    Wa_op, Wt_op = rnd16(r.b['Wa'].view), rnd16(r.b['Wt'].view)
    ba, bt = v('ba').view(-1), v('bt').view(-1)
    ik32 = torch.tensor(np.float32(1.0) / np.float32(keep), dtype=torch.float32, device=dev)
    tagged = bool(trace.get('check_tag'))

    # ---- operand images
    def padded(W, rows):                 # [rows][K] fp32 -> [rows][Kp or 64] in the image's dtype, zero padded
        out = torch.zeros(rows, 64 if fusedp else Kp, dtype=torch.bfloat16 if bf else torch.float32, device=dev)
        out[:, :K] = W.to(out.dtype)
        return out
    Wa_p, Wt_p = padded(r.b['Wa'].view, Ca), padded(r.b['Wt'].view, C)
    if fusedp:
        wcatT = r.raw(pl['WcatT'], 128 * C * 2).view(torch.bfloat16).view(C // 64, 128, 64)
        exp = torch.cat([Wa_p.view(C // 64, 64, 64).permute(0, 2, 1), Wt_p.view(C // 64, 64, 64).permute(0, 2, 1)],
                        dim=1)
        _exact(c, wcatT.float(), exp.float(), 'WcatT')
        wcat2 = r.raw(pl['Wcat2'], C * 128 * 2).view(torch.bfloat16).view(C, 128)
        _exact(c, wcat2.float(), torch.cat([Wt_p, Wa_p], dim=1).float(), 'Wcat2')
        bcat = r.raw(pl['bcat'], 512).view(torch.float32)
        eb = torch.zeros(128, dtype=torch.float32, device=dev)
        eb[:K], eb[64:64 + K] = r.b['ba'].view.view(-1), r.b['bt'].view.view(-1)
        _exact(c, bcat, eb, 'bcat')
    else:
        wdt = torch.bfloat16 if bf else torch.float32
        if trace['cat']:
            img = r.raw(pl['off_wtp'], C * 2 * Kp * 2).view(torch.bfloat16).view(C, 2 * Kp)
            _exact(c, img.float(), torch.cat([Wt_p, Wa_p], dim=1).float(), '[Wt, Wa] image')
        else:
            img = r.raw(pl['off_wap'], Ca * Kp * esz).view(wdt).view(Ca, Kp)
            _exact(c, img.float(), Wa_p.float(), 'Wa image')
            if has_bwd or trace['fast']:
                img = r.raw(pl['off_wtp'], C * Kp * esz).view(wdt).view(C, Kp)
                _exact(c, img.float(), Wt_p.float(), 'Wt image')
        bap = r.raw(pl['off_bap'], Kp * 4).view(torch.float32)
        eb = torch.zeros(Kp, dtype=torch.float32, device=dev)
        eb[:K] = r.b['ba'].view.view(-1)
        _exact(c, bap, eb, 'ba image')

    # ---- keep bits, dropout(X)
    mask = None
    A_t, t_scale = X, 1.0                # the A operand of the T / dWt products and the scale on their accumulators
    if train:
        m8 = cof.dropout_mask((R, C), keep, SEED, OFFSET, device=dev)
        mask = m8.double()
        frac = float(mask.mean())
        assert abs(frac - keep) < 0.05, '{}: {:.1%} of the elements kept'.format(c['name'], frac)
        if fusedp:
            got = r.raw(pl['maskbits'], R * C // 8)
            tag = r.raw(pl['bits_tag'], 40).view(torch.int64)
            thr = (gp.keep_thresh(keep) << 32) | 0x6b656570
            if tagged:                   # the step's last launch left the NEXT step's map behind, and says so
                nxt = cof.dropout_mask((R, C), keep, SEED, OFFSET + 1, device=dev)
                _exact(c, got, _pack(nxt), 'keep bits of the next step')
                assert tag.tolist() == [SEED, OFFSET + 1, thr, R * C // 8, OFFSET], tag.tolist()
            else:
                _exact(c, got, _pack(m8), 'keep bits')
                assert tag.tolist()[:4] == [SEED, OFFSET, thr, R * C // 8], tag.tolist()
            A_t, t_scale = X * mask, 1.0 / keep
        else:
            xd32 = (r.b['X'].view.float() * ik32) * m8.float()        # fl32(x * fl32(1 / keep)), dropped -> 0
            if trace['fast']:
                _exact(c, r.raw(pl['off_bits'], R * C // 8), _pack(m8), 'keep bits')
                xd = r.raw(pl['off_xd'], R * C * 2).view(torch.bfloat16).view(R, C)
                _exact(c, xd.float(), xd32.to(torch.bfloat16).float(), 'dropout(X)')
                A_t = xd.double()        # the products read the kernel's own tensor
            else:
                A_t = rnd16(xd32)        # formed by the stager (drop_a), rounded to bf16 on the bf16 MFMA

    # ---- Z = Xatt . Wa + ba, T = dropout(X) . Wt + bt
    zb = _prod(Xa, Wa_op, Ca, add=[ba])
    tb = _prod(A_t, Wt_op, C, extra=2 * EPS32, scale=t_scale, add=[bt])
    _check(c, r.b['Tsave'].view, tb, 'T')
    folded = trace['fwd_act'] == 'folded'
    attk = v('att')
    if not folded:
        ldz = 64 if fusedp else Kp
        Zk = r.raw(pl['off_z'], R * ldz * 4).view(torch.float32).view(R, ldz)
        _check(c, Zk[:, :K], zb, 'Z')
        _exact(c, Zk[:, K:], torch.zeros(R, ldz - K, device=dev), 'Z pad columns')
        zk = Zk[:, :K].double()
        if act == 'softmax':
            a = mp.softmax_p(Bnd(zk.view(N, P, K).permute(0, 2, 1)))
            _check(c, attk.view(N, P, K).permute(0, 2, 1), a, 'att')
        else:
            _exact(c, r.b['att'].view, (torch.relu(Zk[:, :K]) if act == 'relu' else Zk[:, :K]).contiguous(), 'att')
    else:                                # the folded kernel keeps Z in registers: att against the float64 Z
        _check(c, attk, Bnd(torch.relu(zb.ref) if act == 'relu' else zb.ref, zb.err), 'att')
    if act == 'relu':
        frac = float((attk > 0).double().mean())
        assert 0.25 <= frac <= 0.75, '{}: {:.1%} of the relu gates open'.format(c['name'], frac)
    Tk = v('Tsave')                      # everything below reads the kernel's own att and T
    if c['topdown']:
        _exact(c, r.b['topdown'].view.float(), r.b['Tsave'].view.to(tdt).float(), 'topdown')

    # ---- logits = mean_p att * T
    prod = (attk * Tk).view(N, P, K)
    lg = Bnd(prod.sum(1) / P, C_ACC * (P + 8) * EPS32 * prod.abs().sum(1) / P)
    _check(c, r.b['logits'].view, lg, 'logits')

    # ---- loss, G, probs, pred from the kernel's own logits
    lk = v('logits')
    if c['entry'] in ('step', 'eval'):
        pr = torch.softmax(lk, dim=1)
        tol = C_ACC * (K + 16) * EPS32
        lab = r.labels
        lse = torch.logsumexp(lk, dim=1)
        per = lse - lk.gather(1, lab[:, None])[:, 0]
        mag = lse.abs() + lk.abs().amax(dim=1)
        loss = v('loss').view(N + 1)
        _check(c, loss[1:], Bnd(per, tol * mag), 'loss per example')
        _check(c, loss[:1], Bnd(per.mean().reshape(1), (tol * mag).mean().reshape(1) + tol * per.abs().mean()),
               'loss')
        if c['entry'] == 'eval':
            _check(c, r.b['probs'].view, Bnd(pr, tol * pr), 'probs')
            assert torch.equal(r.pred, lk.argmax(dim=1)), 'pred'
            return
        onehot = torch.nn.functional.one_hot(lab, K).double()
        _check(c, r.b['G'].view, Bnd((pr - onehot) / N, tol * (pr + onehot) / N), 'G')
    Gk = v('G')                          # own G

    # ---- dT = (G / P) att, dZ = act'((G / P) T)
    g = (Gk / P).repeat_interleave(P, dim=0)                       # [R, K]
    dT = Bnd(g * attk, 4 * EPS32 * (g * attk).abs())
    dA = g * Tk
    if act == 'softmax':
        corr = (attk * dA).view(N, P, K)
        cs, cm = corr.sum(1, keepdim=True), corr.abs().sum(1, keepdim=True)
        ref = attk.view(N, P, K) * (dA.view(N, P, K) - cs)
        err = attk.view(N, P, K).abs() * (4 * EPS32 * dA.view(N, P, K).abs() + C_ACC * (P + 8) * EPS32 * cm) + \
            2 * EPS32 * ref.abs()
        dZ = Bnd(ref.reshape(R, K), err.reshape(R, K))
    else:
        gate = (attk > 0).double() if act == 'relu' else 1.0
        dZ = Bnd(dA * gate, 4 * EPS32 * (dA * gate).abs())
    if fusedp:
        raw = r.raw(pl['dTdZ'], R * 128 * 2).view(torch.bfloat16).view(R, 128)
        dTk, dZk, padw = raw[:, :K], raw[:, 64:64 + K], [raw[:, K:64], raw[:, 64 + K:]]
    elif trace['cat']:
        raw = r.raw(pl['off_dt'], R * 2 * Kp * 2).view(torch.bfloat16).view(R, 2 * Kp)
        dTk, dZk, padw = raw[:, :K], raw[:, Kp:Kp + K], [raw[:, K:Kp], raw[:, Kp + K:]]
    else:
        a, b = (r.raw(pl[o], R * Kp * esz).view(tdt).view(R, Kp) for o in ('off_dt', 'off_dz'))
        dTk, dZk, padw = a[:, :K], b[:, :K], [a[:, K:], b[:, K:]]
    _check(c, dTk, dT, 'dT', bf16=bf)
    _check(c, dZk, dZ, 'dZ', bf16=bf)
    for w in padw:
        _exact(c, w.float(), torch.zeros_like(w, dtype=torch.float32), 'dT, dZ pad columns')
    dTs, dZs = dTk.double(), dZk.double()            # dW and dX read the STORED values

    # ---- dbt, dba: column sums of the unrounded values
    for name, b in (('dbt', dT), ('dba', dZ)):
        zero = name == 'dba' and act == 'softmax'    # identically zero: the elementwise bound alone
        _check(c, r.b[name].view, Bnd(b.ref.sum(0), C_ACC * (R + 8) * EPS32 * b.ref.abs().sum(0) + b.err.sum(0)), name,
               zero_ref=zero)

    # ---- dWt = dropout(X)^T . dT, dWa = Xatt^T . dZ
    _check(c, r.b['dWt'].view, _prod(A_t.t(), dTs, R, extra=2 * EPS32, scale=t_scale), 'dWt')
    _check(c, r.b['dWa'].view, _prod(Xa.t(), dZs, R), 'dWa', zero_ref=act == 'softmax')

    # ---- dX = (dT . Wt^T) * mask / keep + dZ . Wa^T   (Ca != C or a separate Xatt: the second product is dXatt)
    m = mask / keep if train else 1.0
    p1, p1m = (dTs @ Wt_op.t()) * m, (dTs.abs() @ Wt_op.abs().t()) * m
    p2, p2m = dZs @ Wa_op.t(), dZs.abs() @ Wa_op.abs().t()
    u_out = U_BF16 if bf else EPS32
    if c['Ca'] is None:
        err = (C_ACC * (2 * Kp + 8) + 2) * EPS32 * (p1m + p2m)
        if trace['dx'] == 'two':         # the first product is stored in dX's dtype and read back (beta = 1)
            err = err + u_out * (1 + u_out) * p1.abs()       # (the final rounding acts on the rounded first product)
        _check(c, r.b['dX'].view, Bnd(p1 + p2, err), 'dX', bf16=bf)
    else:
        _check(c, r.b['dX'].view, Bnd(p1, (C_ACC * (Kp + 8) + 2) * EPS32 * p1m), 'dX', bf16=bf)
        _check(c, r.b['dXatt'].view, Bnd(p2, C_ACC * (Kp + 8) * EPS32 * p2m), 'dXatt', bf16=bf)


def _separate_equivalent(c, r):
    """The one-call step's outputs from the separate entry points, as bits."""
    r.restore()
    if c['wimg']:
        r.weight_images()
    r.fwd()
    N, K = c['N'], c['K']
    st = gp.stream_ptr()
    if c['entry'] == 'step':
        r._ok(r.lib.apa_softmax_xent_fwd_bwd(r.p('logits'), r.labels.data_ptr(), r.p('loss'), r.p('G'), None, None, N, K,
                                             1.0, 1.0, st), 'xent')
        r.bwd(keep_counter=True)
    else:
        r._ok(r.lib.apa_softmax_xent_fwd_bwd(r.p('logits'), r.labels.data_ptr(), r.p('loss'), None, r.p('probs'),
                                             r.pred.data_ptr(), N, K, 1.0, 1.0, st), 'xent')
    torch.cuda.synchronize()
    r.check_guards()
    return r.bits()


def _run_case(c, dev):
    lib = pc.load_pc_probe()
    r = _Run(c, dev, lib)
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    for k in r.outs:
        assert torch.isfinite(r.b[k].view.float()).all(), '{}: {} not completely written'.format(c['name'], k)
    exp = expected(c)
    lit = dict(c['expect'])
    if 'topdown_t' in lit:
        lit['topdown'] = lit.pop('topdown_t')
    for k, e in lit.items():             # the hand-written values and the transcription must agree with each other ...
        assert exp.get(k, e) == e, '{}: expect[{}] = {} but the dispatch conditions give {}'.format(
            c['name'], k, e, exp[k])
    exp.update(lit)
    if exp.get('dx') == 'fused' or exp.get('dw') == 'fused':     # geometry: the product's own functions
        geo = pc.geometry(r.R, c['C'])
        for k in ('upb', 'dx_splits', 'rbs') if exp.get('dx') == 'fused' else ():
            exp.setdefault(k, geo[k])
        for k in ('dw_S', 'dw_rows', 'dw_ctiles'):
            exp.setdefault(k, geo[k])
    if exp.get('bwd_act') in ('f32', 'bf16'):
        Kp = r.plan['Kp']
        ps = pc.psplit(c['N'], (Kp + 63) // 64, c['P'], ACT_CODE[c['act']])
        exp.setdefault('ps', ps)
        exp.setdefault('tail_nrows', c['N'] * ps)
    if c['wide'] is not None:
        assert pc.wide_serves(r.R, c['C'], 2 * r.plan['Kp']) == c['wide']
    elif exp.get('path_bwd') == 'generic' and exp.get('cat'):
        assert not pc.wide_serves(r.R, c['C'], 2 * r.plan['Kp']), 'the case table says the wide kernel refuses'
    bad = {k: (trace[k], e) for k, e in exp.items() if trace[k] != e}                    # ... and with the run
    assert not bad, '{}: trace mismatch (got, expected): {} in {}'.format(c['name'], bad, trace)
    if c['wimg']:
        fz = pc.support(c['N'], c['P'], c['C'], r.Ca, c['K'], c['dt'], 0)[0]
        assert r.tw['wimg_fused'] == int(fz) and r.tw['prep_wimg'] == ('weights' if fz else 'none')
        assert r.tw['wimg_cat'] == int(r.bf and r.Ca == c['C'] and c['C'] % 8 == 0)
        assert r.tw['wimg_maps'] == r.nmaps == 3 + (6 if fz else 0)
    if r.counter is not None:
        assert int(r.counter) == OFFSET + (1 if r.train else 0), 'the dropout counter advances once per training step'
    with torch.no_grad():
        _check_case(c, r, trace)
    first = r.bits()
    r.restore()
    trace2 = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    assert trace2 == trace
    second = r.bits()
    for k in first:
        assert torch.equal(first[k], second[k]), '{}: {} differs between two identical calls'.format(c['name'], k)
    if c['entry'] in ('step', 'eval'):
        sep = _separate_equivalent(c, r)
        for k in first:
            assert torch.equal(first[k], sep[k]), '{}: {} differs from the separate entry points'.format(c['name'], k)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_pc_path(gpu, c):
    _run_case(c, gpu)


@pytest.mark.parametrize('c', MIS_CASES, ids=[c['name'] for c in MIS_CASES])
def test_pc_path_misaligned(gpu, c):
    _run_case(c, gpu)


def teardown_module(module):
    """With APA_PC_FIGURES=<path>: the per-stage figures of this run as a table (profiles/r09_pc_paths.md)."""
    path = os.environ.get('APA_PC_FIGURES')
    if path and FIGS:
        with open(path, 'w') as f:
            f.write('| case | stage | max err / bound | bound / max ref |\n|---|---|---|---|\n')
            for name, stage, a, b in FIGS:
                f.write('| {} | {} | {:.3f} | {:.2e} |\n'.format(name, stage, a, b))
