"""Every path of the PoseLogits head (csrc/apa_pose_head.hip) against float64, stage by stage.

Each case runs the product's entry points through the test-only probe library (tests/_pose_probe.py), asserts the
traced dispatch (W1 operand, Pl kernel and instance, backward rows family with its block shape, gradient form,
dW2 / column-sum / dW1 forms, dX accumulation) and then compares every stage, elementwise under the bound derived in
tests/_pose_probe.py, with float64 computed from THE TENSORS THAT STAGE'S KERNEL READ:
  * Ppre from X, the W1 operand and b1;  Pl (and, in the one-call step, att, dPl and the pose loss) from the kernel's
    own Ppre / Pl;
  * dPpre (read out of the workspace) from the kernel's own Ppre -- its gates are `Ppre > 0` of that tensor, so no
    element is ambiguous and none is left out --, dPl, W2 and the external gradient;
  * dW2, db2 (dWa, dba) from own Ppre and dPl (dZ); db1 from the float64 dPpre with its bound carried along;
  * dW1 and dX from the kernel's own dPpre and the W1 operand, with the given dX under beta = 1 and the pooling's
    rank-1 share (read from the pooling workspace) in the one-call step.
Every input, output and workspace sits in a NaN-guarded allocation: outputs finite, no guard element changed.  Every
case runs twice and repeats bit for bit.  No case, element or stage is skipped or masked.

Inputs (positive-mean recipe: |ref| stays of the order of mag, so every bound is below 1 % of max |ref|, which
`check` asserts; verified in float64 alone for the extreme shapes of this table before the first GPU run):
X = relu(U(-0.25, 1)) * rowscale U(0.5, 1.5); W1 = U(-0.25, 1) / C; b1[c] = -median_r (X W1)[r, c] * U(0.9, 1.1) (half of
the gates open: 25 % .. 75 % asserted); W2 = U(-0.25, 1) / Cp; dPl = U(-0.25, 1); ext_row = U(0, 1); ext_col and a dense
ext = U(-0.25, 1).  One-call step: labels all 0 and column 0 of Wt = U(2, 4) / C, so that dz -- and with it dZ, the
rank-1 factor the pose head receives -- has one sign and dWa / dba do not cancel.
"""
import ctypes
import os
import zlib

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests import _pose_probe as pp
from tests._m1_probe import Bnd, C_ACC, EPS32, U_BF16

pytestmark = pytest.mark.gpu

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
TDT = {F32: torch.float32, BF16: torch.bfloat16}
KEEP = 0.5
STEP_K = 51
APA_POSE_WS_FROM_FWD = 2   # include/apa.h


def case(name, N, P, C, Cp, J, *, dt=BF16, form='plain', dpl=True, entry='sep', beta=0, reuse=False, mis=(),
         images=(), train=False, **expect):
    """form: plain / ext (dense dPpre_ext) / rank1; dpl=False: dPl = NULL; beta: accumulate onto a given dX;
    reuse: APA_POSE_WS_FROM_FWD; mis: {buffer: element offset}; images (step): 'w1', 'w2t' caller-kept images."""
    return dict(name=name, N=N, P=P, C=C, Cp=Cp, J=J, dt=dt, form=form, dpl=dpl, entry=entry, beta=beta, reuse=reuse,
                mis=dict(mis), images=tuple(images), train=train, expect=expect)


# Expected traces are read off the dispatch conditions of apa_pose_head.hip (pose_pl_fast / pose_pl_product /
# pose_pl_launch, pose_rows_route = pose_rows_mfma_ok + pose_bwd_rows_ok, pose_rows_lds / pose_rows_per_block, the arms
# pose_rows_mfma / pose_rows_valu / pose_rows_dppre, pose_w1_operand, pose_dw1_splits + gemm_launch's tail rule in
# pose_head_bwd_big) -- not off a run.
#   mfma:  bf16, dPl, J = 16, Cp % 128 = 0, 256 <= Cp <= 1024, 16-byte aligned, no dense ext;  nw = Cp / 64,
#          wpb = 3 if nw % 3 == 0 else 4 if nw % 4 == 0 else 2, ngrp = nw / wpb, G = 2 iff R >= 2048
#   valu:  dPl, J <= 16, Cp <= 1024, 8-byte aligned Ppre / ext, 16 rows fit 64 KB;  rpb = 32 iff R >= 4065 and 32 rows fit
#   dppre: everything else;  jm = 16 iff J <= 16
CASES = [
    # ---- rows = mfma: every (wpb, ngrp), G 1 / 2, R1 on / off, ragged last groups
    case('mfma_cp256_plain_r100', 1, 100, 64, 256, 16, pl='fast', pl_ks=8, rows='mfma', wpb=4, ngrp=1, G=1,
         form_t='plain', dw2='rows', colsum='own', dw1_splits=1, w1_fwd='bf16_copy', w1_bwd='bf16_copy', dx_beta=0),
    # R = 2075: R % 64 = 27 -- the last block's first group is ragged and its second group is empty
    case('mfma_cp384_rank1_r2075_g2', 25, 83, 64, 384, 16, form='rank1', pl='gemm', rows='mfma', wpb=3, ngrp=2, G=2,
         form_t='rank1', colsum='tail'),
    case('mfma_cp512_plain_r2100_g2_beta1', 21, 100, 64, 512, 16, beta=1, pl='fast', pl_ks=16, rows='mfma', wpb=4,
         ngrp=2, G=2, form_t='plain', dx_beta=1, colsum='tail'),
    case('mfma_cp640_rank1_r500', 5, 100, 64, 640, 16, form='rank1', pl='gemm', rows='mfma', wpb=2, ngrp=5, G=1,
         form_t='rank1', colsum='own'),
    case('mfma_cp896_plain_r2050_g2', 50, 41, 64, 896, 16, pl='gemm', rows='mfma', wpb=2, ngrp=7, G=2,
         form_t='plain'),
    case('mfma_cp1024_rank1_r777_reuse', 7, 111, 64, 1024, 16, form='rank1', reuse=True, pl='fast', pl_ks=32,
         rows='mfma', wpb=4, ngrp=4, G=1, form_t='rank1', w1_bwd='reused', colsum='tail'),
    # ---- the shipped shapes (nets_factory.py POSE_PRELOGITS = 768; 16 and 13 keypoints)
    case('ship_bf16_j16_n32', 32, 196, 2048, 768, 16, form='rank1', beta=1, reuse=True, pl='fast', pl_ks=24,
         rows='mfma', wpb=3, ngrp=4, G=2, form_t='rank1', colsum='tail', dw1_splits=4, w1_bwd='reused', dx_beta=1),
    case('ship_bf16_j13_n32', 32, 196, 2048, 768, 13, form='rank1', beta=1, pl='fast', pl_ks=24, rows='valu',
         rpb=32, form_t='rank1', colsum='own', dx_beta=1),
    case('ship_f32_j16_n32', 32, 196, 2048, 768, 16, dt=F32, form='rank1', beta=1, pl='gemm', rows='valu', rpb=16,
         form_t='rank1', w1_fwd='f32', w1_bwd='f32', colsum='own'),
    case('ship_f32_j13_n32', 32, 196, 2048, 768, 13, dt=F32, form='plain', pl='gemm', rows='valu', rpb=16,
         form_t='plain', w1_fwd='f32'),
    # 33 x 15 x 15: R = 7425, R % 64 = 1
    case('ship_bf16_j16_n33_p225', 33, 225, 2048, 768, 16, form='rank1', pl='fast', pl_ks=24, rows='mfma', wpb=3,
         ngrp=4, G=2, form_t='rank1', colsum='tail'),
    case('ship_bf16_j13_n33_p225', 33, 225, 2048, 768, 13, form='plain', pl='fast', pl_ks=24, rows='valu', rpb=32,
         form_t='plain'),
    # ---- rows = valu, 32 rows per block (R >= 4065) on each side of the 64 KB tile limit, per (dtype, form)
    case('valu_f32_plain_cp384_rpb32', 41, 100, 64, 384, 16, dt=F32, pl='gemm', rows='valu', rpb=32, form_t='plain'),
    case('valu_f32_plain_cp512_rpb16', 41, 100, 64, 512, 16, dt=F32, rows='valu', rpb=16, form_t='plain'),
    case('valu_f32_ext_cp128_rpb32', 41, 100, 64, 128, 13, dt=F32, form='ext', rows='valu', rpb=32, form_t='ext'),
    case('valu_f32_ext_cp256_rpb16', 41, 100, 64, 256, 16, dt=F32, form='ext', rows='valu', rpb=16, form_t='ext'),
    case('valu_f32_rank1_cp384_rpb32', 41, 100, 64, 384, 13, dt=F32, form='rank1', rows='valu', rpb=32,
         form_t='rank1'),
    case('valu_f32_rank1_cp512_rpb16', 41, 100, 64, 512, 16, dt=F32, form='rank1', rows='valu', rpb=16,
         form_t='rank1'),
    case('valu_bf16_plain_cp896_j13_rpb32', 41, 100, 64, 896, 13, pl='gemm', rows='valu', rpb=32, form_t='plain'),
    case('valu_bf16_plain_cp1024_j13_rpb16', 41, 100, 64, 1024, 13, pl='fast', pl_ks=32, rows='valu', rpb=16,
         form_t='plain'),
    case('valu_bf16_ext_cp384_rpb32', 41, 100, 64, 384, 16, form='ext', rows='valu', rpb=32, form_t='ext'),
    case('valu_bf16_ext_cp512_rpb16', 41, 100, 64, 512, 16, form='ext', pl='fast', pl_ks=16, rows='valu', rpb=16,
         form_t='ext'),
    case('valu_bf16_rank1_cp896_j13_rpb32', 41, 100, 64, 896, 13, form='rank1', rows='valu', rpb=32,
         form_t='rank1'),
    case('valu_bf16_rank1_cp1024_j13_rpb16', 41, 100, 64, 1024, 13, form='rank1', rows='valu', rpb=16,
         form_t='rank1'),
    # ---- rows = valu at small R: idle threads (Cp / 2 = 100 is not a multiple of 64), J = 16 (permuted partials) and
    # J < 16, R % 16 != 0; bf16 when the MFMA form is refused for Cp % 128 != 0
    case('valu_f32_cp200_j16_r301', 7, 43, 96, 200, 16, dt=F32, form='rank1', rows='valu', rpb=16, form_t='rank1'),
    case('valu_bf16_cp200_j7_r301', 7, 43, 96, 200, 7, form='plain', pl='gemm', rows='valu', rpb=16, form_t='plain'),
    case('valu_bf16_cp320_j16_ext_r95', 5, 19, 96, 320, 16, form='ext', beta=1, pl='gemm', rows='valu', rpb=16,
         form_t='ext', dx_beta=1),
    # Pl fast with J < 16 and R % 64 != 0 at KS 8 / 16 (24 / 32: ship_bf16_j13_*, valu_bf16_*_cp1024_j13_*)
    case('valu_bf16_cp256_j13_r333', 9, 37, 64, 256, 13, pl='fast', pl_ks=8, rows='valu', rpb=16, form_t='plain'),
    case('valu_bf16_cp512_j5_r333', 9, 37, 64, 512, 5, form='rank1', pl='fast', pl_ks=16, rows='valu', rpb=16,
         form_t='rank1'),
    # ---- rows = dppre
    case('dppre_f32_cp2048_j32_rank1_r203', 7, 29, 64, 2048, 32, dt=F32, form='rank1', pl='gemm', rows='dppre',
         jm=32, form_t='rank1', dw2='gemm', colsum='own'),
    case('dppre_bf16_cp512_j20_ext_r301', 7, 43, 64, 512, 20, form='ext', pl='gemm', rows='dppre', jm=32,
         form_t='ext', dw2='gemm'),
    case('dppre_bf16_cp768_j32_plain_r150', 3, 50, 64, 768, 32, pl='gemm', rows='dppre', jm=32, form_t='plain',
         dw2='gemm'),
    case('dppre_f32_cp256_nodpl_ext_r100', 4, 25, 64, 256, 16, dt=F32, form='ext', dpl=False, rows='dppre', jm=16,
         form_t='ext', dw2='memset'),
    case('dppre_bf16_cp1024_nodpl_rank1_r203', 7, 29, 64, 1024, 16, form='rank1', dpl=False, rows='dppre', jm=16,
         form_t='rank1', dw2='memset'),
    # fp32, Cp = 1024: 16 rows of the VALU tile exceed 64 KB -> dppre with its contiguous W2 slice at J = 16
    case('dppre_f32_cp1024_j16_plain_r203', 7, 29, 64, 1024, 16, dt=F32, rows='dppre', jm=16, form_t='plain',
         dw2='gemm'),
    case('dppre_bf16_cp2048_j13_rank1_r99', 3, 33, 64, 2048, 13, form='rank1', pl='gemm', rows='dppre', jm=16,
         form_t='rank1', dw2='gemm'),
    # bf16 dense ext at Cp = 1024: the VALU tile pair exceeds 64 KB
    case('dppre_bf16_cp1024_j16_ext_r203', 7, 29, 64, 1024, 16, form='ext', pl='fast', pl_ks=32, rows='dppre', jm=16,
         form_t='ext', dw2='gemm'),
    # ---- the one-call step (apa_pose_attn_train_step): FUSED and W2T forms of every KS, WA on both rows kernels
    case('step_bf16_cp768_g2', 11, 196, 2048, 768, 16, entry='step', pl='fast', pl_ks=24, pl_fused=1, pl_w2t=0,
         rows='mfma', wpb=3, ngrp=4, G=2, wa=1, form_t='rank1', w1_fwd='bf16_copy', w1_bwd='reused', dx_beta=1),
    # training at the shipped batch: the pooling's dX share is formed in the dX product's rank-1 epilogue (dx_beta = 0;
    # taken when the wide bf16 kernel serves the product -- at least 192 tiles of <= 224 rows x 256 columns)
    case('step_bf16_cp768_images_train', 32, 196, 2048, 768, 16, entry='step', images=('w1', 'w2t'), train=True,
         pl='fast', pl_ks=24, pl_fused=1, pl_w2t=1, rows='mfma', wpb=3, ngrp=4, G=2, wa=1, form_t='rank1',
         w1_fwd='shadow', w1_bwd='shadow', dx_beta=0, colsum='tail'),
    case('step_bf16_cp256', 4, 196, 2048, 256, 16, entry='step', pl='fast', pl_ks=8, pl_fused=1, pl_w2t=0,
         rows='mfma', wpb=4, ngrp=1, G=1, wa=1, form_t='rank1'),
    case('step_bf16_cp256_w2t', 4, 196, 2048, 256, 16, entry='step', images=('w2t',), pl_ks=8, pl_fused=1, pl_w2t=1,
         rows='mfma', wa=1, w1_fwd='bf16_copy'),
    case('step_bf16_cp512', 4, 196, 2048, 512, 16, entry='step', pl_ks=16, pl_fused=1, pl_w2t=0, rows='mfma',
         wpb=4, ngrp=2, wa=1),
    case('step_bf16_cp512_w2t_train', 32, 196, 2048, 512, 16, entry='step', images=('w1', 'w2t'), train=True,
         pl_ks=16, pl_fused=1, pl_w2t=1, rows='mfma', wa=1, w1_bwd='shadow', dx_beta=0),
    case('step_bf16_cp1024', 4, 196, 2048, 1024, 16, entry='step', pl_ks=32, pl_fused=1, pl_w2t=0, rows='mfma',
         wpb=4, ngrp=4, wa=1),
    case('step_bf16_cp1024_w2t', 4, 196, 2048, 1024, 16, entry='step', images=('w2t',), pl_ks=32, pl_fused=1,
         pl_w2t=1, rows='mfma', wa=1),
    # a 4-byte-aligned dPl: the MFMA form is refused, the VALU kernel's WA form serves the fused step
    case('step_bf16_cp768_dpl4_valu_wa', 4, 196, 2048, 768, 16, entry='step', mis={'dPl': 1}, pl_fused=1,
         rows='valu', rpb=16, wa=1, form_t='rank1', colsum='own'),
    # fp32: the four-call fall-back
    case('step_f32_cp768_fallback', 4, 196, 2048, 768, 16, dt=F32, entry='step', pl='gemm', pl_fused=0, rows='valu',
         rpb=16, wa=0, form_t='rank1', w1_fwd='f32', w1_bwd='f32', dx_beta=1),
]

# Buffers at the offsets the dispatcher itself tests for and routes to a fall-back.  The fall-back kernels then issue
# vector loads from 4- or 8-byte-aligned addresses; kept in a test function of their own.
MIS_CASES = [
    # bf16 Ppre at an 8-byte offset: Pl leaves the fast kernel (16-byte rows); the rows pass stays VALU (8 bytes suffice)
    case('mis_bf16_ppre8_pl_gemm', 5, 40, 64, 256, 16, mis={'Ppre': 4}, pl='gemm', rows='valu', rpb=16,
         form_t='plain'),
    # bf16 / fp32 Ppre 4-byte aligned: the rows pass is refused -> dppre
    case('mis_bf16_ppre4_dppre', 5, 40, 64, 256, 16, form='rank1', mis={'Ppre': 2}, pl='gemm', rows='dppre', jm=16,
         form_t='rank1', dw2='gemm'),
    case('mis_f32_ppre4_dppre', 5, 40, 64, 256, 13, dt=F32, mis={'Ppre': 1}, rows='dppre', jm=16, form_t='plain',
         dw2='gemm'),
    # W2 not 16-byte aligned at J = 16: rows pass refused -> dppre reads its contiguous slice from a 4-byte address
    case('mis_f32_w2_4_dppre', 5, 40, 64, 256, 16, dt=F32, form='ext', mis={'W2': 1}, rows='dppre', jm=16,
         form_t='ext', dw2='gemm'),
    case('mis_bf16_w2_8_dppre', 5, 40, 64, 512, 16, mis={'W2': 2}, pl='fast', pl_ks=16, rows='dppre', jm=16,
         form_t='plain', dw2='gemm'),
    # 4-byte-aligned dPl: MFMA refused -> bf16 VALU with J = 16
    case('mis_bf16_dpl4_valu', 5, 40, 64, 384, 16, form='rank1', mis={'dPl': 1}, rows='valu', rpb=16,
         form_t='rank1'),
    # W1 not 16-byte aligned: bf16 features multiply the caller's fp32 W1 (rounded by the GEMM's staging code)
    case('mis_bf16_w1_4_f32_operand', 5, 40, 64, 256, 16, mis={'W1': 1}, w1_fwd='f32', w1_bwd='f32', rows='mfma'),
]


# ------------------------------------------------------------------------------------------ figures for the profile
FIGS = []


def _check(c, got, b, stage, **kw):
    """mp.check, after recording max |err| / bound and max bound / max |ref| of the stage."""
    g = got.double().reshape(b.ref.shape)
    tol = b.err + (U_BF16 * b.ref.abs() if kw.get('bf16') else 0.0)
    nz = tol > 0
    r_err = float(((g - b.ref).abs()[nz] / tol[nz]).max()) if bool(nz.any()) else 0.0
    if bool(((g - b.ref).abs()[~nz] > 0).any()):
        r_err = float('inf')
    r_bnd = float(b.err.max() / b.ref.abs().max()) if float(b.ref.abs().max()) > 0 else 0.0
    FIGS.append((c['name'], stage, r_err, r_bnd))
    print('POSE_FIG {} {} err/bound {:.4f} bound/ref {:.3e}'.format(c['name'], stage, r_err, r_bnd))
    mp.check(got, b, '{}: {}'.format(c['name'], stage), **kw)


def _prod(a, b, L, extra=0.0, add=None):
    """a @ b accumulated in fp32 over L terms (+ addends `add`: list of float64 tensors inside the same chain)."""
    ref, mag = a @ b, a.abs() @ b.abs()
    for t in add or ():
        ref, mag = ref + t, mag + t.abs()
    return Bnd(ref, (C_ACC * (L + 8) * EPS32 + extra) * mag), mag


# ------------------------------------------------------------------------------------------ one case on the device
class _Run:
    def __init__(self, c, dev, lib):
        self.c, self.dev, self.lib = c, dev, lib
        N, P, C, Cp, J = c['N'], c['P'], c['C'], c['Cp'], c['J']
        R = N * P
        self.R, dt, tdt = R, c['dt'], TDT[c['dt']]
        self.bf = dt == BF16
        gen = torch.Generator(device=dev)
        gen.manual_seed(zlib.crc32(c['name'].encode()))
        rnd = lambda *s: torch.rand(*s, generator=gen, device=dev, dtype=torch.float64)
        ro = lambda *s: rnd(*s) * 1.25 - 0.25
        mis = c['mis']

        def buf(name, rows, cols, dtype, data=None):
            g = gp.Guarded(rows, cols, cols, dtype, dev, off=mis.get(name, 0), data=data)
            self.b[name] = g
            return g

        self.b = {}
        X = (torch.relu(ro(R, C)) * (0.5 + rnd(R, 1))).to(tdt)
        W1 = (ro(C, Cp) / C).float()
        W1v = W1.to(torch.bfloat16) if self.bf else W1
        S = X.double() @ W1v.double()
        b1 = (-S.median(dim=0).values * (0.9 + 0.2 * rnd(Cp))).float()
        del S
        buf('X', R, C, tdt, X)
        buf('W1', C, Cp, torch.float32, W1)
        buf('b1', 1, Cp, torch.float32, b1)
        buf('W2', Cp, J, torch.float32, (ro(Cp, J) / Cp).float())
        buf('b2', 1, J, torch.float32, (torch.randn(J, generator=gen, device=dev) * 0.1))
        self.outs = ['Ppre', 'Pl', 'dX', 'dW1', 'db1', 'dW2', 'db2']
        buf('Ppre', R, Cp, tdt)
        buf('Pl', R, J, torch.float32)
        buf('dX', R, C, tdt)
        buf('dW1', C, Cp, torch.float32)
        buf('db1', 1, Cp, torch.float32)
        buf('dW2', Cp, J, torch.float32)
        buf('db2', 1, J, torch.float32)
        self.plan = pp.plan(N, P, C, Cp, J, dt)
        self.ws_bytes = int(lib.apa_pose_head_workspace_bytes(N, P, C, Cp, J, dt))
        assert self.ws_bytes == self.plan['total'] and self.plan['R'] == R
        buf('ws', 1, (self.ws_bytes + 3) // 4, torch.float32)
        self.dX0 = None
        if c['entry'] == 'sep':
            if c['dpl']:
                buf('dPl', R, J, torch.float32, ro(R, J).float())
            if c['form'] == 'ext':
                buf('ext', R, Cp, tdt, ro(R, Cp).to(tdt))
            elif c['form'] == 'rank1':
                buf('ext_row', 1, R, torch.float32, rnd(R).float())
                buf('ext_col', 1, Cp, torch.float32, ro(Cp).float())
            if c['beta']:
                self.dX0 = ro(R, C).to(tdt)
                self.b['dX'].view.copy_(self.dX0)
        else:
            K = STEP_K
            self.flags = cof.APA_FLAG_TRAIN if c['train'] else 0
            buf('Wa', 1, Cp, torch.float32, (ro(Cp) / Cp).float())
            buf('ba', 1, 1, torch.float32, torch.full((1,), 0.05, device=dev))
            Wt = ro(C, K) / C
            Wt[:, 0] = (2.0 + 2.0 * rnd(C)) / C
            buf('Wt', C, K, torch.float32, Wt.float())
            buf('bt', 1, K, torch.float32, (torch.randn(K, generator=gen, device=dev) * 0.1))
            self.labels = torch.zeros(N, dtype=torch.int64, device=dev)
            buf('lbl', R, J, torch.float32, ro(R, J).float())
            self.valid = (rnd(N, J) < 0.75).to(torch.uint8)
            self.valid[0, :] = 1
            for name, rows, cols in (('att', 1, R), ('logits', N, K), ('zsave', N, C), ('abar', 1, N),
                                     ('loss_action', 1, 1 + N), ('loss_pose', 1, 1), ('G', N, K), ('dPl', R, J),
                                     ('dZ', 1, R), ('dWa', 1, Cp), ('dba', 1, 1), ('dWt', C, K), ('dbt', 1, K)):
                buf(name, rows, cols, torch.float32)
                self.outs.append(name)
            self.wsp_bytes = int(lib.apa_attn_pool_workspace_bytes(N, P, C, Cp, K, 1, self.flags))
            buf('ws_pool', 1, (self.wsp_bytes + 3) // 4, torch.float32)
            self.w1img = self.w2timg = None
            if 'w1' in c['images']:
                self.w1img = gp.Guarded(C, Cp, Cp, torch.bfloat16, dev, data=W1.to(torch.bfloat16))
                self.b['w1img'] = self.w1img
            if 'w2t' in c['images']:
                img = cof.pose_w2t_image(self.b['W2'].view.contiguous())
                self.w2timg = gp.Guarded(16, Cp + 16, Cp + 16, torch.bfloat16, dev, data=img)
                self.b['w2timg'] = self.w2timg
        for g in self.b.values():
            g.snapshot()

    def p(self, name):
        return self.b[name].ptr if name in self.b else None

    def restore(self):
        for g in self.b.values():
            g.restore()

    def check_guards(self):
        for name, g in self.b.items():
            g.check_guards('{}: {}'.format(self.c['name'], name))

    def bits(self):
        out = {k: self.b[k].bits() for k in self.outs}
        out['dPpre'] = self.dppre().contiguous().view(torch.int32 if not self.bf else torch.int16).clone()
        return out

    def dppre(self):
        """the kernel's dPpre, out of the workspace (PosePlan::off_dppre)."""
        tdt = TDT[self.c['dt']]
        esz = 2 if self.bf else 4
        raw = self.b['ws'].view.view(-1).view(torch.uint8)
        o = self.plan['off_dppre']
        return raw[o:o + self.R * self.c['Cp'] * esz].view(tdt).view(self.R, self.c['Cp'])

    def _ok(self, rc, what):
        assert rc == 0, '{}: {} returned {} ({})'.format(self.c['name'], what, rc, self.lib.apa_last_error().decode())

    def run(self):
        c, lib, p = self.c, self.lib, self.p
        N, P, C, Cp, J, dt = c['N'], c['P'], c['C'], c['Cp'], c['J'], c['dt']
        st = gp.stream_ptr()
        t1, t2 = pp.PoseTrace(), pp.PoseTrace()
        if c['entry'] == 'step':
            io = cof.ApaPoseAttnStepIO()
            for f in ('X', 'W1', 'b1', 'W2', 'b2', 'Wa', 'ba', 'Wt', 'bt', 'Ppre', 'Pl', 'att', 'logits', 'zsave',
                      'abar', 'loss_action', 'loss_pose', 'G', 'dPl', 'dZ', 'dX', 'dW1', 'db1', 'dW2', 'db2', 'dWa',
                      'dba', 'dWt', 'dbt'):
                setattr(io, f, p(f))
            io.W1_bf16 = self.w1img.ptr if self.w1img is not None else None
            io.W2T_bf16 = self.w2timg.ptr if self.w2timg is not None else None
            io.labels, io.pose_labels, io.pose_valid = self.labels.data_ptr(), p('lbl'), self.valid.data_ptr()
            io.action_wt, io.pose_wt, io.grad_scale = 1.0, 1.0, 1.0
            io.ws_pool, io.ws_pool_bytes = p('ws_pool'), self.wsp_bytes
            io.ws_pose, io.ws_pose_bytes = p('ws'), self.ws_bytes
            self._ok(lib.apa_probe_pose_attn_train_step(ctypes.addressof(t1), ctypes.addressof(io), N, P, C, Cp, J,
                                                        STEP_K, self.flags, KEEP, 1234, 5, dt, st), 'step')
            return t1.as_dict()
        self._ok(lib.apa_probe_pose_head_fwd(ctypes.addressof(t1), p('X'), p('W1'), p('b1'), p('W2'), p('b2'),
                                             p('Ppre'), p('Pl'), p('ws'), self.ws_bytes, N, P, C, Cp, J, dt, st), 'fwd')
        acc = (1 if c['beta'] else 0) | (APA_POSE_WS_FROM_FWD if c['reuse'] else 0)
        if c['form'] == 'rank1':
            rc = lib.apa_probe_pose_head_bwd_rank1ext(
                ctypes.addressof(t2), p('X'), p('W1'), p('W2'), p('Ppre'), p('dPl'), p('ext_row'), p('ext_col'),
                p('dX'), acc, p('dW1'), p('db1'), p('dW2'), p('db2'), p('ws'), self.ws_bytes, N, P, C, Cp, J, dt, st)
        else:
            rc = lib.apa_probe_pose_head_bwd(
                ctypes.addressof(t2), p('X'), p('W1'), p('W2'), p('Ppre'), p('dPl'), p('ext'), p('dX'), acc,
                p('dW1'), p('db1'), p('dW2'), p('db2'), p('ws'), self.ws_bytes, N, P, C, Cp, J, dt, st)
        self._ok(rc, 'bwd')
        d = t1.as_dict()
        for k, v in t2.as_dict().items():
            if v not in (0, 'none'):
                d[k] = v
        d['dx_beta'] = t2.dx_beta
        return d


# ------------------------------------------------------------------------------------------ float64 stages
def _check_case(c, r, trace):
    N, P, C, Cp, J, R, bf = c['N'], c['P'], c['C'], c['Cp'], c['J'], r.R, r.bf
    v = lambda name: r.b[name].view.double()
    rnd16 = lambda t: t.to(torch.bfloat16).double() if bf else t.double()   # the operand rule of tests/_gemm_probe.py
    step = c['entry'] == 'step'
    mfma = trace['rows'] == 'mfma'
    X, b1, b2 = v('X'), v('b1').view(-1), v('b2').view(-1)
    W1v = rnd16(r.b['W1'].view)        # bf16 copy, caller-kept image (same values) or fp32 W1 rounded by the stager
    W2 = v('W2')

    # ---- Ppre = relu(X . W1op + b1)
    pre, _ = _prod(X, W1v, C, add=[b1])
    _check(c, r.b['Ppre'].view, Bnd(torch.relu(pre.ref), pre.err), 'Ppre', bf16=bf)
    del pre
    Pk = v('Ppre')                      # everything below reads the kernel's own Ppre
    gate = Pk > 0
    frac = float(gate.double().mean())
    assert 0.25 <= frac <= 0.75, '{}: {:.1%} of the relu gates open'.format(c['name'], frac)

    # ---- Pl = Ppre . W2 + b2 (bf16 features: W2 rounded to bf16 by pose_pl_kernel / the GEMM's stager)
    pl, _ = _prod(Pk, rnd16(r.b['W2'].view), Cp, add=[b2])
    _check(c, r.b['Pl'].view, pl, 'Pl')
    del pl
    dPl = ext_row = ext_col = None
    if step:
        Plk, lbl = v('Pl'), v('lbl')
        wa, ba = v('Wa').view(-1), v('ba').view(-1)
        # attention logits (identity attention): exact fp32 FMAs on the unrounded wa
        att, _ = _prod(Pk, wa[:, None], Cp, add=[ba])
        _check(c, r.b['att'].view, Bnd(att.ref.view(-1), att.err.view(-1)), 'att')
        # pose loss: dPl = gcoef * valid * (Pl - lbl), six fp32 roundings at most (the difference, gcoef's product and
        # quotient, two products); loss = 0.5 wt / (N N P) * sum valid (Pl - lbl)^2 over R J non-negative terms: in the
        # fused Pl kernel a lane's chain of 4, a 6-level wave tree, <= 2 adds across the block's waves, then the
        # block partials (one per 64 rows, per 32 with the W2^T image) summed in a fixed order by the column-sum
        # launch -- at most nblk + 12 roundings on any term; the four-call fall-back's loss kernel: any order, R J
        valid = r.valid.double()[:, None, :].expand(N, P, J).reshape(R, J)
        dd = (Plk - lbl) * valid
        gcoef = 1.0 / (float(N) * N * P)
        _check(c, r.b['dPl'].view, Bnd(gcoef * dd, 6 * EPS32 * (gcoef * dd).abs()), 'dPl')
        loss = 0.5 * gcoef * (dd * dd).sum().view(1)
        L = (R + 31) // 32 + 12 if trace['pl_w2t'] else (R + 63) // 64 + 12 if trace['pl_fused'] else R * J
        _check(c, r.b['loss_pose'].view, Bnd(loss, C_ACC * (L + 8) * EPS32 * loss), 'loss_pose')
        dPl, ext_row, ext_col = v('dPl'), v('dZ').view(-1), wa      # own dPl; dZ as the pooling half left it
    else:
        if c['dpl']:
            dPl = v('dPl')
        if c['form'] == 'rank1':
            ext_row, ext_col = v('ext_row').view(-1), v('ext_col').view(-1)

    # ---- dPpre = (dPl . W2^T + ext) * [Ppre > 0]   (fp32 W2 and dPl; the MFMA form splits both: SPLIT2)
    zero = torch.zeros(R, Cp, dtype=torch.float64, device=X.device)
    g, gm = zero, zero
    if dPl is not None:
        g, gm = dPl @ W2.t(), dPl.abs() @ W2.abs().t()
    if ext_row is not None:
        t = ext_row[:, None] * ext_col[None, :]
        g, gm = g + t, gm + t.abs()
    elif c['form'] == 'ext':
        g, gm = g + v('ext'), gm + v('ext').abs()
    g, gm = g * gate, gm * gate
    eg = (C_ACC * (J + 8) * EPS32 + (pp.SPLIT2 if mfma else 0.0)) * gm
    _check(c, r.dppre(), Bnd(g, eg), 'dPpre', bf16=bf)
    dk = r.dppre().double()             # dW1 and dX read the kernel's own dPpre

    # ---- dW2 = Ppre^T . dPl, db2 = sum_r dPl, db1 = sum_r dPpre (the unrounded values)
    if dPl is not None:
        if trace['dw2'] == 'gemm':      # the split-K GEMM: bf16 features round dPl to bf16 in its stager
            dw2, _ = _prod(Pk.t(), rnd16(r.b['dPl'].view), R)
        else:
            dw2, _ = _prod(Pk.t(), dPl, R, extra=pp.SPLIT1 if mfma else 0.0)
        _check(c, r.b['dW2'].view, dw2, 'dW2')
        s = dPl.sum(0)
        _check(c, r.b['db2'].view, Bnd(s, C_ACC * (R + 8) * EPS32 * dPl.abs().sum(0)), 'db2')
    else:
        assert trace['dw2'] == 'memset'
        assert not bool(r.b['dW2'].view.any()) and not bool(r.b['db2'].view.any()), 'dW2 / db2 without dPl must be 0'
        FIGS.append((c['name'], 'dW2,db2 (exact zeros)', 0.0, 0.0))
    _check(c, r.b['db1'].view, Bnd(g.sum(0), C_ACC * (R + 8) * EPS32 * gm.sum(0) + eg.sum(0)), 'db1')
    if step and trace['wa']:            # dWa = Ppre^T . dZ, dba = sum_r dZ on the same pass (dZ split on the MFMA form)
        dwa, _ = _prod(Pk.t(), ext_row[:, None], R, extra=pp.SPLIT1 if mfma else 0.0)
        _check(c, r.b['dWa'].view, Bnd(dwa.ref.view(-1), dwa.err.view(-1)), 'dWa')
        _check(c, r.b['dba'].view, Bnd(ext_row.sum().view(1), C_ACC * (R + 8) * EPS32 * ext_row.abs().sum().view(1)),
               'dba')
    del g, gm, eg

    # ---- dW1 = X^T . dPpre
    dw1, _ = _prod(X.t(), dk, R)
    _check(c, r.b['dW1'].view, dw1, 'dW1')
    del dw1

    # ---- dX = dPpre . W1op^T (+ the given dX | + the pooling's share)
    add, extra_err = [], 0.0
    if step:
        off_dz, off_bits = pp.pool_offsets(N, P, C, Cp, STEP_K)
        raw = r.b['ws_pool'].view.view(-1).view(torch.uint8)
        dz = raw[off_dz:off_dz + N * C * 4].view(torch.float32).view(N, C).double()
        attk = v('att').view(-1)
        share = (attk / P)[:, None] * dz.repeat_interleave(P, dim=0)
        if trace['dx_beta'] == 0:       # formed in the dX product's epilogue from att, dz and the keep bits
            if c['train']:
                by = raw[off_bits:off_bits + R * C // 8].to(torch.int32)
                bit = ((by[:, None] >> torch.arange(8, device=by.device)[None, :]) & 1).reshape(R, C).double()
                share = share * bit / KEEP
        else:                           # written by the pooling's backward in dX's dtype, then accumulated onto
            assert not c['train']
            extra_err = (U_BF16 if bf else EPS32) * share.abs()
        add = [share]
    elif c['beta']:
        add = [r.dX0.double()]
    dx, _ = _prod(dk, W1v.t(), Cp, add=add)
    _check(c, r.b['dX'].view, Bnd(dx.ref, dx.err + extra_err), 'dX', bf16=bf)


def _run_case(c, dev):
    lib = pp.load_pose_probe()
    r = _Run(c, dev, lib)
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    exp = dict(c['expect'])
    if 'form_t' in exp:
        exp['form'] = exp.pop('form_t')
    if c['entry'] == 'sep':
        exp.setdefault('pl_fused', 0)
        exp.setdefault('pl_w2t', 0)
        exp.setdefault('wa', 0)
        exp.setdefault('dx_beta', int(bool(c['beta'])))
        exp.setdefault('w1_bwd', 'reused' if c['reuse'] else None)
    bad = {k: (trace[k], e) for k, e in exp.items() if e is not None and trace[k] != e}
    assert not bad, '{}: trace mismatch (got, expected): {} in {}'.format(c['name'], bad, trace)
    assert (trace['colsum'] == 'tail') <= (trace['dw1_splits'] > 1)      # the tail rides on a split-K reduce only
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


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_pose_path(gpu, c):
    _run_case(c, gpu)


@pytest.mark.parametrize('c', MIS_CASES, ids=[c['name'] for c in MIS_CASES])
def test_pose_path_misaligned(gpu, c):
    _run_case(c, gpu)


def test_pose_step_rejects_what_it_documents(gpu):
    """apa_pose_attn_train_step: APA_FLAG_RELU_INPUT / APA_FLAG_RNG_EXTERNAL are refused with APA_ERR_UNSUPPORTED
    before anything is launched."""
    lib = pp.load_pose_probe()
    c = case('reject', 2, 16, 64, 256, 16, entry='step')
    r = _Run(c, gpu, lib)
    io = cof.ApaPoseAttnStepIO()
    for f, _ in io._fields_:
        if f not in ('action_wt', 'pose_wt', 'grad_scale', 'ws_pool_bytes', 'ws_pose_bytes', 'W1_bf16', 'W2T_bf16'):
            setattr(io, f, r.p('X'))
    t = pp.PoseTrace()
    for flag in (cof.APA_FLAG_RELU_INPUT, cof.APA_FLAG_RNG_EXTERNAL):
        rc = lib.apa_probe_pose_attn_train_step(ctypes.addressof(t), ctypes.addressof(io), 2, 16, 64, 256, 16, STEP_K,
                                                flag, 1.0, 0, 0, BF16, gp.stream_ptr())
        assert rc == gp.APA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    r.check_guards()


def teardown_module(module):
    """With APA_POSE_FIGURES=<path>: the per-stage figures of this run as a table (profiles/r08_pose_paths.md)."""
    path = os.environ.get('APA_POSE_FIGURES')
    if path and FIGS:
        with open(path, 'w') as f:
            f.write('| case | stage | max err / bound | bound / max ref |\n|---|---|---|---|\n')
            for name, stage, a, b in FIGS:
                f.write('| {} | {} | {:.3f} | {:.2e} |\n'.format(name, stage, a, b))
