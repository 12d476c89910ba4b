#!/usr/bin/env python
"""Supplementary workloads for the MFMA-bound rows of SURVEY.md section 8 and the evaluation step.
`/bench.py` imports the builders below and reports them in the `extra` object of its JSON line (the
headline stays the cfg 002 training workload); run this file directly for one workload at a time:

  cfg003    pose-regularised attention, bf16 (BASELINE configs[2]): PoseLogits head fwd (X.W1+relu,
            Ppre.W2) -> attention from pose_pre_logits -> pose L2 + softmax-xent -> backward of
            both heads.  Dense work: 1.864 GFLOP/img in the pose head.
  perclass  per-class bottom-up maps (M == K), HMDB-51 shape (K = 51, bf16) or K = 393:
            1.893 GFLOP/img at K = 393, 0.246 at K = 51.
  eval002   BASELINE configs[1]: cfg 002 evaluation step (forward + softmax + argmax, one call).
  eval003   cfg 003 evaluation step, bf16: the one-call apa_pose_attn_eval_step (attention logits out of the
            pose-head product's epilogue, pose_pre_logits never written) against the sequence cof.pose_head_fwd +
            cof.HeadEvalStep, alternating in one process; prints both medians and HIP-event times per host call.

  video_perclass / video003
            a batch of CLIPS, 8 x 4 frames x 14x14x2048 bf16, K = 51, temporal attention on, for the per-class (HMDB-51)
            head and the cfg 003 head: the one-call clip step (apa_*_train_step_clips: frame pooling, temporal attention
            and the clip loss inside the call) against the module path (network_fn + gen_losses + backward), alternating
            in one process, medians of five; also the flat one-call step at N = 32 of the same head, whose per-image
            cross-entropy is folded into its neighbours, and the clip loss's own two launches.

  hico002 / charades_clips
            the multi-label datasets on the class-agnostic head (M = 1), bf16: HICO, 32 x 14x14x2048 images, K = 600,
            and Charades, 8 clips x 4 frames, K = 157, temporal attention on.  Three variants alternate in one process,
            medians of five: the one-call multi-label step (apa_attn_head_train_step_multilabel), the module path
            (network_fn + gen_losses + autograd) and the softmax one-call step of the same shape.

  frozen002_fp8 / eval002_fp8
            cfg 002 on an FP8 E4M3 feature cache (Fp8Features) against the same step on the bf16 maps: the frozen
            one-call training step / the one-call evaluation step, alternating in one process, medians of five and
            their spread, the streaming kernels by HIP events with their bytes per second; --batch 512 for the
            bandwidth-bound size
  cached002_fp8 / cached002_bf16
            cfg 002 frozen one-call training step from a RESIDENT feature cache (--cache-images, at least 2048 maps
            14x14x2048, FP8 E4M3 or bf16; --batch 512 for the bandwidth-bound size), three variants alternating in one
            process, medians of five and their spread: (a) the gathered step (apa_attn_head_train_step_cached) with a
            fresh shuffled index per step, (b) gather + rebind + the plain step -- the loop without the gathered
            kernels --, (c) the plain step on one fixed contiguous batch.
  cached_perclass_bf16
            the same three variants for the HMDB-51 per-class head (M = K = 51, bf16, weight images kept by the caller)
            from a resident bf16 cache of --cache-images (2048) maps 14x14x2048, --batch 32.
  cached003_bf16 / eval003_cached_bf16
            the same three variants for the cfg 003 head (pose head 2048 -> 768 -> 16, attention from pose_pre_logits,
            K = 393, caller-held W1 shadow and W2^T image; custom_ops/pose_cache.py) from a resident bf16 cache:
            (a) includes the PoseLabelTable.gather of the step's pose labels, (b) the same label gather.  --steps 100.
  cached_hmdb_perclass_clips_bf16
            cached_hmdb_clips_bf16 with the per-class head (M = K = 51): 81 videos x 25 frames, 8 clips x 4 frames,
            temporal attention; evaluation at 4 x 25.
  epoch002_fp8 / epoch002_bf16
            a whole frozen-feature EPOCH of cfg 002 from the resident cache of cached002_* (--cache-images 2048, --batch
            32: 64 steps, momentum SGD behind every step, a fresh order per epoch), three routes alternating in one
            process, medians of five epochs, wall clock (one synchronise per epoch) and device events: (a) the epoch
            call (apa_epoch_order + apa_attn_head_train_epoch_cached: one foreign call per epoch), (b) the lean loop
            (HeadTrainStep.rebind + run + BoundMomentumSGD.run per step), (c) the deploy loop (FusedHeadStep on a
            CachedBatch + opt.step() per step); and the validation pass, FusedHeadEval.evaluate_cache against the loop
            of FusedHeadEval.__call__ + meter.update.
  epoch_hmdb_clips_fp8 / epoch_hmdb_clips_bf16 / epoch_charades_fp8 / epoch_charades_bf16
            a whole frozen-feature EPOCH of clips at the shapes of cached_hmdb_clips_* / cached_charades_* (81 videos x
            25 frames, --clips 8 x --frames 4 per step: 10 steps, temporal attention, momentum SGD behind every step),
            three routes alternating in one process, medians of five epochs, wall clock and device events as
            epoch002_*: (a) the epoch call (apa_epoch_order + apa_attn_head_train_epoch_cached_clips, draws keyed on the
            device), (b) the lean loop (torch.rand + sample_clips(out=) + HeadTrainStep.run + BoundMomentumSGD.run per
            step), (c) the deploy loop (sample_clips + FusedHeadStep on the CachedClips + opt.step() per step); and the
            validation pass at 4 x 25 uniform frames, FusedHeadEval.evaluate_videos against the per-batch loop.
  cached_hmdb_clips_fp8 / cached_hmdb_clips_bf16 / cached_charades_fp8 / cached_charades_bf16
            one-call CLIP training step from a resident FRAME cache (--cache-images maps in videos of 25 frames, FP8 E4M3
            or bf16): --clips 8 x --frames 4, temporal attention, M = 1; K = 51 with the softmax cross-entropy (HMDB-51)
            or K = 157 with 'multi-label' (Charades).  Three variants alternating in one process, medians of five and
            their spread: (a) the device sampler with fresh draws per step + the cached clip step
            (apa_sample_clip_frames, apa_attn_head_train_step_cached_clips), (b) the sampler + gather + rebind + the
            plain clip step, (c) the plain clip step on one fixed batch; and the evaluation step at 4 clips x 25 frames,
            (a) against (b).
  explain002
            class attention maps of T = 1 and T = 5 chosen classes at the cfg 002 shape (32 x 14x14x2048 fp32, K = 393):
            the one-call evaluation step + cof.attn_explain against the per-op forward with want_topdown=True + torch.gather,
            alternating in one process, medians of five; the explain pass over X and m1s_pool_fwd_kernel by HIP events
            against the 8 TB/s peak.
  frozen002 / frozen003 / frozen_perclass
            the one-call training steps on FROZEN features (APA_FLAG_FROZEN_INPUT: no dX is computed or stored) against
            the same step as it runs today, at the BASELINE shapes (32 x 14x14x2048; cfg 002 fp32 K = 393, cfg 003 bf16
            K = 393, HMDB-51 per-class bf16 K = 51), alternating in one process, medians of five; frozen002 also
            prints the HIP-event times of the two M == 1 streaming kernels for both forms.

  eval_video_perclass / eval_video002 / eval_hico002 / eval_charades_clips
            the evaluation step of the clip and multi-label datasets: HMDB-51's test protocol (4 clips x 25 frames x
            14x14x2048 bf16, K = 51, per-class maps), 8 x 4 frames fp32 K = 51 M = 1 with temporal attention, HICO (32
            images bf16, K = 600, sigmoid scores) and Charades (8 x 4 frames bf16, K = 157, temporal attention, sigmoid
            scores).  Two variants alternate in one process, medians of five: `one_call`
            (apa_attn_head_eval_step_clips: frame pooling, scores and predictions inside the call) and `sequence`, the
            calls deploy.FusedHeadEval made before that entry point existed (HeadEvalStep.run, cof.frame_pool_fwd,
            eval_utils.predict).

  map393    The metric of a validation pass, T = 7000 accumulated score rows of K = 393 classes (--samples / --classes;
            --multi-hot for sigmoid scores against multi-hot targets, e.g. the HICO-like 9600 x 600): the host route
            (eval_utils.Evaluation.result(): one copy, K argsorts, voc_ap loops) against the device route
            (eval_utils.DeviceEvaluation.result(): three launches, one small copy), alternating in one process.
  rank2_002 / rank3_002
            NET.USE_POSE_PRELOGITS_BASED_ATTENTION_RANK = 2 (identity attention) / 3 (relu) on the cfg 002 shape (32 x
            14x14x2048 fp32, K = 393, training).  Three variants alternate in one process, medians of five: `rank_one_call`
            (apa_attn_head_train_step_rank: all R maps in one pass over conv5 per direction), `module_path` (network_fn
            with fuse_ranks=False + gen_losses + autograd: two or R passes of the rank-1 op) and `rank1_one_call`, the
            rank-1 one-call step of the same shape, for scale.

Each builder returns (step_fn, info): `step_fn()` enqueues one step on the current stream; `info`
carries the workload name and the algorithmic work per image.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK = {'bf16': 2500.0, 'f32': 157.3}  # TFLOP/s, dense (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0


L3_BYTES = 256 << 20    # Infinity Cache (MI355X_MICROARCH.md)


def _features(N, P, C, dtype, dev, seed=42):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.relu(torch.randn(N, P, C, generator=g, device=dev)).to(dtype)


def _n_sets(per_set_bytes, rotate):
    """how many (X, dX) buffer sets a workload cycles through: enough that 1.5 x the 256 MiB Infinity Cache lies
    between two uses of the same set (bench.py's headline rule), so that no step finds its feature map cached from
    the previous one.  rotate = 1: one set (kernel-by-kernel profiling of a variant)."""
    if rotate and rotate > 0:
        return int(rotate)
    return max(3, -(-int(1.5 * L3_BYTES) // int(per_set_bytes)))


def _round_robin(runs):
    state = {'i': 0}
    n = len(runs)

    def step():
        runs[state['i'] % n]()
        state['i'] += 1
    return step


def _rot_note(R, per_set_bytes):
    return '; X/dX rotated over {} sets ({:.0f} MB live; workspace and activations shared, as in a training loop)'.format(R, R * per_set_bytes / 1e6) if R > 1 else \
        '; ONE buffer set (features stay in the Infinity Cache between steps)'


def _clip_kwargs(dev, K, frames, temporal):
    """HeadTrainStep / PoseAttnTrainStep keywords of a clip batch (frames > 1): the TemporalAttention conv at its
    initial values (N(0, 1e-3) weights, bias 1 / F, nets_factory.py:366-368) and its gradient buffers"""
    if frames <= 1:
        return {}
    kw = dict(frames=frames)
    if temporal:
        g = torch.Generator().manual_seed(7)
        kw['temporal'] = ((torch.randn(K, generator=g) * 1e-3).to(dev), torch.full((1,), 1.0 / frames, device=dev))
        kw['temporal_grads'] = (torch.empty(K, device=dev), torch.empty(1, device=dev))
    return kw


def build_cfg003(cof, dev, N=32, H=14, K=393, dtype='bf16', rank1=True, one_call=True, rotate=0, frames=1,
                 temporal=False):
    """frames > 1 (one-call form only): the N maps are the folded frames of N / frames clips"""
    C, Cp, J, P = 2048, 768, 16, H * H
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(42)
    per_set = 2 * N * P * C * (2 if dtype == 'bf16' else 4)
    R = _n_sets(per_set, rotate) if (one_call and rank1) else 1
    X = _features(N, P, C, td, dev)
    W1 = (torch.randn(C, Cp, generator=g) / C ** 0.5).to(dev); b1 = torch.zeros(Cp, device=dev)
    W2 = (torch.randn(Cp, J, generator=g) / Cp ** 0.5).to(dev); b2 = torch.zeros(J, device=dev)
    Wa = (torch.randn(Cp, 1, generator=g) / Cp ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    labels = torch.randint(0, K, (N // frames,), generator=g).to(dev)
    lbl = torch.rand(N, P, J, generator=g).to(dev)
    valid = (torch.rand(N, J, generator=g) > 0.3).to(dev)
    flags = cof.attn_flags(False, False, True)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    state = {'pws': None}
    wa_flat = Wa.view(-1)
    # caller-owned activations and gradients: the attention part of the step (pooling forward, softmax
    # cross-entropy, pooling backward) is ONE host call bound to them (cof.HeadTrainStep, the call the
    # headline configuration uses); its attention input is the pose head's Ppre, its attention-branch
    # gradient crosses back to the pose head in rank-1 form (dZ, wa)
    Ppre = torch.empty((N, P, Cp), dtype=td, device=dev)
    Pl = torch.empty((N, P, J), dtype=torch.float32, device=dev)
    dX = torch.empty_like(X)
    dZ = torch.empty((N * P,), dtype=torch.float32, device=dev)
    grads = (dX, dZ, torch.empty_like(Wa), torch.empty_like(ba), torch.empty_like(Wt), torch.empty_like(bt))
    if one_call and rank1:
        # the whole step as ONE host call (apa_pose_attn_train_step): neighbouring ops share launches, and the bf16
        # operand copy of W1 is the caller's -- in a training loop the optimizer's own launch keeps it current
        # (apa_momentum_sgd_step_shadow), here the weights do not change between steps
        w1_bf16 = W1.to(torch.bfloat16).contiguous()
        w2t_bf16 = cof.pose_w2t_image(W2)      # ... and so is the bf16 image of W2^T the Pl product reads
        new = lambda t: torch.empty_like(t)
        pgrads = (new(W1), new(b1), new(W2), new(b2), new(Wa), new(ba), new(Wt), new(bt))
        clip = _clip_kwargs(dev, K, frames, temporal)
        sts = []
        for r in range(R):        # one bound step per (X, dX) set; everything else is shared, as in bench.py's headline:
            #                       weights, parameter gradients, activations, workspaces, dropout counter
            Xr = X if r == 0 else _features(N, P, C, td, dev, seed=42 + r)
            sts.append(cof.PoseAttnTrainStep(Xr, (W1, b1, W2, b2, Wa, ba, Wt, bt), labels, lbl, valid,
                                             (dX if r == 0 else new(Xr),) + pgrads,
                                             flags=flags, keep_prob=0.2, seed=42, offset=ctr, w1_bf16=w1_bf16,
                                             w2t_bf16=w2t_bf16, share_with=sts[0] if sts else None, **clip))
        info = {'workload': 'cfg003 pose-regularised attention head fwd+bwd (pose head 2048->768->16 + M=1 '
                            'pooling + pose L2 + softmax-xent), one host call; per-GPU batch {} x {}x{}x{} {}, K={}, '
                            'dropout keep=0.2'.format(N, H, H, C, dtype, K) + _rot_note(R, per_set),
                'bound': 'mfma', 'dtype': dtype, 'N': N, 'rotate': R,
                'flops_per_image': 3 * (2.0 * P * C * Cp + 2.0 * P * Cp * J)}
        return _round_robin([st.run for st in sts]), info
    if rank1:
        head = cof.HeadTrainStep(X, Ppre, Wa, ba, Wt, bt, labels, grads, flags=flags, keep_prob=0.2, seed=42,
                                 offset=ctr, dxatt_rank1=True)

    def step():
        _, _, state['pws'] = cof.pose_head_fwd(X, W1, b1, W2, b2, workspace=state['pws'], out=(Ppre, Pl))
        _, dPl = cof.pose_l2_loss_fwd_bwd(Pl, lbl, valid)
        if rank1:
            head.run()
            cof.pose_head_bwd(X, W1, W2, Ppre, dPl, None, dX=dX, accumulate_dX=True, workspace=state['pws'],
                              ws_from_fwd=True, ext_rank1=(dZ, wa_flat))
            return
        logits, att, zs, ab, _, state['aws'] = cof.attn_pool_fwd(X, Ppre, Wa, ba, Wt, bt, flags=flags,
                                                                 keep_prob=0.2, seed=42, offset=ctr,
                                                                 workspace=state.get('aws'))
        _, G, _, _ = cof.softmax_xent_fwd_bwd(logits, labels)
        dXs, dXatt, *_ = cof.attn_pool_bwd(X, Ppre, Wa, ba, Wt, bt, att, zs, ab, G, flags=flags, keep_prob=0.2,
                                           seed=42, offset=ctr, workspace=state['aws'])
        cof.pose_head_bwd(X, W1, W2, Ppre, dPl, dXatt, dX=dXs, accumulate_dX=True, workspace=state['pws'],
                          ws_from_fwd=True)

    info = {'workload': 'cfg003 pose-regularised attention head fwd+bwd (pose head 2048->768->16 + M=1 '
                        'pooling + pose L2 + softmax-xent); per-GPU batch {} x {}x{}x{} {}, K={}, dropout '
                        'keep=0.2'.format(N, H, H, C, dtype, K),
            'bound': 'mfma', 'dtype': dtype, 'N': N,
            'flops_per_image': 3 * (2.0 * P * C * Cp + 2.0 * P * Cp * J)}      # fwd + 2x bwd
    return step, info


def build_posebwd(cof, dev, N=32, H=14, dtype='bf16', accumulate=False):
    """the pose head's backward call alone (dPpre rows pass, column sums, dW1 split-K + reduce, dX product) --
    with accumulate=False the dX product runs with beta = 0, the form a plain library GEMM is timed in
    (tools/hipblaslt_ref.py): for kernel-by-kernel comparisons under rocprofv3."""
    C, Cp, J, P = 2048, 768, 16, H * H
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(42)
    X = _features(N, P, C, td, dev)
    W1 = (torch.randn(C, Cp, generator=g) / C ** 0.5).to(dev); b1 = torch.zeros(Cp, device=dev)
    W2 = (torch.randn(Cp, J, generator=g) / Cp ** 0.5).to(dev); b2 = torch.zeros(J, device=dev)
    dPl = torch.randn(N, P, J, generator=g).to(dev)
    Ppre, Pl, ws = cof.pose_head_fwd(X, W1, b1, W2, b2)
    dX = torch.zeros_like(X)

    def step():
        cof.pose_head_bwd(X, W1, W2, Ppre, dPl, None, dX=dX, accumulate_dX=accumulate, workspace=ws)
    info = {'workload': 'pose head backward call alone (beta = {}); per-GPU batch {} x {}x{}x{} {}'.format(
                int(accumulate), N, H, H, C, dtype),
            'bound': 'mfma', 'dtype': dtype, 'N': N, 'flops_per_image': 2 * (2.0 * P * C * Cp)}
    return step, info


def build_perclass(cof, dev, N=32, H=14, K=51, dtype='bf16', rotate=0, weight_images=True, frames=1, temporal=False):
    """frames > 1: the N maps are the folded frames of N / frames clips (apa_attn_head_train_step_clips)"""
    C, P = 2048, H * H
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(42)
    per_set = 2 * N * P * C * (2 if dtype == 'bf16' else 4)
    R = _n_sets(per_set, rotate)
    X = _features(N, P, C, td, dev)
    Wa = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(K, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    labels = torch.randint(0, K, (N // frames,), generator=g).to(dev)
    flags = cof.attn_flags(False, False, True)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    pg = (torch.empty_like(Wa), torch.empty_like(ba), torch.empty_like(Wt), torch.empty_like(bt))
    clip = _clip_kwargs(dev, K, frames, temporal)
    sts = []
    for r in range(R):            # one host call per step, one bound step per (X, dX) set
        Xr = X if r == 0 else _features(N, P, C, td, dev, seed=42 + r)
        # the padded / concatenated bf16 operand images of the weights live in the step's workspace and are kept
        # current at weight-update time (APA_FLAG_WEIGHT_IMAGES: deploy.MomentumSGD.attach_weight_images rewrites them
        # in the optimiser's own launch); here the weights do not change between steps
        sts.append(cof.HeadTrainStep(Xr, Xr, Wa, ba, Wt, bt, labels, (torch.empty_like(Xr), None) + pg, flags=flags,
                                     keep_prob=0.2, seed=42, offset=ctr, weight_images=weight_images,
                                     share_with=sts[0] if sts else None, **clip))
    esz = X.element_size()
    info = {'workload': 'per-class bottom-up maps (M=K, HMDB-51 shape when K=51) attention head fwd+bwd; '
                        'per-GPU batch {} x {}x{}x{} {}, K={}, dropout keep=0.2'.format(N, H, H, C, dtype, K) +
                        ('; weight images kept by the optimiser launch' if weight_images else '') + _rot_note(R, per_set),
            # K = 51: 0.25 GFLOP/img against 3*P*C*s bytes -> HBM-bound; K = 393: MFMA-bound
            'bound': 'hbm' if K <= 128 else 'mfma', 'dtype': dtype, 'N': N, 'rotate': R,
            'flops_per_image': 3 * (2 * 2.0 * P * C * K),              # Z and T products, fwd + 2x bwd
            'bytes_per_image': 3.0 * P * C * esz}
    return _round_robin([st.run for st in sts]), info


def _bucket_and_optimizer(dev, params, regularized, shadows=None):
    """flat gradient bucket + the momentum-SGD of the shipped configs (src/train.py:90-94; lr small enough that the
    synthetic weights stay put over thousands of timed updates, WEIGHT_DECAY as in experiments/*.yaml)"""
    from attentionalpoolingaction_amd import deploy
    bucket = deploy.GradientBucket({n: p.shape for n, p in params.items()}, dev)
    opt = deploy.MomentumSGD(params, bucket, lr=1e-7, momentum=0.9, weight_decay=5e-4, regularized=regularized,
                             bf16_shadows=shadows)
    return bucket, opt


def build_update(cof, dev, which='cfg003', prepared=True, iter_size=1, N=32, H=14, K=None, rotate=0):
    """One parameter UPDATE of a training loop, i.e. what a driver-timed `step` line leaves out (VERDICT r05 Weak #5):
    ITER_SIZE head steps (src/train.py:529-566) + the fused momentum-SGD launch.

      prepared=True   the bf16 operand copies the steps read (cfg 003: W1 shadow, W2^T image; per-class head: the
                      padded / concatenated weight images) are rewritten by the OPTIMISER'S launch
                      (apa_momentum_sgd_step_shadow / _images) -- the shipped arrangement (deploy.FusedHeadStep)
      prepared=False  the steps convert / build them from the fp32 weights in every call, the optimiser launch is the
                      plain apa_momentum_sgd_step -- the arrangement of rounds 1-3
    Both arms do the same arithmetic on the same buffers; the difference is where the preparation runs."""
    C, P = 2048, H * H
    td = torch.bfloat16
    g = torch.Generator().manual_seed(42)
    per_set = 2 * N * P * C * 2
    R = _n_sets(per_set, rotate)
    X = _features(N, P, C, td, dev)
    flags = cof.attn_flags(False, False, True)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    new = lambda t: torch.empty_like(t)
    if which == 'cfg003':
        K = K or 393
        Cp, J = 768, 16
        W1 = (torch.randn(C, Cp, generator=g) / C ** 0.5).to(dev); b1 = torch.zeros(Cp, device=dev)
        W2 = (torch.randn(Cp, J, generator=g) / Cp ** 0.5).to(dev); b2 = torch.zeros(J, device=dev)
        Wa = (torch.randn(Cp, 1, generator=g) / Cp ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
        Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
        labels = torch.randint(0, K, (N,), generator=g).to(dev)
        lbl = torch.rand(N, P, J, generator=g).to(dev)
        valid = (torch.rand(N, J, generator=g) > 0.3).to(dev)
        params = {'pose_w1': W1, 'pose_b1': b1, 'pose_w2': W2, 'pose_b2': b2, 'att_weights': Wa, 'att_biases': ba,
                  'td_weights': Wt, 'td_biases': bt}
        w1_bf16 = torch.empty(W1.shape, dtype=torch.bfloat16, device=dev) if prepared else None
        bucket, opt = _bucket_and_optimizer(dev, params, ['pose_w1', 'pose_w2', 'att_weights', 'td_weights'],
                                            {'pose_w1': w1_bf16} if prepared else None)
        w2t = None
        if prepared:
            w2t = cof.pose_w2t_image(W2)
            opt.add_image('pose_w2', cof.pose_w2t_image_map(w2t, W2), owner=w2t,
                          refresh=lambda: w2t[:J, :Cp].copy_(W2.t()))
        v = bucket.views
        sts = []
        for r in range(R):
            Xr = X if r == 0 else _features(N, P, C, td, dev, seed=42 + r)
            sts.append(cof.PoseAttnTrainStep(
                Xr, (W1, b1, W2, b2, Wa, ba, Wt, bt), labels, lbl, valid,
                (new(Xr), v['pose_w1'], v['pose_b1'], v['pose_w2'], v['pose_b2'], v['att_weights'], v['att_biases'],
                 v['td_weights'], v['td_biases']), flags=flags, keep_prob=0.2, seed=42, offset=ctr, w1_bf16=w1_bf16,
                w2t_bf16=w2t, share_with=sts[0] if sts else None))
        name = 'cfg003 head step (one host call)'
    else:
        K = K or 51
        Wa = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(K, device=dev)
        Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
        labels = torch.randint(0, K, (N,), generator=g).to(dev)
        params = {'att_weights': Wa, 'att_biases': ba, 'td_weights': Wt, 'td_biases': bt}
        bucket, opt = _bucket_and_optimizer(dev, params, ['att_weights', 'td_weights'])
        v = bucket.views
        sts = []
        for r in range(R):
            Xr = X if r == 0 else _features(N, P, C, td, dev, seed=42 + r)
            sts.append(cof.HeadTrainStep(Xr, Xr, Wa, ba, Wt, bt, labels,
                                         (new(Xr), None, v['att_weights'], v['att_biases'], v['td_weights'],
                                          v['td_biases']), flags=flags, keep_prob=0.2, seed=42, offset=ctr,
                                         weight_images=prepared, share_with=sts[0] if sts else None))
        if prepared:       # the R bound steps share ONE workspace, hence one set of images
            opt.attach_weight_images(sts[0], {'Wa': 'att_weights', 'ba': 'att_biases', 'Wt': 'td_weights',
                                              'bt': 'td_biases'})
        name = 'HMDB-51 per-class head step (K={}, one host call)'.format(K)
    rr = _round_robin([st.run for st in sts])
    scale = 1.0 / iter_size

    def update():
        for _ in range(iter_size):
            rr()
        opt.step(grad_scale=scale)
    info = {'workload': 'one UPDATE = {} x {} + the fused momentum-SGD launch ({}); per-GPU batch {} x {}x{}x{} bf16'
                        .format(iter_size, name,
                                'operand copies rewritten by the optimiser launch' if prepared else
                                'plain launch; the steps prepare their bf16 operands themselves',
                                N, H, H, C) + _rot_note(R, per_set),
            'dtype': 'bf16', 'N': N * iter_size, 'rotate': R, 'iter_size': iter_size, 'prepared': bool(prepared)}
    return update, info


def run_update_pair(cof, dev, which, min_ms=50.0, repeats=5, rotate=0):
    """the four driver-timed numbers VERDICT r05 asks for: us per update with the preparation in the optimiser's
    launch vs in every step, at TRAIN.ITER_SIZE 1 and 2"""
    out = {}
    for it in (1, 2):
        row = {}
        for prepared in (True, False):
            fn, info = build_update(cof, dev, which, prepared=prepared, iter_size=it, rotate=rotate)
            sec, reps = timed(fn, 50, 5, min_ms=min_ms, repeats=repeats)
            row['prepared_by_optimizer_us' if prepared else 'prepared_per_step_us'] = round(sec * 1e6, 2)
            row['repeats'] = reps
            row.setdefault('workload', info['workload'] if prepared else None)
            del fn
            torch.cuda.empty_cache()
        row['saving_us_per_update'] = round(row['prepared_per_step_us'] - row['prepared_by_optimizer_us'], 2)
        out['iter_size_%d' % it] = row
    return out


def build_rank1(cof, dev, N=32, H=14, K=51, dtype='bf16', rotate=0):
    """class-agnostic bottom-up map (M = 1, the shipped HMDB / MPII attention configs) on bf16 features:
    the headline op, one host call per step."""
    C, P = 2048, H * H
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(42)
    X = _features(N, P, C, td, dev)
    Wa = (torch.randn(C, 1, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    labels = torch.randint(0, K, (N,), generator=g).to(dev)
    flags = cof.attn_flags(False, False, True)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    per_set = 2 * N * P * C * X.element_size()
    R = _n_sets(per_set, rotate)
    pg = (torch.empty_like(Wa), torch.empty_like(ba), torch.empty_like(Wt), torch.empty_like(bt))
    sts = []
    for r in range(R):
        Xr = X if r == 0 else _features(N, P, C, td, dev, seed=42 + r)
        sts.append(cof.HeadTrainStep(Xr, Xr, Wa, ba, Wt, bt, labels, (torch.empty_like(Xr), None) + pg, flags=flags,
                                     keep_prob=0.2, seed=42, offset=ctr, share_with=sts[0] if sts else None))
    info = {'workload': 'class-agnostic map (M=1) attention head fwd + softmax-xent + bwd; per-GPU batch {} x {}x{}x{} '
                        '{}, K={}, dropout keep=0.2'.format(N, H, H, C, dtype, K) + _rot_note(R, per_set),
            'bound': 'hbm', 'dtype': dtype, 'N': N, 'rotate': R, 'flops_per_image': 0.0,
            'bytes_per_image': 3.0 * P * C * X.element_size()}
    return _round_robin([st.run for st in sts]), info


RANK_WORKLOADS = {'rank2_002': (2, False), 'rank3_002': (3, True)}      # (rank, relu attention)


def build_rank(cof, dev, which, N=32, H=14, K=393, rotate=0):
    """NET.USE_POSE_PRELOGITS_BASED_ATTENTION_RANK = 2 (identity attention) / 3 (relu) on the cfg 002 shape
    (N x 14x14x2048 fp32, K = 393, training, keep 0.2), as round-robin step functions over rotating X sets:
      'rank_one_call'   apa_attn_head_train_step_rank: all R maps in one pass over conv5 per direction
      'module_path'     network_fn (fuse_ranks=False) + gen_losses + backward: two (identity) or R (relu) passes of
                        the rank-1 op per direction, dX summed by autograd
      'rank1_one_call'  the rank-1 one-call step of the same shape and activation, for scale (what the R small
                        products and the wider streaming passes add)"""
    from attentionalpoolingaction_amd import config as apa_config, loss as apa_loss, nets_factory
    R, relu = RANK_WORKLOADS[which]
    C, J, P = 2048, 16, H * H
    g = torch.Generator().manual_seed(42)
    per_set = 2 * N * P * C * 4
    nsets = _n_sets(per_set, rotate)
    Xs = [_features(N, P, C, torch.float32, dev, seed=42 + r) for r in range(nsets)]
    labels = torch.randint(0, K, (N,), generator=g).to(dev)
    apa_config.reset_cfg()
    pre = 'USE_POSE_PRELOGITS_BASED_ATTENTION'
    cfg = apa_config.cfg_from_dict({'MODEL_NAME': 'resnet_v1_101',
                                    'NET': {pre: True, pre + '_SINGLE_LAYER_ATT': True, pre + '_RANK': R,
                                            pre + '_RELU_ATT': relu},
                                    'TRAIN': {'LOSS_FN_POSE': '', 'LOSS_FN_ACTION': 'softmax-xentropy'}})
    network_fn = nets_factory.get_network_fn('resnet_v1_101', K, J, cfg, is_training=True, device=dev)
    head = network_fn.head
    with torch.no_grad():       # trained-looking values: maps of both signs, every rank's gates partly open
        head.att_weights.copy_((torch.randn(C, 1, generator=g) / C ** 0.5).to(dev))
        head.att_biases.fill_(0.1)
        for r, (w, b) in enumerate(((-0.7, 0.2), (1.3, -0.15), (0.6, 0.1))[:R - 1]):
            head.att_weights_r[r].fill_(w)
            head.att_biases_r[r].fill_(b)
        for t in [head.td_weights] + list(head.td_weights_r):
            t.copy_((torch.randn(C, K, generator=g) / C ** 0.5).to(dev))
    params = list(head.parameters())
    p = {n: t.data for n, t in head.named_parameters()}
    Wts = [p['td_weights']] + [p['td_weights_r.%d' % r] for r in range(R - 1)]
    bts = [p['td_biases']] + [p['td_biases_r.%d' % r] for r in range(R - 1)]
    cws = [p['att_weights_r.%d' % r] for r in range(R - 1)]
    cbs = [p['att_biases_r.%d' % r] for r in range(R - 1)]
    flags = cof.attn_flags(False, relu, True)
    like = lambda ts: [torch.empty_like(t) for t in ts]
    pg = (torch.empty_like(p['att_weights']), torch.empty_like(p['att_biases']), like(Wts), like(bts), like(cws),
          like(cbs))
    dXs = [torch.empty_like(x) for x in Xs]
    rank_steps, one_steps = [], []
    for r in range(nsets):
        rank_steps.append(cof.RankHeadTrainStep(
            Xs[r], Xs[r], p['att_weights'], p['att_biases'], Wts, bts, cws, cbs, labels, (dXs[r], None) + pg,
            flags=flags, keep_prob=head.keep_prob, seed=42, offset=r,
            workspace=rank_steps[0].workspace if rank_steps else None))
        one_steps.append(cof.HeadTrainStep(
            Xs[r], Xs[r], p['att_weights'], p['att_biases'], Wts[0], bts[0], labels,
            (dXs[r], None, pg[0], pg[1], pg[2][0], pg[3][0]), flags=flags, keep_prob=head.keep_prob, seed=42, offset=r,
            share_with=one_steps[0] if one_steps else None))
    feats = [x.view(N, H, H, C).requires_grad_(True) for x in Xs]
    tc = cfg.TRAIN

    def module_run(r):
        for t in params:
            t.grad = None
        feats[r].grad = None
        logits, ep = network_fn(feats[r])
        losses = apa_loss.gen_losses(labels, logits, tc.LOSS_FN_ACTION, K, tc.LOSS_FN_ACTION_WT, None, None, '', None,
                                     tc.LOSS_FN_POSE_WT, ep, cfg)
        sum(losses).backward()

    steps = {'rank_one_call': _round_robin([st.run for st in rank_steps]),
             'module_path': _round_robin([(lambda r=r: module_run(r)) for r in range(nsets)]),
             'rank1_one_call': _round_robin([st.run for st in one_steps])}
    info = {'workload': 'rank {} ({} attention) on one bottom-up map, cfg 002 shape: per-GPU batch {} x {}x{}x{} fp32, '
                        'K={}, training, keep={}: one-call rank step vs module path (fuse_ranks=False) vs the rank-1 '
                        'one-call step'.format(R, 'relu' if relu else 'identity', N, H, H, C, K, head.keep_prob) +
                        _rot_note(nsets, per_set),
            'bound': 'hbm', 'dtype': 'f32', 'N': N, 'rotate': nsets, 'flops_per_image': 0.0,
            'bytes_per_image': 3.0 * P * C * 4, 'rank': R}
    return steps, info


def run_rank(cof, dev, args, which):
    """The three variants alternate inside every round (one process, same clocks): per variant the median over five
    (or more) rounds of the mean step time of a loop of `steps` steps, and the spread (max - min) of its rounds."""
    steps, info = build_rank(cof, dev, which, args.batch, args.hw, args.classes or 393, rotate=args.rotate)
    if args.only:
        steps = {args.only: steps[args.only]}
    for fn in steps.values():
        for _ in range(max(args.warmup, info['rotate'])):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in steps}
    rounds = 0
    t_all = time.perf_counter()
    while rounds < 5 or time.perf_counter() - t_all < 0.5:
        for k, fn in steps.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            per[k].append((time.perf_counter() - t0) / args.steps)
        rounds += 1
        if rounds >= 200:
            break
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    out = report(info, med.get('rank_one_call', next(iter(med.values()))), rounds)
    out['rank'] = info['rank']
    out['us_per_step'] = {k: round(v * 1e6, 2) for k, v in med.items()}
    out['us_per_step_min'] = {k: round(min(v) * 1e6, 2) for k, v in per.items()}
    out['us_spread'] = {k: round((max(v) - min(v)) * 1e6, 2) for k, v in per.items()}
    if 'rank_one_call' in med and 'module_path' in med:
        gain = (med['module_path'] - med['rank_one_call']) * 1e6
        out['module_over_one_call'] = round(med['module_path'] / med['rank_one_call'], 3)
        out['faster_by_more_than_the_spreads'] = bool(gain > max(out['us_spread']['rank_one_call'],
                                                                 out['us_spread']['module_path']))
    if 'rank_one_call' in med and 'rank1_one_call' in med:
        out['one_call_over_rank1'] = round(med['rank_one_call'] / med['rank1_one_call'], 3)
    return out


def build_multilabel(cof, dev, which, B=32, F=1, H=14, K=600, rotate=0, kind='multi-label'):
    """`which` in ('hico002', 'charades_clips'): M = 1 head on bf16 features, N = B * F maps (F > 1: clips with the
    TemporalAttention conv).  -> ({'multilabel_one_call', 'module_path', 'softmax_one_call'}: step functions over the
    same rotating X sets, info)."""
    from attentionalpoolingaction_amd import config as apa_config, loss as apa_loss, nets_factory
    N, C, J, P = B * F, 2048, 16, H * H
    td = torch.bfloat16
    g = torch.Generator().manual_seed(42)
    Wa = (torch.randn(C, 1, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    multihot = (torch.rand(B, K, generator=g) < 0.1).float().to(dev)
    labels = torch.randint(0, K, (B,), generator=g).to(dev)
    flags = cof.attn_flags(False, False, True)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    per_set = 2 * N * P * C * 2
    R = _n_sets(per_set, rotate)
    pg = (torch.empty_like(Wa), torch.empty_like(ba), torch.empty_like(Wt), torch.empty_like(bt))
    clip = _clip_kwargs(dev, K, F, True)
    Xs = [_features(N, P, C, td, dev, seed=42 + r) for r in range(R)]
    dXs = [torch.empty_like(x) for x in Xs]
    ml_sts, sm_sts = [], []
    for r in range(R):            # both one-call forms on the SAME X / dX sets
        ml_sts.append(cof.HeadTrainStep(Xs[r], Xs[r], Wa, ba, Wt, bt, multihot, (dXs[r], None) + pg, flags=flags,
                                        keep_prob=0.2, seed=42, offset=ctr, action_loss=kind,
                                        share_with=ml_sts[0] if ml_sts else None, **clip))
        sm_sts.append(cof.HeadTrainStep(Xs[r], Xs[r], Wa, ba, Wt, bt, labels, (dXs[r], None) + pg, flags=flags,
                                        keep_prob=0.2, seed=42, offset=ctr, share_with=sm_sts[0] if sm_sts else None,
                                        **clip))
    apa_config.reset_cfg()
    pre = 'USE_POSE_PRELOGITS_BASED_ATTENTION'
    cfg = apa_config.cfg_from_dict({'MODEL_NAME': 'resnet_v1_101',
                                    'NET': {pre: True, pre + '_SINGLE_LAYER_ATT': True, 'USE_TEMPORAL_ATT': F > 1},
                                    'TRAIN': {'LOSS_FN_POSE': '', 'LOSS_FN_ACTION': kind}})
    network_fn = nets_factory.get_network_fn('resnet_v1_101', K, J, cfg, is_training=True, device=dev)
    params = list(network_fn.head.parameters()) + (list(network_fn.temporal.parameters()) if F > 1 else [])
    shape = (B, F, H, H, C) if F > 1 else (B, H, H, C)
    ins = [x.view(*shape).requires_grad_(True) for x in Xs]
    tc = cfg.TRAIN

    def module_run(r):
        for t in params:
            t.grad = None
        ins[r].grad = None
        logits, ep = network_fn(ins[r])
        losses = apa_loss.gen_losses(multihot, logits, tc.LOSS_FN_ACTION, K, tc.LOSS_FN_ACTION_WT, None, None, '', None,
                                     tc.LOSS_FN_POSE_WT, ep, cfg)
        sum(losses).backward()

    steps = {'multilabel_one_call': _round_robin([st.run for st in ml_sts]),
             'module_path': _round_robin([(lambda r=r: module_run(r)) for r in range(R)]),
             'softmax_one_call': _round_robin([st.run for st in sm_sts])}
    what = 'HICO' if which == 'hico002' else 'Charades'
    info = {'workload': '{} shape, {} x {} frame(s) x {}x{}x{} bf16, K={}, {!r} on the class-agnostic (M=1) head{}: '
                        'one-call multi-label step vs module path vs softmax one-call step'.format(
                            what, B, F, H, H, C, K, kind, ', temporal attention' if F > 1 else '') + _rot_note(R, per_set),
            'bound': 'hbm', 'dtype': 'bf16', 'N': N, 'rotate': R, 'flops_per_image': 0.0,
            'bytes_per_image': 3.0 * P * C * 2}
    return steps, info


def run_multilabel(cof, dev, args, which):
    """The three variants alternate inside every round (one process, same clocks): per variant the median over five (or
    more) rounds of the mean step time of a loop of `steps` steps, and the spread (max - min) of those rounds."""
    hico = which == 'hico002'
    steps, info = build_multilabel(cof, dev, which, B=args.batch if hico else args.clips, F=1 if hico else args.frames,
                                   H=args.hw, K=args.classes or (600 if hico else 157), rotate=args.rotate)
    if args.only:
        steps = {args.only: steps[args.only]}
    for fn in steps.values():
        for _ in range(max(args.warmup, info['rotate'])):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in steps}
    rounds = 0
    t_all = time.perf_counter()
    while rounds < 5 or time.perf_counter() - t_all < 0.5:
        for k, fn in steps.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            per[k].append((time.perf_counter() - t0) / args.steps)
        rounds += 1
        if rounds >= 200:
            break
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    out = report(info, med.get('multilabel_one_call', next(iter(med.values()))), rounds)
    out['us_per_step'] = {k: round(v * 1e6, 2) for k, v in med.items()}
    out['us_per_step_min'] = {k: round(min(v) * 1e6, 2) for k, v in per.items()}
    out['us_per_step_spread'] = {k: round((max(v) - min(v)) * 1e6, 2) for k, v in per.items()}
    if 'module_path' in med and 'multilabel_one_call' in med:
        out['module_path_over_one_call'] = round(med['module_path'] / med['multilabel_one_call'], 2)
    return out


def build_eval002(cof, dev, N=32, H=14, K=393, dtype='f32', rotate=0):
    C, P = 2048, H * H
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(42)
    X = _features(N, P, C, td, dev)
    Wa = (torch.randn(C, 1, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    per_set = N * P * C * X.element_size()              # forward only: X is all that streams
    R = _n_sets(per_set, rotate)
    evs = []
    for r in range(R):
        Xr = X if r == 0 else _features(N, P, C, td, dev, seed=42 + r)
        evs.append(cof.HeadEvalStep(Xr, Xr, Wa, ba, Wt, bt, workspace=evs[0].workspace if evs else None))
    info = {'workload': 'cfg002 eval step (attn-pool forward + softmax + argmax, one call); per-GPU batch '
                        '{} x {}x{}x{} {}, K={}'.format(N, H, H, C, dtype, K) + _rot_note(R, per_set).replace('X/dX', 'X'),
            'bound': 'hbm', 'dtype': dtype, 'N': N, 'rotate': R, 'bytes_per_image': 1.0 * P * C * X.element_size()}
    return _round_robin([ev.run for ev in evs]), info


def build_eval003(cof, dev, N=32, H=14, K=393, dtype='bf16', rotate=0):
    """cfg 003 evaluation step: {'fused': the one-call step, 'fused_shadow': the same with a caller-kept bf16 copy of
    W1, 'sequence': cof.pose_head_fwd + cof.HeadEvalStep on the pose head's Ppre} as round-robin step functions over
    the same rotating X sets (outputs and workspaces shared per variant), + info + a function that times every HOST
    CALL of the variants with HIP events."""
    C, Cp, J, P = 2048, 768, 16, H * H
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(42)
    W1 = (torch.randn(C, Cp, generator=g) / C ** 0.5).to(dev); b1 = torch.zeros(Cp, device=dev)
    W2 = (torch.randn(Cp, J, generator=g) / Cp ** 0.5).to(dev); b2 = torch.zeros(J, device=dev)
    Wa = (torch.randn(Cp, 1, generator=g) / Cp ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    params = (W1, b1, W2, b2, Wa, ba, Wt, bt)
    per_set = N * P * C * (2 if dtype == 'bf16' else 4)          # forward only: X is all that streams
    R = _n_sets(per_set, rotate)
    Xs = [_features(N, P, C, td, dev, seed=42 + r) for r in range(R)]
    w1_bf16 = W1.to(torch.bfloat16).contiguous() if dtype == 'bf16' else None
    fused, shadow, seq_eval = [], [], []
    for Xr in Xs:
        fused.append(cof.PoseAttnEvalStep(Xr, params, workspace=fused[0].workspace if fused else None))
        shadow.append(cof.PoseAttnEvalStep(Xr, params, w1_bf16=w1_bf16,
                                           workspace=shadow[0].workspace if shadow else None))
    Ppre = torch.empty((N, P, Cp), dtype=td, device=dev)
    Pl = torch.empty((N, P, J), dtype=torch.float32, device=dev)
    pws = cof.pose_head_fwd(Xs[0], W1, b1, W2, b2, out=(Ppre, Pl))[2]
    for Xr in Xs:
        seq_eval.append(cof.HeadEvalStep(Xr, Ppre, Wa, ba, Wt, bt,
                                         workspace=seq_eval[0].workspace if seq_eval else None))

    def seq_run(r):
        cof.pose_head_fwd(Xs[r], W1, b1, W2, b2, workspace=pws, out=(Ppre, Pl))
        seq_eval[r].run()

    steps = {'fused': _round_robin([st.run for st in fused]),
             'fused_shadow': _round_robin([st.run for st in shadow]),
             'sequence': _round_robin([(lambda r=r: seq_run(r)) for r in range(R)])}

    def call_times(n=40):
        """median HIP-event time of each host call (events recorded on the stream around the call)"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        acc = {'fused: apa_pose_attn_eval_step': [], 'fused_shadow: apa_pose_attn_eval_step': [],
               'sequence: apa_pose_head_fwd': [], 'sequence: apa_attn_head_eval_step': []}
        for i in range(n):
            r = i % R
            for name, sts in (('fused', fused), ('fused_shadow', shadow)):
                ev[0].record(); sts[r].run(); ev[1].record()
                torch.cuda.synchronize()
                acc[name + ': apa_pose_attn_eval_step'].append(ev[0].elapsed_time(ev[1]))
            ev[0].record()
            cof.pose_head_fwd(Xs[r], W1, b1, W2, b2, workspace=pws, out=(Ppre, Pl))
            ev[1].record()
            seq_eval[r].run()
            ev[2].record()
            torch.cuda.synchronize()
            acc['sequence: apa_pose_head_fwd'].append(ev[0].elapsed_time(ev[1]))
            acc['sequence: apa_attn_head_eval_step'].append(ev[1].elapsed_time(ev[2]))
        return {k: round(sorted(v)[len(v) // 2] * 1e3, 2) for k, v in acc.items()}

    info = {'workload': 'cfg003 eval step (pose head 2048->768 + attention from pose_pre_logits + M=1 pooling + softmax '
                        '+ argmax); per-GPU batch {} x {}x{}x{} {}, K={}'.format(N, H, H, C, dtype, K) +
                        _rot_note(R, per_set).replace('X/dX', 'X'),
            'bound': 'mfma', 'dtype': dtype, 'N': N, 'rotate': R, 'flops_per_image': 2.0 * P * C * Cp,
            'routes': lambda: {'fused': fused[0].route, 'fused_shadow': shadow[0].route}}
    return steps, info, call_times


def run_eval003(cof, dev, args):
    """The variants alternate inside every round (one process, same buffers, same clocks): per variant the median over
    the rounds of the mean step time of a loop of `steps` steps."""
    steps, info, call_times = build_eval003(cof, dev, args.batch, args.hw, args.classes or 393, args.dtype or 'bf16',
                                            rotate=args.rotate)
    for fn in steps.values():
        for _ in range(max(args.warmup, info['rotate'])):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in steps}
    rounds = 0
    t_all = time.perf_counter()
    while rounds < 9 or time.perf_counter() - t_all < 0.5:
        for k, fn in steps.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            per[k].append((time.perf_counter() - t0) / args.steps)
        rounds += 1
        if rounds >= 200:
            break
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    out = report(info, med['fused'], rounds)
    out['us_per_step'] = {k: round(v * 1e6, 2) for k, v in med.items()}
    out['us_per_step_min'] = {k: round(min(v) * 1e6, 2) for k, v in per.items()}
    out['routes'] = info['routes']()
    out['us_per_call_hip_events'] = call_times()
    return out


EVAL_CLIPS = {   # clips, frames, dtype, K, per-class maps, temporal attention, multi-label (sigmoid) scores
    'eval_video_perclass': dict(B=4, F=25, dtype='bf16', K=51, per_class=True, temporal=False, multi_label=False),
    'eval_video002': dict(B=8, F=4, dtype='f32', K=51, per_class=False, temporal=True, multi_label=False),
    'eval_hico002': dict(B=32, F=1, dtype='bf16', K=600, per_class=False, temporal=False, multi_label=True),
    'eval_charades_clips': dict(B=8, F=4, dtype='bf16', K=157, per_class=False, temporal=True, multi_label=True),
}


def build_eval_clips(cof, dev, which, H=14, rotate=0):
    """The evaluation step of a clip / multi-label dataset, {'one_call', 'sequence'} as round-robin step functions over
    the same rotating X sets:
      'one_call'  cof.HeadEvalStep(frames=, temporal=, scores=): apa_attn_head_eval_step_clips
      'sequence'  what deploy.FusedHeadEval ran before that entry point: the flat HeadEvalStep (its softmax / argmax over
                  the frame logits are not read), cof.frame_pool_fwd on clips, then eval_utils.predict on the (pooled)
                  logits -- for clips and for the sigmoid scores; its tensors are allocated per call, as they were."""
    from attentionalpoolingaction_amd import eval_utils
    w = EVAL_CLIPS[which]
    B, F, K, C, P = w['B'], w['F'], w['K'], 2048, H * H
    N, M = B * F, (w['K'] if w['per_class'] else 1)
    td = torch.bfloat16 if w['dtype'] == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(42)
    Wa = (torch.randn(C, M, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(M, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    temporal = _clip_kwargs(dev, K, F, True)['temporal'] if w['temporal'] else None
    tw, tb = temporal if temporal else (None, None)
    per_set = N * P * C * (2 if w['dtype'] == 'bf16' else 4)          # forward only: X is all that streams
    R = _n_sets(per_set, rotate)
    Xs = [_features(N, P, C, td, dev, seed=42 + r) for r in range(R)]
    one, seq = [], []
    for Xr in Xs:
        one.append(cof.HeadEvalStep(Xr, Xr, Wa, ba, Wt, bt, frames=F, temporal=temporal,
                                    scores='sigmoid' if w['multi_label'] else 'softmax',
                                    workspace=one[0].workspace if one else None))
        seq.append(cof.HeadEvalStep(Xr, Xr, Wa, ba, Wt, bt, workspace=seq[0].workspace if seq else None))

    def seq_run(r):
        st = seq[r]
        st.run()
        logits = st.logits
        if F > 1:
            logits, _ = cof.frame_pool_fwd(st.logits, F, tw, tb)
        return eval_utils.predict(logits, multi_label=w['multi_label'])

    steps = {'one_call': _round_robin([st.run for st in one]),
             'sequence': _round_robin([(lambda r=r: seq_run(r)) for r in range(R)])}
    info = {'workload': '{}: evaluation step, {} x {} frames x {}x{}x{} {}, K={}, {}, {}, {} scores; one call '
                        '(apa_attn_head_eval_step_clips) against HeadEvalStep.run + frame_pool_fwd + eval_utils.predict'
                        .format(which, B, F, H, H, C, w['dtype'], K, 'per-class maps' if w['per_class'] else 'M = 1',
                                'temporal attention' if w['temporal'] else 'plain mean over the frames',
                                'sigmoid' if w['multi_label'] else 'softmax') +
                        _rot_note(R, per_set).replace('X/dX', 'X'),
            'dtype': w['dtype'], 'N': N, 'rotate': R, 'entry': one[0]._name}
    return steps, info


def run_eval_clips(cof, dev, args, which):
    """The two variants ALTERNATING in one process: five timed loops of each, interleaved; medians, and per variant the
    spread (max - min) of its five loops.  --only: one variant alone (kernel traces); `steps_run` is then the number of
    steps behind the trace's call counts."""
    steps, info = build_eval_clips(cof, dev, which, args.hw, args.rotate)
    if args.only:
        steps = {args.only: steps[args.only]}
    warm = max(args.warmup, info['rotate'])
    for fn in steps.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in steps}
    for _ in range(5):
        for name, fn in steps.items():
            sec, _ = timed(fn, args.steps, 0, min_ms=0.0, repeats=1)
            runs[name].append(sec * 1e6)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    out = {'workload': info['workload'], 'entry': info['entry'], 'dtype': info['dtype'], 'rotate': info['rotate'],
           'us_per_step': {k: round(v, 2) for k, v in med.items()},
           'us_per_step_runs': {k: [round(x, 2) for x in v] for k, v in runs.items()},
           'us_per_step_spread': {k: round(max(v) - min(v), 2) for k, v in runs.items()},
           'steps_run': warm + 5 * args.steps}
    if 'one_call' in med and 'sequence' in med:
        out['one_call_minus_sequence_us'] = round(med['one_call'] - med['sequence'], 2)
        out['one_call_within_sequence_spread'] = bool(
            med['one_call'] - med['sequence'] <= max(runs['sequence']) - min(runs['sequence']))
    return out


def build_video(cof, dev, which, B=8, F=4, H=14, K=51, rotate=0):
    """A clip batch [B,F,H,H,2048] bf16 with temporal attention, `which` in ('perclass', 'cfg003'):
      'clip_one_call'  the one-call clip step (build_perclass / build_cfg003 with frames=F)
      'flat_one_call'  the same head's flat one-call step on N = B * F images (cross-entropy folded)
      'module_path'    network_fn([B,F,H,H,C]) + gen_losses + backward, the only route for a clip before the clip steps
    as round-robin step functions over rotating X sets, + info + a function timing the clip loss's own call."""
    from attentionalpoolingaction_amd import config as apa_config, loss as apa_loss, nets_factory
    N, C, J, P = B * F, 2048, 16, H * H
    build = build_perclass if which == 'perclass' else build_cfg003
    clip_step, info = build(cof, dev, N, H, K, 'bf16', rotate=rotate, frames=F, temporal=True)
    flat_step, _ = build(cof, dev, N, H, K, 'bf16', rotate=rotate)
    R = info['rotate']
    apa_config.reset_cfg()
    pre = 'USE_POSE_PRELOGITS_BASED_ATTENTION'
    if which == 'perclass':
        net, train = {pre: True, pre + '_SINGLE_LAYER_ATT': True, pre + '_PER_CLASS': True}, {'LOSS_FN_POSE': ''}
    else:
        net, train = {pre: True}, {'LOSS_FN_POSE': 'l2'}
    cfg = apa_config.cfg_from_dict({'MODEL_NAME': 'resnet_v1_101', 'NET': dict(net, USE_TEMPORAL_ATT=True),
                                    'TRAIN': dict(train, LOSS_FN_ACTION='softmax-xentropy')})
    network_fn = nets_factory.get_network_fn('resnet_v1_101', K, J, cfg, is_training=True, device=dev)
    params = list(network_fn.head.parameters()) + list(network_fn.temporal.parameters())
    g = torch.Generator().manual_seed(42)
    labels = torch.randint(0, K, (B,), generator=g).to(dev)
    use_pose = which == 'cfg003'
    lbl = torch.rand(N, H, H, J, generator=g).to(dev) if use_pose else None
    valid = (torch.rand(N, J, generator=g) > 0.3).to(dev) if use_pose else None
    clips = [_features(N, P, C, torch.bfloat16, dev, seed=42 + r).view(B, F, H, H, C).requires_grad_(True)
             for r in range(R)]
    tc = cfg.TRAIN

    def module_run(r):
        for t in params:
            t.grad = None
        clips[r].grad = None
        logits, ep = network_fn(clips[r])
        losses = apa_loss.gen_losses(labels, logits, tc.LOSS_FN_ACTION, K, tc.LOSS_FN_ACTION_WT, lbl,
                                     ep.get('PoseLogits') if use_pose else None, tc.LOSS_FN_POSE if use_pose else '',
                                     valid, tc.LOSS_FN_POSE_WT, ep, cfg)
        sum(losses).backward()

    steps = {'clip_one_call': clip_step, 'module_path': _round_robin([(lambda r=r: module_run(r)) for r in range(R)]),
             'flat_one_call': flat_step}

    def clip_loss_us(n=200):
        """median HIP-event time of apa_clip_xent_fwd_bwd alone (its two launches) on [N,K] frame logits"""
        x = torch.randn(N, K, device=dev)
        tw, tb = _clip_kwargs(dev, K, F, True)['temporal']
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ws = torch.empty((max(cof.clip_xent_workspace_bytes(B, F, K), 16),), dtype=torch.uint8, device=dev)
        ts = []
        for _ in range(n):
            ev[0].record()
            cof.clip_xent_fwd_bwd(x, labels, F, tw, tb, workspace=ws)
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]))
        return round(sorted(ts)[len(ts) // 2] * 1e3, 2)

    info = dict(info, workload='clip batch {} x {} frames x {}x{}x{} bf16, K={}, temporal attention, {} head: one-call '
                               'clip step vs module path vs flat one-call step at N={}'.format(
                                   B, F, H, H, C, K, 'per-class (HMDB-51)' if which == 'perclass' else 'cfg 003', N) +
                               _rot_note(R, 2 * N * P * C * 2))
    return steps, info, clip_loss_us


def run_video(cof, dev, args, which):
    """The variants alternate inside every round (one process, same clocks): per variant the median over five (or
    more) rounds of the mean step time of a loop of `steps` steps."""
    steps, info, clip_loss_us = build_video(cof, dev, which, args.clips, args.frames, args.hw, args.classes or 51,
                                            rotate=args.rotate)
    if args.only:
        steps = {args.only: steps[args.only]}
    for fn in steps.values():
        for _ in range(max(args.warmup, info['rotate'])):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in steps}
    rounds = 0
    t_all = time.perf_counter()
    while rounds < 5 or time.perf_counter() - t_all < 0.5:
        for k, fn in steps.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            per[k].append((time.perf_counter() - t0) / args.steps)
        rounds += 1
        if rounds >= 200:
            break
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    out = report(info, med.get('clip_one_call', next(iter(med.values()))), rounds)
    out['us_per_step'] = {k: round(v * 1e6, 2) for k, v in med.items()}
    out['us_per_step_min'] = {k: round(min(v) * 1e6, 2) for k, v in per.items()}
    out['clip_loss_call_us_hip_events'] = clip_loss_us()
    return out


# algorithmic HBM bytes of the four pose-attention kernels (fp32 parameters / F / logits; X and dX in the feature dtype)
def poseatt_kernel_bytes(N, P, C, J, M, K, xbytes):
    R = M * C
    return {
        'pool_fwd': N * P * C * xbytes + N * P * J * 4 + N * R * 4,                 # X, Pl -> F
        'cls_fwd': R * K * 4 + N * R * 4 + N * K * 4,                                # W, F -> logits
        'cls_bwd': 2 * R * K * 4 + N * R * 4 + N * K * 4,                            # W, F, G -> dW, (dF)
        'pool_bwd': 2 * N * P * C * xbytes + 2 * N * P * J * 4,                      # X, Pl -> dX, dPl
    }


def build_poseatt(cof, dev, N=32, H=14, K=393, dtype='f32', rotate=0):
    """USE_POSE_ATTENTION_LOGITS, one training step: pose head fwd, pooling fwd, classifier fwd, softmax-xent,
    pose L2, classifier bwd, pooling bwd, pose head bwd.  X / dX AND W / dW rotate over enough sets that 1.5 x the
    Infinity Cache lies between two uses (the backbone evicts them between real steps).  Returns the step and a
    function that times the four new kernels with HIP events (apa_pose_att_logits_*_ex hooks)."""
    C, P, J, Cp = 2048, H * H, 16, 768
    parts, avged = list(range(J)), False
    M = cof.pose_att_num_maps(parts, avged)
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator().manual_seed(42)
    W1 = (torch.randn(C, Cp, generator=g) * 0.001).to(dev); b1 = torch.zeros(Cp, device=dev)
    W2 = (torch.randn(Cp, J, generator=g) * (2.6 / Cp) ** 0.5).to(dev); b2 = torch.zeros(J, device=dev)
    b = torch.zeros(K, device=dev)
    labels = torch.randint(0, K, (N,), generator=g).to(dev)
    lbl = torch.rand(N, P, J, generator=g).to(dev)
    valid = (torch.rand(N, J, generator=g) > 0.3).to(dev)
    xb = torch.finfo(td).bits // 8
    per_set = 2 * N * P * C * xb + 2 * M * C * K * 4
    R = _n_sets(per_set, rotate)
    sets = []
    for r in range(R):
        X = _features(N, P, C, td, dev, seed=42 + r)
        W = (torch.randn(M * C, K, generator=torch.Generator().manual_seed(7 + r)) * 0.001).to(dev)
        sets.append((X, W, torch.empty_like(X)))
    flags = cof.attn_flags(is_training=True)
    ws = {}

    def step_on(X, W, dX, hooks=None, state={'offset': 0}):
        off = state['offset']
        state['offset'] += 1
        Ppre, Pl, pws = cof.pose_head_fwd(X, W1, b1, W2, b2, workspace=ws.get('pose'))
        ws['pose'] = pws
        F, logits, aws = cof.pose_att_logits_fwd(X, Pl, parts, avged, W, b, flags=flags, keep_prob=0.2, seed=42,
                                                 offset=off, workspace=ws.get('att'), hooks=hooks[0] if hooks else None)
        ws['att'] = aws
        _, G, _, _ = cof.softmax_xent_fwd_bwd(logits, labels)
        _, dPl = cof.pose_l2_loss_fwd_bwd(Pl, lbl, valid)
        _, dPl, dW, db = cof.pose_att_logits_bwd(X, Pl, parts, avged, W, F, G, dPl, dX=dX, flags=flags,
                                                 keep_prob=0.2, seed=42, offset=off, workspace=aws,
                                                 hooks=hooks[1] if hooks else None)
        cof.pose_head_bwd(X, W1, W2, Ppre, dPl, None, dX=dX, accumulate_dX=True, workspace=pws, ws_from_fwd=True)

    def kernel_times(n=20):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        for e in evs:
            e.record()
        hf = cof.make_hooks(prof_fwd=(evs[0], evs[1]), prof_bwd=(evs[2], evs[3]))
        hb = cof.make_hooks(prof_fwd=(evs[4], evs[5]), prof_bwd=(evs[6], evs[7]))
        acc = {'pool_fwd': [], 'cls_fwd': [], 'cls_bwd': [], 'pool_bwd': []}
        for i in range(n):
            X, W, dX = sets[i % R]
            step_on(X, W, dX, hooks=(hf, hb))
            torch.cuda.synchronize()
            acc['pool_fwd'].append(evs[0].elapsed_time(evs[1]))
            acc['cls_fwd'].append(evs[2].elapsed_time(evs[3]))
            acc['pool_bwd'].append(evs[4].elapsed_time(evs[5]))
            acc['cls_bwd'].append(evs[6].elapsed_time(evs[7]))
        byt = poseatt_kernel_bytes(N, P, C, J, M, K, xb)
        out = {}
        for k, v in acc.items():
            v.sort()
            us = v[len(v) // 2] * 1e3
            out[k] = {'us': round(us, 2), 'algorithmic_MB': round(byt[k] / 1e6, 1),
                      'hbm_frac': round(byt[k] / (us * 1e-6) / (HBM_PEAK_GBS * 1e9), 3)}
        return out

    runs = [(lambda s=s: step_on(*s)) for s in sets]
    info = {'workload': 'USE_POSE_ATTENTION_LOGITS training step (pose head 2048->768->16, M={} maps, classifier '
                        '{}x{} fp32, xent, pose L2, backward); per-GPU batch {} x {}x{}x{} {}'.format(
                            M, M * C, K, N, H, H, C, dtype) + _rot_note(R, per_set).replace('X/dX', 'X/dX/W'),
            'bound': 'hbm', 'dtype': dtype, 'N': N, 'rotate': R,
            'bytes_per_image': sum(poseatt_kernel_bytes(N, P, C, J, M, K, xb).values()) / N}
    return _round_robin(runs), info, kernel_times


def build_frozen(cof, dev, which, frozen, N=32, H=14, rotate=0):
    """One-call training steps on FROZEN features (APA_FLAG_FROZEN_INPUT: None in the dX slot) or, frozen=False, the
    same step as it runs today -- the BASELINE shapes: 32 x 14x14x2048; frozen002: cfg 002, fp32, K = 393;
    frozen003: cfg 003, bf16, K = 393; frozen_perclass: HMDB-51 per-class maps, bf16, K = 51.  The feature maps rotate
    over the same number of sets in both forms (sized for the full step's X + dX).  -> (step, steps_list, info)"""
    C, P = 2048, H * H
    dtype = 'f32' if which == 'frozen002' else 'bf16'
    td = torch.float32 if dtype == 'f32' else torch.bfloat16
    K = 51 if which == 'frozen_perclass' else 393
    g = torch.Generator().manual_seed(42)
    per_set = 2 * N * P * C * (4 if dtype == 'f32' else 2)
    R = _n_sets(per_set, rotate)
    Xs = [_features(N, P, C, td, dev, seed=42 + r) for r in range(R)]
    dx = (lambda X: None) if frozen else (lambda X: torch.empty_like(X))
    flags = cof.attn_flags(False, False, True)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    labels = torch.randint(0, K, (N,), generator=g).to(dev)
    new = lambda t: torch.empty_like(t)
    sts = []
    if which == 'frozen003':
        Cp, J = 768, 16
        W1 = (torch.randn(C, Cp, generator=g) / C ** 0.5).to(dev); b1 = torch.zeros(Cp, device=dev)
        W2 = (torch.randn(Cp, J, generator=g) / Cp ** 0.5).to(dev); b2 = torch.zeros(J, device=dev)
        Wa = (torch.randn(Cp, 1, generator=g) / Cp ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
        Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
        lbl = torch.rand(N, P, J, generator=g).to(dev)
        valid = (torch.rand(N, J, generator=g) > 0.3).to(dev)
        params = (W1, b1, W2, b2, Wa, ba, Wt, bt)
        pgrads = tuple(new(t) for t in params)
        w1_bf16, w2t_bf16 = W1.to(torch.bfloat16).contiguous(), cof.pose_w2t_image(W2)
        for X in Xs:
            sts.append(cof.PoseAttnTrainStep(X, params, labels, lbl, valid, (dx(X),) + pgrads, flags=flags,
                                             keep_prob=0.2, seed=42, offset=ctr, w1_bf16=w1_bf16, w2t_bf16=w2t_bf16,
                                             share_with=sts[0] if sts else None))
    else:
        M = K if which == 'frozen_perclass' else 1
        Wa = (torch.randn(C, M, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(M, device=dev)
        Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
        pg = (new(Wa), new(ba), new(Wt), new(bt))
        for X in Xs:
            sts.append(cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, labels, (dx(X), None) + pg, flags=flags, keep_prob=0.2,
                                         seed=42, offset=ctr, weight_images=M > 1, share_with=sts[0] if sts else None))
    info = {'dtype': dtype, 'N': N, 'K': K, 'rotate': R,
            'shape': '{} x {}x{}x{} {}, K={}, dropout keep=0.2'.format(N, H, H, C, dtype, K)}
    return _round_robin([st.run for st in sts]), sts, info


def run_frozen(cof, dev, args, which):
    """The frozen step and today's step ALTERNATING in one process: five timed loops of each, interleaved; medians.
    The yardstick is the full step of the same process.  frozen002 also reports the two streaming kernels of the
    M == 1 head by HIP events (apa_hooks prof_*, cof.KernelTimer) for both forms."""
    full, full_sts, info = build_frozen(cof, dev, which, False, args.batch, args.hw, args.rotate)
    froz, froz_sts, _ = build_frozen(cof, dev, which, True, args.batch, args.hw, args.rotate)
    for _ in range(args.warmup):
        full(); froz()
    torch.cuda.synchronize()
    assert all(st.frozen_input for st in froz_sts), 'the library refused the flag: the frozen form ran the full step'
    runs = {'full': [], 'frozen': []}
    for _ in range(5):
        for name, fn in (('full', full), ('frozen', froz)):
            sec, _ = timed(fn, args.steps, 0, min_ms=0.0, repeats=1)
            runs[name].append(sec * 1e6)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    out = {'workload': '{}: one-call training step on frozen features (APA_FLAG_FROZEN_INPUT) against the same step '
                       'writing dX, alternating in one process; {}'.format(which, info['shape']) +
                       _rot_note(info['rotate'], 2 * info['N'] * args.hw * args.hw * 2048 * (4 if info['dtype'] == 'f32' else 2)),
           'us_per_step': {k: round(v, 2) for k, v in med.items()},
           'us_per_step_runs': {k: [round(x, 2) for x in v] for k, v in runs.items()},
           'frozen_over_full': round(med['frozen'] / med['full'], 4), 'dtype': info['dtype'], 'rotate': info['rotate']}
    if which == 'frozen002':        # per-kernel HIP-event times of the two streaming passes, one step each form in turn
        n = 20
        kt = {'full': cof.KernelTimer(n), 'frozen': cof.KernelTimer(n)}
        for i in range(n):
            for name, sts in (('full', full_sts), ('frozen', froz_sts)):
                sts[i % len(sts)].run(hooks=kt[name].hooks(i))
        torch.cuda.synchronize()
        med_us = lambda v: round(sorted(v)[len(v) // 2] * 1e3, 2)
        out['kernels_us'] = {name: {'m1s_pool_fwd_kernel': med_us(t.fwd_elapsed_ms()),
                                    'm1s_bwd_main_kernel': med_us(t.bwd_elapsed_ms())} for name, t in kt.items()}
        for t in kt.values():
            t.close()
    return out


def build_fp8(cof, dev, train, fp8, N=32, H=14, rotate=0):
    """cfg 002 on cached conv5 features, 14x14x2048, K = 393: the frozen one-call training step (train=True, dropout
    keep 0.2, None in the dX slot) or the one-call evaluation step, on an FP8 E4M3 cache (fp8=True: Fp8Features, the
    bf16 maps quantised) or on the bf16 maps themselves.  Each form rotates over enough sets of ITS OWN size that 1.5 x
    the Infinity Cache lies between two uses of a set.  -> (step, steps_list, info)"""
    C, P, K = 2048, H * H, 393
    g = torch.Generator().manual_seed(42)
    per_set = N * P * C * (1 if fp8 else 2)
    R = _n_sets(per_set, rotate)
    Xs = []
    for r in range(R):
        X = _features(N, P, C, torch.bfloat16, dev, seed=42 + r)
        if fp8:
            X, status = cof.quantize_features(X)
            assert int(status.sum()) == 0
        Xs.append(X)
    Wa = (torch.randn(C, 1, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    labels = torch.randint(0, K, (N,), generator=g).to(dev)
    sts = []
    if train:
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        pg = tuple(torch.empty_like(t) for t in (Wa, ba, Wt, bt))
        for X in Xs:
            sts.append(cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, labels, (None, None) + pg,
                                         flags=cof.attn_flags(False, False, True), keep_prob=0.2, seed=42, offset=ctr,
                                         share_with=sts[0] if sts else None))
    else:
        for X in Xs:
            sts.append(cof.HeadEvalStep(X, X, Wa, ba, Wt, bt, workspace=sts[0].workspace if sts else None))
    info = {'N': N, 'rotate': R, 'bytes_per_step': per_set, 'params': (Wa, ba, Wt, bt), 'features': Xs,
            'shape': '{} x {}x{}x{}, K={}'.format(N, H, H, C, K) + (', dropout keep=0.2' if train else '')}
    return _round_robin([st.run for st in sts]), sts, info


def run_fp8(cof, dev, args, which):
    """frozen002_fp8 / eval002_fp8: the FP8 and the bf16 form ALTERNATING in one process, five timed loops of each,
    interleaved; medians and the loops' spread.  Then the streaming kernels of both forms by HIP events (apa_hooks
    prof_*: the pooling pass of the forward half, the main pass of the backward half) with their algorithmic bytes per
    second -- the feature bytes each pass reads once -- against the HBM peak."""
    train = which == 'frozen002_fp8'
    forms = {}
    for name, fp8 in (('bf16', False), ('fp8', True)):
        forms[name] = build_fp8(cof, dev, train, fp8, args.batch, args.hw, args.rotate)
    for _ in range(args.warmup):
        for step, _, _ in forms.values():
            step()
    torch.cuda.synchronize()
    if train:
        assert all(st.frozen_input for _, sts, _ in forms.values() for st in sts)
    runs = {k: [] for k in forms}
    for _ in range(5):
        for name, (step, _, _) in forms.items():
            sec, _ = timed(step, args.steps, 0, min_ms=0.0, repeats=1)
            runs[name].append(sec * 1e6)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    info = forms['fp8'][2]
    out = {'workload': '{}: cfg 002 one-call {} step on an FP8 E4M3 feature cache against the same step on the bf16 '
                       'maps, alternating in one process; {}; each form rotates over its own sets ({} bf16 / {} fp8)'.format(
                           which, 'frozen training' if train else 'evaluation', info['shape'],
                           forms['bf16'][2]['rotate'], info['rotate']),
           'us_per_step': {k: round(v, 2) for k, v in med.items()},
           'us_per_step_runs': {k: [round(x, 2) for x in v] for k, v in runs.items()},
           'us_per_step_spread': {k: round(max(v) - min(v), 2) for k, v in runs.items()},
           'fp8_over_bf16': round(med['fp8'] / med['bf16'], 4)}
    n = 20
    med_us = lambda v: sorted(v)[len(v) // 2] * 1e3
    out['kernels_us'], out['kernels_gbs'], out['kernels_frac_of_hbm_peak'] = {}, {}, {}
    for name, (_, sts, inf) in forms.items():
        kt = cof.KernelTimer(n)
        Wa, ba, Wt, bt = inf['params']
        for i in range(n):
            if train:
                sts[i % len(sts)].run(hooks=kt.hooks(i))
            else:       # the evaluation step takes no hooks: its pooling pass through the forward entry point
                X = inf['features'][i % len(sts)]
                cof.attn_pool_fwd(X, X, Wa, ba, Wt, bt, workspace=sts[0].workspace, hooks=kt.hooks(i))
        torch.cuda.synchronize()
        t = {'pool_fwd': med_us(kt.fwd_elapsed_ms())}
        if train:
            t['bwd_main'] = med_us(kt.bwd_elapsed_ms())
        kt.close()
        out['kernels_us'][name] = {k: round(v, 2) for k, v in t.items()}
        out['kernels_gbs'][name] = {k: round(inf['bytes_per_step'] / v / 1e3, 1) for k, v in t.items()}
        out['kernels_frac_of_hbm_peak'][name] = {k: round(inf['bytes_per_step'] / v / 1e3 / HBM_PEAK_GBS, 4)
                                                 for k, v in t.items()}
    return out


def build_cached(cof, dev, fp8, N=512, H=14, T=2048, per_class=False):
    """cfg 002 frozen one-call training step (dropout keep 0.2, K = 393) from a RESIDENT cache of T 14x14x2048 maps (FP8
    E4M3 or bf16) with its labels, three ways: (a) the gathered step on cache.select(index), a fresh shuffled index
    per step (epoch() views, re-bound); (b) today's loop: cache.gather(index) + labels[index] + rebind + the plain
    step; (c) the plain step on one fixed contiguous batch of the cache.  per_class: the HMDB-51 per-class head instead
    (M = K = 51, weight images kept by the caller, as frozen_perclass runs it).  -> ({name: step}, info)"""
    C, P, K = 2048, H * H, 51 if per_class else 393
    M = K if per_class else 1
    T = max(int(T), 4 * N)
    g = torch.Generator().manual_seed(42)
    labels = torch.randint(0, K, (T,), generator=g).to(dev)
    cache = cof.FeatureCache.empty((T, H, H, C), torch.float8_e4m3fn if fp8 else torch.bfloat16, dev, labels=labels)
    for first in range(0, T, 256):
        n = min(256, T - first)
        status = cache.write(first, _features(n, P, C, torch.bfloat16, dev, seed=42 + first).view(n, H, H, C))
        assert int(status.sum()) == 0
    Wa = (torch.randn(C, M, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(M, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    pg = tuple(torch.empty_like(t) for t in (Wa, ba, Wt, bt))
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    kw = dict(flags=cof.attn_flags(False, False, True), keep_prob=0.2, seed=42, offset=ctr, weight_images=per_class)
    batches = [b for e in range(4) for b in cache.epoch(N, seed=e)]        # four epochs' shuffled batches, int32 views
    batch0 = cache.select(batches[0])
    st_a = cof.HeadTrainStep(batch0, batch0, Wa, ba, Wt, bt, None, (None, None) + pg, **kw)
    X0 = cache.gather(batches[0])
    st_b = cof.HeadTrainStep(X0, X0, Wa, ba, Wt, bt, labels[:N].clone(), (None, None) + pg, **kw)
    f = cache.features
    Xc = cof.Fp8Features.from_parts(f.codes[:N], f.scale[:N]) if fp8 else f[:N]
    st_c = cof.HeadTrainStep(Xc, Xc, Wa, ba, Wt, bt, labels[:N].contiguous(), (None, None) + pg, **kw)
    state = {'a': 0, 'b': 0}

    def step_a():
        st_a.rebind(index=batches[state['a'] % len(batches)])
        state['a'] += 1
        st_a.run()

    def step_b():
        idx = batches[state['b'] % len(batches)]
        state['b'] += 1
        st_b.rebind(X=cache.gather(idx), labels=labels[idx.long()])
        st_b.run()

    bytes_img = P * C * (1 if fp8 else 2)
    info = {'N': N, 'T': T, 'shape': '{} of {} x {}x{}x{}, K={}, dropout keep=0.2'.format(N, T, H, H, C, K),
            'feature_bytes_per_step': 2 * N * bytes_img, 'gather_bytes_per_step': 2 * N * bytes_img,
            'cache_bytes': T * bytes_img, 'steps': (st_a, st_b, st_c)}
    return {'a_gathered': step_a, 'b_gather_rebind_plain': step_b, 'c_plain_fixed': st_c.run}, info


def run_cached(cof, dev, args, which):
    """cached002_fp8 / cached002_bf16: the three variants ALTERNATING in one process, five timed loops of each,
    interleaved; medians and the loops' spread.  a - c: what the gathered step costs over the plain step on a fixed
    batch (the dependent index read, and a fresh batch from HBM where (c)'s one batch may stay in the Infinity Cache);
    a / b: against the only route a shuffled epoch had."""
    fp8 = which == 'cached002_fp8'
    per_class = which == 'cached_perclass_bf16'
    forms, info = build_cached(cof, dev, fp8, args.batch, args.hw, args.cache_images, per_class=per_class)
    for _ in range(args.warmup):
        for step in forms.values():
            step()
    torch.cuda.synchronize()
    assert all(st.frozen_input for st in info['steps'])
    runs = {k: [] for k in forms}
    for _ in range(5):
        for name, step in forms.items():
            sec, _ = timed(step, args.steps, 0, min_ms=0.0, repeats=1)
            runs[name].append(sec * 1e6)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    return {'workload': '{}: {} frozen one-call training step from a resident {} feature cache, three variants '
                        'alternating in one process; {}'.format(which, 'HMDB-51 per-class' if per_class else 'cfg 002',
                                                                'FP8 E4M3' if fp8 else 'bf16', info['shape']),
            'us_per_step': {k: round(v, 2) for k, v in med.items()},
            'us_per_step_runs': {k: [round(x, 2) for x in v] for k, v in runs.items()},
            'us_per_step_spread': {k: round(max(v) - min(v), 2) for k, v in runs.items()},
            'a_minus_c_us': round(med['a_gathered'] - med['c_plain_fixed'], 2),
            'a_over_b': round(med['a_gathered'] / med['b_gather_rebind_plain'], 4),
            'feature_bytes_per_step': info['feature_bytes_per_step'],
            'gather_bytes_per_step': info['gather_bytes_per_step'], 'cache_bytes': info['cache_bytes'],
            'clamped_ids': int(info['steps'][0]._cached.cache.status)}


def build_cached003(cof, dev, N=32, H=14, T=2048, train=True):
    """cfg 003 (pose head 2048 -> 768 -> 16, attention from pose_pre_logits, K = 393) from a RESIDENT bf16 cache of T
    14x14x2048 maps, three ways: (a) the cached step (custom_ops/pose_cache.py) on a fresh shuffled index per step,
    PoseLabelTable.gather included when training; (b) cache.gather(index) + rebind + the plain frozen step, plus the
    same label gather; (c) the plain step on one fixed batch.  Training: dropout keep 0.2, a caller-held W1 shadow and
    W2^T image.  -> ({name: step}, info)"""
    from attentionalpoolingaction_amd.custom_ops import pose_cache
    C, P, Cp, J, K = 2048, H * H, 768, 16, 393
    T = max(int(T), 4 * N)
    g = torch.Generator().manual_seed(42)
    labels = torch.randint(0, K, (T,), generator=g).to(dev)
    cache = cof.FeatureCache.empty((T, H, H, C), torch.bfloat16, dev, labels=labels)
    for first in range(0, T, 256):
        n = min(256, T - first)
        cache.write(first, _features(n, P, C, torch.bfloat16, dev, seed=42 + first).view(n, H, H, C))
    rn = lambda *s: torch.randn(*s, generator=g)
    params = tuple(t.to(dev) for t in (rn(C, Cp) / C ** 0.5, torch.zeros(Cp), rn(Cp, J) / Cp ** 0.5, torch.zeros(J),
                                       rn(Cp, 1) / Cp ** 0.5, torch.zeros(1), rn(C, K) / C ** 0.5, torch.zeros(K)))
    table = pose_cache.PoseLabelTable(rn(T, H, H, J).to(dev), (torch.rand(T, J, generator=g) < 0.8).to(dev))
    batches = [b for e in range(4) for b in cache.epoch(N, seed=e)]
    w1b = params[0].to(torch.bfloat16)
    f = cache.features
    state = {'a': 0, 'b': 0}
    if train:
        w2t = cof.pose_w2t_image(params[2])
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        kw = dict(flags=cof.attn_flags(False, False, True), keep_prob=0.2, seed=42, offset=ctr, w1_bf16=w1b, w2t_bf16=w2t)
        grads = lambda: [None] + [torch.empty_like(t) for t in params]
        rows = [table.new_batch(N) for _ in range(3)]
        for lab, val in rows:
            table.gather(batches[0], lab, val, clamp=False)
        st_a = pose_cache.PoseAttnTrainStepCached(cache.select(batches[0]), params, None, rows[0][0].view(N, P, J),
                                                  rows[0][1], grads(), **kw)
        st_b = cof.PoseAttnTrainStep(cache.gather(batches[0]).view(N, P, C), params, labels[:N].clone(),
                                     rows[1][0].view(N, P, J), rows[1][1], grads(), **kw)
        st_c = cof.PoseAttnTrainStep(f[:N].view(N, P, C), params, labels[:N].contiguous(), rows[2][0].view(N, P, J),
                                     rows[2][1], grads(), **kw)
    else:
        st_a = pose_cache.PoseAttnEvalStepCached(cache.select(batches[0]), params, None, w1_bf16=w1b)
        st_b = cof.PoseAttnEvalStep(cache.gather(batches[0]).view(N, P, C), params, None, w1_bf16=w1b)
        st_c = cof.PoseAttnEvalStep(f[:N].view(N, P, C), params, None, w1_bf16=w1b)

    def step_a():
        idx = batches[state['a'] % len(batches)]
        state['a'] += 1
        if train:
            table.gather(idx, rows[0][0], rows[0][1], clamp=False)
        st_a.rebind(index=idx)
        st_a.run()

    def step_b():
        idx = batches[state['b'] % len(batches)]
        state['b'] += 1
        if train:
            table.gather(idx, rows[1][0], rows[1][1], clamp=False)
            st_b.rebind(X=cache.gather(idx).view(N, P, C), labels=labels[idx.long()])
        else:
            st_b.rebind(X=cache.gather(idx).view(N, P, C))
        st_b.run()

    def step_a_clamped():   # (a) with the table's default: the ids clamped first, a third launch (what deploy pays)
        idx = batches[state['a'] % len(batches)]
        state['a'] += 1
        table.gather(idx, rows[0][0], rows[0][1])
        st_a.rebind(index=idx)
        st_a.run()

    def step_a_bare():      # (a) without the PoseLabelTable.gather: what its launches cost
        idx = batches[state['a'] % len(batches)]
        state['a'] += 1
        st_a.rebind(index=idx)
        st_a.run()

    info = {'N': N, 'T': T, 'shape': '{} of {} x {}x{}x{}, Cp={}, J={}, K={}{}'.format(
        N, T, H, H, C, Cp, J, K, ', dropout keep=0.2' if train else ''),
            'gather_bytes_per_step': 2 * N * P * C * 2, 'pose_label_bytes_per_step': N * P * J * 4 + N * J,
            'cache_bytes': T * P * C * 2, 'cache': cache, 'steps': (st_a, st_b, st_c)}
    forms = {'a_cached': step_a, 'b_gather_rebind_plain': step_b, 'c_plain_fixed': st_c.run}
    if train:
        forms['a_without_label_gather'] = step_a_bare
        forms['a_label_gather_clamped'] = step_a_clamped
    return forms, info


def run_cached003(cof, dev, args, which):
    """cached003_bf16 / eval003_cached_bf16: the three variants ALTERNATING in one process, five timed loops of each,
    interleaved; medians and the loops' spread (as run_cached)."""
    train = which == 'cached003_bf16'
    forms, info = build_cached003(cof, dev, args.batch, args.hw, args.cache_images, train)
    if args.only in forms:      # one variant alone (a kernel trace of it)
        forms = {args.only: forms[args.only]}
    for _ in range(args.warmup):
        for step in forms.values():
            step()
    torch.cuda.synchronize()
    runs = {k: [] for k in forms}
    for _ in range(5):
        for name, step in forms.items():
            sec, _ = timed(step, args.steps, 0, min_ms=0.0, repeats=1)
            runs[name].append(sec * 1e6)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    return {'workload': '{}: cfg 003 one-call {} step from a resident bf16 feature cache, three variants alternating '
                        'in one process; {}'.format(which, 'frozen training' if train else 'evaluation', info['shape']),
            'us_per_step': {k: round(v, 2) for k, v in med.items()},
            'us_per_step_runs': {k: [round(x, 2) for x in v] for k, v in runs.items()},
            'us_per_step_spread': {k: round(max(v) - min(v), 2) for k, v in runs.items()},
            'a_minus_c_us': round(med['a_cached'] - med['c_plain_fixed'], 2) if len(med) > 1 else None,
            'a_over_b': round(med['a_cached'] / med['b_gather_rebind_plain'], 4) if len(med) > 1 else None,
            'gather_bytes_per_step': info['gather_bytes_per_step'],
            'pose_label_bytes_per_step': info['pose_label_bytes_per_step'], 'cache_bytes': info['cache_bytes'],
            'clamped_ids': int(info['cache'].status)}


def _measure_routes(forms, steps):
    """{name: callable that enqueues one pass of `steps` steps} ALTERNATING, five timed passes each after one untimed:
    per pass the wall clock around it with ONE synchronise at its end and a pair of device events around it; medians per
    step, the five figures, the wall / device ratio and the spread (max - min) of the five wall figures"""
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    wall, device = {k: [] for k in forms}, {k: [] for k in forms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        for name, fn in forms.items():
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e6 / steps)
            device[name].append(e0.elapsed_time(e1) * 1e3 / steps)
    med = lambda v: sorted(v)[len(v) // 2]
    return {k: {'wall_us_per_step': round(med(wall[k]), 2), 'device_us_per_step': round(med(device[k]), 2),
                'wall_over_device': round(med(wall[k]) / med(device[k]), 3),
                'wall_spread_us': round(max(wall[k]) - min(wall[k]), 2),
                'wall_runs': [round(x, 2) for x in wall[k]], 'device_runs': [round(x, 2) for x in device[k]]}
            for k in forms}


def _epoch_cfg002(dev, K, training):
    from attentionalpoolingaction_amd import config as apa_config, nets_factory
    apa_config.reset_cfg()
    pre = 'USE_POSE_PRELOGITS_BASED_ATTENTION'
    cfg = apa_config.cfg_from_dict({'MODEL_NAME': 'resnet_v1_101', 'NET': {pre: True, pre + '_SINGLE_LAYER_ATT': True},
                                    'TRAIN': {'LOSS_FN_POSE': '', 'LOSS_FN_ACTION': 'softmax-xentropy'}})
    return nets_factory.get_network_fn('resnet_v1_101', K, 16, cfg, is_training=training, device=dev), cfg


def run_epoch(cof, dev, args, which):
    """epoch002_fp8 / epoch002_bf16: a whole frozen-feature epoch of cfg 002 (K = 393, dropout keep 0.2, momentum SGD
    behind every step) from the resident cache of cached002_*: --cache-images / --batch steps per epoch (2048 / 32 =
    64), a fresh order per epoch.  Three routes ALTERNATE in one process, medians of five epochs each, every epoch
    timed by wall clock around it with ONE synchronise at its end, and by a pair of device events around it:
      a_epoch_call   cache.order(out=) + HeadTrainEpoch.run: one foreign call per epoch
      b_lean_loop    cache.epoch() views; HeadTrainStep.rebind(index=) + run() + BoundMomentumSGD.run() per step
      c_deploy_loop  deploy.FusedHeadStep(cache.select(index), None) + opt.step() per step
    and the validation pass over the same cache: deploy.FusedHeadEval.evaluate_cache (one call, scores into the meter's
    rows) against the loop of FusedHeadEval.__call__ + meter.update."""
    from attentionalpoolingaction_amd import deploy
    fp8 = which == 'epoch002_fp8'
    N, H, T = args.batch, args.hw, args.cache_images - args.cache_images % args.batch
    C, P, K = 2048, H * H, 393
    steps = T // N
    g = torch.Generator().manual_seed(42)
    labels = torch.randint(0, K, (T,), generator=g).to(dev)
    cache = cof.FeatureCache.empty((T, H, H, C), torch.float8_e4m3fn if fp8 else torch.bfloat16, dev, labels=labels)
    for first in range(0, T, 256):
        n = min(256, T - first)
        status = cache.write(first, _features(n, P, C, torch.bfloat16, dev, seed=42 + first).view(n, H, H, C))
        assert int(status.sum()) == 0
    Wa0, Wt0 = torch.randn(C, 1, generator=g) / C ** 0.5, torch.randn(C, K, generator=g) / C ** 0.5
    lr, momentum, wd = 1e-3, 0.9, [1e-4, 0.0, 1e-4, 0.0]
    kw = dict(flags=cof.attn_flags(False, False, True), keep_prob=0.2, seed=42)

    def lean_state():
        w = [Wa0.clone().to(dev), torch.zeros(1, device=dev), Wt0.clone().to(dev), torch.zeros(K, device=dev)]
        grad = torch.zeros((sum(t.numel() for t in w),), device=dev)
        o, views = 0, []
        for t in w:
            views.append(grad[o:o + t.numel()].view(t.shape))
            o += t.numel()
        return w, grad, torch.zeros_like(grad), tuple(views), torch.zeros(1, dtype=torch.int64, device=dev)

    # (a) one call per epoch
    wa, ga, acca, va, ctra = lean_state()
    ep = cof.HeadTrainEpoch(cache, N, *wa, va, wa, wd, ga, acca, steps=steps, momentum=momentum, offset=ctra, **kw)
    order_a = torch.empty((T,), dtype=torch.int32, device=dev)
    lrs = [lr] * steps
    state = {'a': 0, 'b': 0, 'c': 0}

    def epoch_a():
        cache.order(7, state['a'], out=order_a)
        state['a'] += 1
        ep.run(order_a, lrs)

    # (b) the lean loop
    wb, gb, accb, vb, ctrb = lean_state()
    b0 = cache.select(torch.arange(N, dtype=torch.int32, device=dev))
    st_b = cof.HeadTrainStep(b0, b0, *wb, None, (None, None) + vb, offset=ctrb, **kw)
    sgd_b = cof.BoundMomentumSGD(wb, wd, gb, accb)

    def epoch_b():
        state['b'] += 1
        for idx in cache.epoch(N, seed=state['b']):
            st_b.rebind(index=idx)
            st_b.run()
            sgd_b.run(lr, momentum, 1.0)

    # (c) the deploy loop
    network_fn, cfg = _epoch_cfg002(dev, K, True)
    with torch.no_grad():
        network_fn.head.att_weights.copy_(Wa0.to(dev).view_as(network_fn.head.att_weights))
        network_fn.head.td_weights.copy_(Wt0.to(dev).view_as(network_fn.head.td_weights))
    fused = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
    opt = fused.make_optimizer(lr)

    def epoch_c():
        state['c'] += 1
        for idx in cache.epoch(N, seed=state['c']):
            fused(cache.select(idx), None)
            opt.step()

    # (d) the deploy layer's own epoch call, for what it adds to (a)
    net_d, cfg_d = _epoch_cfg002(dev, K, True)
    fused_d = deploy.FusedHeadStep(net_d, cfg_d, frozen_features=True)
    fused_d.make_optimizer(lr)

    def epoch_d():
        fused_d.train_epoch(cache, N, cache.order(9, fused_d.head._step, out=order_a))

    # the validation pass
    net_e, cfg_e = _epoch_cfg002(dev, K, False)
    ev = deploy.FusedHeadEval(net_e, cfg_e)
    meter_a, meter_b = ev.new_evaluation(T), ev.new_evaluation(T)
    all_ids = torch.arange(T, dtype=torch.int32, device=dev)

    def eval_a():
        meter_a.reset()
        ev.evaluate_cache(cache, N, meter=meter_a, order=all_ids)

    def eval_b():
        meter_b.reset()
        for a in range(0, T, N):
            idx = all_ids[a:a + N]
            scores, _, _ = ev(cache.select(idx))
            meter_b.update(scores, labels[a:a + N])

    measure = lambda forms: _measure_routes(forms, steps)

    train = measure({'a_epoch_call': epoch_a, 'b_lean_loop': epoch_b, 'c_deploy_loop': epoch_c,
                     'd_deploy_train_epoch': epoch_d})
    evals = measure({'a_evaluate_cache': eval_a, 'b_call_loop': eval_b})
    fastest = min(('a_epoch_call', 'b_lean_loop', 'c_deploy_loop'), key=lambda k: train[k]['wall_us_per_step'])
    return {'workload': '{}: cfg 002 frozen epoch from a resident {} cache, {} steps of N={} over {} x {}x{}x{}, K={}, '
                        'three routes alternating in one process, medians of five epochs'.format(
                            which, 'FP8 E4M3' if fp8 else 'bf16', steps, N, T, H, H, C, K),
            'steps_per_epoch': steps, 'train': train, 'fastest_train_route_by_wall': fastest, 'eval': evals,
            'fastest_eval_route_by_wall': min(evals, key=lambda k: evals[k]['wall_us_per_step']),
            'clamped_ids': int(cache.status)}


CLIP_EPOCHS = {'epoch_hmdb_clips_fp8': (51, 'softmax-xentropy', True), 'epoch_hmdb_clips_bf16': (51, 'softmax-xentropy', False),
               'epoch_charades_fp8': (157, 'multi-label', True), 'epoch_charades_bf16': (157, 'multi-label', False)}


def _clip_epoch_net(dev, K, loss, training):
    from attentionalpoolingaction_amd import config as apa_config, nets_factory
    apa_config.reset_cfg()
    pre = 'USE_POSE_PRELOGITS_BASED_ATTENTION'
    cfg = apa_config.cfg_from_dict({'MODEL_NAME': 'resnet_v1_101',
                                    'NET': {pre: True, pre + '_SINGLE_LAYER_ATT': True, 'USE_TEMPORAL_ATT': True},
                                    'TRAIN': {'LOSS_FN_POSE': '', 'LOSS_FN_ACTION': loss}})
    return nets_factory.get_network_fn('resnet_v1_101', K, 16, cfg, is_training=training, device=dev), cfg


def run_clip_epoch(cof, dev, args, which):
    """epoch_hmdb_clips_* / epoch_charades_*: a whole frozen-feature epoch of CLIPS (the shapes of cached_hmdb_clips_* /
    cached_charades_*: --clips x --frames frames per step from videos of 25 frames, temporal attention, dropout keep
    0.2, M = 1; K = 51 softmax cross-entropy or K = 157 'multi-label'; momentum SGD behind every step), one epoch = the
    81 videos' worth of steps.  Three routes ALTERNATE in one process, medians of five epochs each, by wall clock (ONE
    synchronise at the end of an epoch) and by a pair of device events:
      a_epoch_call   cof.epoch_order(V, out=) + ClipTrainEpoch.run: one foreign call per epoch, keyed draws
      b_lean_loop    per step: torch.rand + sample_clips(u=, out=) + HeadTrainStep.run + BoundMomentumSGD.run
      c_deploy_loop  per step: sample_clips(out=) + deploy.FusedHeadStep(clips, None) + opt.step()
    plus d, the deploy layer's own call (train_video_epoch), and the validation pass at 4 x 25 uniform frames:
    deploy.FusedHeadEval.evaluate_videos (one call) against the loop of sample_clips + FusedHeadEval.__call__ +
    meter.update."""
    from attentionalpoolingaction_amd import deploy
    from attentionalpoolingaction_amd.custom_ops import clip_epoch
    K, loss, fp8 = CLIP_EPOCHS[which]
    B, F, H, NF, eval_B, eval_F = args.clips, args.frames, args.hw, 25, 4, 25
    C, P = 2048, H * H
    V = max(int(args.cache_images) // NF, 4 * max(B, eval_B))
    T = V * NF
    steps = V // B
    g = torch.Generator().manual_seed(42)
    cache = cof.FeatureCache.empty((T, H, H, C), torch.float8_e4m3fn if fp8 else torch.bfloat16, dev)
    for first in range(0, T, 256):
        n = min(256, T - first)
        status = cache.write(first, _features(n, P, C, torch.bfloat16, dev, seed=42 + first).view(n, H, H, C))
        assert int(status.sum()) == 0
    ml = loss != 'softmax-xentropy'
    vlab = None if ml else torch.randint(0, K, (V,), generator=g).to(dev)
    vtar = (torch.rand(V, K, generator=g) < 0.05).float().to(dev) if ml else None
    cache.set_videos(torch.arange(V) * NF, torch.full((V,), NF), labels=vlab, targets=vtar)
    Wa0, Wt0 = torch.randn(C, 1, generator=g) / C ** 0.5, torch.randn(C, K, generator=g) / C ** 0.5
    tw0 = torch.randn(K, generator=g) * 0.01
    lr, momentum, wd = 1e-3, 0.9, [1e-4, 0.0, 1e-4, 0.0, 1e-4, 0.0]
    kw = dict(flags=cof.attn_flags(False, False, True), keep_prob=0.2, seed=42, action_loss=loss)
    lab = lambda c: c.targets if ml else c.labels

    def lean_state():
        w = [Wa0.clone().to(dev), torch.zeros(1, device=dev), Wt0.clone().to(dev), torch.zeros(K, device=dev),
             tw0.clone().to(dev), torch.full((1,), 1.0 / F, device=dev)]
        grad = torch.zeros((sum(t.numel() for t in w),), device=dev)
        o, views = 0, []
        for t in w:
            views.append(grad[o:o + t.numel()].view(t.shape))
            o += t.numel()
        return w, grad, torch.zeros_like(grad), tuple(views), torch.zeros(1, dtype=torch.int64, device=dev)

    state = {'a': 0, 'b': 0, 'c': 0, 'd': 0}
    lrs = [lr] * steps
    # (a) one call per epoch
    wa, ga, acca, va, ctra = lean_state()
    ep = clip_epoch.ClipTrainEpoch(cache, B, F, *wa[:4], va[:4], wa, wd, ga, acca, steps=steps, temporal=(wa[4], wa[5]),
                                   temporal_grads=(va[4], va[5]), momentum=momentum, offset=ctra, **kw)
    order_a = torch.empty((V,), dtype=torch.int32, device=dev)

    def epoch_a():
        cof.epoch_order(V, 7, state['a'], dev, out=order_a)
        ep.run(order_a[:steps * B], lrs, seed=7, epoch=state['a'])
        state['a'] += 1

    # (b) the lean loop
    wb, gb, accb, vb, ctrb = lean_state()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    clips_b = cache.sample_clips(torch.arange(B, dtype=torch.int32, device=dev), F, mode='random-segment', generator=gen)
    st_b = cof.HeadTrainStep(clips_b, clips_b, *wb[:4], lab(clips_b), (None, None) + vb[:4], offset=ctrb, frames=F,
                             temporal=(wb[4], wb[5]), temporal_grads=(vb[4], vb[5]), **kw)
    sgd_b = cof.BoundMomentumSGD(wb, wd, gb, accb)

    def epoch_b():
        state['b'] += 1
        for vids in cache.video_epoch(B, seed=state['b']):
            u = torch.rand((B * F,), dtype=torch.float32, device=dev, generator=gen)
            cache.sample_clips(vids, F, mode='random-segment', u=u, out=clips_b)
            st_b.run()
            sgd_b.run(lr, momentum, 1.0)

    # (c) the deploy loop, (d) the deploy layer's own epoch call
    def deploy_net(training):
        net, cfg = _clip_epoch_net(dev, K, loss, training)
        with torch.no_grad():
            net.head.att_weights.copy_(Wa0.to(dev).view_as(net.head.att_weights))
            net.head.td_weights.copy_(Wt0.to(dev).view_as(net.head.td_weights))
            net.temporal['weights'].copy_(tw0.to(dev).view_as(net.temporal['weights']))
        return net, cfg
    net_c, cfg_c = deploy_net(True)
    fused = deploy.FusedHeadStep(net_c, cfg_c, frozen_features=True)
    opt = fused.make_optimizer(lr)
    clips_c = cache.sample_clips(torch.arange(B, dtype=torch.int32, device=dev), F, mode='random-segment', generator=gen)

    def epoch_c():
        state['c'] += 1
        for vids in cache.video_epoch(B, seed=state['c']):
            cache.sample_clips(vids, F, mode='random-segment', generator=gen, out=clips_c)
            fused(clips_c, None)
            opt.step()

    net_d, cfg_d = deploy_net(True)
    fused_d = deploy.FusedHeadStep(net_d, cfg_d, frozen_features=True)
    fused_d.make_optimizer(lr)

    def epoch_d():
        cof.epoch_order(V, 9, state['d'], dev, out=order_a)
        fused_d.train_video_epoch(cache, B, F, order_a[:steps * B], seed=9, epoch=state['d'])
        state['d'] += 1

    train = _measure_routes({'a_epoch_call': epoch_a, 'b_lean_loop': epoch_b, 'c_deploy_loop': epoch_c,
                             'd_deploy_train_video_epoch': epoch_d}, steps)

    # the validation pass: eval_B videos x 25 uniform frames per step, all V videos
    net_e, cfg_e = deploy_net(False)
    ev = deploy.FusedHeadEval(net_e, cfg_e)
    meter_a, meter_b = ev.new_evaluation(V), ev.new_evaluation(V)
    all_ids = torch.arange(V, dtype=torch.int32, device=dev)
    esteps = (V + eval_B - 1) // eval_B

    def eval_a():
        meter_a.reset()
        ev.evaluate_videos(cache, eval_B, eval_F, meter=meter_a, order=all_ids)

    def eval_b():
        meter_b.reset()
        for a in range(0, V, eval_B):
            clips = cache.sample_clips(all_ids[a:a + eval_B], eval_F)
            scores, _, _ = ev(clips)
            meter_b.update(scores, lab(clips))

    evals = _measure_routes({'a_evaluate_videos': eval_a, 'b_call_loop': eval_b}, esteps)
    assert torch.equal(meter_a._scores[:V], meter_b._scores[:V])
    fastest = min(('a_epoch_call', 'b_lean_loop', 'c_deploy_loop'), key=lambda k: train[k]['wall_us_per_step'])
    a, b = train['a_epoch_call'], train['b_lean_loop']
    return {'workload': '{}: frozen clip epoch from a resident {} frame cache, {} steps of {} clips x {} frames over {} '
                        'videos x {} frames ({}x{}x{}), K={}, {}, temporal attention, three routes alternating in one '
                        'process, medians of five epochs'.format(which, 'FP8 E4M3' if fp8 else 'bf16', steps, B, F, V,
                                                                  NF, H, H, C, K, loss),
            'steps_per_epoch': steps, 'train': train, 'fastest_train_route_by_wall': fastest,
            'epoch_call_minus_lean_loop_us': round(a['wall_us_per_step'] - b['wall_us_per_step'], 2),
            'epoch_call_beats_lean_loop_by_more_than_its_spread':
                bool(b['wall_us_per_step'] - a['wall_us_per_step'] > b['wall_spread_us']),
            'eval_shape': '{} videos x {} frames per step, {} steps'.format(eval_B, eval_F, esteps), 'eval': evals,
            'fastest_eval_route_by_wall': min(evals, key=lambda k: evals[k]['wall_us_per_step']),
            'clamped_ids': int(cache.status)}


CACHED_CLIPS = {'cached_hmdb_clips_fp8': (51, 'softmax-xentropy', True), 'cached_hmdb_clips_bf16': (51, 'softmax-xentropy', False),
                'cached_charades_fp8': (157, 'multi-label', True), 'cached_charades_bf16': (157, 'multi-label', False),
                'cached_hmdb_perclass_clips_bf16': (51, 'softmax-xentropy', False)}
PER_CLASS_CLIPS = ('cached_hmdb_perclass_clips_bf16',)      # M = K (the HMDB-51 configuration) instead of M = 1


def build_cached_clips(cof, dev, which, B=8, F=4, H=14, T=2048, eval_B=4, eval_F=25):
    """One-call clip training step (temporal attention, dropout keep 0.2, M = 1; K = 51 softmax cross-entropy or K = 157
    'multi-label') from a RESIDENT frame cache of videos of 25 frames (14x14x2048 maps, FP8 E4M3 or bf16), three ways:
    (a) the device sampler (random-segment, fresh draws per step, out= the bound CachedClips) + the cached clip step;
    (b) the sampler + cache.gather(index) + rebind + the plain clip step; (c) the plain clip step on one fixed batch.
    And an evaluation step at eval_B x eval_F frames (uniform sampling): (a) cached, (b) gather + rebind.
    -> ({name: step}, {name: eval step}, info)"""
    K, loss, fp8 = CACHED_CLIPS[which]
    C, P, NF = 2048, H * H, 25
    V = max(int(T) // NF, 4 * max(B, eval_B))
    T = V * NF
    g = torch.Generator().manual_seed(42)
    cache = cof.FeatureCache.empty((T, H, H, C), torch.float8_e4m3fn if fp8 else torch.bfloat16, dev)
    for first in range(0, T, 256):
        n = min(256, T - first)
        status = cache.write(first, _features(n, P, C, torch.bfloat16, dev, seed=42 + first).view(n, H, H, C))
        assert int(status.sum()) == 0
    ml = loss != 'softmax-xentropy'
    vlab = None if ml else torch.randint(0, K, (V,), generator=g).to(dev)
    vtar = (torch.rand(V, K, generator=g) < 0.05).float().to(dev) if ml else None
    cache.set_videos(torch.arange(V) * NF, torch.full((V,), NF), labels=vlab, targets=vtar)
    M = K if which in PER_CLASS_CLIPS else 1
    Wa = (torch.randn(C, M, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(M, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    tw = (torch.randn(K, generator=g) * 0.01).to(dev); tb = torch.full((1,), 1.0 / F, device=dev)
    pg = tuple(torch.empty_like(t) for t in (Wa, ba, Wt, bt))
    tg = (torch.empty_like(tw), torch.empty_like(tb))
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    kw = dict(flags=cof.attn_flags(False, False, True), keep_prob=0.2, seed=42, offset=ctr, frames=F, temporal=(tw, tb),
              temporal_grads=tg, action_loss=loss, weight_images=M > 1)
    lab = lambda c: c.targets if ml else c.labels
    batches = [b for e in range(4) for b in cache.video_epoch(B, seed=e)]      # four epochs' shuffled video batches
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    clips_a = cache.sample_clips(batches[0], F, mode='random-segment', generator=gen)
    clips_b = cache.sample_clips(batches[0], F, mode='random-segment', generator=gen)
    st_a = cof.HeadTrainStep(clips_a, clips_a, Wa, ba, Wt, bt, lab(clips_a), (None, None) + pg, **kw)
    X0 = cache.gather(clips_b.index)
    st_b = cof.HeadTrainStep(X0, X0, Wa, ba, Wt, bt, lab(clips_b), (None, None) + pg, **kw)
    f = cache.features
    Xc = cof.Fp8Features.from_parts(f.codes[:B * F], f.scale[:B * F]) if fp8 else f[:B * F]
    st_c = cof.HeadTrainStep(Xc, Xc, Wa, ba, Wt, bt, lab(clips_a).clone(), (None, None) + pg, **kw)
    state = {'a': 0, 'b': 0, 'ea': 0, 'eb': 0}

    def step_a():
        cache.sample_clips(batches[state['a'] % len(batches)], F, mode='random-segment', generator=gen, out=clips_a)
        state['a'] += 1
        st_a.run()

    def step_b():
        cache.sample_clips(batches[state['b'] % len(batches)], F, mode='random-segment', generator=gen, out=clips_b)
        state['b'] += 1
        st_b.rebind(X=cache.gather(clips_b.index), labels=lab(clips_b))
        st_b.run()

    # evaluation: eval_B clips of all 25 frames, uniform sampling, sigmoid scores for the multi-label head
    etb = torch.full((1,), 1.0 / eval_F, device=dev)
    ebatches = [b for b in cache.video_epoch(eval_B, seed=9, shuffle=False)]
    ekw = dict(frames=eval_F, temporal=(tw, etb), scores='sigmoid' if ml else 'softmax')
    eclips_a, eclips_b = cache.sample_clips(ebatches[0], eval_F), cache.sample_clips(ebatches[0], eval_F)
    ev_a = cof.HeadEvalStep(eclips_a, eclips_a, Wa, ba, Wt, bt, **ekw)
    E0 = cache.gather(eclips_b.index)
    ev_b = cof.HeadEvalStep(E0, E0, Wa, ba, Wt, bt, **ekw)

    def eval_a():
        cache.sample_clips(ebatches[state['ea'] % len(ebatches)], eval_F, out=eclips_a)
        state['ea'] += 1
        ev_a.run()

    def eval_b():
        cache.sample_clips(ebatches[state['eb'] % len(ebatches)], eval_F, out=eclips_b)
        state['eb'] += 1
        ev_b.rebind(X=cache.gather(eclips_b.index))
        ev_b.run()

    bytes_img = P * C * (1 if fp8 else 2)
    info = {'shape': '{} clips x {} frames of {} videos x {} frames ({} maps {}x{}x{}), K={}, {}, temporal attention, '
                     'dropout keep=0.2'.format(B, F, V, NF, T, H, H, C, K, loss) + (', per-class maps (M = K)' if M > 1 else ''),
            'eval_shape': '{} clips x {} frames'.format(eval_B, eval_F),
            'feature_bytes_per_step': 2 * B * F * bytes_img, 'gather_bytes_per_step': 2 * B * F * bytes_img,
            'cache_bytes': T * bytes_img, 'steps': (st_a, st_b, st_c), 'cache': cache}
    return ({'a_sampler_cached_clips': step_a, 'b_sampler_gather_rebind_plain': step_b, 'c_plain_fixed': st_c.run},
            {'a_sampler_cached_clips': eval_a, 'b_sampler_gather_rebind_plain': eval_b}, info)


def run_cached_clips(cof, dev, args, which):
    """cached_hmdb_clips_* / cached_charades_*: the variants ALTERNATING in one process, five timed loops of each,
    interleaved; medians and the loops' spread -- run_cached's protocol, for the training step and for evaluation."""
    forms, evals, info = build_cached_clips(cof, dev, which, args.clips, args.frames, args.hw, args.cache_images)
    out = {'workload': '{}: frozen one-call clip training step from a resident {} frame cache, three variants '
                       'alternating in one process; {}'.format(which, 'FP8 E4M3' if CACHED_CLIPS[which][2] else 'bf16',
                                                               info['shape'])}
    for tag, group in (('', forms), ('eval_', evals)):
        for _ in range(args.warmup):
            for step in group.values():
                step()
        torch.cuda.synchronize()
        runs = {k: [] for k in group}
        for _ in range(5):
            for name, step in group.items():
                sec, _ = timed(step, args.steps, 0, min_ms=0.0, repeats=1)
                runs[name].append(sec * 1e6)
        med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
        out[tag + 'us_per_step'] = {k: round(v, 2) for k, v in med.items()}
        out[tag + 'us_per_step_runs'] = {k: [round(x, 2) for x in v] for k, v in runs.items()}
        out[tag + 'us_per_step_spread'] = {k: round(max(v) - min(v), 2) for k, v in runs.items()}
        out[tag + 'a_over_b'] = round(med['a_sampler_cached_clips'] / med['b_sampler_gather_rebind_plain'], 4)
        if not tag:
            out['a_minus_c_us'] = round(med['a_sampler_cached_clips'] - med['c_plain_fixed'], 2)
    assert all(st.frozen_input for st in info['steps'])
    out.update(eval_shape=info['eval_shape'], feature_bytes_per_step=info['feature_bytes_per_step'],
               gather_bytes_per_step=info['gather_bytes_per_step'], cache_bytes=info['cache_bytes'],
               clamped_ids=int(info['cache'].status))
    return out


def run_explain002(cof, dev, args):
    """Class attention maps of T chosen classes at the cfg 002 benchmark shape (32 x 14x14x2048 fp32, K = 393), T = 1 and
    T = 5: the one-call evaluation step + cof.attn_explain against the only other route, the per-op forward with
    want_topdown=True (all K maps, [N,P,K]) + torch.gather of the chosen classes, both producing scores, prediction,
    the top-down and the combined maps of the same fixed classes.  The two alternate in one process, medians of five
    loops; X rotates over enough sets that no step finds its map cached.  Also: the explain pass over X and the
    evaluation step's m1s_pool_fwd_kernel (the same bytes) by HIP events, against the 8 TB/s peak."""
    N, H, C, K = args.batch, args.hw, 2048, args.classes or 393
    P = H * H
    g = torch.Generator().manual_seed(42)
    Wa = (torch.randn(C, 1, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(1, device=dev)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(K, device=dev)
    per_set = N * P * C * 4
    R = _n_sets(per_set, args.rotate)
    Xs = [_features(N, P, C, torch.float32, dev, seed=42 + r) for r in range(R)]
    evs = []
    for X in Xs:
        evs.append(cof.HeadEvalStep(X, X, Wa, ba, Wt, bt, workspace=evs[0].workspace if evs else None))
    out = {'workload': 'explain002: evaluation step + attn_explain against the per-op forward with want_topdown=True + '
                       'torch.gather, alternating in one process; {} x {}x{}x{} f32, K={}'.format(N, H, H, C, K) +
                       _rot_note(R, per_set).replace('X/dX', 'X'),
           'dtype': 'f32', 'rotate': R, 'x_bytes': per_set}
    for T in (1, 5):
        cls = torch.stack([(torch.arange(N) * 7 + 13 * t) % K for t in range(T)], dim=1).to(dev)
        cls32 = cls.to(torch.int32)
        idx = cls.view(N, 1, T).expand(N, P, T)
        ws = torch.empty((int(evs[0].lib.apa_attn_explain_workspace_bytes(N, P, C, K, T, 0)),), dtype=torch.uint8, device=dev)
        state = {'a': 0, 'b': 0, 'mod_ws': None}

        def explain_route():
            ev = evs[state['a'] % R]
            state['a'] += 1
            ev.run()
            return cof.attn_explain(ev._keep[0], ev.att, Wt, bt, cls32, workspace=ws)

        def module_route():
            X = Xs[state['b'] % R]
            state['b'] += 1
            logits, att, _, _, topdown, state['mod_ws'] = cof.attn_pool_fwd(X, X, Wa, ba, Wt, bt, want_topdown=True,
                                                                            workspace=state['mod_ws'])
            probs = torch.softmax(logits, -1)
            pred = torch.argmax(logits, 1)
            td = torch.gather(topdown, 2, idx)
            return td, att * td, probs, pred

        for _ in range(args.warmup):
            explain_route(); module_route()
        torch.cuda.synchronize()
        runs = {'explain': [], 'module': []}
        for _ in range(5):
            for name, fn in (('explain', explain_route), ('module', module_route)):
                sec, _ = timed(fn, args.steps, 0, min_ms=0.0, repeats=1)
                runs[name].append(sec * 1e6)
        med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
        # the pass over X alone, and the evaluation step's pooling pass over the same bytes, by HIP events
        n = 20
        kt_e, kt_p = cof.KernelTimer(n), cof.KernelTimer(n)
        for i in range(n):
            X = Xs[i % R]
            _, att, _, _, _, state['mod_ws'] = cof.attn_pool_fwd(X, X, Wa, ba, Wt, bt, workspace=state['mod_ws'],
                                                                 hooks=kt_p.hooks(i))
            cof.attn_explain(X, att, Wt, bt, cls32, workspace=ws, hooks=kt_e.hooks(i))
        torch.cuda.synchronize()
        med_us = lambda v: sorted(v)[len(v) // 2] * 1e3
        k_e, k_p = med_us(kt_e.fwd_elapsed_ms()), med_us(kt_p.fwd_elapsed_ms())
        kt_e.close(); kt_p.close()
        out['T=%d' % T] = {
            'us_per_step': {k: round(v, 2) for k, v in med.items()},
            'us_per_step_runs': {k: [round(x, 2) for x in v] for k, v in runs.items()},
            'explain_over_module': round(med['explain'] / med['module'], 4),
            'kernels_us': {'explain_main_kernel': round(k_e, 2), 'm1s_pool_fwd_kernel': round(k_p, 2)},
            'explain_main_kernel_frac_of_hbm_peak': round(per_set / (k_e * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
            'm1s_pool_fwd_kernel_frac_of_hbm_peak': round(per_set / (k_p * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
            'module_route_topdown_bytes': N * P * K * 4, 'explain_route_map_bytes': 2 * N * T * P * 4}
    return out


def run_map393(cof, dev, args):
    """The metric of a validation pass: eval_utils.Evaluation.result() (one copy to the host, then K argsorts and
    voc_ap loops in numpy) against eval_utils.DeviceEvaluation.result() (cof.average_precision: three launches, one
    small copy) on the same accumulated scores -- softmax of random logits, T = --samples (7000), K = --classes (393).
    --multi-hot: sigmoid scores and multi-hot targets (the HICO-like case, e.g. --samples 9600 --classes 600); the
    host route is then what Evaluation.result() does with single labels -- one copy, calc_pr_ovr_noref per class --
    since Evaluation itself takes single labels only.  The two routes alternate in one process: five runs each, a host
    run one call, a device run --steps calls.  Also: the three launches alone by device events around
    cof.average_precision with a preallocated workspace."""
    from attentionalpoolingaction_amd import eval_utils
    T, K, multi = args.samples or 7000, args.classes or 393, args.multi_hot
    g = torch.Generator().manual_seed(42)
    logits = torch.randn(T, K, generator=g) * 3.0
    if multi:
        scores = torch.sigmoid(logits).to(dev)
        truth = (torch.rand(T, K, generator=g) < 0.02).float().to(dev)
    else:
        scores = torch.softmax(logits, -1).to(dev)
        truth = torch.randint(0, K, (T,), generator=g).to(dev)
    batch = 512
    meter = eval_utils.DeviceEvaluation(T, K, dev, multi_label=multi)
    old = eval_utils.Evaluation()
    for at in range(0, T, batch):
        meter.update(scores[at:at + batch], truth[at:at + batch])
        if not multi:
            old.update(scores[at:at + batch], truth[at:at + batch])

    def host_route():
        if not multi:
            return old.result()
        both = torch.cat([scores.double(), truth.double()], dim=1).cpu().numpy()      # one copy, as Evaluation.result()
        s, t = both[:, :K].astype(np.float32), both[:, K:]
        aps = [eval_utils.calc_pr_ovr_noref(t[:, k], s[:, k])[3] for k in range(K) if (t[:, k] > 0).any()]
        return {'mAP': float(np.mean(aps)), 'aps': aps}

    ref, got = host_route(), meter.result()
    for _ in range(args.warmup):
        meter.result()
    torch.cuda.synchronize()
    runs = {'host': [], 'device': []}
    for _ in range(5):
        t0 = time.perf_counter()
        host_route()
        torch.cuda.synchronize()
        runs['host'].append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            meter.result()
        torch.cuda.synchronize()
        runs['device'].append((time.perf_counter() - t0) * 1e6 / args.steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    # the launches alone
    ws = torch.empty((cof.average_precision_workspace_bytes(T, K),), dtype=torch.uint8, device=dev)
    out_buf = torch.empty((cof.average_precision_result_bytes(K),), dtype=torch.uint8, device=dev)
    kw = dict(targets=truth) if multi else dict(labels=truth)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for e0, e1 in ev:
        e0.record()
        cof.average_precision(scores, workspace=ws, out=out_buf, **kw)
        e1.record()
    torch.cuda.synchronize()
    launches = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return {'workload': 'map393: Evaluation.result() (host numpy) against DeviceEvaluation.result() (three launches), '
                        'alternating in one process; T={} K={} {}'.format(T, K, 'multi-hot sigmoid' if multi else
                                                                          'single-label softmax'),
            'T': T, 'K': K, 'multi_hot': bool(multi),
            'us_per_result': {k: round(v, 1) for k, v in med.items()},
            'us_per_result_runs': {k: [round(x, 1) for x in v] for k, v in runs.items()},
            'spread': {k: round((max(v) - min(v)) / med[k], 4) for k, v in runs.items()},
            'host_over_device': round(med['host'] / med['device'], 2),
            'three_launches_us_by_events': {'median': round(launches[len(launches) // 2], 1),
                                            'min': round(launches[0], 1), 'max': round(launches[-1], 1)},
            'key_bytes': int(ws.numel()), 'copy_back_bytes': int(out_buf.numel()),
            'mAP': {'host': ref['mAP'], 'device': got['mAP'], 'abs_diff': abs(ref['mAP'] - got['mAP'])},
            'classes_with_positives': len(got['aps'])}


SWEEPS = {'sweep002_bf16': torch.bfloat16, 'sweep002_fp32': torch.float32}


def run_sweep(cof, dev, args, which):
    """sweep002_bf16 / sweep002_fp32: H = 4 cfg 002 heads on a RESIDENT cache of T 14x14x2048 maps (K = 393, dropout
    keep 0.2, a fresh shuffled index per step), three training routes ALTERNATING in one process, medians of five
    loops of `--steps` steps and the loops' spread:
      a_multihead     one apa_multihead_train_step_cached + one apa_momentum_sgd_step_heads
      b_four_single   four HeadTrainStep cached steps + four BoundMomentumSGD updates on the same batches
      c_one_single    one single-head step + update, for scale
    and the evaluation step against four HeadEvalStep calls the same way."""
    from attentionalpoolingaction_amd.custom_ops import multihead as mh
    Hh, C, K, hw, N = 4, 2048, args.classes or 393, args.hw, args.batch
    P = hw * hw
    T = max(int(args.cache_images), 4 * N)
    g = torch.Generator().manual_seed(42)
    labels = torch.randint(0, K, (T,), generator=g).to(dev)
    cache = cof.FeatureCache.empty((T, hw, hw, C), SWEEPS[which], dev, labels=labels)
    for first in range(0, T, 256):
        n = min(256, T - first)
        cache.write(first, _features(n, P, C, torch.bfloat16, dev, seed=42 + first).view(n, hw, hw, C))
    Wa = (torch.randn(Hh, C, generator=g) / C ** 0.5).to(dev); ba = torch.zeros(Hh, device=dev)
    Wt = (torch.randn(Hh, C, K, generator=g) / C ** 0.5).to(dev); bt = torch.zeros(Hh, K, device=dev)
    batches = [b for e in range(4) for b in cache.epoch(N, seed=e)]
    batch0 = cache.select(batches[0])
    lrs, moms = [1e-3, 3e-4, 1e-4, 3e-5], [0.9] * Hh
    # (a)
    st_a = mh.MultiHeadTrainStep(batch0, Wa, ba, Wt, bt, 'cache', keep_prob=0.2, seed=42)
    acc_a = torch.zeros_like(st_a.grad_flat)
    sgd_a = mh.MultiHeadSGD([Wa, ba, Wt, bt], [1e-4, 0.0, 1e-4, 0.0], st_a.grad_flat, acc_a, lrs, moms)
    # (b), (c): single heads on copies of the rows
    singles, wsets = [], []
    for h in range(Hh):
        w = [Wa[h].clone().view(C, 1), ba[h:h + 1].clone(), Wt[h].clone(), bt[h].clone()]
        flat = torch.zeros(sum(t.numel() for t in w), device=dev)
        views, o = [], 0
        for t in w:
            views.append(flat[o:o + t.numel()].view(t.shape))
            o += t.numel()
        st = cof.HeadTrainStep(batch0, batch0, *w, None, (None, None) + tuple(views),
                               flags=cof.attn_flags(False, False, True), keep_prob=0.2, seed=42, offset=0)
        opt = cof.BoundMomentumSGD(w, [1e-4, 0.0, 1e-4, 0.0], flat, torch.zeros_like(flat))
        singles.append((st, opt))
        wsets.append(w)
    state = {'a': 0, 'b': 0, 'c': 0, 'ea': 0, 'eb': 0}

    def nxt(k):
        idx = batches[state[k] % len(batches)]
        state[k] += 1
        return idx, state[k]

    def step_a():
        idx, s = nxt('a')
        st_a.rebind(index=idx, offset=s)
        st_a.run()
        sgd_a.run()

    def step_b():
        idx, s = nxt('b')
        for h, (st, opt) in enumerate(singles):
            st.rebind(index=idx, offset=s)
            st.run()
            opt.run(lrs[h], moms[h])

    def step_c():
        idx, s = nxt('c')
        st, opt = singles[0]
        st.rebind(index=idx, offset=s)
        st.run()
        opt.run(lrs[0], moms[0])

    # both evaluation routes read the cache's labels and log the loss; route (a) also writes the fused scores
    ev_a = mh.MultiHeadEvalStep(batch0, Wa, ba, Wt, bt, 'cache')
    ev_b = [cof.HeadEvalStep(batch0, batch0, *w) for w in wsets]

    def eval_a():
        idx, _ = nxt('ea')
        ev_a.rebind(index=idx)
        ev_a.run()

    def eval_b():
        idx, _ = nxt('eb')
        for ev in ev_b:
            ev.rebind(index=idx)
            ev.run()

    forms = {'a_multihead': step_a, 'b_four_single': step_b, 'c_one_single': step_c, 'eval_a_multihead': eval_a,
             'eval_b_four_single': eval_b}
    if args.only:
        forms = {k: v for k, v in forms.items() if k == args.only}
    for _ in range(args.warmup):
        for step in forms.values():
            step()
    torch.cuda.synchronize()
    runs = {k: [] for k in forms}
    for _ in range(5):
        for name, step in forms.items():
            sec, _ = timed(step, args.steps, 0, min_ms=0.0, repeats=1)
            runs[name].append(sec * 1e6)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    out = {'workload': '{}: H = 4 cfg 002 heads from a resident {} cache, {} of {} x {}x{}x{}, K={}, dropout keep=0.2, '
                       'routes alternating in one process'.format(which, 'bf16' if which.endswith('bf16') else 'fp32', N, T,
                                                                  hw, hw, C, K),
           'us_per_step': {k: round(v, 2) for k, v in med.items()},
           'us_per_step_runs': {k: [round(x, 2) for x in v] for k, v in runs.items()},
           'us_per_step_spread': {k: round(max(v) - min(v), 2) for k, v in runs.items()}}
    if 'a_multihead' in med and 'b_four_single' in med:
        out['a_over_b'] = round(med['a_multihead'] / med['b_four_single'], 4)
    if 'eval_a_multihead' in med and 'eval_b_four_single' in med:
        out['eval_a_over_b'] = round(med['eval_a_multihead'] / med['eval_b_four_single'], 4)
    return out


def timed(fn, steps, warmup, min_ms=50.0, repeats=5):
    """median over >= `repeats` timed loops of `steps` steps each (>= min_ms of device time in total)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per, total = [], 0.0
    while len(per) < repeats or total < min_ms * 1e-3:
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        per.append(dt / steps)
        total += dt
        if len(per) >= 200:
            break
    per.sort()
    return per[len(per) // 2], len(per)


def report(info, sec, repeats):
    N = info['N']
    out = {'workload': info['workload'], 'images_per_sec': round(N / sec, 1), 'ms_per_step': round(sec * 1e3, 5),
           'repeats': repeats, 'dtype': info['dtype'], 'rotate': info.get('rotate', 1)}
    if info['bound'] == 'mfma':
        tflops = N * info['flops_per_image'] / sec / 1e12
        out['roofline'] = {'bound': 'mfma', 'achieved': round(tflops, 2), 'peak': PEAK[info['dtype']],
                           'unit': 'TFLOP/s', 'frac': round(tflops / PEAK[info['dtype']], 4),
                           'algorithmic_gflop_per_image': round(info['flops_per_image'] / 1e9, 3),
                           'note': 'whole step (all kernels) against the dense MFMA peak'}
    else:
        gbs = N * info['bytes_per_image'] / sec / 1e9
        out['roofline'] = {'bound': 'hbm', 'achieved': round(gbs, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                           'frac': round(gbs / HBM_PEAK_GBS, 4),
                           'algorithmic_bytes_per_image': info['bytes_per_image'],
                           'note': 'whole step (all kernels) against the HBM peak'}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg003', choices=['cfg003', 'perclass', 'eval002', 'eval003', 'rank1', 'posebwd', 'posebwd_acc', 'update003',
                                                         'update_perclass', 'poseatt', 'video_perclass', 'video003',
                                                         'hico002', 'charades_clips', 'frozen002', 'frozen003',
                                                         'frozen_perclass', 'frozen002_fp8', 'eval002_fp8',
                                                         'cached002_fp8', 'cached002_bf16', 'cached_perclass_bf16',
                                                         'cached003_bf16', 'eval003_cached_bf16',
                                                         'epoch002_fp8',
                                                         'epoch002_bf16', 'explain002', 'map393'] + sorted(SWEEPS) +
                    sorted(EVAL_CLIPS) + sorted(RANK_WORKLOADS) + sorted(CACHED_CLIPS) + sorted(CLIP_EPOCHS))
    ap.add_argument('--clips', type=int, default=8, help='video_*: clips per batch')
    ap.add_argument('--frames', type=int, default=4, help='video_*: frames per clip')
    ap.add_argument('--only', default=None, choices=['clip_one_call', 'module_path', 'flat_one_call',
                                                     'multilabel_one_call', 'softmax_one_call', 'one_call',
                                                     'sequence', 'rank_one_call', 'rank1_one_call', 'a_cached',
                                                     'b_gather_rebind_plain', 'c_plain_fixed', 'a_multihead',
                                                     'b_four_single', 'c_one_single', 'eval_a_multihead',
                                                     'eval_b_four_single'],
                    help='video_* / hico002 / charades_clips / eval_* / rank* / cached003_bf16 / eval003_cached_bf16: run '
                         'one variant alone (kernel traces)')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--cache-images', type=int, default=2048, help='cached002_*: images in the resident cache')
    ap.add_argument('--hw', type=int, default=14)
    ap.add_argument('--classes', type=int, default=None)
    ap.add_argument('--samples', type=int, default=None, help='map393: accumulated score rows (default 7000)')
    ap.add_argument('--multi-hot', action='store_true', help='map393: sigmoid scores against multi-hot targets')
    ap.add_argument('--dtype', default=None, choices=['bf16', 'f32'])
    ap.add_argument('--per-op', action='store_true',
                    help='cfg003: drive the step as separate calls (pose head fwd, pose loss, attention train step, '
                         'pose head bwd) instead of the one-call apa_pose_attn_train_step')
    ap.add_argument('--no-rank1', action='store_true',
                    help='cfg003: materialise the [N,P,768] attention-branch gradient between the two backward calls')
    ap.add_argument('--no-weight-images', action='store_true',
                    help='perclass: rebuild the padded bf16 weight images in every step (the round-4 form)')
    ap.add_argument('--rotate', type=int, default=0,
                    help='number of (X, dX) buffer sets cycled through; 0 = enough for 1.5 x the Infinity Cache')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    dev = torch.device('cuda:0')
    if args.workload in ('update003', 'update_perclass'):
        print(json.dumps(run_update_pair(cof, dev, 'cfg003' if args.workload == 'update003' else 'perclass',
                                         rotate=args.rotate)))
        return
    if args.workload == 'eval003':
        print(json.dumps(run_eval003(cof, dev, args)))
        return
    if args.workload in ('video_perclass', 'video003'):
        print(json.dumps(run_video(cof, dev, args, 'perclass' if args.workload == 'video_perclass' else 'cfg003')))
        return
    if args.workload in ('hico002', 'charades_clips'):
        print(json.dumps(run_multilabel(cof, dev, args, args.workload)))
        return
    if args.workload in EVAL_CLIPS:
        print(json.dumps(run_eval_clips(cof, dev, args, args.workload)))
        return
    if args.workload in RANK_WORKLOADS:
        print(json.dumps(run_rank(cof, dev, args, args.workload)))
        return
    if args.workload in ('frozen002_fp8', 'eval002_fp8'):
        print(json.dumps(run_fp8(cof, dev, args, args.workload)))
        return
    if args.workload in ('cached002_fp8', 'cached002_bf16', 'cached_perclass_bf16'):
        print(json.dumps(run_cached(cof, dev, args, args.workload)))
        return
    if args.workload in ('cached003_bf16', 'eval003_cached_bf16'):
        print(json.dumps(run_cached003(cof, dev, args, args.workload)))
        return
    if args.workload in ('epoch002_fp8', 'epoch002_bf16'):
        print(json.dumps(run_epoch(cof, dev, args, args.workload)))
        return
    if args.workload in SWEEPS:
        print(json.dumps(run_sweep(cof, dev, args, args.workload)))
        return
    if args.workload in CACHED_CLIPS:
        print(json.dumps(run_cached_clips(cof, dev, args, args.workload)))
        return
    if args.workload in CLIP_EPOCHS:
        print(json.dumps(run_clip_epoch(cof, dev, args, args.workload)))
        return
    if args.workload.startswith('frozen'):
        print(json.dumps(run_frozen(cof, dev, args, args.workload)))
        return
    if args.workload == 'explain002':
        print(json.dumps(run_explain002(cof, dev, args)))
        return
    if args.workload == 'map393':
        print(json.dumps(run_map393(cof, dev, args)))
        return
    if args.workload == 'poseatt':
        step, info, kernel_times = build_poseatt(cof, dev, args.batch, args.hw, args.classes or 393,
                                                 args.dtype or 'f32', rotate=args.rotate)
        sec, reps = timed(step, args.steps, args.warmup)
        out = report(info, sec, reps)
        out['us_per_step'] = round(sec * 1e6, 2)
        out['kernels'] = kernel_times()
        print(json.dumps(out))
        return
    if args.workload == 'cfg003':
        step, info = build_cfg003(cof, dev, args.batch, args.hw, args.classes or 393, args.dtype or 'bf16',
                                  rank1=not args.no_rank1, one_call=not args.per_op, rotate=args.rotate)
    elif args.workload in ('posebwd', 'posebwd_acc'):
        step, info = build_posebwd(cof, dev, args.batch, args.hw, args.dtype or 'bf16',
                                   accumulate=args.workload == 'posebwd_acc')
    elif args.workload == 'rank1':
        step, info = build_rank1(cof, dev, args.batch, args.hw, args.classes or 51, args.dtype or 'bf16',
                                 rotate=args.rotate)
    elif args.workload == 'eval002':
        step, info = build_eval002(cof, dev, args.batch, args.hw, args.classes or 393, args.dtype or 'f32',
                                   rotate=args.rotate)
    else:
        step, info = build_perclass(cof, dev, args.batch, args.hw, args.classes or 51, args.dtype or 'bf16',
                                    rotate=args.rotate, weight_images=not args.no_weight_images)
    sec, reps = timed(step, args.steps, args.warmup)
    print(json.dumps(report(info, sec, reps)))


if __name__ == '__main__':
    main()
