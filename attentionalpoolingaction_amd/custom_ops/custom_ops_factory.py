"""Loader + thin python wrappers for libapa_hip.so (the MI355X attentional-pooling library).

Shaped like the reference's plugin layer, /root/reference/src/custom_ops/custom_ops_factory.py:
the shared object lives next to this file (reference :7-18 resolves `<op>.so` relative to
`__file__` and calls tf.load_op_library at import time) and every op is exposed as a small python
wrapper.  Here the library is a plain C-ABI .so (include/apa.h) bound with ctypes; tensors are
torch tensors used purely as device-memory handles (data_ptr + current stream).

There is NO CPU fallback: if the library is missing, or a tensor is not on the GPU, the wrappers
raise.  The oracle under /oracle is test infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, c_char_p, c_float, c_int, c_int64, c_size_t, c_uint, c_uint8, c_uint64,
                    c_void_p)
from typing import Optional, Tuple

import numpy as np
import torch  # imported BEFORE the CDLL so that libamdhip64.so.7 resolves to torch's runtime

cur_path = os.path.realpath(__file__)
ROOT_PATH = os.path.dirname(cur_path)
LIB_NAME = 'libapa_hip.so'
LIB_PATH = os.path.join(ROOT_PATH, LIB_NAME)

APA_DTYPE_F32 = 0
APA_DTYPE_BF16 = 1
APA_DTYPE_FP8_E4M3 = 2   # a cached feature map: OCP E4M3 codes + one fp32 scale per image (Fp8Features)
APA_FLAG_SOFTMAX_ATT = 1
APA_FLAG_RELU_ATT = 2
APA_FLAG_TRAIN = 4
APA_FLAG_RNG_DEVICE = 8
APA_FLAG_RELU_INPUT = 16  # X in memory is the pre-activation map: relu fused into both passes
APA_FLAG_DXATT_RANK1 = 32  # attn_pool_bwd returns dZ [N*P] instead of dXatt = dZ (x) Wa
APA_FLAG_RNG_EXTERNAL = 128  # `seed` is the address of a caller-supplied, bit-packed dropout keep mask
APA_FLAG_WEIGHT_IMAGES = 256  # per-class maps: the operand images in the workspace are kept current by the caller
APA_FLAG_FROZEN_INPUT = 512  # the features are frozen: the backward half writes no dX (the pointer may be NULL)
APA_POSE_WS_FROM_FWD = 2    # bits of apa_pose_head_bwd's accumulate_dX
APA_POSE_NO_DX = 4
APA_ERR_UNSUPPORTED = -2
APA_SCORES_SOFTMAX = 0   # eval.py:197
APA_SCORES_SIGMOID = 1   # eval.py:194-195 (TRAIN.LOSS_FN_ACTION starts with 'multi-label')
APA_CLIP_FRAMES_UNIFORM = 0          # apa_sample_clip_frames: frame i = min(step * i, n - 1)
APA_CLIP_FRAMES_RANDOM_SEGMENT = 1   # one draw inside each of the F segments
CLIP_FRAME_MODES = {'uniform': APA_CLIP_FRAMES_UNIFORM, 'random-segment': APA_CLIP_FRAMES_RANDOM_SEGMENT}
APA_WIMG_MAX = 12
APA_RANK_MAX = 4         # attention maps chained from one bottom-up map (apa_rank_maps)
APA_EXPLAIN_MAX_CLASSES = 8   # classes per image of one apa_attn_explain call
APA_AP_MAX_SAMPLES = 16384    # rows of one apa_average_precision call (a class's keys are sorted in one block's LDS)
APA_WIMG_ROLES = {0: 'Wa', 1: 'ba', 2: 'Wt', 3: 'bt'}

# every symbol include/apa.h declares: name -> (restype, argtypes)
_SIGNATURES = {
    'apa_version': (c_int, []),
    'apa_last_error': (c_char_p, []),
    'apa_status_string': (c_char_p, [c_int]),
    'apa_attn_pool_workspace_bytes': (c_size_t, [c_int] * 6 + [c_uint]),
    'apa_attn_pool_fwd': (c_int, [c_void_p] * 12 + [c_size_t] + [c_int] * 6 +
                          [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    'apa_attn_pool_bwd': (c_int, [c_void_p] * 17 + [c_size_t] + [c_int] * 6 +
                          [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    # the *_ex forms take a `const apa_hooks*` first (NULL = no hooks)
    'apa_attn_pool_fwd_ex': (c_int, [c_void_p] * 13 + [c_size_t] + [c_int] * 6 +
                             [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    'apa_attn_pool_bwd_ex': (c_int, [c_void_p] * 18 + [c_size_t] + [c_int] * 6 +
                             [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    'apa_dropout_mask': (c_int, [c_void_p, c_size_t, c_float, c_uint64, c_uint64, c_void_p]),
    'apa_fp8_features_bytes': (c_size_t, [c_int, c_int, c_int]),
    'apa_quantize_features_fp8': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'apa_dequantize_features_fp8': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    # a resident feature cache read by image index: `const apa_feature_cache*` first, then the *_ex arguments (the
    # evaluation step: then those of apa_attn_head_eval_step_clips)
    'apa_attn_pool_fwd_cached': (c_int, [c_void_p] * 14 + [c_size_t] + [c_int] * 6 +
                                 [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    'apa_attn_pool_bwd_cached': (c_int, [c_void_p] * 19 + [c_size_t] + [c_int] * 6 +
                                 [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    'apa_attn_head_train_step_cached': (c_int, [c_void_p] * 9 + [c_float, c_float] + [c_void_p] * 13 +
                                        [c_size_t] + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64, c_int,
                                                                    c_void_p]),
    'apa_attn_head_eval_step_cached': (c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 15 + [c_size_t] + [c_int] * 6 +
                                       [c_uint, c_int, c_void_p]),
    'apa_quantize_features_fp8_at': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                             c_void_p]),
    # clips / sigmoid losses from a frame cache: (cache, ml or NULL, clip or NULL, hooks), then the arguments of
    # apa_attn_head_train_step_cached from X on; (cache, clip or NULL, kind), then those of the evaluation step
    'apa_attn_head_train_step_cached_clips': (c_int, [c_void_p] * 11 + [c_float, c_float] + [c_void_p] * 13 +
                                              [c_size_t] + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64, c_int,
                                                                          c_void_p]),
    'apa_attn_head_eval_step_cached_clips': (c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 15 + [c_size_t] +
                                             [c_int] * 6 + [c_uint, c_int, c_void_p]),
    'apa_sample_clip_frames': (c_int, [c_void_p] * 10 + [c_int] * 5 + [c_void_p]),
    # a whole epoch over the cache: (order, T, seed, epoch, stream); (`const apa_epoch*`, `const apa_epoch_sgd*`), then
    # every argument of apa_attn_head_train_step_cached; (`const apa_epoch*`, the descriptor, the kind), then the
    # arguments of apa_attn_head_eval_step_cached from X on
    'apa_epoch_order': (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_void_p]),
    'apa_attn_head_train_epoch_cached': (c_int, [c_void_p] * 11 + [c_float, c_float] + [c_void_p] * 13 +
                                         [c_size_t] + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64, c_int,
                                                                     c_void_p]),
    'apa_attn_head_eval_epoch_cached': (c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 15 + [c_size_t] +
                                        [c_int] * 6 + [c_uint, c_int, c_void_p]),
    'apa_pose_head_workspace_bytes': (c_size_t, [c_int] * 6),
    'apa_pose_head_fwd': (c_int, [c_void_p] * 8 + [c_size_t] + [c_int] * 6 + [c_void_p]),
    'apa_pose_head_bwd': (c_int, [c_void_p] * 7 + [c_int] + [c_void_p] * 5 + [c_size_t] + [c_int] * 6 +
                          [c_void_p]),
    'apa_pose_head_bwd_rank1ext': (c_int, [c_void_p] * 8 + [c_int] + [c_void_p] * 5 + [c_size_t] + [c_int] * 6 +
                                   [c_void_p]),
    'apa_softmax_xent_fwd_bwd': (c_int, [c_void_p] * 6 + [c_int, c_int, c_float, c_float, c_void_p]),
    'apa_pose_l2_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'apa_pose_l2_loss_fwd_bwd': (c_int, [c_void_p] * 6 + [c_size_t, c_int, c_int, c_int, c_float,
                                                          c_float, c_void_p]),
    'apa_action_loss_fwd_bwd': (c_int, [c_int] + [c_void_p] * 4 + [c_int, c_int, c_float, c_float, c_float, c_void_p]),
    'apa_pose_sampled_loss_fwd_bwd': (c_int, [c_void_p] * 7 + [c_int, c_int, c_int, c_float, c_float, c_void_p]),
    'apa_resize_bilinear_tf1': (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    'apa_pose_to_heatmap_out_ht': (c_int64, [c_int64, c_int64, c_int64]),
    'apa_pose_to_heatmap': (c_int, [POINTER(c_int64), c_int64, c_int64, c_int64, c_int64, c_int,
                                    c_float, c_int, POINTER(c_float), POINTER(c_uint8)]),
    'apa_spatial_mean_bwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'apa_zero_out_channels': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    'apa_pose_label_replay_resize': (c_int, [POINTER(c_uint8)] + [c_int] * 11 + [c_float, POINTER(c_float)]),
    'apa_pose_labels_device': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    'apa_image_aug_size': (c_int, [c_int] * 4 + [POINTER(ctypes.c_int32)]),
    'apa_preprocess_images_workspace_bytes': (c_size_t, [c_int, c_int, POINTER(ctypes.c_int32), c_int]),
    'apa_preprocess_images': (c_int, [c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                      c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # class attention maps and overlays (apa_explain.hip)
    'apa_attn_explain_workspace_bytes': (c_size_t, [c_int] * 6),
    'apa_attn_explain': (c_int, [c_void_p] * 11 + [c_size_t] + [c_int] * 6 + [c_uint, c_int, c_void_p]),
    'apa_attention_overlay_workspace_bytes': (c_size_t, [c_int, c_int]),
    'apa_attention_overlay': (c_int, [c_void_p] * 5 + [c_size_t] + [c_int] * 6 + [c_void_p]),
    # average precision, mAP and accuracy of accumulated scores (apa_metrics.hip)
    'apa_average_precision_workspace_bytes': (c_size_t, [c_int, c_int]),
    'apa_average_precision': (c_int, [c_void_p] * 3 + [c_int, c_int] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    'apa_frame_pool_fwd': (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p]),
    'apa_frame_pool_bwd': (c_int, [c_void_p] * 8 + [c_int] * 3 + [c_void_p]),
    'apa_clip_xent_workspace_bytes': (c_size_t, [c_int] * 3),
    'apa_clip_xent_fwd_bwd': (c_int, [c_void_p] * 11 + [c_size_t] + [c_int] * 3 + [c_float, c_float, c_void_p]),
    # the clip forms take a `const apa_clip_pool*` first
    'apa_clip_step_workspace_bytes': (c_size_t, [c_int] * 7 + [c_uint]),
    'apa_attn_head_train_step_clips': (c_int, [c_void_p] * 9 + [c_float, c_float] + [c_void_p] * 13 +
                                       [c_size_t] + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64, c_int,
                                                                   c_void_p]),
    'apa_pose_attn_train_step_clips': (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_uint, c_float, ctypes.c_uint64,
                                                                                    ctypes.c_uint64, c_int, c_void_p]),
    # the sigmoid action losses take a `const apa_multilabel*` first (the steps: then `const apa_clip_pool*` or NULL)
    'apa_multilabel_loss_fwd_bwd': (c_int, [c_void_p] * 4 + [c_int, c_int, c_float, c_float, c_void_p]),
    'apa_clip_multilabel_fwd_bwd': (c_int, [c_void_p] * 11 + [c_size_t] + [c_int] * 3 + [c_float, c_float, c_void_p]),
    'apa_attn_head_train_step_multilabel': (c_int, [c_void_p] * 9 + [c_float, c_float] + [c_void_p] * 13 +
                                            [c_size_t] + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64, c_int,
                                                                        c_void_p]),
    'apa_pose_attn_train_step_multilabel': (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_uint, c_float, ctypes.c_uint64,
                                                                                   ctypes.c_uint64, c_int, c_void_p]),
    'apa_attn_head_train_step': (c_int, [c_void_p] * 7 + [c_float, c_float] + [c_void_p] * 13 +
                                 [c_size_t] + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64, c_int,
                                                             c_void_p]),
    # ..._WITH_POSE_FEAT: `const apa_concat_feat*`, `const apa_hooks*`, then the plain arguments
    'apa_attn_pool_fwd_cat': (c_int, [c_void_p] * 14 + [c_size_t] + [c_int] * 6 +
                              [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    'apa_attn_pool_bwd_cat': (c_int, [c_void_p] * 19 + [c_size_t] + [c_int] * 6 +
                              [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    # rank > 1 with one bottom-up map: `const apa_rank_maps*` first, then the plain arguments (no topdown, no hooks)
    'apa_attn_pool_rank_workspace_bytes': (c_size_t, [c_int] * 6),
    'apa_attn_pool_rank_fwd': (c_int, [c_void_p] * 12 + [c_size_t] + [c_int] * 6 +
                               [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    'apa_attn_pool_rank_bwd': (c_int, [c_void_p] * 18 + [c_size_t] + [c_int] * 6 +
                               [c_uint, c_float, c_uint64, c_uint64, c_int, c_void_p]),
    'apa_attn_head_train_step_rank': (c_int, [c_void_p] * 8 + [c_float, c_float] + [c_void_p] * 13 +
                                      [c_size_t] + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64, c_int,
                                                                  c_void_p]),
    'apa_attn_head_train_step_ex': (c_int, [c_void_p] * 8 + [c_float, c_float] + [c_void_p] * 13 +
                                    [c_size_t] + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64, c_int,
                                                                c_void_p]),
    'apa_attn_head_eval_step': (c_int, [c_void_p] * 15 + [c_size_t] + [c_int] * 6 + [c_uint, c_int, c_void_p]),
    # evaluation of clips / sigmoid scores: `const apa_clip_pool*` (or NULL) and the scores kind first
    'apa_clip_scores': (c_int, [c_int] + [c_void_p] * 9 + [c_int] * 3 + [c_void_p]),
    'apa_attn_head_eval_step_clips': (c_int, [c_void_p, c_int] + [c_void_p] * 15 + [c_size_t] + [c_int] * 6 +
                                      [c_uint, c_int, c_void_p]),
    'apa_pose_attn_eval_step_clips': (c_int, [c_void_p, c_int, c_void_p] + [c_int] * 6 + [c_uint, c_int, c_void_p]),
    'apa_momentum_sgd_step': (c_int, [c_int, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float),
                                      c_void_p, c_void_p, c_float, c_float, c_float, c_void_p]),
    'apa_momentum_sgd_step_shadow': (c_int, [c_int, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float),
                                             c_void_p, c_void_p, c_float, c_float, c_float, POINTER(c_void_p),
                                             c_void_p]),
    'apa_per_class_weight_images': (c_int, [c_void_p] * 5 + [c_size_t] + [c_int] * 6 + [c_void_p, POINTER(c_int),
                                                                                       c_void_p]),
    'apa_momentum_sgd_step_images': (c_int, [c_int, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float),
                                             c_void_p, c_void_p, c_float, c_float, c_float, POINTER(c_void_p),
                                             c_void_p, POINTER(c_int), c_int, c_void_p]),
    'apa_adam_step': (c_int, [c_int, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float), c_void_p, c_void_p,
                              c_void_p, c_float, c_float, c_float, c_float, c_float, POINTER(c_void_p), c_void_p]),
    'apa_rmsprop_step': (c_int, [c_int, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_float), c_void_p, c_void_p,
                                 c_void_p, c_float, c_float, c_float, c_float, c_float, POINTER(c_void_p), c_void_p]),
    'apa_pose_attn_train_step': (c_int, [c_void_p] + [c_int] * 6 + [c_uint, c_float, ctypes.c_uint64,
                                                                    ctypes.c_uint64, c_int, c_void_p]),
    # `const apa_pose_attn_eval_io*` first
    'apa_pose_attn_eval_workspace_bytes': (c_size_t, [c_int] * 6 + [c_uint, c_int, c_int]),
    'apa_pose_attn_eval_step': (c_int, [c_void_p] + [c_int] * 6 + [c_uint, c_int, c_void_p]),
    'apa_accumulate_gradients': (c_int, [c_void_p, POINTER(c_void_p), c_int, c_size_t, c_float, c_void_p]),
    'apa_accumulate_gradients_div': (c_int, [c_void_p, POINTER(c_void_p), c_int, c_size_t, c_float, c_void_p]),
    'apa_clip_by_norm_workspace_bytes': (c_size_t, [c_int, POINTER(c_size_t)]),
    'apa_clip_by_norm_prepare': (c_int, [c_int, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_void_p),
                                         POINTER(c_float), POINTER(ctypes.c_ubyte), c_void_p, c_size_t,
                                         POINTER(c_int), c_void_p]),
    'apa_clip_by_norm_run': (c_int, [c_void_p, c_int, c_int, c_float, c_void_p]),
    'apa_pose_att_logits_workspace_bytes': (c_size_t, [c_int] * 5),
    'apa_pose_att_logits_fwd': (c_int, [c_void_p, c_void_p, POINTER(ctypes.c_int32), c_int, c_int] + [c_void_p] * 5 +
                                [c_size_t] + [c_int] * 5 + [c_uint, c_float, ctypes.c_uint64, ctypes.c_uint64, c_int,
                                                            c_void_p]),
    'apa_pose_att_logits_bwd': (c_int, [c_void_p, c_void_p, POINTER(ctypes.c_int32), c_int, c_int] + [c_void_p] * 4 +
                                [c_int] + [c_void_p] * 4 + [c_size_t] + [c_int] * 5 +
                                [c_uint, c_float, ctypes.c_uint64, ctypes.c_uint64, c_int, c_void_p]),
    'apa_pose_att_logits_fwd_ex': (c_int, [c_void_p, c_void_p, c_void_p, POINTER(ctypes.c_int32), c_int, c_int] +
                                   [c_void_p] * 5 + [c_size_t] + [c_int] * 5 +
                                   [c_uint, c_float, ctypes.c_uint64, ctypes.c_uint64, c_int, c_void_p]),
    'apa_pose_att_logits_bwd_ex': (c_int, [c_void_p, c_void_p, c_void_p, POINTER(ctypes.c_int32), c_int, c_int] +
                                   [c_void_p] * 4 + [c_int] + [c_void_p] * 4 + [c_size_t] + [c_int] * 5 +
                                   [c_uint, c_float, ctypes.c_uint64, ctypes.c_uint64, c_int, c_void_p]),
    'apa_prof_event_create': (c_int, [POINTER(c_void_p)]),
    'apa_prof_event_destroy': (c_int, [c_void_p]),
    'apa_prof_event_record': (c_int, [c_void_p, c_void_p]),
    'apa_prof_event_elapsed_ms': (c_int, [c_void_p, c_void_p, POINTER(c_float)]),
}

_lib = None


class ApaError(RuntimeError):
    pass


def exported_symbols():
    """Names the header declares (used by the CPU-side ABI test)."""
    return sorted(_SIGNATURES)


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen libapa_hip.so from this directory (like custom_ops_factory.py:11-18) and bind every
    entry point.  Fails loudly when the library has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get('APA_LIB_PATH') or LIB_PATH      # APA_LIB_PATH: compare two builds (tools/ab_libs.sh)
    if not os.path.exists(p):
        raise ApaError(
            '{} not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` or '
            '`make -C attentionalpoolingaction_amd/csrc`. There is no CPU fallback.'.format(p))
    lib = ctypes.CDLL(p)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == missing export
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        lib = load_library()
        raise ApaError('{} failed: {} ({})'.format(
            what, lib.apa_status_string(rc).decode(), lib.apa_last_error().decode()))


def _dev_ptr(t: Optional[torch.Tensor], name: str, dtype=None) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise ApaError('{} must live in GPU memory (got device {}); the HIP path has no CPU '
                       'fallback'.format(name, t.device))
    if not t.is_contiguous():
        raise ApaError('{} must be contiguous'.format(name))
    if dtype is not None and t.dtype != dtype:
        raise ApaError('{} must be {} (got {})'.format(name, dtype, t.dtype))
    return t.data_ptr()


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _feat_dtype(t) -> int:
    if isinstance(t, CachedBatch):
        t = t.cache.features
    if isinstance(t, Fp8Features):
        return APA_DTYPE_FP8_E4M3
    if t.dtype == torch.float32:
        return APA_DTYPE_F32
    if t.dtype == torch.bfloat16:
        return APA_DTYPE_BF16
    raise ApaError('feature maps must be float32 or bfloat16, got {}'.format(t.dtype))


# --------------------------------------------------------------------------------------------
# FP8 feature cache (include/apa.h: APA_DTYPE_FP8_E4M3)
# --------------------------------------------------------------------------------------------
FP8_E4M3_MAX = 448.0


def fp8_scale_offset(N: int, P: int, C: int) -> int:
    """byte offset of the N fp32 scales: the first 256-byte boundary behind the N*P*C codes"""
    return (N * P * C + 255) // 256 * 256


def fp8_features_bytes(N: int, P: int, C: int) -> int:
    """apa_fp8_features_bytes, restated (a cache can be laid out without the library)"""
    return fp8_scale_offset(N, P, C) + 4 * N


class Fp8Features(object):
    """A cached conv5 map in OCP FP8 E4M3 with one fp32 scale per image, as ONE uint8 buffer in the layout the
    library reads (include/apa.h): N*P*C codes in [N,P,C] order, then -- at the next 256-byte boundary -- N scales;
    element value = scale[n] * decode(code).  `codes` (torch.float8_e4m3fn, `shape`) and `scale` (float32 [N]) are
    views of that buffer.  Pass one as `X` (and the same object as `Xatt`) to attn_pool_fwd / attn_pool_bwd(want_dx=
    False) / HeadTrainStep(grads[0] = None) / HeadEvalStep: the class-agnostic head on frozen features.  Build one
    with quantize_features(), or with from_parts() from a cache that keeps codes and scales in separate arrays."""

    dtype = torch.float8_e4m3fn

    def __init__(self, buffer: torch.Tensor, shape):
        shape = tuple(int(d) for d in shape)
        if len(shape) < 2:
            raise ApaError('Fp8Features: [N, ..., C] expected')
        N, C = shape[0], shape[-1]
        n = int(np.prod(shape))
        P = n // (N * C)
        if C % 16:
            raise ApaError('Fp8Features: C = {} is not a multiple of 16'.format(C))
        if buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous() or \
                buffer.numel() < fp8_features_bytes(N, P, C):
            raise ApaError('Fp8Features: a contiguous 1-D uint8 buffer of fp8_features_bytes(N, P, C) bytes expected')
        if buffer.data_ptr() % 16:
            raise ApaError('Fp8Features: the buffer must be 16-byte aligned')
        self.buffer, self.shape = buffer, shape
        off = fp8_scale_offset(N, P, C)
        self.codes = buffer[:n].view(torch.float8_e4m3fn).view(shape)
        self.scale = buffer[off:off + 4 * N].view(torch.float32)

    # what the wrappers ask of a feature tensor
    device = property(lambda self: self.buffer.device)
    is_cuda = property(lambda self: self.buffer.is_cuda)

    def dim(self) -> int:
        return len(self.shape)

    def numel(self) -> int:
        return int(np.prod(self.shape))

    def is_contiguous(self) -> bool:
        return True

    def data_ptr(self) -> int:
        return self.buffer.data_ptr()

    def flat(self) -> 'Fp8Features':
        """the same buffer seen as [N, P, C]"""
        N, C = self.shape[0], self.shape[-1]
        return Fp8Features(self.buffer, (N, self.numel() // (N * C), C))

    @classmethod
    def empty(cls, shape, device) -> 'Fp8Features':
        shape = tuple(int(d) for d in shape)
        N, C = shape[0], shape[-1]
        P = int(np.prod(shape)) // (N * C)
        return cls(torch.zeros((fp8_features_bytes(N, P, C),), dtype=torch.uint8, device=device), shape)

    @classmethod
    def from_parts(cls, codes: torch.Tensor, scale: torch.Tensor) -> 'Fp8Features':
        """Pack a batch gathered from a cache that keeps `codes` ([N, ..., C], float8_e4m3fn or uint8) and `scale`
        ([N] float32) apart -- a training loop's random minibatch: `Fp8Features.from_parts(all_codes[idx],
        all_scales[idx])`.  One allocation and two copies on the codes' device."""
        if codes.dtype not in (torch.float8_e4m3fn, torch.uint8):
            raise ApaError('Fp8Features.from_parts: codes must be float8_e4m3fn (or their uint8 bits)')
        if scale.numel() != codes.shape[0]:
            raise ApaError('Fp8Features.from_parts: one scale per image expected')
        out = cls.empty(codes.shape, codes.device)
        out.codes.view(torch.uint8).copy_(codes.contiguous().view(torch.uint8))
        out.scale.copy_(scale.reshape(-1).to(torch.float32))
        return out

    def dequantize(self, dtype=torch.float32) -> torch.Tensor:
        """scale[n] * decode(code) as a float32 / bfloat16 tensor of `shape`: the device's own decode for a CUDA
        cache (apa_dequantize_features_fp8), torch's for a CPU one."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ApaError('Fp8Features.dequantize: float32 or bfloat16')
        N, C = self.shape[0], self.shape[-1]
        if not self.is_cuda:
            s = self.scale.view((N,) + (1,) * (len(self.shape) - 1))
            return (self.codes.to(torch.float32) * s).to(dtype)
        out = torch.empty(self.shape, dtype=dtype, device=self.device)
        rc = load_library().apa_dequantize_features_fp8(
            self.data_ptr(), out.data_ptr(), APA_DTYPE_F32 if dtype == torch.float32 else APA_DTYPE_BF16, N,
            self.numel() // (N * C), C, _stream_ptr())
        _check(rc, 'apa_dequantize_features_fp8')
        return out


def quantize_features(X: torch.Tensor):
    """(Fp8Features, status) = quantize_features(X): X [N, ..., C] float32 / bfloat16, C a multiple of 16.  Per image, in
    fp32 with IEEE division (include/apa.h): amax = max |x|, scale = amax / 448, inv = 448 / amax (both 0 when amax
    is 0), code = rne_e4m3(x * inv).  status int32 [N]: 1 = the image holds a non-finite value (codes and scale are
    zero then).  A CUDA tensor makes the device call (apa_quantize_features_fp8); a CPU tensor runs the same rule in
    torch, bit for bit -- a cache can be built and inspected without a GPU."""
    if X.dtype not in (torch.float32, torch.bfloat16):
        raise ApaError('quantize_features: float32 or bfloat16 features expected, got {}'.format(X.dtype))
    N, C = X.shape[0], X.shape[-1]
    P = X.numel() // (N * C)
    out = Fp8Features.empty(X.shape, X.device)
    status = torch.zeros((N,), dtype=torch.int32, device=X.device)
    if X.is_cuda:
        rc = load_library().apa_quantize_features_fp8(_dev_ptr(X, 'X'), APA_DTYPE_F32 if X.dtype == torch.float32
                                                      else APA_DTYPE_BF16, out.data_ptr(), status.data_ptr(), N, P, C,
                                                      _stream_ptr())
        _check(rc, 'apa_quantize_features_fp8')
        return out, status
    codes, scale, bad = _quantize_rule_cpu(X)
    out.codes.copy_(codes)
    out.scale.copy_(scale)
    status.copy_(bad)
    return out, status


def _quantize_rule_cpu(X: torch.Tensor):
    """(codes float8_e4m3fn like X, scale float32 [N], status int32 [N]): the quantisation rule in torch on the CPU"""
    N = X.shape[0]
    x = X.to(torch.float32).reshape(N, -1)
    bad = ~torch.isfinite(x).all(dim=1)
    amax = torch.where(bad, torch.zeros(()), x.abs().amax(dim=1))
    live = amax > 0
    m = torch.full((), FP8_E4M3_MAX, dtype=torch.float32)
    one = torch.ones((), dtype=torch.float32)
    scale = torch.where(live, amax / m, torch.zeros(()))
    inv = torch.where(live, m / torch.where(live, amax, one), torch.zeros(()))
    y = torch.where(live[:, None], x * inv[:, None], torch.zeros(()))
    return y.to(torch.float8_e4m3fn).view(X.shape), scale, bad.to(torch.int32)


# --------------------------------------------------------------------------------------------
# a resident feature cache read by image index (include/apa.h: apa_feature_cache)
# --------------------------------------------------------------------------------------------
class ApaFeatureCache(ctypes.Structure):
    """`apa_feature_cache` of include/apa.h (field order is the ABI)."""
    _fields_ = [('index', c_void_p), ('cache_images', c_int), ('labels_cached', c_int), ('status', c_void_p)]


def _index_tensor(who: str, index, device, n_images: Optional[int] = None) -> torch.Tensor:
    """`index` (tensor or sequence of image ids) as a contiguous int32 tensor on `device`; an int32 tensor that already
    is one passes through uncopied (an epoch's views)."""
    t = index if isinstance(index, torch.Tensor) else torch.as_tensor(list(index), dtype=torch.int64)
    if t.dim() != 1 or t.numel() < 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ApaError('{}: a non-empty 1-D integer index expected'.format(who))
    if t.dtype != torch.int32 or t.device != torch.device(device) or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.int32).contiguous()
    if n_images is not None and t.numel() != n_images:
        raise ApaError('{}: an index of {} images expected (got {})'.format(who, n_images, t.numel()))
    return t


class FeatureCache(object):
    """T cached conv5 maps [T,H,W,C] (float32 / bfloat16 tensor, or one Fp8Features of N = T) that stay where they are:
    a batch is the cache plus a vector of image ids (`select`), which the gathered kernels read through -- no gathered
    copy per step.  `labels`: optional int64 [T], read through the same index when a step is given `labels=None`.
    `status` (int32 [1] on the cache's device): how many ids outside [0, T) the forward passes met and clamped since it
    was last zeroed.  `gather` makes the copy a loop without the gathered kernels makes; it is the comparison route."""

    def __init__(self, features, labels: Optional[torch.Tensor] = None):
        fp8 = isinstance(features, Fp8Features)
        if not fp8 and features.dtype not in (torch.float32, torch.bfloat16):
            raise ApaError('FeatureCache: float32 / bfloat16 features or an Fp8Features expected')
        if features.dim() < 3 or not features.is_contiguous():
            raise ApaError('FeatureCache: contiguous [T, ..., C] features expected')
        self.features, self.shape = features, tuple(int(d) for d in features.shape)
        self.T = self.shape[0]
        self.device = features.device
        if labels is not None and (labels.dtype != torch.int64 or labels.numel() != self.T or
                                   labels.device != self.device or not labels.is_contiguous()):
            raise ApaError('FeatureCache: labels int64 [{}] on the cache\'s device expected'.format(self.T))
        self.labels = labels
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.V, self.video_first, self.video_frames = 0, None, None     # set_videos
        self.video_labels, self.video_targets = None, None

    fp8 = property(lambda self: isinstance(self.features, Fp8Features))
    dtype = property(lambda self: self.features.dtype)

    @classmethod
    def empty(cls, shape, dtype, device, labels: Optional[torch.Tensor] = None) -> 'FeatureCache':
        """a zeroed cache of `shape` = [T,H,W,C]; dtype torch.float32 / bfloat16 / float8_e4m3fn"""
        if dtype == torch.float8_e4m3fn:
            return cls(Fp8Features.empty(shape, device), labels)
        return cls(torch.zeros(tuple(shape), dtype=dtype, device=device), labels)

    def write(self, first: int, features: torch.Tensor) -> torch.Tensor:
        """Images [first, first + n) <- `features` [n,H,W,C] float32 / bfloat16 on the cache's device: cast (fp32 / bf16
        cache) or quantised into place (FP8: apa_quantize_features_fp8_at; a CPU cache applies the same rule in torch,
        bit for bit).  Returns the int32 [n] status of quantize_features (zeros for a cast)."""
        n, first = int(features.shape[0]), int(first)
        if tuple(features.shape[1:]) != self.shape[1:] or first < 0 or first + n > self.T:
            raise ApaError('FeatureCache.write: [n,{}] features for slots inside [0, {}) expected'.format(
                ','.join(str(d) for d in self.shape[1:]), self.T))
        if features.dtype not in (torch.float32, torch.bfloat16) or features.device != self.device:
            raise ApaError('FeatureCache.write: float32 / bfloat16 features on the cache\'s device expected')
        status = torch.zeros((n,), dtype=torch.int32, device=self.device)
        if not self.fp8:
            self.features[first:first + n].copy_(features)
            return status
        f = self.features
        if not f.is_cuda:
            codes, scale, bad = _quantize_rule_cpu(features)
            f.codes[first:first + n].copy_(codes)
            f.scale[first:first + n].copy_(scale)
            status.copy_(bad)
            return status
        C = self.shape[-1]
        src = features.contiguous()
        rc = load_library().apa_quantize_features_fp8_at(
            _dev_ptr(src, 'features'), APA_DTYPE_F32 if src.dtype == torch.float32 else APA_DTYPE_BF16, f.data_ptr(),
            self.T, first, status.data_ptr(), n, src.numel() // (n * C), C, _stream_ptr())
        _check(rc, 'apa_quantize_features_fp8_at')
        return status

    def gather(self, index):
        """the batch as a copy: features[index] (an Fp8Features for an FP8 cache: from_parts(codes[index],
        scale[index])) -- what a loop without the gathered kernels does every step"""
        idx = _index_tensor('FeatureCache.gather', index, self.device).long()
        if self.fp8:
            return Fp8Features.from_parts(self.features.codes[idx], self.features.scale[idx])
        return self.features[idx]

    def select(self, index) -> 'CachedBatch':
        """the batch without a copy: this cache and `index` (int32 on the cache's device, or converted once)"""
        return CachedBatch(self, index)

    def epoch(self, batch_size: int, seed: int, shuffle: bool = True, drop_last: bool = True):
        """One permutation of the T image ids per call, drawn on the cache's device from `seed` (arange without
        `shuffle`), yielded as its `batch_size`-long int32 views; the short last batch is dropped or yielded."""
        if batch_size < 1:
            raise ApaError('FeatureCache.epoch: batch_size >= 1 expected')
        if shuffle:
            g = torch.Generator(device=self.device)
            g.manual_seed(int(seed))
            perm = torch.randperm(self.T, generator=g, device=self.device).to(torch.int32)
        else:
            perm = torch.arange(self.T, dtype=torch.int32, device=self.device)
        end = self.T - self.T % batch_size if drop_last else self.T
        for a in range(0, end, batch_size):
            yield perm[a:min(a + batch_size, end)]

    def order(self, seed: int, epoch: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The visiting order of epoch `epoch` of the run keyed by `seed`: all T image ids, int32 on the cache's device,
        by the counter-based rule of include/apa.h (`epoch_order`: one launch on a GPU cache, the host restatement on
        a CPU one -- the same bits).  `out`: an int32 [T] tensor rewritten in place, so that an epoch call bound to it
        follows without a rebind.  `epoch` / `video_epoch` (torch.randperm) are other orders."""
        return epoch_order(self.T, seed, epoch, self.device, out=out)

    # ---- a cache of video FRAMES: clips sampled on the device (include/apa.h: apa_sample_clip_frames) ----
    def set_videos(self, first, count, labels: Optional[torch.Tensor] = None,
                   targets: Optional[torch.Tensor] = None) -> None:
        """The cache holds the frames of V videos: video v owns the slots [first[v], first[v] + count[v]).  `labels`
        int64 [V] and / or `targets` float32 multi-hot [V,K] (on the cache's device) are what `sample_clips` hands out
        per clip.  Validated once, here, on the host: count >= 1, first >= 0, first + count <= T, shapes, devices."""
        who = 'FeatureCache.set_videos'
        f = first.detach().cpu() if isinstance(first, torch.Tensor) else torch.as_tensor(list(first))
        c = count.detach().cpu() if isinstance(count, torch.Tensor) else torch.as_tensor(list(count))
        if f.dim() != 1 or c.dim() != 1 or f.numel() < 1 or f.numel() != c.numel() or \
                f.dtype.is_floating_point or c.dtype.is_floating_point or f.dtype == torch.bool or c.dtype == torch.bool:
            raise ApaError('{}: first and count are integer vectors of one length V >= 1'.format(who))
        f, c = f.long(), c.long()
        if int(c.min()) < 1:
            raise ApaError('{}: every video has at least one frame (count >= 1)'.format(who))
        if int(f.min()) < 0 or int((f + c).max()) > self.T:
            raise ApaError('{}: every video lies inside the cache: 0 <= first, first + count <= {}'.format(who, self.T))
        V = int(f.numel())
        if labels is not None and (labels.dtype != torch.int64 or tuple(labels.shape) != (V,) or
                                   labels.device != self.device or not labels.is_contiguous()):
            raise ApaError('{}: labels int64 [{}] on the cache\'s device expected'.format(who, V))
        if targets is not None and (targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[0] != V or
                                    targets.shape[1] < 1 or targets.device != self.device or
                                    not targets.is_contiguous()):
            raise ApaError('{}: targets float32 [{}, K] on the cache\'s device expected'.format(who, V))
        self.V = V
        self.video_first = f.to(device=self.device, dtype=torch.int32).contiguous()
        self.video_frames = c.to(device=self.device, dtype=torch.int32).contiguous()
        self.video_labels, self.video_targets = labels, targets

    def sample_clips(self, videos, frames: int, mode: str = 'uniform', u: Optional[torch.Tensor] = None,
                     generator: Optional[torch.Generator] = None, out: Optional['CachedClips'] = None) -> 'CachedClips':
        """B clips of `frames` frames each, one per entry of `videos` (ids into set_videos' tables; int32 on the cache's
        device passes uncopied), as a CachedClips: the batch's frame index and the clips' labels / targets, written by
        ONE launch (apa_sample_clip_frames; no host synchronisation).  mode 'uniform': the reference's evenly spaced
        frames; 'random-segment': one frame inside each of the F segments, from the uniform draws `u` float32 [B*frames]
        in [0,1) -- given, or drawn here from `generator` (torch.rand on the cache's device).  `out`: a previous
        CachedClips of the same B and `frames` whose buffers are rewritten in place -- a step bound to it needs no
        rebind.  A video id outside [0,V) is clamped and counted in the cache's `status`."""
        who = 'FeatureCache.sample_clips'
        if self.video_first is None:
            raise ApaError('{}: set_videos first'.format(who))
        if mode not in CLIP_FRAME_MODES:
            raise ApaError('{}: mode must be one of {} (got {!r})'.format(who, tuple(CLIP_FRAME_MODES), mode))
        F = int(frames)
        if F < 1:
            raise ApaError('{}: frames >= 1 expected'.format(who))
        vid = _index_tensor(who, videos, self.device)
        B = int(vid.numel())
        if B * F > 2 ** 31 - 1:
            raise ApaError('{}: B * frames past 2^31 - 1'.format(who))
        if u is not None and (u.dtype != torch.float32 or u.numel() != B * F or u.device != self.device or
                              not u.is_contiguous()):
            raise ApaError('{}: u float32 [{}] on the cache\'s device expected'.format(who, B * F))
        if out is not None and (not isinstance(out, CachedClips) or out.cache is not self or out.frames != F or
                                out.index.numel() != B * F):
            raise ApaError('{}: out must be a CachedClips of this cache with the same B and frames'.format(who))
        if not self.features.is_cuda:
            raise ApaError('{}: the cache must live in GPU memory; the HIP path has no CPU fallback'.format(who))
        if mode == 'random-segment' and u is None:
            u = torch.rand((B * F,), dtype=torch.float32, device=self.device, generator=generator)
        clips = out if out is not None else CachedClips(self, B, F)
        K = 0 if self.video_targets is None else int(self.video_targets.shape[1])
        rc = load_library().apa_sample_clip_frames(
            self.video_first.data_ptr(), self.video_frames.data_ptr(), _dev_ptr(self.video_labels, 'labels'),
            _dev_ptr(self.video_targets, 'targets'), vid.data_ptr(), _dev_ptr(u, 'u'), clips.index.data_ptr(),
            _dev_ptr(clips.labels, 'labels'), _dev_ptr(clips.targets, 'targets'), self.status.data_ptr(), self.V, B, F,
            K, CLIP_FRAME_MODES[mode], _stream_ptr())
        _check(rc, 'apa_sample_clip_frames')
        clips.videos = vid
        return clips

    def video_epoch(self, batch_videos: int, seed: int, shuffle: bool = True, drop_last: bool = True):
        """`epoch` over the V videos of set_videos: one permutation of the video ids per call, drawn on the cache's
        device from `seed`, yielded as its `batch_videos`-long int32 views (what `sample_clips` takes as `videos`)."""
        if self.video_first is None:
            raise ApaError('FeatureCache.video_epoch: set_videos first')
        if batch_videos < 1:
            raise ApaError('FeatureCache.video_epoch: batch_videos >= 1 expected')
        if shuffle:
            g = torch.Generator(device=self.device)
            g.manual_seed(int(seed))
            perm = torch.randperm(self.V, generator=g, device=self.device).to(torch.int32)
        else:
            perm = torch.arange(self.V, dtype=torch.int32, device=self.device)
        end = self.V - self.V % batch_videos if drop_last else self.V
        for a in range(0, end, batch_videos):
            yield perm[a:min(a + batch_videos, end)]


class CachedBatch(object):
    """N images of a FeatureCache named by an int32 index: pass one as `X` (and the same object as `Xatt`) to
    attn_pool_fwd / attn_pool_bwd(want_dx=False) / HeadTrainStep(grads[0] = None) / HeadEvalStep.  Nothing is copied;
    the kernels fetch image index[n] where they fetch image n of a plain batch, and the results are those of the same
    call on `cache.gather(index)`, bit for bit."""

    def __init__(self, cache: FeatureCache, index):
        self.cache = cache
        self.index = _index_tensor('CachedBatch', index, cache.device)
        self.shape = (int(self.index.numel()),) + cache.shape[1:]

    # what the wrappers ask of a feature tensor
    device = property(lambda self: self.cache.device)
    is_cuda = property(lambda self: self.cache.features.is_cuda)
    dtype = property(lambda self: self.cache.features.dtype)

    def dim(self) -> int:
        return len(self.shape)

    def numel(self) -> int:
        return int(np.prod(self.shape))

    def is_contiguous(self) -> bool:
        return True

    def data_ptr(self) -> int:
        return self.cache.features.data_ptr()

    def flat(self) -> 'CachedBatch':
        return self

    def descriptor(self, labels_cached: bool = False) -> ApaFeatureCache:
        """the apa_feature_cache of this batch (keep it, and this object, alive while calls that use it are in flight)"""
        if not self.index.is_cuda:
            raise ApaError('CachedBatch: the index must live in GPU memory; the HIP path has no CPU fallback')
        return ApaFeatureCache(self.index.data_ptr(), self.cache.T, 1 if labels_cached else 0,
                               self.cache.status.data_ptr())


class CachedClips(CachedBatch):
    """B clips of `frames` frames of a FeatureCache of video frames (`FeatureCache.sample_clips`): a CachedBatch of
    N = B * frames images whose `index` the sampler writes on the device, with the clips' `labels` int64 [B] and / or
    `targets` float32 [B,K] beside it (None where set_videos had none).  The buffers are this object's own:
    `sample_clips(..., out=clips)` rewrites them in place, so a step bound to them follows without a rebind."""

    def __init__(self, cache: FeatureCache, B: int, frames: int):
        dev = cache.device
        CachedBatch.__init__(self, cache, torch.zeros((int(B) * int(frames),), dtype=torch.int32, device=dev))
        self.frames, self.videos = int(frames), None
        self.labels = None if cache.video_labels is None else torch.zeros((int(B),), dtype=torch.int64, device=dev)
        self.targets = None if cache.video_targets is None else torch.zeros(
            (int(B), int(cache.video_targets.shape[1])), dtype=torch.float32, device=dev)


# --------------------------------------------------------------------------------------------
# a whole epoch over the cache (include/apa.h: apa_epoch_order, apa_epoch, apa_epoch_sgd)
# --------------------------------------------------------------------------------------------
class ApaEpoch(ctypes.Structure):
    """`apa_epoch` of include/apa.h (field order is the ABI)."""
    _fields_ = [('order', c_void_p), ('count', c_int)]


class ApaEpochSgd(ctypes.Structure):
    """`apa_epoch_sgd` of include/apa.h (field order is the ABI)."""
    _fields_ = [('nseg', c_int), ('weights', c_void_p), ('sizes', c_void_p), ('weight_decay', c_void_p),
                ('grad_flat', c_void_p), ('acc_flat', c_void_p), ('lr', c_void_p), ('momentum', c_float),
                ('grad_scale', c_float)]


_EPOCH_ROUNDS = 6
_M64 = (1 << 64) - 1


def _mix64(s: int, o: int) -> int:
    """the dropout key's splitmix64 step (include/apa.h: apa_epoch_order), python integers mod 2^64"""
    z = (s + 0x9E3779B97F4A7C15 * (o + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _epoch_hash(x: np.ndarray, k0: int, k1: int) -> np.ndarray:
    """the dropout mask's two-round 24-bit multiply-xorshift mix on uint64 lanes that hold 32-bit values"""
    u, m32, m24 = np.uint64, np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFF)
    x = x ^ u(k0)
    x = x ^ (x >> u(16))
    x = ((x & m24) * u(0xB5297B)) & m32
    x = x ^ (x >> u(13))
    x = x ^ u(k1)
    x = x ^ (x >> u(17))
    x = ((x & m24) * u(0x68E31D)) & m32
    return x ^ (x >> u(15))


def _epoch_order_rule_cpu(T: int, seed: int, epoch: int) -> torch.Tensor:
    """apa_epoch_order's rule restated in numpy (include/apa.h), bit for bit: int32 [T] on the CPU.  A keyed six-round
    alternating Feistel network on the smallest power-of-two domain >= max(T, 4), walked until the image is < T."""
    T = int(T)
    if not 1 <= T < 2 ** 31:
        raise ApaError('epoch_order: 1 <= T < 2^31 expected (got {})'.format(T))
    b = max(2, (T - 1).bit_length())
    lb = b // 2
    rb = np.uint64(b - lb)
    mL, mR = np.uint64((1 << lb) - 1), np.uint64((1 << (b - lb)) - 1)
    h = _mix64(int(seed) & _M64, int(epoch) & _M64)
    keys = [_mix64(h, r) for r in range(_EPOCH_ROUNDS)]

    def perm(x):
        L, R = x >> rb, x & mR
        for r, z in enumerate(keys):
            if r % 2 == 0:
                L = L ^ (_epoch_hash(R, z & 0xFFFFFFFF, z >> 32) & mL)
            else:
                R = R ^ (_epoch_hash(L, z & 0xFFFFFFFF, z >> 32) & mR)
        return (L << rb) | R

    x = perm(np.arange(T, dtype=np.uint64))
    while True:
        walk = np.nonzero(x >= np.uint64(T))[0]
        if walk.size == 0:
            return torch.from_numpy(x.astype(np.int32))
        x[walk] = perm(x[walk])


def epoch_order(T: int, seed: int, epoch: int, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """order int32 [T]: order[i] = the image visited at position i of epoch `epoch` of the run keyed by `seed`, a
    permutation of [0, T) that is a pure function of (T, seed, epoch) (include/apa.h: apa_epoch_order).  On a GPU
    `device` it is ONE launch -- no sort, no workspace, no host synchronisation, capturable; on the CPU the host
    restatement of the same rule gives the same bits.  `out`: an int32 [T] tensor on `device`, rewritten in place."""
    T, device = int(T), torch.device(device)
    if not 1 <= T < 2 ** 31:
        raise ApaError('epoch_order: 1 <= T < 2^31 expected (got {})'.format(T))
    if out is not None and (out.dtype != torch.int32 or out.dim() != 1 or out.numel() != T or
                            out.device.type != device.type or not out.is_contiguous()):
        raise ApaError('epoch_order: out must be a contiguous int32 [{}] tensor on {}'.format(T, device))
    if out is None:
        out = torch.empty((T,), dtype=torch.int32, device=device)
    if device.type != 'cuda':
        out.copy_(_epoch_order_rule_cpu(T, seed, epoch))
        return out
    rc = load_library().apa_epoch_order(out.data_ptr(), T, int(seed) & _M64, int(epoch) & _M64, _stream_ptr())
    _check(rc, 'apa_epoch_order')
    return out


def _cached(who: str, X, Xatt, frozen: bool = True) -> Optional['CachedBatch']:
    """X as a CachedBatch, or None for a plain feature tensor; a cache supplies its own attention input and is frozen"""
    if not isinstance(X, CachedBatch):
        return None
    if Xatt is not X or not frozen:
        raise ApaError('{}: a CachedBatch is frozen (no gradient for X: want_dx=False / grads[0] = None) and supplies '
                       'its own attention input (Xatt must be the same object)'.format(who))
    return X


def cached_per_class_served(cb, K: int) -> bool:
    """Does the library serve per-class maps (M == K) on this CachedBatch?  The C rule (apa_capi.hip: cache_form_why,
    the shape half of pc_fused_supported): a bf16 cache on the fused K <= 64 route."""
    C = int(cb.shape[-1])
    return (not cb.cache.fp8 and cb.dtype == torch.bfloat16 and 1 <= int(K) <= 64 and C % 256 == 0 and C <= 8192)


class KeepMask(object):
    """A dropout keep mask drawn OUTSIDE the library (the reference's tf.nn.dropout: floor(keep_prob + U),
    nets_factory.py:143-146,296), bit-packed for APA_FLAG_RNG_EXTERNAL: pass it as `seed=` to any of the
    attentional-pooling wrappers (forward AND backward).  Build one with pack_keep_mask()."""

    def __init__(self, bits: torch.Tensor, n_elems: int):
        self.bits, self.n_elems = bits, int(n_elems)


def pack_keep_mask(*parts: torch.Tensor, device='cuda') -> KeepMask:
    """{0,1} / bool tensors in the flat element order of the [N,P,C] feature map (for the *_cat ops followed
    by the [N,P,J] extra channels): concatenated and packed LSB-first -- bit (e & 7) of byte e >> 3 is
    element e (include/apa.h, APA_FLAG_RNG_EXTERNAL)."""
    flat = torch.cat([p.reshape(-1).to(device=device, dtype=torch.uint8) for p in parts])
    n = flat.numel()
    pad = (-n) % 64                                          # whole 8-byte words
    if pad:
        flat = torch.cat([flat, torch.zeros(pad, dtype=torch.uint8, device=flat.device)])
    w = (1 << torch.arange(8, device=flat.device, dtype=torch.int32))
    bits = ((flat.view(-1, 8) != 0).to(torch.int32) * w).sum(dim=1).to(torch.uint8).contiguous()
    return KeepMask(bits, n)


def _rng_key(seed, offset, flags):
    """-> (seed, offset, flags) as the C ABI takes them.  offset: an int is passed by value; a 1-element
    int64 CUDA tensor by address (APA_FLAG_RNG_DEVICE) so that hipGraph replays read -- and the backward
    advances -- it.  seed: an int keys the library's own counter hash; a KeepMask replays an external mask
    (APA_FLAG_RNG_EXTERNAL: its address travels in `seed`)."""
    if isinstance(seed, KeepMask):
        if isinstance(offset, torch.Tensor):
            raise ApaError('an external keep mask excludes the device-side dropout counter')
        if not seed.bits.is_cuda:
            raise ApaError('the packed keep mask must live on the GPU')
        return seed.bits.data_ptr(), 0, flags | APA_FLAG_RNG_EXTERNAL
    if isinstance(offset, torch.Tensor):
        if not (offset.is_cuda and offset.dtype == torch.int64 and offset.numel() == 1):
            raise ApaError('a device-side dropout counter must be a 1-element int64 CUDA tensor')
        return int(seed), offset.data_ptr(), flags | APA_FLAG_RNG_DEVICE
    return int(seed), int(offset), flags


class ApaHooks(ctypes.Structure):
    """`apa_hooks` of include/apa.h: per-call ordering / timing aids, passed explicitly to the *_ex
    entry points (the library keeps no per-thread or global state)."""
    _fields_ = [('grad_ready_event', c_void_p), ('td_weights_ready_event', c_void_p),
                ('prof_fwd_start', c_void_p), ('prof_fwd_stop', c_void_p),
                ('prof_bwd_start', c_void_p), ('prof_bwd_stop', c_void_p)]


def _event_handle(event):
    """torch.cuda.Event (recorded at least once, so that its handle exists), raw hipEvent_t or None."""
    if event is None:
        return None
    if isinstance(event, torch.cuda.Event):
        return event.cuda_event
    if isinstance(event, c_void_p):
        return event.value
    return int(event)


def make_hooks(grad_ready=None, td_weights_ready=None, prof_fwd=None, prof_bwd=None) -> ApaHooks:
    """Build an apa_hooks struct.  grad_ready / td_weights_ready: events (see include/apa.h);
    prof_fwd / prof_bwd: (start, stop) event pairs that receive the dispatch timestamps of the two
    streaming kernels.  Keep the returned object (and the events) alive while calls that use it are in
    flight."""
    h = ApaHooks()
    h.grad_ready_event = _event_handle(grad_ready)
    h.td_weights_ready_event = _event_handle(td_weights_ready)
    if prof_fwd is not None:
        h.prof_fwd_start, h.prof_fwd_stop = _event_handle(prof_fwd[0]), _event_handle(prof_fwd[1])
    if prof_bwd is not None:
        h.prof_bwd_start, h.prof_bwd_stop = _event_handle(prof_bwd[0]), _event_handle(prof_bwd[1])
    return h


def _hooks_ptr(hooks):
    return None if hooks is None else ctypes.addressof(hooks)


def attn_flags(softmax_att=False, relu_att=False, is_training=False, relu_input=False) -> int:
    return ((APA_FLAG_SOFTMAX_ATT if softmax_att else 0) | (APA_FLAG_RELU_ATT if relu_att else 0) |
            (APA_FLAG_TRAIN if is_training else 0) | (APA_FLAG_RELU_INPUT if relu_input else 0))


# --------------------------------------------------------------------------------------------
# attentional pooling
# --------------------------------------------------------------------------------------------
def attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags=0) -> int:
    return int(load_library().apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags))


def attn_pool_fwd(X, Xatt, Wa, ba, Wt, bt, *, flags=0, keep_prob=1.0, seed=0, offset=0,
                  workspace=None, want_topdown=False, hooks=None):
    """logits, att, zsave, abar, topdown, workspace = attn_pool_fwd(...)

    X [N,P,C] (or [N,H,W,C]) f32/bf16; Xatt same tensor object as X (cfg 002) or [N,P,Ca];
    Wa [Ca,M], ba [M], Wt [C,K], bt [K] f32.  See include/apa.h: apa_attn_pool_fwd.
    """
    lib = load_library()
    N = X.shape[0]
    C = X.shape[-1]
    P = X.numel() // (N * C)
    Ca = Xatt.shape[-1]
    M = Wa.shape[1]
    K = Wt.shape[1]
    dt = _feat_dtype(X)
    dev = X.device
    cb = _cached('attn_pool_fwd', X, Xatt)
    logits = torch.empty((N, K), dtype=torch.float32, device=dev)
    att = torch.empty((N, P, M), dtype=torch.float32, device=dev)
    # saved for backward: M == 1 -> z [N,C] + abar [N]; per-class -> the fp32 top-down map [N,P,K]
    zsave = torch.empty((N, C) if M == 1 else (N, P, K), dtype=torch.float32, device=dev)
    abar = torch.empty((N,), dtype=torch.float32, device=dev) if M == 1 else None
    if want_topdown and isinstance(X, (Fp8Features, CachedBatch)):
        raise ApaError('attn_pool_fwd: the TopDownAttention dump is not served on a feature cache')
    topdown = torch.empty((N, P, K), dtype=X.dtype, device=dev) if want_topdown else None
    need = int(lib.apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    xatt_ptr = _dev_ptr(X, 'X') if Xatt is X else _dev_ptr(Xatt, 'Xatt', X.dtype)
    seed, offset, flags = _rng_key(seed, offset, flags)
    fn, pre = lib.apa_attn_pool_fwd_ex, ()
    if cb is not None:      # a FeatureCache read by index: the descriptor in front of the same arguments
        desc = cb.descriptor()
        fn, pre = lib.apa_attn_pool_fwd_cached, (ctypes.addressof(desc),)
    rc = fn(
        *pre, _hooks_ptr(hooks), _dev_ptr(X, 'X'), xatt_ptr, _dev_ptr(Wa, 'Wa', torch.float32),
        _dev_ptr(ba, 'ba', torch.float32), _dev_ptr(Wt, 'Wt', torch.float32),
        _dev_ptr(bt, 'bt', torch.float32), logits.data_ptr(), att.data_ptr(),
        _dev_ptr(zsave, 'zsave'), _dev_ptr(abar, 'abar'), _dev_ptr(topdown, 'topdown'),
        workspace.data_ptr(), workspace.numel(), N, P, C, Ca, K, M, flags, float(keep_prob),
        int(seed), offset, dt, _stream_ptr())
    _check(rc, 'apa_attn_pool_fwd')
    return logits, att, zsave, abar, topdown, workspace


def attn_pool_bwd(X, Xatt, Wa, ba, Wt, bt, att, zsave, abar, G, *, flags=0, keep_prob=1.0, seed=0,
                  offset=0, workspace=None, out=None, dxatt_rank1=False, hooks=None, want_dx=True):
    """dX, dXatt, dWa, dba, dWt, dbt = attn_pool_bwd(...).  `out` may supply preallocated
    (dX, dXatt, dWa, dba, dWt, dbt) buffers (e.g. views into a flat DP gradient bucket).
    `dxatt_rank1=True` (separate attention input, one bottom-up map): the second result is dZ, f32
    [N*P], with dXatt = dZ (x) Wa left to the consumer (APA_FLAG_DXATT_RANK1).
    `want_dx=False` (frozen features, APA_FLAG_FROZEN_INPUT): no gradient for X is computed or stored, the first
    result is None and `out[0]` may be None; everything else is bit-identical.  Where the library refuses the flag
    (APA_ERR_UNSUPPORTED: the dense per-class route) the call is repeated without it on a scratch dX -- the full
    cost, the same results, still None for dX."""
    lib = load_library()
    N = X.shape[0]
    C = X.shape[-1]
    P = X.numel() // (N * C)
    Ca = Xatt.shape[-1]
    M = Wa.shape[1]
    K = Wt.shape[1]
    dt = _feat_dtype(X)
    dev = X.device
    fused = Xatt is X
    fp8 = isinstance(X, Fp8Features)
    if fp8 and (want_dx or (out is not None and out[0] is not None)):
        raise ApaError('attn_pool_bwd: an Fp8Features cache has no gradient: pass want_dx=False (and out[0] = None)')
    cb = _cached('attn_pool_bwd', X, Xatt, frozen=not want_dx and (out is None or out[0] is None))
    fn, pre = lib.apa_attn_pool_bwd_ex, ()
    if cb is not None:      # a FeatureCache read by index: the descriptor in front of the same arguments
        desc = cb.descriptor()
        fn, pre = lib.apa_attn_pool_bwd_cached, (ctypes.addressof(desc),)
    if dxatt_rank1 and not fused:
        flags |= APA_FLAG_DXATT_RANK1
    if not want_dx:
        flags |= APA_FLAG_FROZEN_INPUT
    if out is None:
        dX = torch.empty_like(X) if want_dx else None
        if fused:
            dXatt = None
        elif dxatt_rank1:
            dXatt = torch.empty((N * P,), dtype=torch.float32, device=dev)
        else:
            dXatt = torch.empty_like(Xatt)
        dWa = torch.empty_like(Wa)
        dba = torch.empty_like(ba)
        dWt = torch.empty_like(Wt)
        dbt = torch.empty_like(bt)
    else:
        dX, dXatt, dWa, dba, dWt, dbt = out
    need = int(lib.apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    xatt_ptr = _dev_ptr(X, 'X') if fused else _dev_ptr(Xatt, 'Xatt', X.dtype)
    seed, offset, flags = _rng_key(seed, offset, flags)

    def call(dx, fl):
        return fn(
            *pre, _hooks_ptr(hooks), _dev_ptr(X, 'X'), xatt_ptr, _dev_ptr(Wa, 'Wa', torch.float32),
            _dev_ptr(ba, 'ba', torch.float32), _dev_ptr(Wt, 'Wt', torch.float32),
            _dev_ptr(bt, 'bt', torch.float32), _dev_ptr(att, 'att', torch.float32),
            _dev_ptr(zsave, 'zsave'), _dev_ptr(abar, 'abar'), _dev_ptr(G, 'G', torch.float32),
            _dev_ptr(dx, 'dX'), _dev_ptr(dXatt, 'dXatt'), _dev_ptr(dWa, 'dWa'), _dev_ptr(dba, 'dba'),
            _dev_ptr(dWt, 'dWt'), _dev_ptr(dbt, 'dbt'), workspace.data_ptr(), workspace.numel(), N, P,
            C, Ca, K, M, fl, float(keep_prob), int(seed), offset, dt, _stream_ptr())
    rc = call(dX, flags)
    if rc == APA_ERR_UNSUPPORTED and not want_dx and not fp8 and cb is None:      # a route without the arm: the full call, dX to scratch
        rc = call(torch.empty_like(X), flags & ~APA_FLAG_FROZEN_INPUT)
    _check(rc, 'apa_attn_pool_bwd')
    return (dX if want_dx else None), dXatt, dWa, dba, dWt, dbt


class ApaConcatFeat(ctypes.Structure):
    """`apa_concat_feat` of include/apa.h (..._WITH_POSE_FEAT, nets_factory.py:289-295)."""
    _fields_ = [('Xext', c_void_p), ('J', c_int), ('zext', c_void_p), ('dXext', c_void_p)]


def attn_pool_fwd_cat(X, Xatt, Xext, Wa, ba, Wt, bt, *, flags=0, keep_prob=1.0, seed=0, offset=0,
                      workspace=None, hooks=None):
    """logits, att, zsave, abar, zext, workspace = attn_pool_fwd_cat(...): attentional pooling over
    concat(X, Xext) without forming it (include/apa.h: apa_attn_pool_fwd_cat).  Xext [N,P,J] (or
    [N,H,W,J]) f32; Wt is the full [C+J, K] td_weights; M == 1."""
    lib = load_library()
    N, C = X.shape[0], X.shape[-1]
    P = X.numel() // (N * C)
    Ca, M, K, J = Xatt.shape[-1], Wa.shape[1], Wt.shape[1], Xext.shape[-1]
    if Wt.shape[0] != C + J or Xext.numel() != N * P * J:
        raise ApaError('attn_pool_fwd_cat: Wt must be [C+J, K] and Xext [N,P,J]')
    dev = X.device
    logits = torch.empty((N, K), dtype=torch.float32, device=dev)
    att = torch.empty((N, P, M), dtype=torch.float32, device=dev)
    zsave = torch.empty((N, C), dtype=torch.float32, device=dev)
    abar = torch.empty((N,), dtype=torch.float32, device=dev)
    zext = torch.empty((N, J), dtype=torch.float32, device=dev)
    need = int(lib.apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    cat = ApaConcatFeat(_dev_ptr(Xext, 'Xext', torch.float32), J, zext.data_ptr(), None)
    xatt_ptr = _dev_ptr(X, 'X') if Xatt is X else _dev_ptr(Xatt, 'Xatt', X.dtype)
    seed, offset, flags = _rng_key(seed, offset, flags)
    rc = lib.apa_attn_pool_fwd_cat(
        ctypes.addressof(cat), _hooks_ptr(hooks), _dev_ptr(X, 'X'), xatt_ptr, _dev_ptr(Wa, 'Wa', torch.float32),
        _dev_ptr(ba, 'ba', torch.float32), _dev_ptr(Wt, 'Wt', torch.float32),
        _dev_ptr(bt, 'bt', torch.float32), logits.data_ptr(), att.data_ptr(), zsave.data_ptr(),
        abar.data_ptr(), None, workspace.data_ptr(), workspace.numel(), N, P, C, Ca, K, M, flags,
        float(keep_prob), int(seed), offset, _feat_dtype(X), _stream_ptr())
    _check(rc, 'apa_attn_pool_fwd_cat')
    return logits, att, zsave, abar, zext, workspace


def attn_pool_bwd_cat(X, Xatt, Xext, zext, Wa, ba, Wt, bt, att, zsave, abar, G, *, flags=0, keep_prob=1.0,
                      seed=0, offset=0, workspace=None, hooks=None):
    """dX, dXatt, dXext, dWa, dba, dWt, dbt = attn_pool_bwd_cat(...); dWt is [C+J, K]."""
    lib = load_library()
    N, C = X.shape[0], X.shape[-1]
    P = X.numel() // (N * C)
    Ca, M, K, J = Xatt.shape[-1], Wa.shape[1], Wt.shape[1], Xext.shape[-1]
    dev = X.device
    fused = Xatt is X
    dX = torch.empty_like(X)
    dXatt = None if fused else torch.empty_like(Xatt)
    dXext = torch.empty_like(Xext)
    dWa, dba, dWt, dbt = torch.empty_like(Wa), torch.empty_like(ba), torch.empty_like(Wt), torch.empty_like(bt)
    need = int(lib.apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    cat = ApaConcatFeat(_dev_ptr(Xext, 'Xext', torch.float32), J, _dev_ptr(zext, 'zext', torch.float32),
                        dXext.data_ptr())
    xatt_ptr = _dev_ptr(X, 'X') if fused else _dev_ptr(Xatt, 'Xatt', X.dtype)
    seed, offset, flags = _rng_key(seed, offset, flags)
    rc = lib.apa_attn_pool_bwd_cat(
        ctypes.addressof(cat), _hooks_ptr(hooks), _dev_ptr(X, 'X'), xatt_ptr, _dev_ptr(Wa, 'Wa', torch.float32),
        _dev_ptr(ba, 'ba', torch.float32), _dev_ptr(Wt, 'Wt', torch.float32),
        _dev_ptr(bt, 'bt', torch.float32), _dev_ptr(att, 'att', torch.float32), _dev_ptr(zsave, 'zsave'),
        _dev_ptr(abar, 'abar'), _dev_ptr(G, 'G', torch.float32), dX.data_ptr(), _dev_ptr(dXatt, 'dXatt'),
        dWa.data_ptr(), dba.data_ptr(), dWt.data_ptr(), dbt.data_ptr(), workspace.data_ptr(),
        workspace.numel(), N, P, C, Ca, K, M, flags, float(keep_prob), int(seed), offset, _feat_dtype(X),
        _stream_ptr())
    _check(rc, 'apa_attn_pool_bwd_cat')
    return dX, dXatt, dXext, dWa, dba, dWt, dbt


class ApaRankMaps(ctypes.Structure):
    """`apa_rank_maps` of include/apa.h: ranks 1 .. R-1 of NET.USE_POSE_PRELOGITS_BASED_ATTENTION_RANK = R (entry
    r-1 for rank r; rank 0 travels in the flat argument list)."""
    _fields_ = [('extra', c_int),
                ('chain_w', c_void_p * (APA_RANK_MAX - 1)), ('chain_b', c_void_p * (APA_RANK_MAX - 1)),
                ('Wt', c_void_p * (APA_RANK_MAX - 1)), ('bt', c_void_p * (APA_RANK_MAX - 1)),
                ('dchain_w', c_void_p * (APA_RANK_MAX - 1)), ('dchain_b', c_void_p * (APA_RANK_MAX - 1)),
                ('dWt', c_void_p * (APA_RANK_MAX - 1)), ('dbt', c_void_p * (APA_RANK_MAX - 1)),
                ('z0', c_void_p)]


def _bind_rank_maps(who, Wts, bts, chain_w, chain_b, z0, grads=None) -> ApaRankMaps:
    """Wts / bts: R tensors [C,K] / [K] (rank 0 first); chain_w / chain_b: R - 1 one-element tensors (the weights and
    biases of 'Conv2d_PrePose_Attn<r>'); grads = (dWts, dbts, dchain_w, dchain_b) of the same shapes, backward only.
    The rank is checked here: the library would refuse it too (APA_ERR_INVALID_ARG)."""
    R = len(Wts)
    if not (2 <= R <= APA_RANK_MAX):
        raise ApaError('{}: rank {} outside 2..{}'.format(who, R, APA_RANK_MAX))
    if len(bts) != R or len(chain_w) != R - 1 or len(chain_b) != R - 1:
        raise ApaError('{}: rank {} needs {} Wt / bt and {} chain weights / biases'.format(who, R, R, R - 1))
    rk = ApaRankMaps()
    rk.extra = R - 1
    for r in range(R - 1):
        if chain_w[r].numel() != 1 or chain_b[r].numel() != 1:
            raise ApaError('{}: the chain convs map one channel to one channel (one float each)'.format(who))
        rk.chain_w[r] = _dev_ptr(chain_w[r], 'chain_w', torch.float32)
        rk.chain_b[r] = _dev_ptr(chain_b[r], 'chain_b', torch.float32)
        rk.Wt[r] = _dev_ptr(Wts[r + 1], 'Wt', torch.float32)
        rk.bt[r] = _dev_ptr(bts[r + 1], 'bt', torch.float32)
        if grads is not None:
            dWts, dbts, dcw, dcb = grads
            rk.dWt[r] = _dev_ptr(dWts[r + 1], 'dWt', torch.float32)
            rk.dbt[r] = _dev_ptr(dbts[r + 1], 'dbt', torch.float32)
            rk.dchain_w[r] = _dev_ptr(dcw[r], 'dchain_w', torch.float32)
            rk.dchain_b[r] = _dev_ptr(dcb[r], 'dchain_b', torch.float32)
    rk.z0 = _dev_ptr(z0, 'z0', torch.float32)
    return rk


def _rank_dims(X, Xatt, Wa, Wts):
    N, C = X.shape[0], X.shape[-1]
    return N, X.numel() // (N * C), C, Xatt.shape[-1], Wts[0].shape[1], Wa.shape[1]


def _rank_workspace(who, lib, workspace, N, P, C, Ca, K, R, dev):
    need = int(lib.apa_attn_pool_rank_workspace_bytes(N, P, C, Ca, K, R - 1))
    if workspace is None or workspace.numel() < max(need, 16):
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    return workspace


def attn_pool_rank_fwd(X, Xatt, Wa, ba, Wts, bts, chain_w, chain_b, *, flags=0, keep_prob=1.0, seed=0, offset=0,
                       workspace=None):
    """logits, att, zsave, abar, z0, workspace = attn_pool_rank_fwd(...): R = len(Wts) attention maps chained from
    ONE bottom-up map, pooled in one pass over X (include/apa.h: apa_attn_pool_rank_fwd).  att [N,P,R], zsave
    [N,R,C], abar [N,R], z0 [N,P] (saved for the backward call)."""
    lib = load_library()
    N, P, C, Ca, K, M = _rank_dims(X, Xatt, Wa, Wts)
    R, dev = len(Wts), X.device
    logits = torch.empty((N, K), dtype=torch.float32, device=dev)
    att = torch.empty((N, P, R), dtype=torch.float32, device=dev)
    zsave = torch.empty((N, R, C), dtype=torch.float32, device=dev)
    abar = torch.empty((N, R), dtype=torch.float32, device=dev)
    z0 = torch.empty((N, P), dtype=torch.float32, device=dev)
    rk = _bind_rank_maps('attn_pool_rank_fwd', Wts, bts, chain_w, chain_b, z0)
    workspace = _rank_workspace('attn_pool_rank_fwd', lib, workspace, N, P, C, Ca, K, R, dev)
    xatt_ptr = _dev_ptr(X, 'X') if Xatt is X else _dev_ptr(Xatt, 'Xatt', X.dtype)
    seed, offset, flags = _rng_key(seed, offset, flags)
    rc = lib.apa_attn_pool_rank_fwd(
        ctypes.addressof(rk), _dev_ptr(X, 'X'), xatt_ptr, _dev_ptr(Wa, 'Wa', torch.float32),
        _dev_ptr(ba, 'ba', torch.float32), _dev_ptr(Wts[0], 'Wt', torch.float32), _dev_ptr(bts[0], 'bt', torch.float32),
        logits.data_ptr(), att.data_ptr(), zsave.data_ptr(), abar.data_ptr(), workspace.data_ptr(), workspace.numel(),
        N, P, C, Ca, K, M, flags, float(keep_prob), int(seed), offset, _feat_dtype(X), _stream_ptr())
    _check(rc, 'apa_attn_pool_rank_fwd')
    return logits, att, zsave, abar, z0, workspace


def attn_pool_rank_bwd(X, Xatt, Wa, ba, Wts, bts, chain_w, chain_b, att, zsave, abar, z0, G, *, flags=0,
                       keep_prob=1.0, seed=0, offset=0, workspace=None, out=None):
    """dX, dXatt, dWa, dba, dWts, dbts, dchain_w, dchain_b = attn_pool_rank_bwd(...); the last four are lists (R, R,
    R - 1, R - 1 tensors).  `out` may supply the eight preallocated (e.g. views into a flat gradient bucket)."""
    lib = load_library()
    N, P, C, Ca, K, M = _rank_dims(X, Xatt, Wa, Wts)
    R, dev, fused = len(Wts), X.device, Xatt is X
    if out is None:
        out = (torch.empty_like(X), None if fused else torch.empty_like(Xatt), torch.empty_like(Wa),
               torch.empty_like(ba), [torch.empty_like(w) for w in Wts], [torch.empty_like(b) for b in bts],
               [torch.empty_like(w) for w in chain_w], [torch.empty_like(b) for b in chain_b])
    dX, dXatt, dWa, dba, dWts, dbts, dcw, dcb = out
    rk = _bind_rank_maps('attn_pool_rank_bwd', Wts, bts, chain_w, chain_b, z0, (dWts, dbts, dcw, dcb))
    workspace = _rank_workspace('attn_pool_rank_bwd', lib, workspace, N, P, C, Ca, K, R, dev)
    xatt_ptr = _dev_ptr(X, 'X') if fused else _dev_ptr(Xatt, 'Xatt', X.dtype)
    seed, offset, flags = _rng_key(seed, offset, flags)
    rc = lib.apa_attn_pool_rank_bwd(
        ctypes.addressof(rk), _dev_ptr(X, 'X'), xatt_ptr, _dev_ptr(Wa, 'Wa', torch.float32),
        _dev_ptr(ba, 'ba', torch.float32), _dev_ptr(Wts[0], 'Wt', torch.float32), _dev_ptr(bts[0], 'bt', torch.float32),
        _dev_ptr(att, 'att', torch.float32), _dev_ptr(zsave, 'zsave', torch.float32),
        _dev_ptr(abar, 'abar', torch.float32), _dev_ptr(G, 'G', torch.float32), _dev_ptr(dX, 'dX', X.dtype),
        None if fused else _dev_ptr(dXatt, 'dXatt', X.dtype), _dev_ptr(dWa, 'dWa', torch.float32),
        _dev_ptr(dba, 'dba', torch.float32), _dev_ptr(dWts[0], 'dWt', torch.float32),
        _dev_ptr(dbts[0], 'dbt', torch.float32), workspace.data_ptr(), workspace.numel(), N, P, C, Ca, K, M, flags,
        float(keep_prob), int(seed), offset, _feat_dtype(X), _stream_ptr())
    _check(rc, 'apa_attn_pool_rank_bwd')
    return dX, dXatt, dWa, dba, dWts, dbts, dcw, dcb


def dropout_mask(shape, keep_prob, seed, offset, device='cuda') -> torch.Tensor:
    """The exact {0,1} mask APA_FLAG_TRAIN applies to X (uint8, `shape` = X.shape)."""
    lib = load_library()
    mask = torch.empty(shape, dtype=torch.uint8, device=device)
    rc = lib.apa_dropout_mask(_dev_ptr(mask, 'mask'), mask.numel(), float(keep_prob), int(seed),
                              int(offset), _stream_ptr())
    _check(rc, 'apa_dropout_mask')
    return mask


# --------------------------------------------------------------------------------------------
# PoseLogits head (nets_factory.py:147-160)
# --------------------------------------------------------------------------------------------
def pose_head_fwd(X, W1, b1, W2, b2, workspace=None, out=None):
    """Ppre [..,Cp] (dtype of X), Pl [..,J] f32, workspace = pose_head_fwd(X [N,P,C] or [N,H,W,C], ...).
    `out=(Ppre, Pl)`: write into these caller-owned buffers (fixed addresses, e.g. for a HeadTrainStep
    bound to Ppre as its attention input)."""
    lib = load_library()
    N, C = X.shape[0], X.shape[-1]
    P = X.numel() // (N * C)
    Cp, J = W1.shape[1], W2.shape[1]
    dt = _feat_dtype(X)
    need = int(lib.apa_pose_head_workspace_bytes(N, P, C, Cp, J, dt))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=X.device)
    if out is not None:
        Ppre, Pl = out
        if Ppre.dtype != X.dtype or Ppre.numel() != N * P * Cp or Pl.dtype != torch.float32 or Pl.numel() != N * P * J:
            raise ApaError('pose_head_fwd: out=(Ppre, Pl) must be {} [N*P*{}] and float32 [N*P*{}]'.format(
                X.dtype, Cp, J))
        _dev_ptr(Ppre, 'Ppre', X.dtype)
        _dev_ptr(Pl, 'Pl', torch.float32)
    else:
        Ppre = torch.empty(tuple(X.shape[:-1]) + (Cp,), dtype=X.dtype, device=X.device)
        Pl = torch.empty(tuple(X.shape[:-1]) + (J,), dtype=torch.float32, device=X.device)
    rc = lib.apa_pose_head_fwd(
        _dev_ptr(X, 'X'), _dev_ptr(W1, 'W1', torch.float32), _dev_ptr(b1, 'b1', torch.float32),
        _dev_ptr(W2, 'W2', torch.float32), _dev_ptr(b2, 'b2', torch.float32), Ppre.data_ptr(),
        Pl.data_ptr(), workspace.data_ptr(), workspace.numel(), N, P, C, Cp, J, dt, _stream_ptr())
    _check(rc, 'apa_pose_head_fwd')
    return Ppre, Pl, workspace


def pose_head_bwd(X, W1, W2, Ppre, dPl, dPpre_ext, *, dX=None, accumulate_dX=False, workspace=None, ws_from_fwd=False,
                  ext_rank1=None, want_dx=True):
    """dX, dW1, db1, dW2, db2 = pose_head_bwd(...).  dPl: pose-loss gradient [..,J] f32 or None;
    dPpre_ext: gradient from the attention branch [..,Cp] (dtype of X) or None.  With
    accumulate_dX the product dPpre.W1^T is ADDED to the given dX buffer.  `ext_rank1=(row, col)`:
    the attention-branch gradient in rank-1 form row [N*P] (x) col [Cp], both f32
    (apa_pose_head_bwd_rank1ext; dPpre_ext must then be None).  `ws_from_fwd=True`: `workspace` is
    the one pose_head_fwd returned and nothing has written to it since (APA_POSE_WS_FROM_FWD: the bf16
    copy of W1 in it is reused).  `want_dx=False` (frozen features, APA_POSE_NO_DX): the dX product is not launched,
    `dX` is not touched and the first result is None."""
    lib = load_library()
    N, C = X.shape[0], X.shape[-1]
    P = X.numel() // (N * C)
    Cp, J = W1.shape[1], W2.shape[1]
    dt = _feat_dtype(X)
    need = int(lib.apa_pose_head_workspace_bytes(N, P, C, Cp, J, dt))
    if workspace is None or workspace.numel() < need:
        if ws_from_fwd:
            raise ApaError('ws_from_fwd needs the workspace of the forward call')
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=X.device)
    acc_flag = (1 if accumulate_dX else 0) | (APA_POSE_WS_FROM_FWD if ws_from_fwd else 0)
    if not want_dx:
        acc_flag, dX = (acc_flag & ~1) | APA_POSE_NO_DX, None
    elif dX is None:
        if accumulate_dX:
            raise ApaError('accumulate_dX needs an existing dX buffer')
        dX = torch.empty_like(X)
    dW1, db1 = torch.empty_like(W1), torch.empty((Cp,), dtype=torch.float32, device=X.device)
    dW2, db2 = torch.empty_like(W2), torch.empty((J,), dtype=torch.float32, device=X.device)
    if ext_rank1 is not None:
        if dPpre_ext is not None:
            raise ApaError('give the attention-branch gradient either as a tensor or in rank-1 form')
        row, col = ext_rank1
        if row.numel() != N * P or col.numel() != Cp:
            raise ApaError('ext_rank1: row must have N*P = {} and col Cp = {} elements'.format(N * P, Cp))
        rc = lib.apa_pose_head_bwd_rank1ext(
            _dev_ptr(X, 'X'), _dev_ptr(W1, 'W1', torch.float32), _dev_ptr(W2, 'W2', torch.float32),
            _dev_ptr(Ppre, 'Ppre', X.dtype), _dev_ptr(dPl, 'dPl', torch.float32),
            _dev_ptr(row, 'ext_row', torch.float32), _dev_ptr(col, 'ext_col', torch.float32),
            _dev_ptr(dX, 'dX', X.dtype), acc_flag, dW1.data_ptr(), db1.data_ptr(),
            dW2.data_ptr(), db2.data_ptr(), workspace.data_ptr(), workspace.numel(), N, P, C, Cp, J, dt,
            _stream_ptr())
        _check(rc, 'apa_pose_head_bwd_rank1ext')
        return dX, dW1, db1, dW2, db2
    rc = lib.apa_pose_head_bwd(
        _dev_ptr(X, 'X'), _dev_ptr(W1, 'W1', torch.float32), _dev_ptr(W2, 'W2', torch.float32),
        _dev_ptr(Ppre, 'Ppre', X.dtype), _dev_ptr(dPl, 'dPl', torch.float32),
        _dev_ptr(dPpre_ext, 'dPpre_ext', X.dtype), _dev_ptr(dX, 'dX', X.dtype),
        acc_flag, dW1.data_ptr(), db1.data_ptr(), dW2.data_ptr(), db2.data_ptr(),
        workspace.data_ptr(), workspace.numel(), N, P, C, Cp, J, dt, _stream_ptr())
    _check(rc, 'apa_pose_head_bwd')
    return dX, dW1, db1, dW2, db2


# --------------------------------------------------------------------------------------------
# pose-heatmap attention head (cfg.NET.USE_POSE_ATTENTION_LOGITS, nets_factory.py:162-189)
# --------------------------------------------------------------------------------------------
def pose_att_num_maps(sel, avged) -> int:
    """M = the selected parts + the averaged map (if any) + the constant map"""
    return len(sel) + (1 if avged else 0) + 1


def _sel_array(sel):
    arr = (ctypes.c_int32 * max(len(sel), 1))(*[int(j) for j in sel])
    return arr, len(sel)


def pose_att_logits_workspace(N, P, C, M, K, device, workspace=None) -> torch.Tensor:
    need = int(load_library().apa_pose_att_logits_workspace_bytes(N, P, C, M, K))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=device)
    return workspace


def pose_att_logits_fwd(X, Pl, sel, avged, W, b, *, flags=0, keep_prob=1.0, seed=0, offset=0, workspace=None,
                        hooks=None):
    """F [N, M*C] f32, logits [N,K] f32, workspace = pose_att_logits_fwd(X [N,..,C], Pl [N,..,J] f32, sel (host
    list of part indices in [0, J)), avged, W [M*C, K], b [K]) -- apa_pose_att_logits_fwd.  `seed` a KeepMask:
    the replayed mask over F's flat index (APA_FLAG_RNG_EXTERNAL)."""
    lib = load_library()
    N, C, J = X.shape[0], X.shape[-1], Pl.shape[-1]
    P = X.numel() // (N * C)
    M = pose_att_num_maps(sel, avged)
    K = W.shape[-1]
    if W.numel() != M * C * K or Pl.numel() != N * P * J:
        raise ApaError('pose_att_logits_fwd: W must be [M*C = {}, K] and Pl [N*P = {}, J]'.format(M * C, N * P))
    workspace = pose_att_logits_workspace(N, P, C, M, K, X.device, workspace)
    F = torch.empty((N, M * C), dtype=torch.float32, device=X.device)
    logits = torch.empty((N, K), dtype=torch.float32, device=X.device)
    s, o, fl = _rng_key(seed, offset, flags)
    arr, n_sel = _sel_array(sel)
    args = (_dev_ptr(X, 'X'), _dev_ptr(Pl, 'Pl', torch.float32), arr, n_sel, 1 if avged else 0,
            _dev_ptr(W, 'W', torch.float32), _dev_ptr(b, 'b', torch.float32), F.data_ptr(), logits.data_ptr(),
            workspace.data_ptr(), workspace.numel(), N, P, C, J, K, fl, float(keep_prob), s, o, _feat_dtype(X),
            _stream_ptr())
    if hooks is not None:
        rc = lib.apa_pose_att_logits_fwd_ex(_hooks_ptr(hooks), *args)
    else:
        rc = lib.apa_pose_att_logits_fwd(*args)
    _check(rc, 'apa_pose_att_logits_fwd')
    return F, logits, workspace


def pose_att_logits_bwd(X, Pl, sel, avged, W, F, G, dPl, *, dX=None, accumulate_dX=False, flags=0, keep_prob=1.0,
                        seed=0, offset=0, workspace=None, hooks=None):
    """dX, dPl, dW, db = pose_att_logits_bwd(...).  dPl [N,..,J] f32 is ACCUMULATED into (pass the pose-loss
    gradient, or zeros); dX is overwritten, or added to with accumulate_dX (then dX must be given)."""
    lib = load_library()
    N, C, J = X.shape[0], X.shape[-1], Pl.shape[-1]
    P = X.numel() // (N * C)
    M = pose_att_num_maps(sel, avged)
    K = W.shape[-1]
    workspace = pose_att_logits_workspace(N, P, C, M, K, X.device, workspace)
    if dX is None:
        if accumulate_dX:
            raise ApaError('accumulate_dX needs an existing dX buffer')
        dX = torch.empty_like(X)
    dW = torch.empty_like(W)
    db = torch.empty((K,), dtype=torch.float32, device=X.device)
    s, o, fl = _rng_key(seed, offset, flags)
    arr, n_sel = _sel_array(sel)
    args = (_dev_ptr(X, 'X'), _dev_ptr(Pl, 'Pl', torch.float32), arr, n_sel, 1 if avged else 0,
            _dev_ptr(W, 'W', torch.float32), _dev_ptr(F, 'F', torch.float32), _dev_ptr(G, 'G', torch.float32),
            _dev_ptr(dX, 'dX', X.dtype), 1 if accumulate_dX else 0, _dev_ptr(dPl, 'dPl', torch.float32),
            dW.data_ptr(), db.data_ptr(), workspace.data_ptr(), workspace.numel(), N, P, C, J, K, fl,
            float(keep_prob), s, o, _feat_dtype(X), _stream_ptr())
    if hooks is not None:
        rc = lib.apa_pose_att_logits_bwd_ex(_hooks_ptr(hooks), *args)
    else:
        rc = lib.apa_pose_att_logits_bwd(*args)
    _check(rc, 'apa_pose_att_logits_bwd')
    return dX, dPl, dW, db


# --------------------------------------------------------------------------------------------
# losses
# --------------------------------------------------------------------------------------------
def softmax_xent_fwd_bwd(logits, labels, *, wt=1.0, grad_scale=1.0, want_grad=True,
                         want_probs=False, want_pred=False):
    """(loss_buf[1+N], G, probs, pred): src/loss.py:74-80 + eval.py:193-197 fused."""
    lib = load_library()
    N, K = logits.shape
    dev = logits.device
    loss = torch.empty((1 + N,), dtype=torch.float32, device=dev)
    G = torch.empty_like(logits) if want_grad else None
    probs = torch.empty_like(logits) if want_probs else None
    pred = torch.empty((N,), dtype=torch.int64, device=dev) if want_pred else None
    rc = lib.apa_softmax_xent_fwd_bwd(
        _dev_ptr(logits, 'logits', torch.float32), _dev_ptr(labels, 'labels', torch.int64),
        loss.data_ptr(), _dev_ptr(G, 'G'), _dev_ptr(probs, 'probs'), _dev_ptr(pred, 'pred'), N, K,
        float(wt), float(grad_scale), _stream_ptr())
    _check(rc, 'apa_softmax_xent_fwd_bwd')
    return loss, G, probs, pred


def pose_l2_loss_fwd_bwd(Pl, lbl, valid, *, wt=1.0, grad_scale=1.0, want_grad=True):
    """(loss[1], dPl): src/loss.py:29-70.  Pl/lbl [N,P,J] (or [N,H,W,J]) f32, valid [N,J] bool/uint8."""
    lib = load_library()
    N = Pl.shape[0]
    J = Pl.shape[-1]
    P = Pl.numel() // (N * J)
    dev = Pl.device
    # a bool tensor already is one 0/1 byte per element: reinterpret, do not launch a conversion
    v8 = (valid.view(torch.uint8) if valid.dtype == torch.bool else valid.to(torch.uint8)).contiguous()
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    dPl = torch.empty_like(Pl) if want_grad else None
    need = int(lib.apa_pose_l2_workspace_bytes(N, P, J))
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    rc = lib.apa_pose_l2_loss_fwd_bwd(
        _dev_ptr(Pl, 'Pl', torch.float32), _dev_ptr(lbl, 'lbl', torch.float32),
        _dev_ptr(v8, 'valid'), loss.data_ptr(), _dev_ptr(dPl, 'dPl'), ws.data_ptr(), ws.numel(),
        N, P, J, float(wt), float(grad_scale), _stream_ptr())
    _check(rc, 'apa_pose_l2_loss_fwd_bwd')
    return loss, dPl


ACTION_LOSS_KINDS = {'l2': 1, 'multi-label': 2, 'multi-label-2': 3}


def action_loss_fwd_bwd(kind: str, logits, labels, *, wt=1.0, grad_scale=1.0, pos_weight=10.0, want_grad=True):
    """loss [1], G [N,K] for the action losses of src/loss.py:81-101 other than softmax cross-entropy
    ('l2': labels int64 [N]; 'multi-label' / 'multi-label-2': labels f32 [N,K] multi-hot)."""
    lib = load_library()
    N, K = logits.shape
    dev = logits.device
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    G = torch.empty((N, K), dtype=torch.float32, device=dev) if want_grad else None
    ldt = torch.int64 if kind == 'l2' else torch.float32
    rc = lib.apa_action_loss_fwd_bwd(ACTION_LOSS_KINDS[kind], _dev_ptr(logits, 'logits', torch.float32),
                                     _dev_ptr(labels, 'labels', ldt), loss.data_ptr(), _dev_ptr(G, 'G'), N, K,
                                     float(wt), float(grad_scale), float(pos_weight), _stream_ptr())
    _check(rc, 'apa_action_loss_fwd_bwd')
    return loss, G


class ApaMultilabel(ctypes.Structure):
    """`apa_multilabel` of include/apa.h: a sigmoid action loss (src/loss.py:88-101) and its f32 multi-hot labels."""
    _fields_ = [('kind', c_int), ('labels', c_void_p), ('pos_weight', c_float)]


STEP_ACTION_LOSSES = ('softmax-xentropy', 'multi-label', 'multi-label-2')


def _multilabel_labels(who, labels, n_loss, K):
    """The label tensor of a sigmoid action loss: float32 [n_loss, K] multi-hot (checked before anything else)."""
    if labels.dtype != torch.float32 or labels.dim() != 2 or tuple(labels.shape) != (n_loss, K):
        raise ApaError('{}: the multi-label losses take float32 multi-hot labels [{}, {}] (got {} {})'.format(
            who, n_loss, K, labels.dtype, tuple(labels.shape)))
    return labels


def _bind_multilabel(who, action_loss, labels, n_loss, K, pos_weight):
    """-> ApaMultilabel for `action_loss` in STEP_ACTION_LOSSES[1:], or None for the softmax cross-entropy."""
    if action_loss not in STEP_ACTION_LOSSES:
        raise ApaError('{}: action_loss must be one of {} (got {!r})'.format(who, STEP_ACTION_LOSSES, action_loss))
    if action_loss == 'softmax-xentropy':
        return None
    _multilabel_labels(who, labels, n_loss, K)
    ml = ApaMultilabel()
    ml.kind, ml.pos_weight = ACTION_LOSS_KINDS[action_loss], float(pos_weight)
    ml.labels = _dev_ptr(labels, 'labels', torch.float32)
    return ml


def multilabel_loss_fwd_bwd(kind: str, logits, labels, *, wt=1.0, grad_scale=1.0, pos_weight=10.0):
    """loss [1+N], G [N,K]: 'multi-label' / 'multi-label-2' (src/loss.py:88-101) on finished logits f32 [N,K], one
    block per row (include/apa.h: apa_multilabel_loss_fwd_bwd).  labels f32 [N,K] multi-hot; loss[1+n] is the row
    mean, loss[0] the weighted batch mean."""
    lib = load_library()
    N, K = logits.shape
    ml = _bind_multilabel('multilabel_loss_fwd_bwd', kind if kind != 'softmax-xentropy' else '', labels, N, K,
                          pos_weight)
    loss = torch.empty((1 + N,), dtype=torch.float32, device=logits.device)
    G = torch.empty((N, K), dtype=torch.float32, device=logits.device)
    rc = lib.apa_multilabel_loss_fwd_bwd(ctypes.addressof(ml), _dev_ptr(logits, 'logits', torch.float32),
                                         loss.data_ptr(), G.data_ptr(), N, K, float(wt), float(grad_scale),
                                         _stream_ptr())
    _check(rc, 'apa_multilabel_loss_fwd_bwd')
    return loss, G


def pose_sampled_loss_fwd_bwd(Pl, lbl, valid, uniform, *, wt=1.0, grad_scale=1.0, want_grad=True):
    """loss [1], dPl, mask = LOSS_FN_POSE_SAMPLED (src/loss.py:36-52); `uniform` = the caller's
    uniform [0,1) draws, same shape as Pl."""
    lib = load_library()
    N, J = Pl.shape[0], Pl.shape[-1]
    P = Pl.numel() // (N * J)
    dev = Pl.device
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    dPl = torch.empty_like(Pl) if want_grad else None
    mask = torch.empty_like(Pl)
    v8 = valid.to(torch.uint8).contiguous()
    rc = lib.apa_pose_sampled_loss_fwd_bwd(_dev_ptr(Pl, 'Pl', torch.float32), _dev_ptr(lbl, 'lbl', torch.float32),
                                           _dev_ptr(v8, 'valid'), _dev_ptr(uniform, 'uniform', torch.float32),
                                           loss.data_ptr(), _dev_ptr(dPl, 'dPl'), mask.data_ptr(), N, P, J,
                                           float(wt), float(grad_scale), _stream_ptr())
    _check(rc, 'apa_pose_sampled_loss_fwd_bwd')
    return loss, dPl, mask


def resize_bilinear_tf1(img, out_h: int, out_w: int):
    """tf.image.resize_images (TF 1.1 legacy bilinear) of an f32 [N,h,w,C] device tensor."""
    lib = load_library()
    N, h, w, C = img.shape
    out = torch.empty((N, out_h, out_w, C), dtype=torch.float32, device=img.device)
    _check(lib.apa_resize_bilinear_tf1(_dev_ptr(img, 'img', torch.float32), out.data_ptr(), N, h, w, C,
                                       int(out_h), int(out_w), _stream_ptr()), 'apa_resize_bilinear_tf1')
    return out


def attn_explain(X, att, Wt, bt, classes, *, flags=0, workspace=None, hooks=None):
    """Top-down and combined attention maps of T chosen classes per image in one pass over X (include/apa.h:
    apa_attn_explain).  X [N,P,C] (or [N,H,W,C]) f32 / bf16, the map the top-down conv reads; att [N,P,M] f32, M == 1 or
    K, the `att` of an evaluation step; Wt [C,K], bt [K] f32; classes [N] or [N,T] integers on the device (any integer
    type: converted to int32 on the device, no host synchronisation).  flags: APA_FLAG_RELU_INPUT or 0.
    Returns (topdown [N,T,P], combined [N,T,P], class_logit [N,T], status): status is an int32 device scalar, the number
    of class ids outside [0,K), which were clamped.  hooks (make_hooks(prof_fwd=...)): an event pair around the pass
    over X."""
    lib = load_library()
    if X.dim() < 3:
        raise ApaError('attn_explain: X must be [N,P,C] or [N,H,W,C]')
    N, C = X.shape[0], X.shape[-1]
    P = X.numel() // max(N * C, 1)
    if tuple(Wt.shape[:1]) != (C,) or Wt.dim() != 2 or bt.numel() != Wt.shape[1]:
        raise ApaError('attn_explain: Wt [C,K] and bt [K] expected')
    K = Wt.shape[1]
    if att.dim() != 3 or tuple(att.shape[:2]) != (N, P):
        raise ApaError('attn_explain: att must be [N,P,M] (got {})'.format(tuple(att.shape)))
    M = att.shape[2]
    if classes.dim() == 1:
        classes = classes.view(-1, 1)
    if classes.dim() != 2 or classes.shape[0] != N or classes.dtype.is_floating_point:
        raise ApaError('attn_explain: classes must be integers [N] or [N,T]')
    T = classes.shape[1]
    cls = classes.to(torch.int32).contiguous()
    dev = X.device
    dt = _feat_dtype(X)
    topdown = torch.empty((N, T, P), dtype=torch.float32, device=dev)
    combined = torch.empty((N, T, P), dtype=torch.float32, device=dev)
    class_logit = torch.empty((N, T), dtype=torch.float32, device=dev)
    status = torch.zeros((), dtype=torch.int32, device=dev)
    need = int(lib.apa_attn_explain_workspace_bytes(N, P, C, K, T, dt))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    _check(lib.apa_attn_explain(_hooks_ptr(hooks), _dev_ptr(X, 'X'), _dev_ptr(att, 'att', torch.float32), _dev_ptr(Wt, 'Wt', torch.float32),
                                _dev_ptr(bt, 'bt', torch.float32), _dev_ptr(cls, 'classes'), topdown.data_ptr(),
                                combined.data_ptr(), class_logit.data_ptr(), status.data_ptr(),
                                _dev_ptr(workspace, 'workspace'), workspace.numel(), N, P, C, K, M, T, int(flags), dt,
                                _stream_ptr()), 'apa_attn_explain')
    return topdown, combined, class_logit, status


def attention_overlay(maps, images, *, want_f32=False):
    """The reference's overlaid heat-map (src/train.py:184-195) at image size (include/apa.h: apa_attention_overlay):
    maps [N,T,h,w] f32, images [N,H,W,3] f32 (the network's input).  Returns the uint8 overlay [N,T,H,W,3]
    (tf.summary.image's scaling per (n,t) image), and with want_f32 the pair (uint8, float32 overlay)."""
    lib = load_library()
    if maps.dim() != 4 or images.dim() != 4 or images.shape[-1] != 3 or images.shape[0] != maps.shape[0]:
        raise ApaError('attention_overlay: maps [N,T,h,w] and images [N,H,W,3] expected (got {} and {})'.format(
            tuple(maps.shape), tuple(images.shape)))
    N, T, h, w = maps.shape
    H, W = images.shape[1:3]
    dev = maps.device
    u8 = torch.empty((N, T, H, W, 3), dtype=torch.uint8, device=dev)
    f32 = torch.empty((N, T, H, W, 3), dtype=torch.float32, device=dev) if want_f32 else None
    ws = torch.empty((max(int(lib.apa_attention_overlay_workspace_bytes(N, T)), 16),), dtype=torch.uint8, device=dev)
    _check(lib.apa_attention_overlay(_dev_ptr(maps, 'maps', torch.float32), _dev_ptr(images, 'images', torch.float32),
                                     None if f32 is None else f32.data_ptr(), _dev_ptr(u8, 'overlay'), ws.data_ptr(),
                                     ws.numel(), N, T, h, w, H, W, _stream_ptr()), 'apa_attention_overlay')
    return (u8, f32) if want_f32 else u8


# --------------------------------------------------------------------------------------------
# average precision, mAP and accuracy (include/apa.h: apa_average_precision)
# --------------------------------------------------------------------------------------------
def average_precision_workspace_bytes(T: int, K: int) -> int:
    """apa_average_precision_workspace_bytes: 0 for a shape the call refuses (T outside 1..APA_AP_MAX_SAMPLES, K < 1)"""
    return int(load_library().apa_average_precision_workspace_bytes(int(T), int(K)))


def average_precision_result_bytes(K: int) -> int:
    """bytes of the one buffer the four results of average_precision are views of"""
    return 8 * K + 24 + 4 * K + 8


def average_precision(scores, labels=None, targets=None, *, workspace=None, out=None):
    """Per-class average precision, mAP and accuracy of accumulated scores on the device (include/apa.h:
    apa_average_precision, which states the ranking rule): scores [T,K] f32; labels [T] int64 (class k's positives are
    labels == k) or targets [T,K] f32 multi-hot (targets[:,k] > 0), exactly one of the two.  Returns
    (ap [K] float64, npos [K] int32, summary [3] float64 = (mAP, accuracy, classes with positives), status [2] int32 =
    (NaN scores, labels outside [0,K))), all on the device, no synchronisation.  The four are views of ONE uint8 buffer
    (`out`, average_precision_result_bytes(K) bytes: ap, summary, npos, status in that order), so a caller can bring
    them to the host with a single copy of their common storage."""
    lib = load_library()
    if scores.dim() != 2:
        raise ApaError('average_precision: scores [T,K] expected (got {})'.format(tuple(scores.shape)))
    if (labels is None) == (targets is None):
        raise ApaError('average_precision: exactly one of labels [T] / targets [T,K] is given')
    T, K = (int(d) for d in scores.shape)
    if labels is not None and tuple(labels.shape) != (T,):
        raise ApaError('average_precision: labels [T] = [{}] expected (got {})'.format(T, tuple(labels.shape)))
    if targets is not None and tuple(targets.shape) != (T, K):
        raise ApaError('average_precision: targets [T,K] = [{},{}] expected (got {})'.format(T, K, tuple(targets.shape)))
    dev = scores.device
    nbytes = average_precision_result_bytes(K)
    if out is None:
        out = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < nbytes or not out.is_contiguous():
        raise ApaError('average_precision: out must be a contiguous uint8 buffer of average_precision_result_bytes(K) bytes')
    ap = out[:8 * K].view(torch.float64)
    summary = out[8 * K:8 * K + 24].view(torch.float64)
    npos = out[8 * K + 24:12 * K + 24].view(torch.int32)
    status = out[12 * K + 24:12 * K + 32].view(torch.int32)
    need = int(lib.apa_average_precision_workspace_bytes(T, K))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    _check(lib.apa_average_precision(_dev_ptr(scores, 'scores', torch.float32), _dev_ptr(labels, 'labels', torch.int64),
                                     _dev_ptr(targets, 'targets', torch.float32), T, K, _dev_ptr(ap, 'ap'),
                                     npos.data_ptr(), summary.data_ptr(), status.data_ptr(),
                                     _dev_ptr(workspace, 'workspace'), workspace.numel(), _stream_ptr()),
           'apa_average_precision')
    return ap, npos, summary, status


# --------------------------------------------------------------------------------------------
# the reference's own custom ops (src/custom_ops/custom_ops_factory.py:20-47)
# --------------------------------------------------------------------------------------------
def pose_to_heatmap(pose_label, im_ht, im_wd, out_wd, out_channels=16, marker_wd_ratio=0.1,
                    do_gauss_blur=True) -> Tuple[np.ndarray, np.ndarray]:
    """Same call surface as custom_ops_factory.py:20-28 (`pose_to_heatmap(*args, **kwargs)`):
    returns (uint8 heatmap [out_ht,out_wd,out_channels] = float heatmap * 255 truncated,
    bool valid [out_channels]).  Host op, like the reference (DEVICE_CPU)."""
    lib = load_library()
    pose = np.ascontiguousarray(np.asarray(pose_label, dtype=np.int64).reshape(-1))
    out_ht = int(lib.apa_pose_to_heatmap_out_ht(int(im_ht), int(im_wd), int(out_wd)))
    if out_ht < 0:
        raise ApaError('apa_pose_to_heatmap_out_ht: bad image size')
    hm = np.zeros((out_ht, int(out_wd), int(out_channels)), dtype=np.float32)
    valid = np.zeros((int(out_channels),), dtype=np.uint8)
    rc = lib.apa_pose_to_heatmap(
        pose.ctypes.data_as(POINTER(c_int64)), pose.size, int(im_ht), int(im_wd), int(out_wd),
        int(out_channels), float(marker_wd_ratio), 1 if do_gauss_blur else 0,
        hm.ctypes.data_as(POINTER(c_float)), valid.ctypes.data_as(POINTER(c_uint8)))
    _check(rc, 'apa_pose_to_heatmap')
    return (hm * np.float32(255.0)).astype(np.uint8), valid.astype(bool)


def pose_to_heatmap_float(pose_label, im_ht, im_wd, out_wd, out_channels=16, marker_wd_ratio=0.1,
                          do_gauss_blur=True) -> Tuple[np.ndarray, np.ndarray]:
    """The raw op outputs (float heatmap in [0,1], bool valid) before the python wrapper's *255."""
    lib = load_library()
    pose = np.ascontiguousarray(np.asarray(pose_label, dtype=np.int64).reshape(-1))
    out_ht = int(lib.apa_pose_to_heatmap_out_ht(int(im_ht), int(im_wd), int(out_wd)))
    hm = np.zeros((max(out_ht, 0), int(out_wd), int(out_channels)), dtype=np.float32)
    valid = np.zeros((int(out_channels),), dtype=np.uint8)
    rc = lib.apa_pose_to_heatmap(
        pose.ctypes.data_as(POINTER(c_int64)), pose.size, int(im_ht), int(im_wd), int(out_wd),
        int(out_channels), float(marker_wd_ratio), 1 if do_gauss_blur else 0,
        hm.ctypes.data_as(POINTER(c_float)), valid.ctypes.data_as(POINTER(c_uint8)))
    _check(rc, 'apa_pose_to_heatmap')
    return hm, valid.astype(bool)


def spatial_mean_bwd(dz: torch.Tensor, shape, dtype) -> torch.Tensor:
    """dX [N,..,C] (`dtype`) = dz [N,C] / P broadcast over the spatial positions: backward of the global
    average pool of the attention-free head (cfg 001)."""
    lib = load_library()
    N, C = int(shape[0]), int(shape[-1])
    P = 1
    for d in shape[1:-1]:
        P *= int(d)
    dX = torch.empty(tuple(shape), dtype=dtype, device=dz.device)
    rc = lib.apa_spatial_mean_bwd(_dev_ptr(dz, 'dz', torch.float32), dX.data_ptr(), N, P, C, _feat_dtype(dX),
                                  _stream_ptr())
    _check(rc, 'apa_spatial_mean_bwd')
    return dX


def zero_out_channels(to_zero: torch.Tensor, channels: torch.Tensor) -> torch.Tensor:
    """custom_ops_factory.py:30-32 / zero_out_channels.cc: out[...,c] = channels[c] ? in : 0."""
    lib = load_library()
    C = to_zero.shape[-1]
    out = torch.empty_like(to_zero)
    ch = channels.to(torch.uint8).contiguous()
    rc = lib.apa_zero_out_channels(_dev_ptr(to_zero, 'to_zero', torch.float32), _dev_ptr(ch, 'channels'),
                                   out.data_ptr(), to_zero.numel() // C, C, _stream_ptr())
    _check(rc, 'apa_zero_out_channels')
    return out


def pose_label_replay_resize(hm_u8: np.ndarray, orig_hw, crop_info, whether_flip: bool, out_side: int,
                             eps: float = 1e-14) -> np.ndarray:
    """src/preprocess_pipeline.py:21-45 + :195-214 on one heat-map: replay crop
    (crop_info = [y, x, h, w] in the coordinates of the orig_hw = (H, W) image) and flip, /255,
    min-max normalise, legacy-bilinear resize to out_side^2.  Host op.  Returns f32 [S,S,J]."""
    lib = load_library()
    hm = np.ascontiguousarray(hm_u8, dtype=np.uint8)
    h, w, J = hm.shape
    out = np.zeros((out_side, out_side, J), dtype=np.float32)
    rc = lib.apa_pose_label_replay_resize(
        hm.ctypes.data_as(POINTER(c_uint8)), h, w, J, int(orig_hw[0]), int(orig_hw[1]),
        int(crop_info[0]), int(crop_info[1]), int(crop_info[2]), int(crop_info[3]),
        1 if whether_flip else 0, int(out_side), float(eps), out.ctypes.data_as(POINTER(c_float)))
    _check(rc, 'apa_pose_label_replay_resize')
    return out


# --------------------------------------------------------------------------------------------
# frame pooling (nets_factory.py:354-374)
# --------------------------------------------------------------------------------------------
def pose_labels_device(poses, geoms, out_wd=200, J=16, marker_wd_ratio=0.1, out_side=15, device='cuda'):
    """The whole label path of src/preprocess_pipeline.py:150-214 for a batch on the device.
    poses: list of int64 arrays (x, y, vis triples, n_people*J of them); geoms: list of
    (im_ht, im_wd, aug_ht, aug_wd, crop_y, crop_x, crop_h, crop_w, flip) -- im_* = the ORIGINAL image
    size (keypoint scaling, preprocess_pipeline.py:155-157), aug_* = preproc_info['image_shape'], the
    size after the aspect-preserving resize, on which crop_* was recorded (:29-36); a 7-tuple
    (im_ht, im_wd, crop...) means aug == im (no resize).  Returns (labels f32 [N,S,S,J] device,
    valid bool [N,J] device, status int32 [N] device)."""
    lib = load_library()
    N = len(poses)
    flat = [np.asarray(p, dtype=np.int64).reshape(-1) for p in poses]
    max_vals = max(max(f.size for f in flat), 3 * J)
    pose_h = np.full((N, max_vals), -1, dtype=np.int64)
    for i, f in enumerate(flat):
        pose_h[i, :f.size] = f
    dev = torch.device(device)
    pose_d = torch.from_numpy(pose_h).to(dev)
    nv_d = torch.tensor([f.size for f in flat], dtype=torch.int32, device=dev)
    g9 = []
    for g in geoms:
        g = [int(v) for v in g]
        if len(g) == 7:
            g = g[:2] + g[:2] + g[2:]
        if len(g) != 9:
            raise ValueError('geom needs 9 (or 7) integers, got {}'.format(len(g)))
        g9.append(g)
    geom_d = torch.tensor(g9, dtype=torch.int32, device=dev)
    labels = torch.empty((N, out_side, out_side, J), dtype=torch.float32, device=dev)
    valid = torch.empty((N, J), dtype=torch.uint8, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    _check(lib.apa_pose_labels_device(pose_d.data_ptr(), nv_d.data_ptr(), geom_d.data_ptr(), N, max_vals,
                                      int(out_wd), int(J), float(marker_wd_ratio), int(out_side),
                                      labels.data_ptr(), valid.data_ptr(), status.data_ptr(), _stream_ptr()),
           'apa_pose_labels_device')
    return labels, valid.bool(), status


def _geom_rows(geoms):
    g9 = []
    for g in geoms:
        g = [int(v) for v in g]
        if len(g) != 9:
            raise ValueError('geom needs 9 integers, got {}'.format(len(g)))
        g9.append(g)
    return g9


def image_aug_size(src_ht: int, src_wd: int, max_wd: int, resize_side: int) -> Tuple[int, int, int, int]:
    """(lh, lw, ah, aw): the size after `_resize_if_needed` (src/preprocess_pipeline.py:5-18, limit max_wd =
    cfg.MAX_INPUT_IMAGE_SIZE) and after the aspect-preserving resize to resize_side (vgg_preprocessing.py:241-294),
    by the reference's float32 rules.  Host function."""
    out = (ctypes.c_int32 * 4)()
    _check(load_library().apa_image_aug_size(int(src_ht), int(src_wd), int(max_wd), int(resize_side), out),
           'apa_image_aug_size')
    return tuple(int(v) for v in out)


def preprocess_images(frames, geoms, max_wd, out_dtype=torch.float32, device='cuda', mean=128.0, out=None):
    """The image half of the input pipeline for a batch on the device (include/apa.h: apa_preprocess_images):
    limit to max_wd, aspect-preserving resize, crop, flip, - mean, straight into the network's NHWC input.
    frames: list of uint8 arrays [T,h,w,3] (or [h,w,3] when T == 1), any sizes, the same T; geoms: list of
    (im_ht, im_wd, aug_ht, aug_wd, crop_y, crop_x, crop_h, crop_w, flip), the rows pose_labels_device takes, all
    with one crop size.  Returns (images [N,T,crop_h,crop_w,3] `out_dtype` device, status int32 [N] device);
    `out=`: write into this buffer."""
    lib = load_library()
    N = len(frames)
    if N == 0 or len(geoms) != N:
        raise ValueError('preprocess_images: {} samples, {} geometry rows'.format(N, len(geoms)))
    arrs = []
    for f in frames:
        a = np.asarray(f)
        if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
            raise ValueError('frames must be uint8 [T,h,w,3] or [h,w,3], got {} {}'.format(a.dtype, a.shape))
        arrs.append(np.ascontiguousarray(a if a.ndim == 4 else a[None]))
    T = arrs[0].shape[0]
    if any(a.shape[0] != T for a in arrs):
        raise ValueError('every sample of a call needs the same number of frames')
    g9 = _geom_rows(geoms)
    crop_h, crop_w = g9[0][6], g9[0][7]
    if crop_h <= 0 or crop_w <= 0 or any(g[6:8] != [crop_h, crop_w] for g in g9):
        raise ValueError('every sample of a call needs the same positive crop size')
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ApaError('images are produced as float32 or bfloat16, got {}'.format(out_dtype))
    # one packed buffer: sample n starts at byte off[n] (no alignment is asked for)
    off = np.zeros((N,), dtype=np.int64)
    off[1:] = np.cumsum([a.size for a in arrs[:-1]])
    packed = np.concatenate([a.reshape(-1) for a in arrs])
    hw = np.asarray([a.shape[1:3] for a in arrs], dtype=np.int32)
    dev = torch.device(device)
    src_d = torch.from_numpy(packed).to(dev)
    off_d = torch.from_numpy(off).to(dev)
    hw_d = torch.from_numpy(hw).to(dev)
    geom_d = torch.tensor(g9, dtype=torch.int32, device=dev)
    if out is None:
        out = torch.empty((N, T, crop_h, crop_w, 3), dtype=out_dtype, device=dev)
    elif out.dtype != out_dtype or out.numel() != N * T * crop_h * crop_w * 3:
        raise ApaError('preprocess_images: out must be {} with {} elements'.format(out_dtype, N * T * crop_h * crop_w * 3))
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    need = int(lib.apa_preprocess_images_workspace_bytes(N, T, hw.ctypes.data_as(POINTER(ctypes.c_int32)), int(max_wd)))
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    _check(lib.apa_preprocess_images(_dev_ptr(src_d, 'frames'), src_d.numel(), off_d.data_ptr(), hw_d.data_ptr(),
                                     geom_d.data_ptr(), N, T, int(max_wd), float(mean), _dev_ptr(out, 'out'),
                                     _feat_dtype(out), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr()),
           'apa_preprocess_images')
    return out.view(N, T, crop_h, crop_w, 3), status


def frame_pool_fwd(logits, frames_per_video, w=None, b=None):
    """pooled [B,K], tatt [B*F] or None."""
    lib = load_library()
    BF, K = logits.shape
    B = BF // frames_per_video
    pooled = torch.empty((B, K), dtype=torch.float32, device=logits.device)
    tatt = torch.empty((BF,), dtype=torch.float32, device=logits.device) if w is not None else None
    rc = lib.apa_frame_pool_fwd(_dev_ptr(logits, 'logits', torch.float32), _dev_ptr(w, 'w', torch.float32),
                                _dev_ptr(b, 'b', torch.float32), pooled.data_ptr(), _dev_ptr(tatt, 'tatt'),
                                B, frames_per_video, K, _stream_ptr())
    _check(rc, 'apa_frame_pool_fwd')
    return pooled, tatt


def frame_pool_bwd(logits, frames_per_video, w, tatt, dpooled):
    """dlogits [B*F,K], dw [K] or None, db [1] or None."""
    lib = load_library()
    BF, K = logits.shape
    B = BF // frames_per_video
    dlogits = torch.empty_like(logits)
    dw = torch.empty((K,), dtype=torch.float32, device=logits.device) if w is not None else None
    db = torch.empty((1,), dtype=torch.float32, device=logits.device) if w is not None else None
    scratch = torch.empty((BF,), dtype=torch.float32, device=logits.device) if w is not None else None
    rc = lib.apa_frame_pool_bwd(_dev_ptr(logits, 'logits', torch.float32), _dev_ptr(w, 'w', torch.float32),
                                _dev_ptr(tatt, 'tatt'), _dev_ptr(dpooled, 'dpooled', torch.float32),
                                dlogits.data_ptr(), _dev_ptr(dw, 'dw'), _dev_ptr(db, 'db'),
                                _dev_ptr(scratch, 'scratch'), B, frames_per_video, K, _stream_ptr())
    _check(rc, 'apa_frame_pool_bwd')
    return dlogits, dw, db


class ApaClipPool(ctypes.Structure):
    """`apa_clip_pool` of include/apa.h: the frame pooling / temporal attention between the head and the action loss
    of a clip batch (nets_factory.py:354-374)."""
    _fields_ = [('frames', c_int), ('w', c_void_p), ('b', c_void_p), ('pooled', c_void_p), ('tatt', c_void_p),
                ('dw', c_void_p), ('db', c_void_p)]


def clip_xent_workspace_bytes(B, F, K) -> int:
    return int(load_library().apa_clip_xent_workspace_bytes(B, F, K))


def _scores_kind(who: str, kind: str) -> int:
    if kind not in ('softmax', 'sigmoid'):
        raise ApaError("{}: scores must be 'softmax' or 'sigmoid', got {!r}".format(who, kind))
    return APA_SCORES_SIGMOID if kind == 'sigmoid' else APA_SCORES_SOFTMAX


def clip_scores(logits, frames_per_video, w=None, b=None, *, kind='softmax', labels=None):
    """(pooled [B,K], tatt [B*F] or None, scores [B,K], pred int64 [B], loss [1+B] or None): frame pooling (with the
    temporal attention w [K], b [1] when given), then the softmax / sigmoid scores and the first-index argmax of the
    pooled rows -- with int64 `labels` [B] (softmax only) also their cross-entropy -- in one launch (include/apa.h:
    apa_clip_scores).  logits f32 [B*F,K]."""
    lib = load_library()
    BF, K = logits.shape
    F = int(frames_per_video)
    if F <= 0 or BF % F:
        raise ApaError('clip_scores: {} frame rows are not a whole number of clips of {} frames'.format(BF, F))
    B = BF // F
    code = _scores_kind('clip_scores', kind)
    dev, f32 = logits.device, torch.float32
    pooled = torch.empty((B, K), dtype=f32, device=dev)
    tatt = torch.empty((BF,), dtype=f32, device=dev) if w is not None else None
    scores = torch.empty((B, K), dtype=f32, device=dev)
    pred = torch.empty((B,), dtype=torch.int64, device=dev)
    loss = torch.empty((1 + B,), dtype=f32, device=dev) if labels is not None else None
    if labels is not None and labels.numel() != B:
        raise ApaError('clip_scores: labels int64 [B] expected, one per clip')
    rc = lib.apa_clip_scores(code, _dev_ptr(logits, 'logits', f32), _dev_ptr(w, 'w', f32), _dev_ptr(b, 'b', f32),
                             _dev_ptr(labels, 'labels', torch.int64), pooled.data_ptr(), _dev_ptr(tatt, 'tatt'),
                             scores.data_ptr(), pred.data_ptr(), _dev_ptr(loss, 'loss'), B, F, K, _stream_ptr())
    _check(rc, 'apa_clip_scores')
    return pooled, tatt, scores, pred, loss


def _bind_eval_clip(who: str, N: int, K: int, frames, temporal, scores: str, labels, dev):
    """What HeadEvalStep / PoseAttnEvalStep add for clips and / or sigmoid scores: (B, kind code, the ApaClipPool or
    None, pooled, tatt, the tensors to keep alive).  frames == 1 without temporal attention: no clip (the logits rows
    are the pooled rows)."""
    code = _scores_kind(who, scores)
    F = int(frames)
    if F <= 0 or N % F:
        raise ApaError('{}: {} feature maps are not a whole number of clips of {} frames'.format(who, N, F))
    B = N // F
    if code == APA_SCORES_SIGMOID and labels is not None:
        raise ApaError('{}: the sigmoid scores take no labels (eval.py computes no loss)'.format(who))
    if labels is not None and labels.numel() != B:
        raise ApaError('{}: labels int64 [{}] expected, one per clip'.format(who, B))
    if F == 1 and temporal is None:
        return B, code, None, None, None, ()
    clip = ApaClipPool()
    clip.frames = F
    pooled = torch.empty((B, K), dtype=torch.float32, device=dev)
    tatt = None
    clip.pooled = pooled.data_ptr()
    if temporal is not None:
        w, b = temporal
        if w.numel() != K or b.numel() != 1:
            raise ApaError('{}: temporal = (w [K], b [1]) expected'.format(who))
        tatt = torch.empty((N,), dtype=torch.float32, device=dev)
        clip.w, clip.b = _dev_ptr(w, 'temporal w', torch.float32), _dev_ptr(b, 'temporal b', torch.float32)
        clip.tatt = tatt.data_ptr()
    return B, code, clip, pooled, tatt, (temporal,)


def clip_xent_fwd_bwd(logits, labels, frames_per_video, w=None, b=None, *, wt=1.0, grad_scale=1.0, workspace=None):
    """(pooled [B,K], tatt [B*F] or None, loss [1+B], G [B*F,K], dw [K] or None, db [1] or None): frame pooling (with
    the temporal attention w [K], b [1] when given), softmax cross-entropy on the pooled logits and the gradient at the
    frame logits, two launches (include/apa.h: apa_clip_xent_fwd_bwd).  logits f32 [B*F,K], labels int64 [B]."""
    lib = load_library()
    BF, K = logits.shape
    F = int(frames_per_video)
    if F <= 0 or BF % F:
        raise ApaError('clip_xent_fwd_bwd: {} frame rows are not a whole number of clips of {} frames'.format(BF, F))
    B = BF // F
    dev, f32 = logits.device, torch.float32
    att = w is not None
    pooled = torch.empty((B, K), dtype=f32, device=dev)
    tatt = torch.empty((BF,), dtype=f32, device=dev) if att else None
    loss = torch.empty((1 + B,), dtype=f32, device=dev)
    G = torch.empty((BF, K), dtype=f32, device=dev)
    dw = torch.empty((K,), dtype=f32, device=dev) if att else None
    db = torch.empty((1,), dtype=f32, device=dev) if att else None
    need = int(lib.apa_clip_xent_workspace_bytes(B, F, K))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    rc = lib.apa_clip_xent_fwd_bwd(
        _dev_ptr(logits, 'logits', f32), _dev_ptr(labels, 'labels', torch.int64), _dev_ptr(w, 'w', f32),
        _dev_ptr(b, 'b', f32), pooled.data_ptr(), _dev_ptr(tatt, 'tatt'), loss.data_ptr(), G.data_ptr(),
        _dev_ptr(dw, 'dw'), _dev_ptr(db, 'db'), workspace.data_ptr(), workspace.numel(), B, F, K, float(wt),
        float(grad_scale), _stream_ptr())
    _check(rc, 'apa_clip_xent_fwd_bwd')
    return pooled, tatt, loss, G, dw, db


def clip_multilabel_fwd_bwd(kind: str, logits, labels, frames_per_video, w=None, b=None, *, wt=1.0, grad_scale=1.0,
                            pos_weight=10.0, workspace=None):
    """clip_xent_fwd_bwd with a sigmoid loss on the pooled logits (include/apa.h: apa_clip_multilabel_fwd_bwd):
    labels f32 [B,K] multi-hot; the same six results."""
    lib = load_library()
    BF, K = logits.shape
    F = int(frames_per_video)
    if F <= 0 or BF % F:
        raise ApaError('clip_multilabel_fwd_bwd: {} frame rows are not a whole number of clips of {} frames'.format(BF, F))
    B = BF // F
    ml = _bind_multilabel('clip_multilabel_fwd_bwd', kind if kind != 'softmax-xentropy' else '', labels, B, K,
                          pos_weight)
    dev, f32 = logits.device, torch.float32
    att = w is not None
    pooled = torch.empty((B, K), dtype=f32, device=dev)
    tatt = torch.empty((BF,), dtype=f32, device=dev) if att else None
    loss = torch.empty((1 + B,), dtype=f32, device=dev)
    G = torch.empty((BF, K), dtype=f32, device=dev)
    dw = torch.empty((K,), dtype=f32, device=dev) if att else None
    db = torch.empty((1,), dtype=f32, device=dev) if att else None
    need = int(lib.apa_clip_xent_workspace_bytes(B, F, K))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    rc = lib.apa_clip_multilabel_fwd_bwd(
        ctypes.addressof(ml), _dev_ptr(logits, 'logits', f32), _dev_ptr(w, 'w', f32), _dev_ptr(b, 'b', f32),
        pooled.data_ptr(), _dev_ptr(tatt, 'tatt'), loss.data_ptr(), G.data_ptr(), _dev_ptr(dw, 'dw'),
        _dev_ptr(db, 'db'), workspace.data_ptr(), workspace.numel(), B, F, K, float(wt), float(grad_scale),
        _stream_ptr())
    _check(rc, 'apa_clip_multilabel_fwd_bwd')
    return pooled, tatt, loss, G, dw, db


def _bind_clip_pool(who, N, K, frames, temporal, temporal_grads, dev, share_with=None):
    """-> (ApaClipPool, pooled, tatt, keep-alive tuple) for the clip form of a bound step: N = B * frames frame maps,
    `temporal = (w [K], b [1])` the TemporalAttention conv or None, `temporal_grads = (dw [K], db [1])` where its
    gradients go (allocated when not given)."""
    F = int(frames)
    if F <= 0 or N % F:
        raise ApaError('{}: N = {} frame maps are not a whole number of clips of {} frames'.format(who, N, F))
    B, f32 = N // F, torch.float32
    clip = ApaClipPool()
    clip.frames = F
    if share_with is not None:
        pooled, tatt = share_with.pooled, share_with.tatt
    else:
        pooled = torch.empty((B, K), dtype=f32, device=dev)
        tatt = torch.empty((N,), dtype=f32, device=dev) if temporal is not None else None
    clip.pooled = pooled.data_ptr()
    keep = ()
    if temporal is not None:
        w, b = temporal
        if w.numel() != K or b.numel() != 1:
            raise ApaError('{}: temporal = (w [K], b [1]) expected'.format(who))
        if temporal_grads is None:
            temporal_grads = (torch.empty((K,), dtype=f32, device=dev), torch.empty((1,), dtype=f32, device=dev))
        dw, db = temporal_grads
        if dw.numel() != K or db.numel() != 1:
            raise ApaError('{}: temporal_grads = (dw [K], db [1]) expected'.format(who))
        clip.w, clip.b = _dev_ptr(w, 'temporal w', f32), _dev_ptr(b, 'temporal b', f32)
        clip.tatt = tatt.data_ptr()
        clip.dw, clip.db = _dev_ptr(dw, 'temporal dw', f32), _dev_ptr(db, 'temporal db', f32)
        keep = (temporal, temporal_grads)
    return clip, pooled, tatt, keep


class HeadTrainStep:
    """apa_attn_head_train_step bound to caller-owned buffers: forward, softmax cross-entropy and
    backward of the head as ONE foreign call per step (the reference runs the same sequence inside
    one `sess.run(train_op)`, src/train.py:529-566).  All marshalling happens once, here; `run()`
    costs one ctypes call plus the kernel launches, which keeps the host ahead of a ~55 us step.

    Outputs live in the attributes `logits [N,K]`, `att [N,P,M]`, `zsave`, `abar`, `loss [1+N]`,
    `G [N,K]`, and in the gradient buffers passed as `grads = (dX, dXatt, dWa, dba, dWt, dbt)`
    (e.g. views into a flat data-parallel bucket).  `offset`: int, or a 1-element int64 CUDA tensor
    (device-side dropout counter, advanced by the backward pass).  `dxatt_rank1=True` (separate attention
    input, M == 1): grads[1] is dZ, float32 [N*P] (APA_FLAG_DXATT_RANK1) -- the form
    pose_head_bwd(ext_rank1=(dZ, wa)) consumes."""

    def __init__(self, X, Xatt, Wa, ba, Wt, bt, labels, grads, *, flags=0, keep_prob=1.0, seed=0,
                 offset=0, loss_wt=1.0, grad_scale=1.0, workspace=None, hooks=None, dxatt_rank1=False,
                 weight_images=False, share_with=None, frames=1, temporal=None, temporal_grads=None,
                 action_loss='softmax-xentropy', pos_weight=10.0):
        """`action_loss='multi-label' | 'multi-label-2'` (src/loss.py:88-101, `pos_weight` for the former): the sigmoid
        losses through apa_attn_head_train_step_multilabel -- `labels` is then float32 multi-hot [N,K] ([B,K] for
        clips); with the default nothing changes.
        `frames` / `temporal` / `temporal_grads`: a batch of CLIPS (apa_attn_head_train_step_clips): X holds the
        N = B * frames folded frames, `labels` is [B], `temporal = (w [K], b [1])` the TemporalAttention conv (None:
        plain mean over the frames) and `temporal_grads = (dw [K], db [1])` its gradient buffers.  The step then also
        exposes `pooled [B,K]` (the clip logits) and `tatt [N]`; `logits` / `G` are the frame logits and their
        gradient, `loss` is [1+B].  With the defaults nothing changes.
        `grads[0] = None` (frozen features): the step runs with APA_FLAG_FROZEN_INPUT and writes no dX; every other
        output is bit-identical.  If the library refuses the flag for the route (APA_ERR_UNSUPPORTED: the dense
        per-class route, K > 64 -- refused before anything is queued), the first run() allocates a scratch dX
        (`self.dX_scratch`) and from then on runs the full step: the same results at the full cost, never a wrong one.
        `weight_images=True` (per-class maps, M == K): the padded / concatenated operand images of the weights
        are built ONCE in this step's workspace (`self.weight_image_maps` describes them) and every run() passes
        APA_FLAG_WEIGHT_IMAGES: the caller keeps them current -- `BoundMomentumSGD(..., images=...)` /
        `deploy.MomentumSGD.attach_weight_images(step, ...)` in the optimiser's own launch, or
        `refresh_weight_images()` after any other change of the weights.
        `X` a CachedBatch (`FeatureCache.select(index)`, passed as `Xatt` too; `grads[0] = None`): the step reads the
        N images `index` names straight from the resident cache (apa_attn_head_train_step_cached), bit-identical to the
        step on `cache.gather(index)`; `labels=None` reads the cache's own labels through the same index;
        `rebind(index=...)` moves the step to another batch of the cache.  M == 1, or per-class maps (M == K,
        `weight_images` included) on a bf16 cache with K <= 64, C % 256 == 0, C <= 8192 (cached_per_class_served: the
        fused per-class route, whose two kernels that read X have gathered instances).  With `frames` / `temporal` /
        a sigmoid `action_loss` the index names the B * frames frames of B clips (a CachedClips of
        `FeatureCache.sample_clips`; apa_attn_head_train_step_cached_clips), `labels` is per clip / per row and must
        be given (the CachedClips' `labels` / `targets`): bit-identical to the same step on the gathered frames.
        `share_with` (another HeadTrainStep of the same shapes): this step is bound to ITS output tensors, workspace
        and weight images -- a training loop has one set of them; only X / dX differ between the bound steps
        (bench.py's rotating feature-map sets)."""
        self.lib = load_library()
        N, C = X.shape[0], X.shape[-1]
        P = X.numel() // (N * C)
        Ca, M, K = Xatt.shape[-1], Wa.shape[1], Wt.shape[1]
        dev = X.device
        fused = Xatt is X
        if dxatt_rank1:     # cfg 003: `dXatt` receives dZ, f32 [N*P]; dXatt = dZ (x) Wa is left to the consumer
            if fused or M != 1:
                raise ApaError('HeadTrainStep: dxatt_rank1 needs a separate attention input and M == 1')
            if grads[1].dtype != torch.float32 or grads[1].numel() != N * P:
                raise ApaError('HeadTrainStep: dxatt_rank1 wants grads[1] = dZ, float32 [N*P]')
            flags |= APA_FLAG_DXATT_RANK1
        dX, dXatt, dWa, dba, dWt, dbt = grads
        # a FeatureCache read by index (apa_attn_head_train_step_cached): `X` is a CachedBatch; `labels=None` reads the
        # cache's own labels through the same index (labels_cached), else `labels` is [N] as ever
        cb = self._cached = _cached('HeadTrainStep', X, Xatt, frozen=dX is None)
        cached_clips = False        # a CachedBatch with clips and / or a sigmoid loss: the *_cached_clips entry point
        if cb is not None:
            # per-class maps (M == K, weight images included): a bf16 cache on the fused K <= 64 route
            per_class = M != 1 and M == K and cached_per_class_served(cb, K)
            if dxatt_rank1 or ((weight_images or M != 1) and not per_class):
                raise ApaError('HeadTrainStep: a CachedBatch feeds the class-agnostic step, flat or on clips (no '
                               'per-class maps, weight images or dxatt_rank1)')
            if share_with is not None and share_with._cached is None:
                raise ApaError('HeadTrainStep: share_with needs another step on a CachedBatch')
            # clips and / or a sigmoid loss: apa_attn_head_train_step_cached_clips; their labels are per clip / per row
            # (FeatureCache.sample_clips hands them out), never read through the frame index
            cached_clips = int(frames) != 1 or temporal is not None or action_loss != 'softmax-xentropy'
            if cached_clips and labels is None:
                raise ApaError('HeadTrainStep: clips and the multi-label losses on a CachedBatch need labels (per clip '
                               '/ per row: CachedClips.labels / .targets); labels=None reads per-image labels only')
            if labels is None and cb.cache.labels is None:
                raise ApaError('HeadTrainStep: labels=None needs a FeatureCache with labels')
            self._fc = cb.descriptor(labels_cached=labels is None)
            if labels is None:
                labels = cb.cache.labels
        self._fp8 = isinstance(cb.cache.features if cb is not None else X, Fp8Features)
        if self._fp8 and (dX is not None or not fused):
            raise ApaError('HeadTrainStep: an Fp8Features cache is frozen (grads[0] must be None) and supplies its own '
                           'attention input (Xatt must be the same object)')
        self.frozen_input = dX is None
        self.dX_scratch = None
        if self.frozen_input:
            flags |= APA_FLAG_FROZEN_INPUT
        self.hooks = hooks            # default apa_hooks of run(); kept alive here
        clips = int(frames) != 1 or temporal is not None
        n_loss = N
        self._pre = ()
        if clips:
            self._clip, self.pooled, self.tatt, self._clip_keep = _bind_clip_pool(
                'HeadTrainStep', N, K, frames, temporal, temporal_grads, dev, share_with)
            self._pre = (ctypes.addressof(self._clip),)
            n_loss = N // int(frames)
            if action_loss == 'softmax-xentropy' and labels.numel() != n_loss:
                raise ApaError('HeadTrainStep: one label per clip expected ({} clips)'.format(n_loss))
        self._n_loss, self._K = n_loss, K
        self._ml = _bind_multilabel('HeadTrainStep', action_loss, labels, n_loss, K, pos_weight)
        if share_with is not None:
            o = share_with
            if tuple(o.logits.shape) != (N, K) or tuple(o.att.shape) != (N, P, M) or o.loss.numel() != 1 + n_loss:
                raise ApaError('HeadTrainStep: share_with needs a step of the same shapes')
            self.logits, self.att, self.zsave, self.abar, self.loss, self.G = o.logits, o.att, o.zsave, o.abar, o.loss, o.G
            workspace = o.workspace
        else:
            self.logits = torch.empty((N, K), dtype=torch.float32, device=dev)
            self.att = torch.empty((N, P, M), dtype=torch.float32, device=dev)
            self.zsave = torch.empty((N, C) if M == 1 else (N, P, K), dtype=torch.float32, device=dev)
            self.abar = torch.empty((N,), dtype=torch.float32, device=dev) if M == 1 else None
            self.loss = torch.empty((1 + n_loss,), dtype=torch.float32, device=dev)
            self.G = torch.empty((N, K), dtype=torch.float32, device=dev)
        if clips:       # the pooling workspace followed by the clip loss's scratch
            need = int(self.lib.apa_clip_step_workspace_bytes(N, int(frames), P, C, Ca, K, M, flags))
        else:
            need = int(self.lib.apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags))
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.workspace = workspace
        self._keep = (X, Xatt, Wa, ba, Wt, bt, labels, grads, offset, seed)
        self.weight_image_maps = []
        if share_with is not None and share_with.weight_image_maps:
            self.weight_image_maps = share_with.weight_image_maps       # built there, in the shared workspace
            flags |= APA_FLAG_WEIGHT_IMAGES
        elif weight_images and M == K and M > 1:
            self.weight_image_maps = per_class_weight_images(Wa, ba, Wt, bt, workspace, N, P, X.dtype)
            if self.weight_image_maps:
                flags |= APA_FLAG_WEIGHT_IMAGES
        seed, off, flags = _rng_key(seed, offset, flags)     # the pointers below stay valid
        # the int64 `labels` argument: every entry point but apa_attn_head_train_step_multilabel has it (the cached clip
        # step keeps it under a sigmoid loss too, NULL then); dX sits 9 arguments behind it
        has_labels_slot = self._ml is None or cached_clips
        self._dx_idx = 15 if has_labels_slot else 14
        self._args = [
            _dev_ptr(X, 'X'), _dev_ptr(X, 'X') if fused else _dev_ptr(Xatt, 'Xatt', X.dtype),
            _dev_ptr(Wa, 'Wa', torch.float32), _dev_ptr(ba, 'ba', torch.float32),
            _dev_ptr(Wt, 'Wt', torch.float32), _dev_ptr(bt, 'bt', torch.float32),
            *((None if self._ml is not None else _dev_ptr(labels, 'labels', torch.int64),) if has_labels_slot else ()),
            float(loss_wt), float(grad_scale),
            self.logits.data_ptr(), self.att.data_ptr(), self.zsave.data_ptr(), _dev_ptr(self.abar, 'abar'),
            self.loss.data_ptr(), self.G.data_ptr(), _dev_ptr(dX, 'dX', X.dtype),
            None if fused else _dev_ptr(dXatt, 'dXatt', torch.float32 if dxatt_rank1 else X.dtype),
            _dev_ptr(dWa, 'dWa', torch.float32),
            _dev_ptr(dba, 'dba', torch.float32), _dev_ptr(dWt, 'dWt', torch.float32),
            _dev_ptr(dbt, 'dbt', torch.float32), workspace.data_ptr(), workspace.numel(), N, P, C, Ca, K, M,
            flags, float(keep_prob), int(seed), off, _feat_dtype(X)]
        self._fn = self.lib.apa_attn_head_train_step_clips if clips else self.lib.apa_attn_head_train_step_ex
        self._name = 'apa_attn_head_train_step_clips' if clips else 'apa_attn_head_train_step'
        if self._ml is not None:    # (ml, clip or NULL, hooks, then the same arguments without `labels`)
            self._pre = (ctypes.addressof(self._ml), ctypes.addressof(self._clip) if clips else None)
            self._fn, self._name = self.lib.apa_attn_head_train_step_multilabel, 'apa_attn_head_train_step_multilabel'
        if cb is not None:          # (the descriptor, hooks, then the same arguments)
            self._pre = (ctypes.addressof(self._fc),)
            self._fn, self._name = self.lib.apa_attn_head_train_step_cached, 'apa_attn_head_train_step_cached'
        if cached_clips:            # (the descriptor, ml or NULL, clip or NULL, hooks, then the cached
            # step's arguments: the `labels` slot stays, NULL under a sigmoid loss)
            self._pre = (ctypes.addressof(self._fc), None if self._ml is None else ctypes.addressof(self._ml),
                         ctypes.addressof(self._clip) if clips else None)
            self._fn = self.lib.apa_attn_head_train_step_cached_clips
            self._name = 'apa_attn_head_train_step_cached_clips'

    def refresh_weight_images(self) -> None:
        """Rebuild the operand images from the current weights (after load_state_dict, or an optimiser that does not
        rewrite them in its own launch)."""
        if self.weight_image_maps:
            X, _, Wa, ba, Wt, bt = self._keep[:6]
            N, C = X.shape[0], X.shape[-1]
            per_class_weight_images(Wa, ba, Wt, bt, self.workspace, N, X.numel() // (N * C), X.dtype)

    def rebind(self, X=None, labels=None, offset=None, index=None) -> None:
        """Point the bound step at another feature map / label tensor of the SAME shape and dtype (a training loop
        whose backbone hands over a fresh conv5 tensor every step) and / or at another dropout offset (int), without
        re-allocating outputs or workspace.  Fused attention input only (Xatt is X).
        `index` (a step on a CachedBatch): another batch of the same cache -- an int32 tensor of the same length on
        the cache's device (an epoch's views pass uncopied); one marshalled pointer changes.
        Under a captured hipGraph: everything rebind changes travels by value (pointers, the int offset), so a graph
        captured BEFORE the rebind keeps replaying the step as captured -- write new indices / labels / features into
        the bound tensors in place instead, and bind the dropout offset to a device counter (`offset=` a 1-element
        int64 CUDA tensor), which the replays read and advance."""
        keep = list(self._keep)
        if index is not None:
            if self._cached is None:
                raise ApaError('HeadTrainStep.rebind: index= needs a step bound to a CachedBatch')
            self._index = _index_tensor('HeadTrainStep.rebind', index, self._cached.cache.device, self._cached.shape[0])
            self._fc.index = self._index.data_ptr()
        if X is not None:
            if self._cached is not None:
                raise ApaError('HeadTrainStep.rebind: a step on a CachedBatch is re-bound with index=')
            if self._args[0] != self._args[1]:
                raise ApaError('HeadTrainStep.rebind: a separate attention input is bound')
            if X.shape != keep[0].shape or X.dtype != keep[0].dtype:
                raise ApaError('HeadTrainStep.rebind: same shape and dtype expected')
            self._args[0] = self._args[1] = _dev_ptr(X, 'X')
            keep[0] = keep[1] = X
        if labels is not None:
            if self._ml is not None:
                _multilabel_labels('HeadTrainStep.rebind', labels, self._n_loss, self._K)
                self._ml.labels = _dev_ptr(labels, 'labels', torch.float32)
            else:
                if self._cached is not None and self._fc.labels_cached:
                    raise ApaError('HeadTrainStep.rebind: the step reads the cache\'s labels through the index')
                self._args[6] = _dev_ptr(labels, 'labels', torch.int64)
            keep[6] = labels
        if offset is not None:
            if isinstance(keep[8], torch.Tensor):
                raise ApaError('HeadTrainStep.rebind: the step was bound to a device-side dropout counter')
            self._args[-2] = int(offset)
            keep[8] = int(offset)
        self._keep = tuple(keep)

    def run(self, stream: Optional[int] = None, hooks=None) -> None:
        """Enqueue one step on `stream` (a raw hipStream_t) or torch's current stream; `hooks`
        (an ApaHooks) overrides the instance's for this call."""
        h = self.hooks if hooks is None else hooks
        rc = self._fn(*self._pre, _hooks_ptr(h), *self._args, _stream_ptr() if stream is None else stream)
        if rc == APA_ERR_UNSUPPORTED and self.frozen_input and not self._fp8 and self._cached is None:     # no arm on this route: the full step, dX to scratch
            # (an FP8 cache has no full step to fall back to: the refusal is raised below)
            self.frozen_input = False
            self.dX_scratch = torch.empty_like(self._keep[0])
            self._args[self._dx_idx] = self.dX_scratch.data_ptr()
            self._args[-5] &= ~APA_FLAG_FROZEN_INPUT
            rc = self._fn(*self._pre, _hooks_ptr(h), *self._args, _stream_ptr() if stream is None else stream)
        if rc != 0:
            _check(rc, self._name)


class RankHeadTrainStep:
    """apa_attn_head_train_step_rank bound to caller-owned buffers, in the style of HeadTrainStep: forward, softmax
    cross-entropy and backward of a rank-R head (one bottom-up map, R = len(Wts) in 2..APA_RANK_MAX) as ONE foreign
    call per step, bit-identical to attn_pool_rank_fwd, softmax_xent_fwd_bwd and attn_pool_rank_bwd in turn.

    Outputs: `logits [N,K]`, `att [N,P,R]`, `zsave [N,R,C]`, `abar [N,R]`, `z0 [N,P]`, `loss [1+N]`, `G [N,K]`, and
    the gradient buffers `grads = (dX, dXatt, dWa, dba, dWts, dbts, dchain_w, dchain_b)` (lists for the last four;
    e.g. views into a flat data-parallel bucket).  `offset`: int, or a 1-element int64 CUDA tensor (device-side
    dropout counter, advanced by the backward half)."""

    def __init__(self, X, Xatt, Wa, ba, Wts, bts, chain_w, chain_b, labels, grads, *, flags=0, keep_prob=1.0, seed=0,
                 offset=0, loss_wt=1.0, grad_scale=1.0, workspace=None):
        self.lib = load_library()
        N, P, C, Ca, K, M = _rank_dims(X, Xatt, Wa, Wts)
        R, dev, fused = len(Wts), X.device, Xatt is X
        dX, dXatt, dWa, dba, dWts, dbts, dcw, dcb = grads
        self.logits = torch.empty((N, K), dtype=torch.float32, device=dev)
        self.att = torch.empty((N, P, R), dtype=torch.float32, device=dev)
        self.zsave = torch.empty((N, R, C), dtype=torch.float32, device=dev)
        self.abar = torch.empty((N, R), dtype=torch.float32, device=dev)
        self.z0 = torch.empty((N, P), dtype=torch.float32, device=dev)
        self.loss = torch.empty((1 + N,), dtype=torch.float32, device=dev)
        self.G = torch.empty((N, K), dtype=torch.float32, device=dev)
        self._rank = _bind_rank_maps('RankHeadTrainStep', Wts, bts, chain_w, chain_b, self.z0, (dWts, dbts, dcw, dcb))
        self.workspace = _rank_workspace('RankHeadTrainStep', self.lib, workspace, N, P, C, Ca, K, R, dev)
        self._keep = (X, Xatt, Wa, ba, Wts, bts, chain_w, chain_b, labels, grads, offset, seed)
        seed, off, flags = _rng_key(seed, offset, flags)     # the pointers below stay valid
        self._args = [
            ctypes.addressof(self._rank), _dev_ptr(X, 'X'),
            _dev_ptr(X, 'X') if fused else _dev_ptr(Xatt, 'Xatt', X.dtype),
            _dev_ptr(Wa, 'Wa', torch.float32), _dev_ptr(ba, 'ba', torch.float32),
            _dev_ptr(Wts[0], 'Wt', torch.float32), _dev_ptr(bts[0], 'bt', torch.float32),
            _dev_ptr(labels, 'labels', torch.int64), float(loss_wt), float(grad_scale),
            self.logits.data_ptr(), self.att.data_ptr(), self.zsave.data_ptr(), self.abar.data_ptr(),
            self.loss.data_ptr(), self.G.data_ptr(), _dev_ptr(dX, 'dX', X.dtype),
            None if fused else _dev_ptr(dXatt, 'dXatt', X.dtype), _dev_ptr(dWa, 'dWa', torch.float32),
            _dev_ptr(dba, 'dba', torch.float32), _dev_ptr(dWts[0], 'dWt', torch.float32),
            _dev_ptr(dbts[0], 'dbt', torch.float32), self.workspace.data_ptr(), self.workspace.numel(), N, P, C, Ca,
            K, M, flags, float(keep_prob), int(seed), off, _feat_dtype(X)]

    def rebind(self, X=None, labels=None, offset=None) -> None:
        """Another feature map / label tensor of the SAME shape and dtype, and / or another dropout offset (int).
        Fused attention input only (Xatt is X)."""
        keep = list(self._keep)
        if X is not None:
            if self._args[1] != self._args[2]:
                raise ApaError('RankHeadTrainStep.rebind: a separate attention input is bound')
            if X.shape != keep[0].shape or X.dtype != keep[0].dtype:
                raise ApaError('RankHeadTrainStep.rebind: same shape and dtype expected')
            self._args[1] = self._args[2] = _dev_ptr(X, 'X')
            keep[0] = keep[1] = X
        if labels is not None:
            self._args[7] = _dev_ptr(labels, 'labels', torch.int64)
            keep[8] = labels
        if offset is not None:
            if isinstance(keep[10], torch.Tensor):
                raise ApaError('RankHeadTrainStep.rebind: the step was bound to a device-side dropout counter')
            self._args[-2] = int(offset)
            keep[10] = int(offset)
        self._keep = tuple(keep)

    def run(self, stream: Optional[int] = None) -> None:
        rc = self.lib.apa_attn_head_train_step_rank(*self._args, _stream_ptr() if stream is None else stream)
        if rc != 0:
            _check(rc, 'apa_attn_head_train_step_rank')


class ApaPoseAttnStepIO(ctypes.Structure):
    """`apa_pose_attn_step_io` of include/apa.h (field order is the ABI)."""
    _fields_ = ([(n, c_void_p) for n in ('X', 'W1', 'b1', 'W2', 'b2', 'W1_bf16', 'W2T_bf16', 'Wa', 'ba', 'Wt', 'bt', 'labels',
                                          'pose_labels', 'pose_valid')] +
                [('action_wt', c_float), ('pose_wt', c_float), ('grad_scale', c_float)] +
                [(n, c_void_p) for n in ('Ppre', 'Pl', 'att', 'logits', 'zsave', 'abar', 'loss_action', 'loss_pose',
                                          'G', 'dPl', 'dZ', 'dX', 'dW1', 'db1', 'dW2', 'db2', 'dWa', 'dba', 'dWt',
                                          'dbt')] +
                [('ws_pool', c_void_p), ('ws_pool_bytes', c_size_t), ('ws_pose', c_void_p),
                 ('ws_pose_bytes', c_size_t)])


class PoseAttnTrainStep:
    """apa_pose_attn_train_step bound to caller-owned buffers: the whole cfg 003 head step (PoseLogits head ->
    attention from pose_pre_logits -> dropout + pooling -> pose L2 + softmax cross-entropy -> every gradient) as ONE
    foreign call, like the reference's one sess.run per step (src/train.py:529-566).

    `params = (W1, b1, W2, b2, Wa, ba, Wt, bt)` fp32; `grads = (dX, dW1, db1, dW2, db2, dWa, dba, dWt, dbt)`;
    `w1_bf16`: optional bf16 copy of W1 the caller keeps current (BoundMomentumSGD(..., shadows=...)).
    Outputs as attributes: Ppre, Pl, att, logits, zsave, abar, loss_action [1+N], loss_pose [1], G, dPl, dZ."""

    def __init__(self, X, params, labels, pose_labels, pose_valid, grads, *, flags=0, keep_prob=1.0, seed=0,
                 offset=0, action_wt=1.0, pose_wt=1.0, grad_scale=1.0, w1_bf16=None, share_with=None,
                 w2t_bf16=None, frames=1, temporal=None, temporal_grads=None, action_loss='softmax-xentropy',
                 pos_weight=10.0):
        """`action_loss` / `pos_weight`: as for HeadTrainStep (apa_pose_attn_train_step_multilabel; labels float32
        [n_loss, K]); the pose L2 loss stays.
        `frames` / `temporal` / `temporal_grads`: a batch of clips (apa_pose_attn_train_step_clips), as for
        HeadTrainStep: `labels` [B], `loss_action` [1+B], `pooled` [B,K], `tatt` [N]; pose labels stay per frame.
        `share_with`: another PoseAttnTrainStep of the same shapes whose activation / loss buffers and workspaces
        this step is bound to as well (see HeadTrainStep).  `w2t_bf16`: optional bf16 [16, Cp + 16] image of W2^T (rows
        J.. and the pad columns zero) the caller keeps current -- `pose_w2t_image(W2)` builds it, `pose_w2t_image_map(image, W2)` describes
        it for `BoundMomentumSGD(..., images=...)`.
        `grads[0] = None` (frozen features): APA_FLAG_FROZEN_INPUT -- the pooling pass stores no dX and the pose
        head's dX product is not launched; every other output is bit-identical.  Should the library refuse the flag
        (APA_ERR_UNSUPPORTED), run() allocates a scratch dX and runs the full step, as HeadTrainStep does."""
        self.lib = load_library()
        W1, b1, W2, b2, Wa, ba, Wt, bt = params
        dX, dW1, db1, dW2, db2, dWa, dba, dWt, dbt = grads
        self.frozen_input = dX is None
        self.dX_scratch = None
        if self.frozen_input:
            flags |= APA_FLAG_FROZEN_INPUT
        N, C = X.shape[0], X.shape[-1]
        P = X.numel() // (N * C)
        Cp, J, K = W1.shape[1], W2.shape[1], Wt.shape[1]
        dev, f32 = X.device, torch.float32
        if tuple(W1.shape) != (C, Cp) or Wa.numel() != Cp or tuple(Wt.shape) != (C, K):
            raise ApaError('PoseAttnTrainStep: W1 [C,Cp], Wa [Cp,1], Wt [C,K] expected')
        if pose_valid.dtype == torch.bool:
            pose_valid = pose_valid.to(torch.uint8)
        new = lambda *shape, dt=f32: torch.empty(shape, dtype=dt, device=dev)
        clips = int(frames) != 1 or temporal is not None
        n_loss = N
        self._pre = ()
        if clips:
            self._clip, self.pooled, self.tatt, self._clip_keep = _bind_clip_pool(
                'PoseAttnTrainStep', N, K, frames, temporal, temporal_grads, dev, share_with)
            self._pre = (ctypes.addressof(self._clip),)
            n_loss = N // int(frames)
        self._n_loss, self._K = n_loss, K
        self._ml = _bind_multilabel('PoseAttnTrainStep', action_loss, labels, n_loss, K, pos_weight)
        _shared = ('Ppre', 'Pl', 'att', 'logits', 'zsave', 'abar', 'loss_action', 'loss_pose', 'G', 'dPl', 'dZ')
        if share_with is not None:
            if tuple(share_with.Ppre.shape) != (N, P, Cp) or share_with.Ppre.dtype != X.dtype or \
                    tuple(share_with.logits.shape) != (N, K) or share_with.loss_action.numel() != 1 + n_loss:
                raise ApaError('PoseAttnTrainStep: share_with needs a step of the same shapes')
            for name in _shared:
                setattr(self, name, getattr(share_with, name))
        else:
            self.Ppre, self.Pl, self.att = new(N, P, Cp, dt=X.dtype), new(N, P, J), new(N, P, 1)
            self.logits, self.zsave, self.abar = new(N, K), new(N, C), new(N)
            self.loss_action, self.loss_pose = new(1 + n_loss), new(1)
            self.G, self.dPl, self.dZ = new(N, K), new(N, P, J), new(N * P)
        dt = _feat_dtype(X)
        seed, off, flags = _rng_key(seed, offset, flags)
        if flags & APA_FLAG_RNG_EXTERNAL:
            raise ApaError('PoseAttnTrainStep: an external keep mask is served by the per-op entry points')
        if share_with is not None:
            self.ws_pool, self.ws_pose = share_with.ws_pool, share_with.ws_pose
        else:
            if clips:   # the pooling workspace followed by the clip loss's scratch
                pool_bytes = int(self.lib.apa_clip_step_workspace_bytes(N, int(frames), P, C, Cp, K, 1, flags))
            else:
                pool_bytes = int(self.lib.apa_attn_pool_workspace_bytes(N, P, C, Cp, K, 1, flags))
            self.ws_pool = torch.empty((max(pool_bytes, 16),), dtype=torch.uint8, device=dev)
            self.ws_pose = torch.empty((max(int(self.lib.apa_pose_head_workspace_bytes(N, P, C, Cp, J, dt)), 16),),
                                       dtype=torch.uint8, device=dev)
        self._keep = (X, params, labels, pose_labels, pose_valid, grads, offset, w1_bf16, w2t_bf16)
        io = ApaPoseAttnStepIO()
        io.X = _dev_ptr(X, 'X')
        for name, t in (('W1', W1), ('b1', b1), ('W2', W2), ('b2', b2), ('Wa', Wa), ('ba', ba), ('Wt', Wt), ('bt', bt),
                        ('pose_labels', pose_labels), ('dW1', dW1), ('db1', db1), ('dW2', dW2), ('db2', db2),
                        ('dWa', dWa), ('dba', dba), ('dWt', dWt), ('dbt', dbt)):
            setattr(io, name, _dev_ptr(t, name, f32))
        io.W1_bf16 = None if w1_bf16 is None else _dev_ptr(w1_bf16, 'w1_bf16', torch.bfloat16)
        io.W2T_bf16 = None
        if w2t_bf16 is not None:
            if tuple(w2t_bf16.shape) != (16, Cp + 16) or J > 16 or not w2t_bf16.is_contiguous():
                raise ApaError('PoseAttnTrainStep: w2t_bf16 is a contiguous bf16 [16, Cp + 16] image of W2^T (J <= 16; '
                               'pose_w2t_image)')
            io.W2T_bf16 = _dev_ptr(w2t_bf16, 'w2t_bf16', torch.bfloat16)
        if w1_bf16 is not None and w1_bf16.numel() != W1.numel():
            raise ApaError('PoseAttnTrainStep: w1_bf16 must have W1\'s element count')
        io.labels = None if self._ml is not None else _dev_ptr(labels, 'labels', torch.int64)
        io.pose_valid = _dev_ptr(pose_valid, 'pose_valid', torch.uint8)
        if pose_labels.numel() != N * P * J or pose_valid.numel() != N * J or \
                (self._ml is None and labels.numel() != n_loss):
            raise ApaError('PoseAttnTrainStep: labels [N] (one per clip for a clip batch), pose_labels [N,P,J], '
                           'pose_valid [N,J] expected')
        io.action_wt, io.pose_wt, io.grad_scale = float(action_wt), float(pose_wt), float(grad_scale)
        io.dX = _dev_ptr(dX, 'dX', X.dtype)
        for name in ('Ppre', 'Pl', 'att', 'logits', 'zsave', 'abar', 'loss_action', 'loss_pose', 'G', 'dPl', 'dZ'):
            setattr(io, name, getattr(self, name).data_ptr())
        io.ws_pool, io.ws_pool_bytes = self.ws_pool.data_ptr(), self.ws_pool.numel()
        io.ws_pose, io.ws_pose_bytes = self.ws_pose.data_ptr(), self.ws_pose.numel()
        self._io = io
        self._args = [ctypes.addressof(io), N, P, C, Cp, J, K, flags, float(keep_prob), int(seed), off, dt]
        self._fn = self.lib.apa_pose_attn_train_step_clips if clips else self.lib.apa_pose_attn_train_step
        self._name = 'apa_pose_attn_train_step_clips' if clips else 'apa_pose_attn_train_step'
        if self._ml is not None:    # (ml, clip or NULL, then the same arguments)
            self._pre = (ctypes.addressof(self._ml), ctypes.addressof(self._clip) if clips else None)
            self._fn, self._name = self.lib.apa_pose_attn_train_step_multilabel, 'apa_pose_attn_train_step_multilabel'

    def rebind(self, X=None, labels=None, pose_labels=None, pose_valid=None, offset=None) -> None:
        """Point the bound step at other inputs of the same shapes / dtypes and / or another dropout offset (int)
        without re-allocating outputs or workspaces (see HeadTrainStep.rebind)."""
        keep = list(self._keep)
        io = self._io
        if X is not None:
            if X.shape != keep[0].shape or X.dtype != keep[0].dtype:
                raise ApaError('PoseAttnTrainStep.rebind: same shape and dtype expected')
            io.X = _dev_ptr(X, 'X')
            keep[0] = X
        if labels is not None:
            if self._ml is not None:
                _multilabel_labels('PoseAttnTrainStep.rebind', labels, self._n_loss, self._K)
                self._ml.labels = _dev_ptr(labels, 'labels', torch.float32)
            else:
                io.labels = _dev_ptr(labels, 'labels', torch.int64)
            keep[2] = labels
        if pose_labels is not None:
            if pose_labels.numel() != keep[3].numel():
                raise ApaError('PoseAttnTrainStep.rebind: pose_labels [N,P,J] expected')
            io.pose_labels = _dev_ptr(pose_labels, 'pose_labels', torch.float32)
            keep[3] = pose_labels
        if pose_valid is not None:
            if pose_valid.dtype == torch.bool:
                pose_valid = pose_valid.to(torch.uint8)
            io.pose_valid = _dev_ptr(pose_valid, 'pose_valid', torch.uint8)
            keep[4] = pose_valid
        if offset is not None:
            if isinstance(keep[6], torch.Tensor):
                raise ApaError('PoseAttnTrainStep.rebind: the step was bound to a device-side dropout counter')
            self._args[10] = int(offset)
            keep[6] = int(offset)
        self._keep = tuple(keep)

    def run(self, stream: Optional[int] = None) -> None:
        rc = self._fn(*self._pre, *self._args, _stream_ptr() if stream is None else stream)
        if rc == APA_ERR_UNSUPPORTED and self.frozen_input:     # the full step, dX to scratch
            self.frozen_input = False
            self.dX_scratch = torch.empty_like(self._keep[0])
            self._io.dX = self.dX_scratch.data_ptr()
            self._args[7] &= ~APA_FLAG_FROZEN_INPUT
            rc = self._fn(*self._pre, *self._args, _stream_ptr() if stream is None else stream)
        if rc != 0:
            _check(rc, self._name)


class HeadEvalStep:
    """apa_attn_head_eval_step bound to caller-owned inputs: forward + softmax probabilities + argmax
    (+ per-example loss when `labels` is given) as ONE foreign call (eval.py:181-197).  Outputs:
    `logits`, `att`, `probs` [N,K], `pred` [N] int64, `loss` [1+N] or None.

    `frames` > 1 (the N maps are the folded frames of B = N / frames clips), `temporal = (w [K], b [1])` (the
    TemporalAttention conv) and / or `scores='sigmoid'` (the multi-label datasets, no labels): the step is
    apa_attn_head_eval_step_clips -- `logits` stays the [N,K] frame logits, `pooled` [B,K] and `tatt` [N] (None without
    them) are further outputs, and `probs`, `pred`, `labels`, `loss` are per clip (B in place of N).  With the defaults
    nothing changes.

    `X` a CachedBatch (`FeatureCache.select(index)`, passed as `Xatt` too): apa_attn_head_eval_step_cached on the images
    `index` names (softmax or sigmoid scores); `labels=None` with softmax scores on a flat batch reads the cache's own
    labels, if it has any, through the index; `rebind(index=...)` moves the step to another batch of the cache
    (M == 1, or per-class maps where cached_per_class_served says so).  With
    `frames` > 1 or `temporal` the index names the frames of B clips (a CachedClips of `FeatureCache.sample_clips`;
    apa_attn_head_eval_step_cached_clips) and `labels`, if given, is per clip; `labels=None` computes no loss there --
    the cache's per-image labels are not read for a clip, `temporal` on single frames (`frames=1`) included."""

    def __init__(self, X, Xatt, Wa, ba, Wt, bt, labels=None, *, flags=0, workspace=None, frames=1, temporal=None,
                 scores='softmax'):
        self.lib = load_library()
        N, C = X.shape[0], X.shape[-1]
        P = X.numel() // (N * C)
        Ca, M, K = Xatt.shape[-1], Wa.shape[1], Wt.shape[1]
        dev = X.device
        flags &= ~APA_FLAG_TRAIN
        # a FeatureCache read by index (apa_attn_head_eval_step_cached): `X` is a CachedBatch; `labels=None` with
        # softmax scores reads the cache's own labels, if it has any, through the same index (labels_cached)
        cb = self._cached = _cached('HeadEvalStep', X, Xatt)
        if cb is not None:
            if M != 1 and not (M == K and cached_per_class_served(cb, K)):    # (those: a bf16 cache, the fused route)
                raise ApaError('HeadEvalStep: a CachedBatch feeds the class-agnostic step (no per-class maps)')
            # exactly when _bind_eval_clip below builds a clip (temporal attention on single frames is one too): its
            # labels are per clip, never read through the frame index -- labels=None then means no loss
            cached_clips = int(frames) != 1 or temporal is not None
            use_cached = labels is None and cb.cache.labels is not None and scores == 'softmax' and not cached_clips
            self._fc = cb.descriptor(labels_cached=use_cached)
        B, code, self._clip, self.pooled, self.tatt, keep = _bind_eval_clip('HeadEvalStep', N, K, frames, temporal,
                                                                          scores, labels, dev)
        if cb is not None and use_cached:
            labels = cb.cache.labels
        self.logits = torch.empty((N, K), dtype=torch.float32, device=dev)
        self.att = torch.empty((N, P, M), dtype=torch.float32, device=dev)
        self.zsave = torch.empty((N, C) if M == 1 else (N, P, K), dtype=torch.float32, device=dev)
        self.abar = torch.empty((N,), dtype=torch.float32, device=dev) if M == 1 else None
        self.probs = torch.empty((B, K), dtype=torch.float32, device=dev)
        self.pred = torch.empty((B,), dtype=torch.int64, device=dev)
        self.loss = torch.empty((1 + B,), dtype=torch.float32, device=dev) if labels is not None else None
        need = int(self.lib.apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags))
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.workspace = workspace
        self._keep = (X, Xatt, Wa, ba, Wt, bt, labels)
        self._args = [
            _dev_ptr(X, 'X'), _dev_ptr(X, 'X') if Xatt is X else _dev_ptr(Xatt, 'Xatt', X.dtype),
            _dev_ptr(Wa, 'Wa', torch.float32), _dev_ptr(ba, 'ba', torch.float32),
            _dev_ptr(Wt, 'Wt', torch.float32), _dev_ptr(bt, 'bt', torch.float32),
            _dev_ptr(labels, 'labels', torch.int64), self.logits.data_ptr(), self.att.data_ptr(),
            self.zsave.data_ptr(), _dev_ptr(self.abar, 'abar'), _dev_ptr(self.loss, 'loss'),
            self.probs.data_ptr(), self.pred.data_ptr(), workspace.data_ptr(), workspace.numel(),
            N, P, C, Ca, K, M, flags, _feat_dtype(X)]
        self._fn, self._name, self._pre = self.lib.apa_attn_head_eval_step, 'apa_attn_head_eval_step', ()
        if self._clip is not None or code != APA_SCORES_SOFTMAX:    # (clip or NULL, the kind, then the same arguments)
            self._keep += keep
            self._fn, self._name = self.lib.apa_attn_head_eval_step_clips, 'apa_attn_head_eval_step_clips'
            self._pre = (None if self._clip is None else ctypes.addressof(self._clip), code)
        if cb is not None:      # (the descriptor, clip = NULL, the kind, then the same arguments)
            self._fn, self._name = self.lib.apa_attn_head_eval_step_cached, 'apa_attn_head_eval_step_cached'
            self._pre = (ctypes.addressof(self._fc), None, code)
            if self._clip is not None:      # (the descriptor, the clip, the kind, then the same arguments)
                self._fn = self.lib.apa_attn_head_eval_step_cached_clips
                self._name = 'apa_attn_head_eval_step_cached_clips'
                self._pre = (ctypes.addressof(self._fc), ctypes.addressof(self._clip), code)

    def rebind(self, X=None, index=None, labels=None) -> None:
        """Point the bound step at another feature map of the same shape / dtype (attention from the map itself:
        the step was built with `Xatt is X`).  `index` (a step on a CachedBatch): another batch of the same cache, an
        int32 tensor of the same length on the cache's device.  `labels`: another int64 label tensor of the same
        length, for a step that was built with labels of its own."""
        if labels is not None:
            if self._keep[6] is None or (self._cached is not None and self._fc.labels_cached):
                raise ApaError('HeadEvalStep.rebind: the step was built without labels of its own')
            if labels.numel() != self._keep[6].numel():
                raise ApaError('HeadEvalStep.rebind: labels int64 [{}] expected'.format(self._keep[6].numel()))
            self._args[6] = _dev_ptr(labels, 'labels', torch.int64)
            self._keep = self._keep[:6] + (labels,) + tuple(self._keep[7:])
        if index is not None:
            if self._cached is None:
                raise ApaError('HeadEvalStep.rebind: index= needs a step bound to a CachedBatch')
            self._index = _index_tensor('HeadEvalStep.rebind', index, self._cached.cache.device, self._cached.shape[0])
            self._fc.index = self._index.data_ptr()
        if X is None:
            return
        if self._cached is not None:
            raise ApaError('HeadEvalStep.rebind: a step on a CachedBatch is re-bound with index=')
        if self._keep[1] is not self._keep[0]:
            raise ApaError('HeadEvalStep.rebind: a step with a separate attention input is re-built, not re-bound')
        if X.shape != self._keep[0].shape or X.dtype != self._keep[0].dtype:
            raise ApaError('HeadEvalStep.rebind: same shape and dtype expected')
        self._args[0] = self._args[1] = _dev_ptr(X, 'X')
        self._keep = (X, X) + tuple(self._keep[2:])

    def run(self, stream: Optional[int] = None) -> None:
        rc = self._fn(*self._pre, *self._args, _stream_ptr() if stream is None else stream)
        if rc != 0:
            _check(rc, self._name)


class ApaPoseAttnEvalIO(ctypes.Structure):
    """`apa_pose_attn_eval_io` of include/apa.h (field order is the ABI)."""
    _fields_ = ([(n, c_void_p) for n in ('X', 'W1', 'b1', 'W1_bf16', 'W2', 'b2', 'Wa', 'ba', 'Wt', 'bt', 'labels',
                                          'att', 'logits', 'zsave', 'abar', 'probs', 'pred', 'loss', 'Pl')] +
                [('ws', c_void_p), ('ws_bytes', c_size_t), ('route', POINTER(c_int))])


class PoseAttnEvalStep:
    """apa_pose_attn_eval_step bound to caller-owned inputs: the cfg 003 head at evaluation time (PoseLogits head ->
    attention from pose_pre_logits -> pooling -> softmax probabilities + argmax, eval.py:181-197) as ONE foreign call.

    `params = (W1, b1, W2, b2, Wa, ba, Wt, bt)` fp32; `w1_bf16`: optional bf16 copy of W1 the caller keeps current.
    Outputs as attributes: `att` [N,P,1], `logits`, `zsave`, `abar`, `probs` [N,K], `pred` [N] int64, `loss` [1+N] or
    None, `Pl` [N,P,J] or None (`want_pose_logits=True`).  `route` (after `run()`): 1 = the pose-head product's
    epilogue formed the attention logits and pose_pre_logits was never written; 0 = the composed route.
    `frames`, `temporal`, `scores`: as for HeadEvalStep (apa_pose_attn_eval_step_clips; both routes are kept)."""

    def __init__(self, X, params, labels=None, *, flags=0, w1_bf16=None, want_pose_logits=False, workspace=None,
                 frames=1, temporal=None, scores='softmax'):
        self.lib = load_library()
        W1, b1, W2, b2, Wa, ba, Wt, bt = params
        N, C = X.shape[0], X.shape[-1]
        P = X.numel() // (N * C)
        Cp, J, K = W1.shape[1], W2.shape[1], Wt.shape[1]
        dev, f32 = X.device, torch.float32
        B, code, self._clip, self.pooled, self.tatt, keep = _bind_eval_clip('PoseAttnEvalStep', N, K, frames, temporal,
                                                                          scores, labels, dev)
        if tuple(W1.shape) != (C, Cp) or Wa.numel() != Cp or tuple(Wt.shape) != (C, K) or W2.shape[0] != Cp:
            raise ApaError('PoseAttnEvalStep: W1 [C,Cp], W2 [Cp,J], Wa [Cp,1], Wt [C,K] expected')
        if w1_bf16 is not None and w1_bf16.numel() != W1.numel():
            raise ApaError('PoseAttnEvalStep: w1_bf16 must have W1\'s element count')
        flags &= APA_FLAG_SOFTMAX_ATT | APA_FLAG_RELU_ATT
        dt = _feat_dtype(X)
        new = lambda *shape, dt=f32: torch.empty(shape, dtype=dt, device=dev)
        self.att, self.logits, self.zsave, self.abar = new(N, P, 1), new(N, K), new(N, C), new(N)
        self.probs, self.pred = new(B, K), new(B, dt=torch.int64)
        self.loss = new(1 + B) if labels is not None else None
        self.Pl = new(N, P, J) if want_pose_logits else None
        need = int(self.lib.apa_pose_attn_eval_workspace_bytes(N, P, C, Cp, J, K, flags, dt, int(bool(want_pose_logits))))
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.workspace = workspace
        self._keep = (X, params, labels, w1_bf16)
        self._route = c_int(-1)
        io = ApaPoseAttnEvalIO()
        io.X = _dev_ptr(X, 'X')
        for name, t in (('W1', W1), ('b1', b1), ('W2', W2), ('b2', b2), ('Wa', Wa), ('ba', ba), ('Wt', Wt), ('bt', bt)):
            setattr(io, name, _dev_ptr(t, name, f32))
        io.W1_bf16 = None if w1_bf16 is None else _dev_ptr(w1_bf16, 'w1_bf16', torch.bfloat16)
        io.labels = _dev_ptr(labels, 'labels', torch.int64)
        for name in ('att', 'logits', 'zsave', 'abar', 'probs', 'pred', 'loss', 'Pl'):
            t = getattr(self, name)
            setattr(io, name, None if t is None else t.data_ptr())
        io.ws, io.ws_bytes = workspace.data_ptr(), workspace.numel()
        io.route = ctypes.pointer(self._route)
        self._io = io
        self._args = [ctypes.addressof(io), N, P, C, Cp, J, K, flags, dt]
        self._fn, self._name = self.lib.apa_pose_attn_eval_step, 'apa_pose_attn_eval_step'
        if self._clip is not None or code != APA_SCORES_SOFTMAX:    # (clip or NULL, the kind, then the same arguments)
            self._keep += keep
            self._fn, self._name = self.lib.apa_pose_attn_eval_step_clips, 'apa_pose_attn_eval_step_clips'
            self._args = [None if self._clip is None else ctypes.addressof(self._clip), code] + self._args

    @property
    def route(self) -> Optional[int]:
        """which route the last `run()` took (None before the first one)"""
        return None if self._route.value < 0 else int(self._route.value)

    def rebind(self, X=None, labels=None) -> None:
        """Point the bound step at other inputs of the same shapes / dtypes."""
        keep = list(self._keep)
        if X is not None:
            if X.shape != keep[0].shape or X.dtype != keep[0].dtype:
                raise ApaError('PoseAttnEvalStep.rebind: same shape and dtype expected')
            self._io.X = _dev_ptr(X, 'X')
            keep[0] = X
        if labels is not None:
            if keep[2] is None or labels.numel() != keep[2].numel():
                raise ApaError('PoseAttnEvalStep.rebind: the step was bound without labels (or to another batch size)')
            self._io.labels = _dev_ptr(labels, 'labels', torch.int64)
            keep[2] = labels
        self._keep = tuple(keep)

    def run(self, stream: Optional[int] = None) -> None:
        rc = self._fn(*self._args, _stream_ptr() if stream is None else stream)
        if rc != 0:
            _check(rc, self._name)


class ApaWeightImage(ctypes.Structure):
    """`apa_weight_image` of include/apa.h (field order is the ABI): where the optimiser's launch stores the updated
    element (c, k) of one head parameter inside a per-class workspace."""
    _fields_ = [('dst', c_void_p), ('role', c_int), ('is_f32', c_int), ('cols', c_int), ('c_shift', c_int),
                ('a', c_int), ('b', c_int), ('d', c_int), ('e', c_int)]


def per_class_weight_images(Wa, ba, Wt, bt, workspace, N, P, dtype):
    """apa_per_class_weight_images: build, inside `workspace`, every padded / concatenated operand image the
    per-class head (M == K) would otherwise rebuild in each call, and return their descriptions
    [(role 'Wa'|'ba'|'Wt'|'bt', ApaWeightImage), ...] for `BoundMomentumSGD(..., images=...)`.  Calls that then
    pass APA_FLAG_WEIGHT_IMAGES with this workspace skip the per-step weight preparation.  `dtype`: the FEATURE
    dtype the images are for (torch.bfloat16 / torch.float32)."""
    lib = load_library()
    Ca, K = Wa.shape
    C = Wt.shape[0]
    if tuple(Wt.shape) != (C, K) or ba.numel() != K or bt.numel() != K:
        raise ApaError('per_class_weight_images: Wa [Ca,K], ba [K], Wt [C,K], bt [K] expected (M == K)')
    maps = (ApaWeightImage * APA_WIMG_MAX)()
    n = c_int(0)
    dt = APA_DTYPE_BF16 if dtype == torch.bfloat16 else APA_DTYPE_F32
    _check(lib.apa_per_class_weight_images(
        _dev_ptr(Wa, 'Wa', torch.float32), _dev_ptr(ba, 'ba', torch.float32), _dev_ptr(Wt, 'Wt', torch.float32),
        _dev_ptr(bt, 'bt', torch.float32), workspace.data_ptr(), workspace.numel(), N, P, C, Ca, K, dt,
        ctypes.addressof(maps), ctypes.byref(n), _stream_ptr()), 'apa_per_class_weight_images')
    out = []
    for i in range(n.value):
        m = ApaWeightImage()
        ctypes.memmove(ctypes.addressof(m), ctypes.addressof(maps[i]), ctypes.sizeof(ApaWeightImage))
        out.append((APA_WIMG_ROLES[m.role], m))
    return out


def pose_w2t_image(W2: torch.Tensor) -> torch.Tensor:
    """bf16 [16, Cp + 16] image of W2^T (W2 [Cp, J <= 16]; rows J.. and the 16 pad columns zero) -- the LDS image of
    the Pl product, which copies it verbatim: `PoseAttnTrainStep(w2t_bf16=...)`."""
    Cp, J = W2.shape
    img = torch.zeros((16, Cp + 16), dtype=torch.bfloat16, device=W2.device)
    img[:J, :Cp].copy_(W2.t())
    return img


def pose_w2t_image_map(image: torch.Tensor, W2: torch.Tensor) -> ApaWeightImage:
    """where the optimiser's launch stores the updated element (c, j) of W2 inside `image`: image[j, c]."""
    m = ApaWeightImage()
    m.dst, m.role, m.is_f32, m.cols, m.c_shift = image.data_ptr(), 0, 0, int(W2.shape[1]), 0
    m.a, m.b, m.d, m.e = 1, 0, int(image.shape[1]), 0
    return m


class _OptimizerArgs:
    """The argument arrays of every fused optimiser launch (apa_momentum_sgd_step[_shadow|_images], apa_adam_step,
    apa_rmsprop_step), validated and marshalled in one place.  `weights`: fp32 device tensors in bucket order;
    `weight_decay`: one float per tensor; `flats`: ((name, fp32 tensor in the bucket layout), ...); `shadows`: None or
    one entry per tensor (None = no shadow) of contiguous bf16 tensors that receive the UPDATED weights rounded to bf16;
    `images`: [(segment index, ApaWeightImage), ...] rewritten from the updated weights (momentum only).
    `head` = (n, pointers, sizes, decays, *flat pointers), `sh` = the shadow table or None, `images` = (image array
    address, segment array, count) or None.  The object holds every tensor and array it points at."""

    def __init__(self, weights, weight_decay, flats, shadows=None, images=None, who='optimiser'):
        n = len(weights)
        total = sum(w.numel() for w in weights)
        for name, f in flats:
            if f.numel() != total:
                raise ValueError('%s: %s holds %d elements, the parameters %d' % (who, name, f.numel(), total))
        self.keep = (list(weights), list(flats), shadows, images)
        ptrs = [_dev_ptr(w, 'weights[%d]' % i, torch.float32) for i, w in enumerate(weights)]
        self.head = (n, (c_void_p * n)(*ptrs), (c_size_t * n)(*[w.numel() for w in weights]),
                     (c_float * n)(*[float(x) for x in weight_decay])) + \
            tuple(_dev_ptr(f, name, torch.float32) for name, f in flats)
        self.sh = None
        if shadows is not None and any(t is not None for t in shadows):
            for w_, t in zip(weights, shadows):
                if t is not None and (t.dtype != torch.bfloat16 or t.numel() != w_.numel() or not t.is_contiguous()):
                    raise ApaError('%s: a shadow must be a contiguous bf16 tensor of its weight\'s size' % who)
            self.sh = (c_void_p * n)(*[None if t is None else _dev_ptr(t, 'shadow', torch.bfloat16) for t in shadows])
        self.images = None
        if images:
            ni = len(images)
            self._arr = (ApaWeightImage * ni)()
            self._seg = (c_int * ni)(*[int(i) for i, _ in images])
            for q, (_, m) in enumerate(images):
                ctypes.memmove(ctypes.addressof(self._arr[q]), ctypes.addressof(m), ctypes.sizeof(ApaWeightImage))
            self.images = (ctypes.addressof(self._arr), self._seg, ni)


class BoundMomentumSGD:
    """One fused momentum-SGD launch with its argument arrays marshalled ONCE (the optimiser's counterpart of
    HeadTrainStep): acc = m*acc + (grad_scale*g + wd_i*w_i); w_i -= lr*acc for every parameter, plus the bf16 shadows
    (apa_momentum_sgd_step_shadow: the pose head's W1) and the operand images (apa_momentum_sgd_step_images) rewritten
    from the updated weights in the same launch.  `run(lr, momentum, grad_scale)` is one foreign call.  The per-update
    python cost of marshalling (~40 us of ctypes array building for eight parameters) is of the order of a whole
    HMDB-51 head step; a training loop pays it once per binding."""

    def __init__(self, weights, weight_decay, grad_flat, acc_flat, shadows=None, images=None):
        self.lib = load_library()
        a = self._args = _OptimizerArgs(weights, weight_decay, (('grad_flat', grad_flat), ('acc_flat', acc_flat)),
                                        shadows, images, 'BoundMomentumSGD')
        if a.images:
            self._who, self._tail = 'apa_momentum_sgd_step_images', (a.sh,) + a.images
        elif a.sh is not None:
            self._who, self._tail = 'apa_momentum_sgd_step_shadow', (a.sh,)
        else:
            self._who, self._tail = 'apa_momentum_sgd_step', ()
        self._fn = getattr(self.lib, self._who)

    def run(self, lr, momentum=0.9, grad_scale=1.0, stream: Optional[int] = None) -> None:
        st = _stream_ptr() if stream is None else stream
        rc = self._fn(*self._args.head, lr, momentum, grad_scale, *self._tail, st)
        if rc != 0:
            _check(rc, self._who)


def _epoch_order_arg(who: str, order: torch.Tensor, cache: FeatureCache) -> torch.Tensor:
    if not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or order.dim() != 1 or \
            not order.is_contiguous() or order.device != cache.device:
        raise ApaError('{}: order must be a contiguous int32 vector on the cache\'s device (FeatureCache.order)'
                       .format(who))
    return order


def _epoch_outputs(who: str, obj, outputs, shapes, dev) -> None:
    """set obj.<name> for every (name, shape, dtype) of `shapes`: the caller's tensor from `outputs` (same element
    count and dtype, contiguous, on `dev`) or a fresh one"""
    outputs = dict(outputs or {})
    for name, shape, dtype in shapes:
        t = outputs.pop(name, None)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif t.dtype != dtype or t.numel() != int(np.prod(shape)) or not t.is_contiguous() or t.device != dev:
            raise ApaError('{}: outputs[{!r}] must be a contiguous {} tensor of {} elements on {}'.format(
                who, name, dtype, int(np.prod(shape)), dev))
        setattr(obj, name, t)
    if outputs:
        raise ApaError('{}: unknown outputs {}'.format(who, sorted(outputs)))


def _epoch_cache(who: str, cache: FeatureCache):
    """(N-independent) shape of a cache an epoch call can read: (P, C, dtype code)"""
    if not isinstance(cache, FeatureCache):
        raise ApaError('{}: a FeatureCache expected'.format(who))
    if not cache.features.is_cuda:
        raise ApaError('{}: the cache must live in GPU memory; the HIP path has no CPU fallback'.format(who))
    C = cache.shape[-1]
    return int(np.prod(cache.shape[1:])) // C, C, _feat_dtype(cache.features)


class HeadTrainEpoch:
    """apa_attn_head_train_epoch_cached bound to caller-owned buffers, everything marshalled ONCE: a whole epoch of
    frozen-feature training on a resident FeatureCache -- `steps` times (the gathered one-call step on the next `N` ids
    of `order`, then the fused momentum-SGD update with that step's learning rate) -- as ONE foreign call, bit-identical
    in every output, weight and accumulator to the loop of `HeadTrainStep.rebind(index=, offset=) + run()` and
    `BoundMomentumSGD.run(lr[s], ...)`.

    `grads = (dWa, dba, dWt, dbt)`: where the step writes its gradients -- views of `grad_flat`, the flat bucket the
    update reads; `weights` / `weight_decay` / `grad_flat` / `acc_flat`: BoundMomentumSGD's arguments (segments the
    step does not write decay on whatever their window of `grad_flat` holds).  `labels=None`: the cache's own labels,
    read through the order; else pass `labels` int64 [count], in visiting order, to `run`.  `offset`: the dropout
    offset of the first step (step s uses offset + s), or a 1-element int64 CUDA tensor (the device counter, which
    advances by itself).  `steps`: the most steps one `run` may take (the loss log's rows).
    Outputs: `loss` [steps, 1+N] (the epoch's log: row s = step s's mean and per-example losses), and the LAST step's
    `logits`, `att`, `zsave`, `abar`, `G`; `outputs={name: tensor}` binds caller-owned buffers in their place."""

    def __init__(self, cache, N, Wa, ba, Wt, bt, grads, weights, weight_decay, grad_flat, acc_flat, *, steps,
                 momentum=0.9, update_grad_scale=1.0, labels_cached=True, flags=0, keep_prob=1.0, seed=0, offset=0,
                 loss_wt=1.0, grad_scale=1.0, workspace=None, hooks=None, outputs=None):
        who = 'HeadTrainEpoch'
        self.lib = load_library()
        P, C, dt = _epoch_cache(who, cache)
        N, steps = int(N), int(steps)
        if N < 1 or steps < 1:
            raise ApaError('{}: N >= 1 and steps >= 1 expected'.format(who))
        if Wa.shape[1] != 1:
            raise ApaError('{}: a feature cache feeds the class-agnostic head (M == 1)'.format(who))
        if labels_cached and cache.labels is None:
            raise ApaError('{}: labels_cached needs a FeatureCache with labels'.format(who))
        K, dev = Wt.shape[1], cache.device
        self.cache, self.N, self.steps, self.hooks = cache, N, steps, hooks
        f32 = torch.float32
        _epoch_outputs(who, self, outputs, (('logits', (N, K), f32), ('att', (N, P, 1), f32), ('zsave', (N, C), f32),
                                            ('abar', (N,), f32), ('loss', (steps, 1 + N), f32), ('G', (N, K), f32)), dev)
        flags |= APA_FLAG_FROZEN_INPUT
        need = int(self.lib.apa_attn_pool_workspace_bytes(N, P, C, C, K, 1, flags))
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.workspace = workspace
        dWa, dba, dWt, dbt = grads
        a = self._opt_args = _OptimizerArgs(weights, weight_decay, (('grad_flat', grad_flat), ('acc_flat', acc_flat)),
                                            who=who)
        self._lr = (c_float * steps)()
        nseg, wptr, sizes, wd, gptr, aptr = a.head
        self._sgd = ApaEpochSgd(nseg, ctypes.addressof(wptr), ctypes.addressof(sizes), ctypes.addressof(wd), gptr, aptr,
                                ctypes.addressof(self._lr), float(momentum), float(update_grad_scale))
        self._ep = ApaEpoch(None, 0)
        self._fc = ApaFeatureCache(None, cache.T, 1 if labels_cached else 0, cache.status.data_ptr())
        self._labels_cached = bool(labels_cached)
        self._keep = (Wa, ba, Wt, bt, grads, offset, seed, None, None)
        seed, off, flags = _rng_key(seed, offset, flags)     # the pointers below stay valid
        self._off_dev = isinstance(offset, torch.Tensor)
        X = cache.features.data_ptr()
        self._args = [
            X, X, _dev_ptr(Wa, 'Wa', torch.float32), _dev_ptr(ba, 'ba', torch.float32),
            _dev_ptr(Wt, 'Wt', torch.float32), _dev_ptr(bt, 'bt', torch.float32),
            _dev_ptr(cache.labels, 'labels', torch.int64) if labels_cached else None,
            float(loss_wt), float(grad_scale),
            self.logits.data_ptr(), self.att.data_ptr(), self.zsave.data_ptr(), self.abar.data_ptr(),
            self.loss.data_ptr(), self.G.data_ptr(), None, None, _dev_ptr(dWa, 'dWa', torch.float32),
            _dev_ptr(dba, 'dba', torch.float32), _dev_ptr(dWt, 'dWt', torch.float32),
            _dev_ptr(dbt, 'dbt', torch.float32), workspace.data_ptr(), workspace.numel(), N, P, C, C, K, 1,
            flags, float(keep_prob), int(seed), off, dt]
        self._pre = (ctypes.addressof(self._ep), ctypes.addressof(self._sgd), ctypes.addressof(self._fc))

    def run(self, order, lr, offset=None, labels=None, stream: Optional[int] = None, hooks=None) -> int:
        """Enqueue the epoch over `order` (int32 on the cache's device, a whole number of batches: FeatureCache.order,
        or its first steps * N entries) with `lr[s]` the learning rate of update s (a sequence of order.numel() / N
        floats, or one float for all).  `offset` (int): another dropout offset for the first step.  `labels`: int64
        [count] in visiting order, for an epoch built with labels_cached=False.  Returns the number of steps.
        Under a captured hipGraph: `lr[s]`, an int `offset` and the addresses of `order` / `labels` are read HERE, when
        the call is enqueued, and are frozen in the graph -- every replay trains with the captured rates (another
        `lr` needs a re-capture); the contents of `order` / `labels`, the device dropout counter (advanced by the
        number of steps per replay), weights and accumulators are re-read from HBM."""
        who = 'HeadTrainEpoch.run'
        order = _epoch_order_arg(who, order, self.cache)
        count = int(order.numel())
        steps = count // self.N
        if steps < 1 or count % self.N or steps > self.steps:
            raise ApaError('{}: {} ids are not 1..{} whole batches of {}'.format(who, count, self.steps, self.N))
        lrs = [float(lr)] * steps if isinstance(lr, (int, float)) else [float(v) for v in lr]
        if len(lrs) != steps:
            raise ApaError('{}: one learning rate per step expected ({} for {} steps)'.format(who, len(lrs), steps))
        self._lr[:steps] = lrs
        if self._labels_cached:
            if labels is not None:
                raise ApaError('{}: the epoch reads the cache\'s labels through the order'.format(who))
        else:
            if labels is None or labels.numel() != count:
                raise ApaError('{}: labels int64 [{}] in visiting order expected'.format(who, count))
            self._args[6] = _dev_ptr(labels, 'labels', torch.int64)
        if offset is not None:
            if self._off_dev:
                raise ApaError('{}: the epoch was bound to a device-side dropout counter'.format(who))
            self._args[-2] = int(offset)
        self._keep = self._keep[:7] + (order, labels)
        self._ep.order, self._ep.count = order.data_ptr(), count
        h = self.hooks if hooks is None else hooks
        rc = self.lib.apa_attn_head_train_epoch_cached(*self._pre, _hooks_ptr(h), *self._args,
                                                       _stream_ptr() if stream is None else stream)
        if rc != 0:
            _check(rc, 'apa_attn_head_train_epoch_cached')
        return steps


class HeadEvalEpoch:
    """apa_attn_head_eval_epoch_cached bound once: a validation pass over `count` images of a resident FeatureCache in
    batches of `N` (the last one shorter) as ONE foreign call, bit-identical to the loop of HeadEvalStep on
    `cache.select(order[s*N:(s+1)*N])`.  `scores`: 'softmax' | 'sigmoid'.  `capacity`: the most rows one `run` may
    visit.  `want_loss` (softmax scores, a cache with labels): the per-step losses, read through the order.
    Outputs: `logits`, `probs` [capacity,K] and `pred` [capacity] (rows [0, count) are written, nothing behind them),
    `loss` [ceil(capacity / N), 1+N] or None, and the LAST step's `att`, `zsave`, `abar`.  `run(..., probs=t)` writes
    the scores into the caller's float32 [count,K] tensor instead (eval_utils.DeviceEvaluation.reserve)."""

    def __init__(self, cache, N, Wa, ba, Wt, bt, *, capacity, flags=0, scores='softmax', want_loss=False,
                 workspace=None, outputs=None):
        who = 'HeadEvalEpoch'
        self.lib = load_library()
        P, C, dt = _epoch_cache(who, cache)
        N, capacity = int(N), int(capacity)
        if N < 1 or capacity < 1:
            raise ApaError('{}: N >= 1 and capacity >= 1 expected'.format(who))
        if Wa.shape[1] != 1:
            raise ApaError('{}: a feature cache feeds the class-agnostic head (M == 1)'.format(who))
        if scores not in ('softmax', 'sigmoid'):
            raise ApaError('{}: scores must be \'softmax\' or \'sigmoid\' (got {!r})'.format(who, scores))
        if want_loss and (scores != 'softmax' or cache.labels is None):
            raise ApaError('{}: want_loss needs softmax scores and a FeatureCache with labels'.format(who))
        K, dev = Wt.shape[1], cache.device
        self.cache, self.N, self.capacity, self.K = cache, N, capacity, K
        flags &= ~APA_FLAG_TRAIN
        f32 = torch.float32
        self.loss = None
        _epoch_outputs(who, self, outputs,
                       (('logits', (capacity, K), f32), ('probs', (capacity, K), f32), ('pred', (capacity,), torch.int64),
                        ('att', (N, P, 1), f32), ('zsave', (N, C), f32), ('abar', (N,), f32)) +
                       ((('loss', ((capacity + N - 1) // N, 1 + N), f32),) if want_loss else ()), dev)
        need = int(self.lib.apa_attn_pool_workspace_bytes(N, P, C, C, K, 1, flags))
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.workspace = workspace
        self._ep = ApaEpoch(None, 0)
        self._fc = ApaFeatureCache(None, cache.T, 1 if want_loss else 0, cache.status.data_ptr())
        self._keep = (Wa, ba, Wt, bt, None, None)
        X = cache.features.data_ptr()
        self._args = [
            X, X, _dev_ptr(Wa, 'Wa', torch.float32), _dev_ptr(ba, 'ba', torch.float32),
            _dev_ptr(Wt, 'Wt', torch.float32), _dev_ptr(bt, 'bt', torch.float32),
            _dev_ptr(cache.labels, 'labels', torch.int64) if want_loss else None, self.logits.data_ptr(),
            self.att.data_ptr(), self.zsave.data_ptr(), self.abar.data_ptr(), _dev_ptr(self.loss, 'loss'),
            self.probs.data_ptr(), self.pred.data_ptr(), workspace.data_ptr(), workspace.numel(),
            N, P, C, C, K, 1, flags, dt]
        self._pre = (ctypes.addressof(self._ep), ctypes.addressof(self._fc),
                     APA_SCORES_SOFTMAX if scores == 'softmax' else APA_SCORES_SIGMOID)

    def run(self, order, count: Optional[int] = None, probs: Optional[torch.Tensor] = None,
            stream: Optional[int] = None) -> int:
        """Enqueue the pass over the first `count` ids of `order` (default: all of it).  Returns the number of steps."""
        who = 'HeadEvalEpoch.run'
        order = _epoch_order_arg(who, order, self.cache)
        count = int(order.numel()) if count is None else int(count)
        if not 1 <= count <= min(int(order.numel()), self.capacity):
            raise ApaError('{}: count = {} outside 1..{} (the order\'s length and the capacity)'.format(
                who, count, min(int(order.numel()), self.capacity)))
        if probs is not None and (tuple(probs.shape) != (count, self.K) or probs.device != self.cache.device):
            raise ApaError('{}: probs float32 [{}, {}] on the cache\'s device expected'.format(who, count, self.K))
        self._args[12] = self.probs.data_ptr() if probs is None else _dev_ptr(probs, 'probs', torch.float32)
        self._keep = self._keep[:4] + (order, probs)
        self._ep.order, self._ep.count = order.data_ptr(), count
        rc = self.lib.apa_attn_head_eval_epoch_cached(*self._pre, *self._args,
                                                      _stream_ptr() if stream is None else stream)
        if rc != 0:
            _check(rc, 'apa_attn_head_eval_epoch_cached')
        return (count + self.N - 1) // self.N


def adam_step(weights, weight_decay, grad_flat, m_flat, v_flat, lr, t, beta1=0.9, beta2=0.999, epsilon=1e-8,
              grad_scale=1.0, shadows=None):
    """tf.train.AdamOptimizer (src/train.py:84-89) as one fused launch; `t` = number of this update (1, 2, ...):
    lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) is formed here, in double precision, like TF's python side."""
    a = _OptimizerArgs(weights, weight_decay, (('grad_flat', grad_flat), ('m_flat', m_flat), ('v_flat', v_flat)),
                       shadows, who='adam_step')
    lr_t = float(lr) * (1.0 - float(beta2) ** int(t)) ** 0.5 / (1.0 - float(beta1) ** int(t))
    _check(load_library().apa_adam_step(*a.head, lr_t, beta1, beta2, epsilon, grad_scale, a.sh, _stream_ptr()),
           'apa_adam_step')


def rmsprop_step(weights, weight_decay, grad_flat, ms_flat, mom_flat, lr, decay=0.9, momentum=0.0, epsilon=1e-10,
                 grad_scale=1.0, shadows=None):
    """tf.train.RMSPropOptimizer (src/train.py:95-100) as one fused launch; `ms_flat` starts at ONE."""
    a = _OptimizerArgs(weights, weight_decay, (('grad_flat', grad_flat), ('ms_flat', ms_flat), ('mom_flat', mom_flat)),
                       shadows, who='rmsprop_step')
    _check(load_library().apa_rmsprop_step(*a.head, lr, decay, momentum, epsilon, grad_scale, a.sh, _stream_ptr()),
           'apa_rmsprop_step')


def _is_dense(t: torch.Tensor) -> bool:
    """non-overlapping and dense in SOME dimension order (contiguous, channels-last, any permutation): the numel
    elements fill [data_ptr, data_ptr + 4 * numel) exactly once"""
    dims = sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def _elementwise_ptr(t: torch.Tensor, name: str) -> int:
    """device pointer of an fp32 tensor an ELEMENTWISE op (plus a whole-tensor reduction) may walk as a flat array in
    memory order: any dense layout -- e.g. the channels-last conv weights of resnet_v1 and their `.grad`."""
    if not t.is_cuda:
        raise ApaError('{} must live in GPU memory (got device {}); the HIP path has no CPU '
                       'fallback'.format(name, t.device))
    if t.dtype != torch.float32:
        raise ApaError('{} must be {} (got {})'.format(name, torch.float32, t.dtype))
    if not _is_dense(t):
        raise ApaError('{} must be dense (contiguous in some dimension order; strides {})'.format(name, t.stride()))
    return t.data_ptr()


class BoundClipByNorm:
    """Per-variable clip-by-norm (TRAIN.CLIP_GRADIENTS: slim.learning.clip_gradient_norms -> tf.clip_by_norm on every
    tensor separately) with the segment table marshalled ONCE into a device workspace: `run(clip)` is two launches on
    the current stream (or `stream`), no host sync, capturable in a hipGraph.

    `tensors`: fp32 device tensors rewritten in place (views of a flat bucket at any 4-byte offset, `.grad` tensors),
    each dense in any dimension order (channels-last included: the op is elementwise plus a whole-tensor norm, so it
    walks memory order); `weights` / `wd`: optional per-tensor weight and coefficient -- t = g + wd * w enters the norm
    and the output (the regulariser's gradient on clone 0); a weight must have its gradient's shape and strides;
    `absent`: optional per-tensor flags, True = the gradient is taken as zero and only written (a variable the
    producer never differentiates).  The constructor marshals the table (one host sync); `run` never does."""

    def __init__(self, tensors, weights=None, wd=None, absent=None, stream: Optional[int] = None):
        self.lib = load_library()
        ts = list(tensors)
        n = len(ts)
        if n == 0:
            raise ApaError('clip_by_norm: no tensors')
        ws_ = list(weights) if weights is not None else [None] * n
        wds = [float(x) for x in wd] if wd is not None else [0.0] * n
        ab = [bool(x) for x in absent] if absent is not None else [False] * n
        if not (len(ws_) == len(wds) == len(ab) == n):
            raise ApaError('clip_by_norm: weights / wd / absent need one entry per tensor')
        gp = []
        for i, t in enumerate(ts):
            gp.append(_elementwise_ptr(t, 'tensors[%d]' % i))
        wp = []
        for i, (w, t, d) in enumerate(zip(ws_, ts, wds)):
            if d != 0.0:
                if w is None or w.numel() != t.numel():
                    raise ApaError('clip_by_norm: tensors[%d] has wd != 0 and needs a weight of its size' % i)
                if t.numel() > 1 and (tuple(w.shape) != tuple(t.shape) or w.stride() != t.stride()) and not (
                        w.is_contiguous() and t.is_contiguous()):
                    raise ApaError('clip_by_norm: weights[%d] (shape %s, strides %s) must lie in memory like its '
                                   'gradient (shape %s, strides %s)' % (i, tuple(w.shape), w.stride(), tuple(t.shape),
                                                                       t.stride()))
                wp.append(_elementwise_ptr(w, 'weights[%d]' % i))
            else:
                wp.append(None)
        self._keep = (ts, ws_)
        self._n = n
        self._g = (c_void_p * n)(*gp)
        self._sizes = (c_size_t * n)(*[t.numel() for t in ts])
        self._w = (c_void_p * n)(*wp)
        self._wd = (c_float * n)(*wds)
        self._ab = (ctypes.c_ubyte * n)(*[1 if x else 0 for x in ab])
        nbytes = int(self.lib.apa_clip_by_norm_workspace_bytes(n, self._sizes))
        self.ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=ts[0].device)
        nch = c_int(0)
        st = _stream_ptr() if stream is None else stream
        _check(self.lib.apa_clip_by_norm_prepare(n, self._g, self._sizes, self._w, self._wd, self._ab,
                                                 self.ws.data_ptr(), self.ws.numel(), ctypes.byref(nch), st),
               'apa_clip_by_norm_prepare')
        self.nchunks = nch.value

    def run(self, clip: float, stream: Optional[int] = None) -> None:
        st = _stream_ptr() if stream is None else stream
        rc = self.lib.apa_clip_by_norm_run(self.ws.data_ptr(), self._n, self.nchunks, float(clip), st)
        if rc != 0:
            _check(rc, 'apa_clip_by_norm_run')


def clip_by_norm_(tensors, clip: float, weights=None, wd=None, absent=None) -> None:
    """tf.clip_by_norm on every tensor of `tensors` separately, in place, on the current stream (see BoundClipByNorm;
    this one-shot form marshals the table on each call -- a training loop keeps a BoundClipByNorm)."""
    if float(clip) <= 0.0:
        return
    BoundClipByNorm(tensors, weights, wd, absent).run(clip)


# --------------------------------------------------------------------------------------------
# measurement hooks (bench.py)
# --------------------------------------------------------------------------------------------
ACC_MAX_PARTS = 8      # APA_ACC_MAX_PARTS (include/apa.h)


def accumulate_gradients(out: torch.Tensor, parts, scale: Optional[float] = None, stream: Optional[int] = None,
                         divisor: Optional[float] = None) -> None:
    """out = (parts[0] + parts[1] + ...) / divisor  -- or  ... * scale --, summed in that order (TRAIN.ITER_SIZE
    accumulation of micro-batch buckets, src/train.py:529-566).  `divisor=ITER_SIZE` is the reference's own
    arithmetic (`ref_grad / float(ITER_SIZE)`, apa_accumulate_gradients_div).  More than APA_ACC_MAX_PARTS
    parts are folded in groups, left to right, so the summation order stays that of the sequential loop."""
    if (scale is None) == (divisor is None):
        raise ApaError('accumulate_gradients: give exactly one of scale / divisor')
    lib = load_library()
    n = out.numel()
    parts = list(parts)
    for p_ in parts:
        if p_.numel() != n:
            raise ApaError('accumulate_gradients: every part must have out.numel() elements')
    st = _stream_ptr() if stream is None else stream
    optr = _dev_ptr(out, 'out', torch.float32)

    def launch(group, last):
        arr = (c_void_p * len(group))(*[_dev_ptr(p_, 'part', torch.float32) for p_ in group])
        if last and divisor is not None:
            rc = lib.apa_accumulate_gradients_div(optr, arr, len(group), n, float(divisor), st)
        else:
            rc = lib.apa_accumulate_gradients(optr, arr, len(group), n, float(scale) if last else 1.0, st)
        _check(rc, 'apa_accumulate_gradients')

    head, rest = parts[:ACC_MAX_PARTS], parts[ACC_MAX_PARTS:]
    launch(head, not rest)
    while rest:                               # out already holds the running sum: it leads the next group
        group, rest = [out] + rest[:ACC_MAX_PARTS - 1], rest[ACC_MAX_PARTS - 1:]
        launch(group, not rest)


class KernelTimer:
    """Per-step event pairs for the two streaming kernels of the M == 1 head (m1s_pool_fwd_kernel,
    m1s_bwd_main_kernel).  `hooks(i)` is the apa_hooks struct to pass to step i: the library launches
    those kernels through hipExtLaunchKernel with the pair attached, so each pair brackets exactly one
    dispatch on its own stream (reads ~1.2 us above rocprofv3's begin -> end of the same kernel)."""

    def __init__(self, n_steps: int, base: Optional[ApaHooks] = None):
        lib = load_library()
        self._lib = lib
        self.fwd, self.bwd, self._hooks = [], [], []
        for _ in range(n_steps):
            f, b = self._new_pair(), self._new_pair()
            self.fwd.append(f)
            self.bwd.append(b)
            h = make_hooks(prof_fwd=f, prof_bwd=b)
            if base is not None:
                h.grad_ready_event, h.td_weights_ready_event = base.grad_ready_event, base.td_weights_ready_event
            self._hooks.append(h)

    def _new_pair(self):
        a, b = c_void_p(), c_void_p()
        _check(self._lib.apa_prof_event_create(ctypes.byref(a)), 'apa_prof_event_create')
        _check(self._lib.apa_prof_event_create(ctypes.byref(b)), 'apa_prof_event_create')
        return a, b

    def hooks(self, i: int) -> ApaHooks:
        return self._hooks[i]

    def _elapsed(self, pairs):
        out = []
        for a, b in pairs:
            ms = c_float()
            _check(self._lib.apa_prof_event_elapsed_ms(a, b, ctypes.byref(ms)), 'apa_prof_event_elapsed_ms')
            out.append(ms.value)
        return out

    def fwd_elapsed_ms(self):
        return self._elapsed(self.fwd)

    def bwd_elapsed_ms(self):
        return self._elapsed(self.bwd)

    def close(self) -> None:
        for a, b in self.fwd + self.bwd:
            self._lib.apa_prof_event_destroy(a)
            self._lib.apa_prof_event_destroy(b)
        self.fwd, self.bwd, self._hooks = [], [], []
