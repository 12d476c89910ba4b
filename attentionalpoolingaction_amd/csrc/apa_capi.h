// apa_capi.h -- what apa_capi.hip hands to the epoch layer (apa_epoch.hip): the one-call steps of the attention head as
// a request and the function that serves it.  Everything else of the host layer stays static in apa_capi.hip.
#pragma once
#include "apa_internal.h"

namespace apa {

// Everything an attention-head training step is handed: the flat argument list of apa_attn_head_train_step, in its
// order, then the optional parts.  cached / sigmoid / clips say which parts the entry point TAKES, not whether the
// pointer is set: a part that is taken and null is refused by its own check, in the entry point's name.
struct HeadTrainStep {
  const void *X, *Xatt; const float *Wa, *ba, *Wt, *bt;
  const int64_t* labels; float loss_wt, grad_scale;
  float *logits, *att, *zsave, *abar, *loss, *G;
  void *dX, *dXatt; float *dWa, *dba, *dWt, *dbt;
  void* ws; size_t ws_bytes; PoolDims dims; unsigned flags; float keep_prob; uint64_t seed, offset; void* stream;
  const apa_hooks* hooks = nullptr;
  const apa_feature_cache* cache = nullptr; bool cached = false;   // X is a cache read through cache->index
  const apa_multilabel* ml = nullptr; bool sigmoid = false;        // a sigmoid loss on ml->labels; `labels` is not read
  const apa_clip_pool* clip = nullptr; bool clips = false;         // the loss is taken on rows pooled over clip->frames
};

// ... and an evaluation step: the flat list of apa_attn_head_eval_step, then the scores kind and the optional parts.
// clips: the entry point takes a clip pool (null: flat rows); a cached step that does not refuses a clip by name.
// Neither cached nor clips: the plain step, attn_head_eval with its own messages (scores_kind is not read).
struct HeadEvalStep {
  const void *X, *Xatt; const float *Wa, *ba, *Wt, *bt;
  const int64_t* labels;
  float *logits, *att, *zsave, *abar, *loss, *probs; int64_t* pred;
  void* ws; size_t ws_bytes; PoolDims dims; unsigned flags; void* stream;
  int scores_kind = APA_SCORES_SOFTMAX;
  const apa_feature_cache* cache = nullptr; bool cached = false;
  const apa_clip_pool* clip = nullptr; bool clips = false;
};

// The step: its refusals in fn's name, in the one order apa_capi.hip writes down, then the launches.
int head_train_step(const char* fn, const HeadTrainStep& r);
int head_eval_step(const char* fn, const HeadEvalStep& r);
// Everything the step would refuse for the request's shape -- per-class maps on a cache among it, which the epoch calls
// keep refusing -- and both halves' pooling checks, in fn's name (an epoch call's); nothing is launched.
int head_train_check(const char* fn, const HeadTrainStep& r);
int head_eval_check(const char* fn, const HeadEvalStep& r);

}  // namespace apa
