"""The contract of clip_scores_kernel (attentionalpoolingaction_amd/csrc/apa_clipscores.hip, include/apa.h:
apa_clip_scores) restated in float64 numpy, and the shapes tests/test_eval_clips_gpu.py runs it on.

    a[r]        = x[r,:] . w + b0                (temporal attention; 1 without)
    pooled[b,k] = (1/F) sum_f x[b,f,k] a[b,f]    (frames in increasing f)
    softmax:  scores = softmax(pooled), pred = first maximal index, loss[1+b] = -log scores[b, labels[b]],
              loss[0] = mean_b loss[1+b]
    sigmoid:  scores = 1 / (1 + exp(-pooled)), pred = first maximal index of pooled
"""
import numpy as np

# (B, F, K): K < 4 | a small general case | the HMDB protocol | last K on the row routine | first K past it |
# rows out of LDS | F > CLIP_LDS_F | the other loss[0] order
SHAPES = [(1, 1, 3), (3, 4, 20), (2, 25, 51), (2, 3, 1024), (2, 3, 1025), (2, 2, 4100), (1, 70, 20), (65, 2, 7)]


def clip_scores_f64(x, frames, w=None, b0=None, kind='softmax', labels=None):
    x = np.asarray(x, dtype=np.float64)
    rows, K = x.shape
    F = int(frames)
    assert rows % F == 0
    B = rows // F
    xr = x.reshape(B, F, K)
    out = {}
    if w is not None:
        a = xr @ np.asarray(w, dtype=np.float64).reshape(K) + float(np.asarray(b0, dtype=np.float64).reshape(-1)[0])
        out['tatt'] = a.reshape(rows)
    else:
        a = np.ones((B, F))
    pooled = np.zeros((B, K))
    for f in range(F):                                   # frames in increasing f
        pooled += xr[:, f, :] * a[:, f, None]
    pooled /= F
    out['pooled'] = pooled
    out['pred'] = pooled.argmax(axis=1)                  # numpy: the FIRST maximal index
    if kind == 'sigmoid':
        assert labels is None
        out['scores'] = 1.0 / (1.0 + np.exp(-pooled))
        return out
    m = pooled.max(axis=1, keepdims=True)
    e = np.exp(pooled - m)
    s = e.sum(axis=1, keepdims=True)
    out['scores'] = e / s
    if labels is not None:
        lab = np.asarray(labels).reshape(B)
        per = -(pooled[np.arange(B), lab] - m[:, 0] - np.log(s[:, 0]))
        out['loss'] = np.concatenate([[per.mean()], per])
    return out


def make_logits(B, F, K, seed):
    """float32 frame logits [B*F, K], temporal weights w [K] and bias b [1], labels [B]: logits of the order of 1 with
    the rows' maxima spread over the columns; a[] of the order of 1/F + small, as the trained conv gives."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((B * F, K)).astype(np.float32)
    w = (rng.standard_normal(K) * (0.3 / np.sqrt(K))).astype(np.float32)
    b = np.array([1.0 / F], dtype=np.float32)
    labels = rng.randint(0, K, size=B).astype(np.int64)
    return x, w, b, labels
