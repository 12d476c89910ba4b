"""Eval consumers of the head's logits.

Reference: /root/reference/src/eval.py:193-197,303-306 (argmax / softmax / accuracy),
/root/reference/src/eval/utils.py:4-16 (`compute_map`) and
/root/reference/src/eval/cap_eval_utils.py:55-109 (`calc_pr_ovr_noref`, `voc_ap`).

`predict` runs the fused HIP softmax/argmax kernel on the GPU; the mAP itself is host-side numpy
like the reference (it runs once per evaluation over [num_samples, K] scores), vectorised but with
the reference's exact ordering rule: scores are ranked by `np.argsort(out)[::-1]`, i.e. ties are
broken by the reversed quicksort order of numpy -- we call the very same numpy routine so the
ranking (and therefore AP under ties) is identical.

`DeviceEvaluation` is the same accumulation with the metric itself on the device (csrc/apa_metrics.hip,
`cof.average_precision`): three launches and one small copy instead of K argsorts on the host.  Its ranking
rule is this project's, written down in include/apa.h:

    scores are ranked in descending order; equal scores are ordered by DESCENDING sample index -- what
    `np.argsort(out, kind='stable')[::-1]` gives.  -0.0 and +0.0 are equal, +-inf are ordinary values; a
    NaN score and a label outside [0,K) are counted and make `result()` raise.

On tie-free scores this is the reference's ranking, and a class's AP carries `voc_ap`'s own bits (the kernel
adds the terms in rank order, as the loop below does); the mean over the classes is within K * 2^-52 of
`np.mean`.  Under ties the host routines above keep numpy's introsort order, which no rule describes; the two
then differ, and only the device route is reproducible by a second implementation.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


def predict(logits, multi_label=False):
    """(scores [N,K] float32, predictions [N] int64) on the device of `logits`
    (eval.py:193-197: tf.argmax(logits,1), tf.nn.softmax(logits,-1)).  `multi_label=True` (TRAIN.LOSS_FN_ACTION
    starts with 'multi-label', eval.py:194-195): the scores are tf.sigmoid(logits), element-wise -- plain tensor
    expressions on whatever device holds the logits; the predictions stay the argmax of the logits."""
    import torch
    if multi_label:
        logits = logits.float()
        return torch.sigmoid(logits), logits.argmax(dim=1)
    from .custom_ops import custom_ops_factory as cof
    labels = torch.zeros((logits.shape[0],), dtype=torch.int64, device=logits.device)
    _, _, probs, pred = cof.softmax_xent_fwd_bwd(logits.contiguous(), labels, want_grad=False,
                                                 want_probs=True, want_pred=True)
    return probs, pred


class Evaluation:
    """The accumulation of eval.py:262-306 without a host round trip per batch: `update(scores, labels)` keeps the
    batch's scores [n,K] and labels [n] where they are (the device of the scores); `result()` concatenates, copies to
    the host ONCE and returns {'accuracy', 'mAP', 'aps'} through `accuracy` / `compute_map` (eval.py:303-306)."""

    def __init__(self):
        self._scores, self._labels = [], []

    def update(self, scores, labels) -> None:
        import torch
        scores = scores.detach()
        labels = torch.as_tensor(labels).detach().reshape(-1).to(scores.device)
        if scores.dim() != 2 or labels.numel() != scores.shape[0]:
            raise ValueError('Evaluation.update: scores [n,K] and labels [n] expected')
        self._scores.append(scores.float().clone())      # (a bound step overwrites its buffers on the next batch)
        self._labels.append(labels.to(torch.int64).clone())

    def __len__(self) -> int:
        return sum(int(s.shape[0]) for s in self._scores)

    def result(self):
        import torch
        if not self._scores:
            raise ValueError('Evaluation.result: nothing was accumulated')
        k = self._scores[0].shape[1]
        # one buffer [n, K + 1] (labels are exact in float64 up to 2^53), one device-to-host copy
        both = torch.cat([torch.cat(self._scores).double(), torch.cat(self._labels).double().unsqueeze(1)], dim=1).cpu()
        both = both.numpy()
        scores, labels = both[:, :k].astype(np.float32), both[:, k].astype(np.int64)
        m, aps = compute_map(scores, labels)
        return {'accuracy': accuracy(scores, labels), 'mAP': m, 'aps': aps}


class DeviceEvaluation:
    """`Evaluation` with everything on the device: a resident [capacity, K] float32 score buffer and a label buffer
    ([capacity] int64; multi_label=True: a [capacity, K] float32 multi-hot target buffer, positives are > 0).

        meter = DeviceEvaluation(capacity, K, device)            # or deploy.FusedHeadEval.new_evaluation(capacity)
        meter.update(scores, labels)                             # device copies at the cursor, no host round trip
        out = meter.result()                                     # three launches, ONE device-to-host copy

    `result()` returns what `Evaluation.result()` returns -- 'accuracy', 'mAP', 'aps' (the classes with positives, in
    class order) -- and adds 'ap_per_class' [K] (0 for a class without positives) and 'npos' [K].  'accuracy' is NaN
    with multi-hot targets.  The ranking rule is the one in this module's docstring.  It raises ValueError when a
    score was NaN or a label lay outside [0,K).  At most cof.APA_AP_MAX_SAMPLES = 16384 rows: a class's ranking is
    sorted in one block's LDS, and there is no multi-pass sort behind it."""

    def __init__(self, capacity: int, num_classes: int, device, multi_label: bool = False):
        import torch
        from .custom_ops import custom_ops_factory as cof
        capacity, num_classes = int(capacity), int(num_classes)
        if capacity < 1 or num_classes < 1:
            raise ValueError('DeviceEvaluation: capacity and num_classes must be positive')
        if capacity > cof.APA_AP_MAX_SAMPLES:
            raise ValueError('DeviceEvaluation: capacity %d exceeds the %d rows one apa_average_precision call ranks'
                             % (capacity, cof.APA_AP_MAX_SAMPLES))
        self.capacity, self.num_classes, self.multi_label = capacity, num_classes, bool(multi_label)
        self.device = torch.device(device)
        self._scores = torch.empty((capacity, num_classes), dtype=torch.float32, device=self.device)
        if self.multi_label:
            self._truth = torch.empty((capacity, num_classes), dtype=torch.float32, device=self.device)
        else:
            self._truth = torch.empty((capacity,), dtype=torch.int64, device=self.device)
        self._n = 0
        self._ws = self._out = None

    def __len__(self) -> int:
        return self._n

    def reset(self) -> None:
        self._n = 0

    def update(self, scores, labels) -> None:
        import torch
        scores = scores.detach()
        labels = torch.as_tensor(labels).detach()
        k = self.num_classes
        if scores.dim() != 2 or scores.shape[1] != k:
            raise ValueError('DeviceEvaluation.update: scores [n,%d] expected (got %s)' % (k, tuple(scores.shape)))
        n = int(scores.shape[0])
        if self.multi_label:
            if tuple(labels.shape) != (n, k):
                raise ValueError('DeviceEvaluation.update: multi-hot targets [n,K] = [%d,%d] expected (got %s)'
                                 % (n, k, tuple(labels.shape)))
        else:
            if labels.numel() != n:
                raise ValueError('DeviceEvaluation.update: labels [n] = [%d] expected (got %s)'
                                 % (n, tuple(labels.shape)))
            labels = labels.reshape(-1)
        if self._n + n > self.capacity:
            raise ValueError('DeviceEvaluation.update: %d rows behind %d overflow the capacity of %d'
                             % (n, self._n, self.capacity))
        self._scores[self._n:self._n + n].copy_(scores, non_blocking=True)     # (casts on the device)
        self._truth[self._n:self._n + n].copy_(labels, non_blocking=True)
        self._n += n

    def reserve(self, n: int):
        """The next `n` rows as views `(scores [n,K], truth [n] or [n,K])` of the meter's own buffers, the cursor
        moved behind them: a producer writes its scores (and the truth) in place instead of handing copies to
        `update` (deploy.FusedHeadEval.evaluate_cache: the evaluation pass's `probs` ARE these rows).  The rows count
        as accumulated at once: write both views before `result()`."""
        n = int(n)
        if n < 1:
            raise ValueError('DeviceEvaluation.reserve: n >= 1 expected (got %d)' % n)
        if self._n + n > self.capacity:
            raise ValueError('DeviceEvaluation.reserve: %d rows behind %d overflow the capacity of %d'
                             % (n, self._n, self.capacity))
        a = self._n
        self._n += n
        return self._scores[a:a + n], self._truth[a:a + n]

    def result(self):
        import torch
        from .custom_ops import custom_ops_factory as cof
        if self._n == 0:
            raise ValueError('DeviceEvaluation.result: nothing was accumulated')
        k, n = self.num_classes, self._n
        if self._ws is None:
            need = cof.average_precision_workspace_bytes(self.capacity, k)
            self._ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=self.device)
            self._out = torch.empty((cof.average_precision_result_bytes(k),), dtype=torch.uint8, device=self.device)
        truth = self._truth[:n]
        cof.average_precision(self._scores[:n], labels=None if self.multi_label else truth,
                              targets=truth if self.multi_label else None, workspace=self._ws, out=self._out)
        host = self._out.cpu()                                   # the one copy: K + 5 numbers and the K counts
        ap = host[:8 * k].view(torch.float64).numpy()
        summary = host[8 * k:8 * k + 24].view(torch.float64).numpy()
        npos = host[8 * k + 24:12 * k + 24].view(torch.int32).numpy()
        status = host[12 * k + 24:12 * k + 32].view(torch.int32).numpy()
        if status[0] or status[1]:
            raise ValueError('DeviceEvaluation.result: %d NaN scores, %d labels outside [0,%d)'
                             % (int(status[0]), int(status[1]), k))
        return {'accuracy': float(summary[1]), 'mAP': float(summary[0]),
                'aps': [float(a) for a, c in zip(ap, npos) if c > 0],
                'ap_per_class': ap.copy(), 'npos': npos.copy()}


def voc_ap(rec: np.ndarray, prec: np.ndarray) -> float:
    """Area under the right-max envelope of precision over the recall steps."""
    mrec = np.concatenate(([0.0], np.asarray(rec, dtype=np.float64).ravel(), [1.0]))
    mpre = np.concatenate(([0.0], np.asarray(prec, dtype=np.float64).ravel(), [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    idx = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    # accumulate left to right like the reference's python loop (same float64 rounding order)
    ap = 0.0
    for d in (mrec[idx] - mrec[idx - 1]) * mpre[idx]:
        ap = ap + d
    return float(ap)


def calc_pr_ovr_noref(counts: np.ndarray, out: np.ndarray):
    """Precision / recall / AP of one class: counts > 0 marks the positives, `out` the scores."""
    counts = np.array(np.asarray(counts) > 0, dtype=np.float32)
    out = np.asarray(out)
    ind = np.argsort(out)[::-1]
    score = out[ind].astype(np.float64)
    tp = counts[ind].astype(np.float64)
    fp = 1.0 - tp
    ctp = np.cumsum(tp)
    P = ctp / (ctp + np.cumsum(fp))
    R = ctp / np.sum(counts)
    return P, R, score, voc_ap(R, P)


def compute_map(all_logits: np.ndarray, all_labels: np.ndarray) -> Tuple[float, List[float]]:
    """mAP over the classes that have at least one positive (eval/utils.py:4-16)."""
    all_logits = np.asarray(all_logits)
    all_labels = np.asarray(all_labels)
    aps: List[float] = []
    for cid in range(all_logits.shape[1]):
        this_labels = (all_labels == cid).astype('float32')
        if np.sum(this_labels) == 0:
            continue        # the reference prints a notice and skips the class
        aps.append(calc_pr_ovr_noref(this_labels, all_logits[:, cid])[3])
    return float(np.mean(aps)), aps


def accuracy(all_scores: np.ndarray, all_labels: np.ndarray) -> float:
    """eval.py:304-305: mean(argmax(scores, 1) == labels)."""
    return float(np.mean(np.asarray(all_scores).argmax(axis=1) == np.asarray(all_labels)))
