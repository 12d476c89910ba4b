"""ctypes glue for the multi-label step's wrapper in the test-only probe library (csrc/apa_m1_probe.hip:
apa_probe_m1_train_step_multilabel), and the float64 error model of the sigmoid action losses that
tests/test_multilabel_step_gpu.py compares the kernels with.

The trace is read RAW: M1Trace.logits == M1_LOGITS_ML (6) says the loss rode in the logits reducer
(m1_logits_ml_kernel); tests/_m1_probe.py's name table predates that value and stays as it is.

Error model, in units of 2^-24, against float64 at the fp32 inputs (x any size, t in [0, 1], pw):
  * gradient  |G - ref|  <= 16 max(1, pw) 2^-24 gscale                  per element
  * loss term |l - ref|  <= 32 2^-24 (|ref| + 1)                        per element
    (a numpy fp32 restatement of ml_term over 4.2 M draws, |x| up to 100, stays within 2.1 and 8.0 of those units)
  * a sum of L terms adds the project's contraction bound C_ACC (L + 8) 2^-24 sum|terms| (tests/_m1_probe.py):
    L = K for a row mean, L = n_loss for the batch mean.
"""
import ctypes

import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _m1_probe as mp

M1_LOGITS_ML = 6
C_ACC, EPS32 = mp.C_ACC, mp.EPS32
KINDS = ('multi-label', 'multi-label-2')


def load():
    """the probe library with the multi-label wrapper bound: (M1Trace*, then the product entry point's arguments)"""
    lib = mp.load_m1_probe()
    fn = lib.apa_probe_m1_train_step_multilabel
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] + list(cof._SIGNATURES['apa_attn_head_train_step_multilabel'][1])
    return lib


def run_traced(step):
    """Run a bound cof.HeadTrainStep (a multi-label one) through the probe wrapper -> the raw M1Trace."""
    assert step._ml is not None
    lib = load()
    tr = mp.M1Trace()
    rc = lib.apa_probe_m1_train_step_multilabel(ctypes.addressof(tr), *step._pre, None, *step._args,
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.apa_last_error()
    return tr


def terms(kind, x, t, pw):
    """float64 (l, l') of src/loss.py:88-101 elementwise"""
    sp = torch.log1p(torch.exp(-x.abs())) + torch.clamp(-x, min=0)          # softplus(-x)
    sg = torch.sigmoid(x)
    if kind == 'multi-label':
        w = 1.0 + (pw - 1.0) * t
        return (1 - t) * x + w * sp, (1 - t) - w * (1 - sg)
    return torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs())), sg - t


def weight(kind, wt):
    """'multi-label' ignores the action-loss weight (loss.py:93-97)"""
    return 1.0 if kind == 'multi-label' else wt


def rows_reference(kind, x, t, pw, wt, gs, x_err=None):
    """-> (loss Bnd [1+N], G Bnd [N,K]) for logits x [N,K] (float64, with an optional elementwise error x_err),
    labels t; the bounds of the module docstring, plus |l'| x_err on a term and max(1, pw)/4 x_err on a gradient
    (|l''| = w sigma (1 - sigma) <= max(1, pw) / 4) when the logits carry an error of their own."""
    N, K = x.shape
    w = weight(kind, wt)
    mx = max(1.0, pw) if kind == 'multi-label' else 1.0
    xe = torch.zeros_like(x) if x_err is None else x_err
    l, d = terms(kind, x, t, pw)
    gscale = w * gs / (N * K)
    G = mp.Bnd(d * gscale, abs(gscale) * (16 * mx * EPS32 + 0.25 * mx * xe))
    le = 32 * EPS32 * (l.abs() + 1) + d.abs() * xe + 0.125 * mx * xe * xe
    row = l.mean(1)
    row_e = le.mean(1) + C_ACC * (K + 8) * EPS32 * l.abs().mean(1)
    tot = w * row.mean()
    tot_e = abs(w) * (row_e.mean() + C_ACC * (N + 8) * EPS32 * row.abs().mean())
    return mp.Bnd(torch.cat([tot.view(1), row]), torch.cat([tot_e.view(1), row_e])), G


def check(got, b, what):
    """|got - ref| <= err elementwise, everything finite"""
    got = got.detach().double().cpu().reshape(b.ref.shape)
    assert torch.isfinite(got).all(), '%s: non-finite output' % what
    bad = (got - b.ref).abs() > b.err
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError('%s: %d of %d elements outside the bound; first flat %d: got %.9g ref %.9g bound %.3g' % (
            what, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), float(b.ref.reshape(-1)[i]),
            float(b.err.reshape(-1)[i])))
    return float(((got - b.ref).abs() / b.err.clamp_min(1e-300)).max())
