"""Device time of the TRAIN.CLIP_GRADIENTS launches (cof.BoundClipByNorm: two launches, csrc/apa_clip.hip) on the two
gradient sets DESIGN.md section 4 reports, with HIP events around `reps` back-to-back runs:

  head      the cfg 003 head bucket (pose W1 | b1 | W2 | b2 | att W | b | td W | b at C = 2048, Cp = 768, J = 16,
            K = 393: 2.39 M floats), the regulariser on the weights (clone 0)
  resnet101 the 312 parameter tensors of resnet_v1.ResNetV1('resnet_v1_101') (42.5 M floats), regulariser on the
            conv weights

Traffic counted: pass 1 reads g (+ w where wd != 0), pass 2 reads g (+ w) and writes g.  HBM fraction against
8 TB/s.  One JSON line per case.

    python tools/bench_clip.py [--reps 50]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from attentionalpoolingaction_amd import resnet_v1                          # noqa: E402
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def head_shapes(C=2048, Cp=768, J=16, K=393):
    return [((C, Cp), True), ((Cp,), False), ((Cp, J), True), ((J,), False), ((Cp, 1), True), ((1,), False),
            ((C, K), True), ((K,), False)]


def resnet_shapes():
    m = resnet_v1.ResNetV1('resnet_v1_101')
    return [(tuple(p.shape), p.dim() == 4) for p in m.parameters()]


def run_case(name, shapes, dev, reps, wd=5e-4):
    sizes = [int(torch.Size(s).numel()) for s, _ in shapes]
    total = sum(sizes)
    flat = torch.randn(total, device=dev) * 1e-3
    wflat = torch.randn(total, device=dev)
    views, wviews, o = [], [], 0
    for n in sizes:
        views.append(flat[o:o + n])
        wviews.append(wflat[o:o + n])
        o += n
    wds = [wd if reg else 0.0 for _, reg in shapes]
    bound = cof.BoundClipByNorm(views, weights=wviews, wd=wds)
    for _ in range(5):
        bound.run(1.0)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        bound.run(1.0)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / reps
    n_w = sum(n for n, w in zip(sizes, wds) if w != 0.0)
    traffic = 4 * (3 * total + 2 * n_w)
    return dict(case=name, segments=len(sizes), floats=total, chunks=bound.nchunks, us=round(us, 2),
                traffic_mb=round(traffic / 1e6, 1), hbm_floor_us=round(traffic / HBM_BYTES_PER_S * 1e6, 2),
                hbm_fraction=round(traffic / HBM_BYTES_PER_S / (us * 1e-6), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for name, shapes in (('head_cfg003', head_shapes()), ('resnet101', resnet_shapes())):
        print(json.dumps(run_case(name, shapes, dev, a.reps)))


if __name__ == '__main__':
    main()
