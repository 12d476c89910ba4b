"""Device time of the image half of the input pipeline (apa_preprocess_images: two launches, csrc/apa_images.hip)
on the workload's geometry, with HIP events around `reps` back-to-back calls on buffers that already live on the
device:

  N = 32 decoded 720x1280 frames, MAX_INPUT_IMAGE_SIZE 512 -> L 288x512, RESIZE_SIDE 480 -> A 480x853,
  random 448x448 crops, every second one flipped, float32 and bfloat16 output

and, for scale, the wall time of the same batch through the numpy float32 restatement (tests/_image_reference.py)
on the host cores of the same box (one process per core in use; the count is printed).  One JSON line per case.

    python tools/bench_preproc.py [--reps 20] [--batch 32] [--host-batch 32]
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor
from multiprocessing import get_context

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SRC_HW, MAX_WD, SIDE, CROP = (720, 1280), 512, 480, 448


def make_batch(n):
    import _image_reference as ir
    rs = np.random.RandomState(0)
    sizes = ir.image_aug_size(SRC_HW[0], SRC_HW[1], MAX_WD, SIDE)
    frames = [rs.randint(0, 256, size=(1,) + SRC_HW + (3,)).astype(np.uint8) for _ in range(n)]
    geoms = [ir.geom_row(SRC_HW[0], SRC_HW[1], sizes, (int(rs.randint(0, sizes[2] - CROP + 1)),
                                                       int(rs.randint(0, sizes[3] - CROP + 1))), (CROP, CROP), i % 2)
             for i in range(n)]
    return frames, geoms


def _host_one(args):
    import _image_reference as ir
    f, g = args
    out, _ = ir.preprocess(f, MAX_WD, SIDE, (g[4], g[5]), (g[6], g[7]), bool(g[8]))
    return float(out[0, 0, 0, 0])


def host_time(frames, geoms):
    cores = len(os.sched_getaffinity(0))
    workers = max(1, min(cores, int(os.environ.get('OMP_NUM_THREADS', cores)), len(frames)))
    with ProcessPoolExecutor(max_workers=workers, mp_context=get_context('fork')) as pool:
        list(pool.map(_host_one, zip(frames[:workers], geoms[:workers])))          # start the workers
        t0 = time.perf_counter()
        list(pool.map(_host_one, zip(frames, geoms)))
        dt = time.perf_counter() - t0
    return dict(case='host_numpy_restatement', batch=len(frames), processes=workers, cores_visible=cores,
                ms=round(dt * 1e3, 1), ms_per_image=round(dt * 1e3 / len(frames), 2))


def device_time(frames, geoms, reps, warmup=3):
    import torch
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    lib = cof.load_library()
    dev = torch.device('cuda:0')
    n = len(frames)
    hw = np.asarray([f.shape[1:3] for f in frames], dtype=np.int32)
    off = np.zeros((n,), dtype=np.int64)
    off[1:] = np.cumsum([f.size for f in frames[:-1]])
    src = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(dev)
    off_d, hw_d = torch.from_numpy(off).to(dev), torch.from_numpy(hw).to(dev)
    geom_d = torch.tensor(geoms, dtype=torch.int32, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    need = int(lib.apa_preprocess_images_workspace_bytes(n, 1, hw.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), MAX_WD))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.empty((n, 1, CROP, CROP, 3), dtype=dtype, device=dev)
        code = cof.APA_DTYPE_F32 if dtype == torch.float32 else cof.APA_DTYPE_BF16
        stream = torch.cuda.current_stream().cuda_stream

        def call():
            rc = lib.apa_preprocess_images(src.data_ptr(), src.numel(), off_d.data_ptr(), hw_d.data_ptr(),
                                           geom_d.data_ptr(), n, 1, MAX_WD, 128.0, out.data_ptr(), code,
                                           status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            assert rc == 0, lib.apa_last_error()
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            call()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / reps
        rows.append(dict(case='apa_preprocess_images', out=str(dtype).replace('torch.', ''), batch=n, reps=reps,
                         us=round(us, 1), us_per_image=round(us / n, 2), src_mb=round(src.numel() / 1e6, 1),
                         out_mb=round(out.numel() * out.element_size() / 1e6, 1), workspace_mb=round(need / 1e6, 1)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--host-batch', type=int, default=32)
    a = ap.parse_args()
    frames, geoms = make_batch(max(a.batch, a.host_batch))
    if a.host_batch > 0:                      # before torch is imported and the GPU opened: the workers are forked
        print(json.dumps(host_time(frames[:a.host_batch], geoms[:a.host_batch])), flush=True)
    for row in device_time(frames[:a.batch], geoms[:a.batch], max(a.reps, 20)):
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
