#!/usr/bin/env python
"""bench.py -- attentional-pooling head, forward + loss + backward, on synthetic conv5 features.

Metric (BASELINE.json): images/sec attn-pool fwd+bwd, N x 14 x 14 x 2048, 393 classes.
One "step" = one pass of the hot path over one batch that is already resident in HBM:
    apa_attn_pool_fwd  ->  apa_softmax_xent_fwd_bwd  ->  apa_attn_pool_bwd  [-> RCCL all-reduce of
    the flat head-gradient bucket when world_size > 1]
Workload (cfg 002 semantics): per-GPU batch 32, 14x14x2048 fp32 features, K=393,
class-agnostic bottom-up map (M=1), training-mode dropout keep=0.2 (nets_factory.py:145).

    python bench.py --gpus 1 --steps 200 --warmup 20            # the headline only
    python bench.py --gpus 1 --steps 200 --warmup 20 --full     # + roofline, extra, cpu_baseline
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

What is timed, and how:
  * The feature map and its gradient are ROTATED over R buffer sets with R * (X + dX) > 256 MiB (the
    Infinity Cache), so a step never finds its X in cache from the previous step: the forward pass
    reads X from HBM.  (Inside one step the backward pass re-reads the X its own forward pass streamed
    a few microseconds earlier; what the cache keeps of it is part of the real workload.)
  * Exactly --steps steps are timed, as one uninterrupted run after --warmup untimed ones (barrier +
    synchronize on both sides).  HIP events cut the run into --repeats consecutive pieces; `ms_per_step` /
    `value` come from the MEDIAN piece (max over ranks).  `steps`, `warmup` echo the flags, `timed_steps`
    counts the timed steps, `repeats` the pieces and `timed_ms_total` is the wall time of the whole run.
  * --dump-outputs DIR: after the timed run, what its last step computed (logits, attention map, loss,
    dX and the weight gradients, as a caller of the step receives them) is written as DIR/<name>.npy in
    float32, at most 64 MB in all.  The inputs are seeded, so two builds can be compared output for output.
  * A plain run stops there: set-up, warm-up, the timed steps, --dump-outputs and the result line.  Everything
    else the benchmark measures takes runs of its own and comes with --full, after the headline:
  * `roofline` (--full): the dominant kernel (m1s_bwd_main_kernel: reads X once, writes dX once).  Its
    duration is read live, over further steps, from a HIP event pair the library attaches to that
    dispatch (hipExtLaunchKernel start / stop events, on the launch stream).  NOTHING is subtracted:
    the pair reads ~1.2 us above rocprofv3's begin -> end of the same kernel (19.5 vs 18.3 us at
    N = 32, 1-3 % at N = 512: profiles/r02_summary.md, r02_n512_summary.md), so `frac` is the
    conservative figure; `roofline.rocprofv3` quotes the committed profiler average of this exact
    workload next to it, labelled with its source file.
  * `extra` (--full): the other BASELINE configs on the same driver-timed line (cfg 002 eval step, cfg 003
    bf16 training step, HMDB-51 per-class bf16 training step, and the headline step at N = 512,
    1.6 GB of features per pass: far outside every cache).
  * `cpu_baseline` (--full): the literal op-by-op PyTorch-CPU restatement of the reference graph (oracle/, a
    *port* -- TF1 cannot run here) timed on this box's host cores.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6290 GB/s measured copy
L3_BYTES = 256 << 20    # Infinity Cache


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200, help='number of timed steps of the headline workload')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32, help='per-GPU batch (cfg 002: 32)')
    ap.add_argument('--hw', type=int, default=14)
    ap.add_argument('--channels', type=int, default=2048)
    ap.add_argument('--classes', type=int, default=393)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--keep-prob', type=float, default=0.2)
    ap.add_argument('--eval-mode', action='store_true', help='no dropout (is_training=False)')
    ap.add_argument('--softmax-att', action='store_true')
    ap.add_argument('--rotate', type=int, default=0,
                    help='number of (X, dX) buffer sets the steps cycle through; 0 = smallest R >= 3 with '
                         'R * (X + dX) >= 1.5 x 256 MiB (Infinity Cache); 1 = the same buffers every step')
    ap.add_argument('--full', action='store_true',
                    help='after the headline, also measure what takes runs of its own: per-kernel durations and '
                         'roofline figures (`roofline`, `roofline_fwd`), the other BASELINE configs (`extra`) and '
                         'the CPU baseline (`cpu_baseline`).  Off: the run times the headline steps and nothing else')
    ap.add_argument('--min-ms', type=float, default=50.0,
                    help='`extra` workloads (--full): repeat their timed loop until this much device time has been '
                         'measured')
    ap.add_argument('--repeats', type=int, default=5,
                    help='headline: the --steps timed steps are split into this many event-timed pieces; `extra` '
                         'workloads: minimum number of timed loops (median reported either way)')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='after the timed steps, write the outputs of the last one as DIR/<name>.npy (float32, '
                         '<= 64 MB in all)')
    ap.add_argument('--graph', action='store_true',
                    help='capture the step in a hipGraph (measured: replay overhead makes it slower than '
                         'eager launches for this step, so off by default); implies --rotate 1')
    ap.add_argument('--overlap', default='auto', choices=['auto', 'on', 'off'],
                    help='N > 1: reduce dWt|dbt (99.7 %% of the bytes) on a communication stream with its own '
                         'RCCL communicator, between the grad-ready and td-weights-ready hooks (apa_hooks), '
                         'and only dWa|dba (8 KB) on the compute stream (deploy.OverlappedGradientSum).  auto (with '
                         '--comm rccl) = decided by a PROBE at start-up: a few steps are timed with each schedule on '
                         'this node (max over ranks) and the faster one is kept')
    ap.add_argument('--comm', default='rccl', choices=['rccl', 'torch', 'gloo'],
                    help='N > 1 gradient sum: direct in-stream ncclAllReduce through librccl (default), '
                         'torch.distributed.all_reduce over RCCL, or over gloo (host-staged; lets two ranks '
                         'share ONE GPU so the whole N > 1 flow can be exercised on a single-GPU box -- a '
                         'functional check, not a performance path)')
    ap.add_argument('--force-dist', action='store_true',
                    help='run the N > 1 code path (RCCL group, side stream, split all-reduce) on one GPU')
    ap.add_argument('--relu-input', action='store_true',
                    help='APA_FLAG_RELU_INPUT: feed the pre-activation map and let the op apply the backbone\'s '
                         'last ReLU on the fly in both passes')
    ap.add_argument('--per-op-calls', action='store_true',
                    help='drive the step as three separately marshalled calls instead of one '
                         'apa_attn_head_train_step call: same kernels, more host time per step')
    ap.add_argument('--iter-size', type=int, default=2,
                    help='--full, extra.cfg002_train_iter_size: TRAIN.ITER_SIZE micro-batches per update (the cfg '
                         '002 / 003 YAMLs say 2), run side by side on separate streams (deploy.OverlappedMicroBatches) '
                         'and, as the yardstick, one after the other; 1 = skip')
    ap.add_argument('--no-extra', action='store_true', help='--full: skip the `extra` workloads')
    ap.add_argument('--extra-only', default='',
                    help='--full: comma-separated subset of the extra workloads (experiments)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full: skip the CPU baseline')
    ap.add_argument('--cpu-seconds', type=float, default=10.0, help='--full: timed seconds of the CPU baseline')
    ap.add_argument('--traffic-bytes', type=float, default=None,
                    help='--full: HBM bytes per launch of the dominant kernel from a separate rocprofv3 --pmc run')
    return ap.parse_args()


def cpu_baseline(args, seconds):
    """Literal reference formulation (materialises T = X' . Wt like the TF graph) on host cores."""
    from oracle import attn_pool_oracle as orc
    g = torch.Generator().manual_seed(42)
    N, H, C, K = args.batch, args.hw, args.channels, args.classes
    X = torch.relu(torch.randn(N, H, H, C, generator=g)).requires_grad_(True)
    Wa = (torch.randn(C, 1, generator=g) / C ** 0.5).requires_grad_(True)
    ba = torch.zeros(1, requires_grad=True)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).requires_grad_(True)
    bt = torch.zeros(K, requires_grad=True)
    labels = torch.randint(0, K, (N,), generator=g)
    train = not args.eval_mode
    mask = (torch.rand(N, H, H, C, generator=g) < args.keep_prob) if train else None
    flags = orc.AttnFlags(softmax_att=args.softmax_att)

    def it():
        for t in (X, Wa, ba, Wt, bt):
            t.grad = None
        logits, _ = orc.attentional_pooling(X, None, None, [Wa], [ba], [Wt], [bt], flags,
                                            is_training=train, keep_prob=args.keep_prob,
                                            dropout_mask=mask)
        orc.action_softmax_xent(logits, labels, K).backward()

    # 256 MKL threads on a 256-core box thrash on this problem size: probe a few thread counts
    # (best of 3 iterations each, after one untimed) and keep the fastest; `cores` reports that count
    best_t, best_thr, probes = None, None, 3
    for thr in sorted({min(os.cpu_count(), c) for c in (8, 16, 32, 64, 128)}):
        torch.set_num_threads(thr)
        it()
        dt = None
        for _ in range(probes):
            t0 = time.perf_counter()
            it()
            d = time.perf_counter() - t0
            dt = d if dt is None else min(dt, d)
        if best_t is None or dt < best_t:
            best_t, best_thr = dt, thr
    torch.set_num_threads(best_thr)
    n, t0 = 0, time.perf_counter()
    while True:
        it()
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds and n >= 3:
            break
    return {'value': round(N * n / el, 2), 'unit': 'images/sec', 'cores': best_thr,
            'kind': 'port',
            'sample': '{} iterations ({:.1f} s) of the same workload (N={}, {}x{}x{}, K={}, fp32, '
                      'literal [N,P,K] top-down formulation, torch {} CPU); {} threads chosen by a best-of-{} '
                      'probe over 8..128 threads on a {}-core host'.format(
                          n, el, N, H, H, C, K, torch.__version__, best_thr, probes, os.cpu_count())}


def _claim_stdout():
    """stdout must carry exactly one JSON line, but gloo ('[Gloo] Rank 0 is connected ...') and RCCL
    ('RCCL version : ...', 'Librccl path : ...') print banners through C stdio, some of them only
    flushed at exit.  Point fd 1 at stderr for the whole run and keep a private handle on the real
    stdout for the result line."""
    sys.stdout.flush()
    real = os.fdopen(os.dup(1), 'w')
    os.dup2(2, 1)
    return real


def _self_launch(n):
    """`python bench.py --gpus N` with no launcher around it: start N ranks of this same command under
    torch.distributed.run on a free loopback port (the line the module docstring shows) and return its
    exit status.  The ranks inherit this process's stdout, so rank 0's single JSON line lands where the
    caller expects it; the launcher's own chatter goes to stderr."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC only on these hosts (RCCL needs it)
    env.setdefault('OMP_NUM_THREADS', '8')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print('bench.py: launching {} ranks: {}'.format(n, ' '.join(cmd)), file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


class HeadWorkload:
    """The cfg 002 training step on `rotate` buffer sets: one HeadTrainStep per (X, dX) set, every
    other buffer (weights, gradient bucket, workspace, dropout counter) shared."""

    def __init__(self, cof, args, dev, rank, world, N, rotate, hooks=None):
        H, C, K = args.hw, args.channels, args.classes
        P = H * H
        self.N, self.P, self.C, self.K = N, P, C, K
        tdtype = torch.float32 if args.dtype == 'f32' else torch.bfloat16
        self.esz = 4 if args.dtype == 'f32' else 2
        if rotate <= 0:
            per_set = 2 * N * P * C * self.esz
            rotate = max(3, -(-int(1.5 * L3_BYTES) // per_set))
        self.rotate = rotate
        g = torch.Generator(device=dev).manual_seed(42 + rank)    # cfg.RNG_SEED = 42
        gw = torch.Generator(device='cpu').manual_seed(42)         # replicated weights
        self.Wa = (torch.randn(C, 1, generator=gw) / C ** 0.5).to(dev)
        self.ba = torch.zeros(1, device=dev)
        self.Wt = (torch.randn(C, K, generator=gw) / C ** 0.5).to(dev)
        self.bt = torch.zeros(K, device=dev)
        self.labels = torch.randint(0, K, (N,), generator=gw).to(dev)
        train = not args.eval_mode
        self.flags = cof.attn_flags(args.softmax_att, False, train, relu_input=args.relu_input)
        self.keep = args.keep_prob if train else 1.0
        # flat fp32 gradient bucket [dWa | dba | dWt | dbt]: one all-reduce per step, no packing copy
        sizes = [C * 1, 1, C * K, K]
        self.bucket = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        views, o = [], 0
        for s in sizes:
            views.append(self.bucket[o:o + s])
            o += s
        self.dWa, self.dba, self.dWt, self.dbt = views[0].view(C, 1), views[1], views[2].view(C, K), views[3]
        self.ws = torch.empty((cof.attn_pool_workspace_bytes(N, P, C, C, K, 1, self.flags),),
                              dtype=torch.uint8, device=dev)
        self.grad_scale = 1.0 / world               # model_deploy.py:223-225: clone loss / num_clones
        # dropout step counter in HBM: read by the kernels, advanced by the backward call, so every
        # step (and every hipGraph replay) draws a fresh mask like a fresh tf.nn.dropout per sess.run
        self.rng_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self.X, self.dX, self.steppers = [], [], []
        for _ in range(rotate):
            x = torch.randn(N, P, C, generator=g, device=dev)
            x = (x if args.relu_input else torch.relu(x)).to(tdtype)
            dx = torch.empty_like(x)
            self.X.append(x)
            self.dX.append(dx)
            # one foreign call per step (apa_attn_head_train_step = the three entry points back to
            # back, arguments marshalled once): keeps the host ahead of the ~50 us step on any CPU
            self.steppers.append(None if args.per_op_calls else cof.HeadTrainStep(
                x, x, self.Wa, self.ba, self.Wt, self.bt, self.labels,
                (dx, None, self.dWa, self.dba, self.dWt, self.dbt), flags=self.flags, keep_prob=self.keep,
                seed=42, offset=self.rng_ctr, grad_scale=self.grad_scale, workspace=self.ws, hooks=hooks))
        self.cof = cof
        self.hooks = hooks
        self.i = 0
        self._last = None

    def last_outputs(self):
        """What a caller of the step received from the last one: forward outputs, loss and every gradient."""
        r = (self.i - 1) % self.rotate
        st = self.steppers[r]
        logits, att, loss = (st.logits, st.att, st.loss) if st is not None else self._last
        return {'logits': logits, 'att': att, 'loss': loss, 'dX': self.dX[r], 'dWa': self.dWa, 'dba': self.dba,
                'dWt': self.dWt, 'dbt': self.dbt}

    def compute(self, hooks=None):
        r = self.i % self.rotate
        self.i += 1
        st = self.steppers[r]
        if st is not None:
            st.run(hooks=hooks)
            return
        cof, X, h = self.cof, self.X[r], (hooks if hooks is not None else self.hooks)
        logits, att, zsave, abar, _, _ = cof.attn_pool_fwd(X, X, self.Wa, self.ba, self.Wt, self.bt,
                                                           flags=self.flags, keep_prob=self.keep, seed=42,
                                                           offset=self.rng_ctr, workspace=self.ws, hooks=h)
        lossbuf, G, _, _ = cof.softmax_xent_fwd_bwd(logits, self.labels, grad_scale=self.grad_scale)
        self._last = (logits, att, lossbuf)
        cof.attn_pool_bwd(X, X, self.Wa, self.ba, self.Wt, self.bt, att, zsave, abar, G, flags=self.flags,
                          keep_prob=self.keep, seed=42, offset=self.rng_ctr, workspace=self.ws,
                          out=(self.dX[r], None, self.dWa, self.dba, self.dWt, self.dbt), hooks=h)


class IterSizeWorkload:
    """One UPDATE of the reference recipe: TRAIN.ITER_SIZE micro-batches of the headline step (per-GPU batch N each)
    whose gradients are summed and divided by ITER_SIZE (src/train.py:529-566).  Lane l has its own gradient
    bucket, workspace and dropout counter; the feature maps rotate over the same kind of buffer sets as the
    headline workload.  `run_overlapped` puts the lanes on separate HIP streams (deploy.OverlappedMicroBatches),
    `run_sequential` runs them back to back on one stream; same kernels and results either way."""

    def __init__(self, cof, args, dev, N, lanes):
        from attentionalpoolingaction_amd import deploy
        H, C, K = args.hw, args.channels, args.classes
        P = H * H
        self.N, self.lanes = N, lanes
        tdtype = torch.float32 if args.dtype == 'f32' else torch.bfloat16
        esz = 4 if args.dtype == 'f32' else 2
        per_set = 2 * N * P * C * esz
        self.rotate = max(2 * lanes + 1, -(-int(1.5 * L3_BYTES) // per_set))
        g = torch.Generator(device=dev).manual_seed(42)
        gw = torch.Generator(device='cpu').manual_seed(42)
        self.Wa = (torch.randn(C, 1, generator=gw) / C ** 0.5).to(dev)
        self.ba = torch.zeros(1, device=dev)
        self.Wt = (torch.randn(C, K, generator=gw) / C ** 0.5).to(dev)
        self.bt = torch.zeros(K, device=dev)
        self.labels = [torch.randint(0, K, (N,), generator=gw).to(dev) for _ in range(lanes)]
        self.flags = cof.attn_flags(args.softmax_att, False, True)
        sizes = [C, 1, C * K, K]
        self.bucket = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        self.lane_buckets = [torch.zeros_like(self.bucket) for _ in range(lanes)]
        self.ws = [torch.empty((cof.attn_pool_workspace_bytes(N, P, C, C, K, 1, self.flags),), dtype=torch.uint8,
                               device=dev) for _ in range(lanes)]
        self.ctr = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(lanes)]
        self.X = [torch.relu(torch.randn(N, P, C, generator=g, device=dev)).to(tdtype) for _ in range(self.rotate)]
        self.dX = [torch.empty_like(x) for x in self.X]
        self._steppers = {}
        self.cof, self.args, self.sizes = cof, args, sizes
        self.sched = deploy.OverlappedMicroBatches([self._stepper(l, l) for l in range(lanes)], self.lane_buckets,
                                                   self.bucket, dev)
        self.i = 0

    def _stepper(self, s, lane):
        if (s, lane) not in self._steppers:
            C, K = self.args.channels, self.args.classes
            b, o, v = self.lane_buckets[lane], 0, []
            for n in self.sizes:
                v.append(b[o:o + n])
                o += n
            self._steppers[(s, lane)] = self.cof.HeadTrainStep(
                self.X[s], self.X[s], self.Wa, self.ba, self.Wt, self.bt, self.labels[lane],
                (self.dX[s], None, v[0].view(C, 1), v[1], v[2].view(C, K), v[3]), flags=self.flags,
                keep_prob=self.args.keep_prob, seed=42 + lane, offset=self.ctr[lane], workspace=self.ws[lane])
        return self._steppers[(s, lane)]

    def _next(self):
        st = [self._stepper((self.i * self.lanes + l) % self.rotate, l) for l in range(self.lanes)]
        self.i += 1
        return st

    def run_overlapped(self):
        self.sched.run(self._next())

    def run_sequential(self):
        self.sched.run_sequential(self._next())


def timed_loops(step, barrier, steps, min_ms, repeats, reduce_max):
    """>= `repeats` loops of `steps` steps, each bracketed by barrier(); until >= min_ms in total.
    Every rank takes the same number of loops (the per-loop time is MAX-reduced over ranks)."""
    per, total, enq = [], 0.0, []
    while True:
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        t_enq = time.perf_counter() - t0        # host time to enqueue the steps (no device wait)
        barrier()
        dt = reduce_max(time.perf_counter() - t0)
        per.append(dt / steps)
        enq.append(t_enq / steps)
        total += dt
        if (len(per) >= repeats and total >= min_ms * 1e-3) or len(per) >= 400:
            break
    return per, enq


def timed_steps(step, barrier, steps, pieces, reduce_max):
    """Exactly `steps` steps as one run between two barriers, cut into `pieces` consecutive pieces by HIP events
    on the launch stream (no synchronisation inside the run).  Returns the seconds per step of every piece (max
    over ranks), the wall time of the whole run (max over ranks) and the host's enqueue time per step."""
    pieces = max(1, min(pieces, steps))
    sizes = [steps // pieces + (1 if i < steps % pieces else 0) for i in range(pieces)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(pieces + 1)]
    barrier()
    t0 = time.perf_counter()
    ev[0].record()
    for i, n in enumerate(sizes):
        for _ in range(n):
            step()
        ev[i + 1].record()
    t_enq = time.perf_counter() - t0
    barrier()
    wall = reduce_max(time.perf_counter() - t0)
    per = [reduce_max(ev[i].elapsed_time(ev[i + 1]) * 1e-3) / n for i, n in enumerate(sizes)]
    return per, wall, t_enq / steps


def dump_outputs(arrays, out_dir, budget=64 * 1000 * 1000):
    """Write every array as out_dir/<name>.npy in float32, at most `budget` bytes in all.  Smallest first, each
    array is written whole if it fits its even share of the budget still left; otherwise a fixed sample of its
    flat elements (the first `share` of a randperm drawn from a generator seeded with 0, in index order) is
    written, the same elements on every run of the same shapes.  Returns {name: shape and count} for the line."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    items = sorted(arrays.items(), key=lambda kv: (kv[1].numel(), kv[0]))
    left = budget - 128 * len(items)            # .npy headers
    info = {}
    for i, (name, t) in enumerate(items):
        flat = t.detach().reshape(-1)
        share = left // (len(items) - i)
        if flat.numel() * 4 <= share:
            a = t.detach().float().cpu().numpy()
        else:
            g = torch.Generator(device=flat.device).manual_seed(0)
            idx = torch.randperm(flat.numel(), generator=g, device=flat.device)[:share // 4].sort().values
            a = flat[idx].float().cpu().numpy()
        np.save(os.path.join(out_dir, name + '.npy'), a)
        left -= a.nbytes
        info[name] = {'shape': list(t.shape), 'saved_elements': int(a.size)}
    return info


def kernel_times(cof, work, step_with_hooks, barrier, n, base_hooks=None):
    """Durations of the two streaming kernels over n live steps: dispatch begin -> end timestamps
    attached by hipExtLaunchKernel (see include/apa.h, apa_hooks.prof_*)."""
    timer = cof.KernelTimer(n, base=base_hooks)
    for i in range(n):
        step_with_hooks(timer.hooks(i))
    barrier()
    f, b = timer.fwd_elapsed_ms(), timer.bwd_elapsed_ms()
    timer.close()
    return f, b


def kernel_rooflines(args, cof, work, step, barrier, base_hooks, workload):
    """--full: `roofline` and `roofline_fwd` of the headline workload.  The two streaming kernels are timed over
    further live steps (eager launches) by the dispatch timestamps the library attaches; their algorithmic bytes
    over that time against the HBM peak, next to the committed profiler figures of exactly this workload."""
    N, P, C, esz = work.N, work.P, work.C, work.esz
    kt_steps = max(20, min(args.steps, 200))
    kf, kb = kernel_times(cof, work, step, barrier, kt_steps, base_hooks=base_hooks)
    kb_avg_ms, kf_avg_ms = sum(kb) / len(kb), sum(kf) / len(kf)
    alg_bytes = 2.0 * N * P * C * esz           # bwd main kernel: read X once + write dX once
    achieved = alg_bytes / (kb_avg_ms * 1e-3) / 1e9
    fwd_bytes = 1.0 * N * P * C * esz
    fwd_achieved = fwd_bytes / (kf_avg_ms * 1e-3) / 1e9

    # HBM traffic of the dominant kernel comes from separate rocprofv3 --pmc passes (they cannot run
    # inside this process): the newest committed summary collected on exactly this workload
    traffic, traffic_source = args.traffic_bytes, ('--traffic-bytes' if args.traffic_bytes is not None else None)
    if traffic is None and not args.softmax_att:
        import glob
        for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', '*_pmc_traffic.json')), reverse=True):
            try:
                pmc = json.load(open(f))
            except (OSError, ValueError):
                continue
            hit = [v for k, v in pmc.items() if 'bwd_main' in k and isinstance(v, dict)
                   and v.get('workload') == workload]
            if hit:
                traffic = hit[0]['hbm_bytes_per_launch']
                traffic_source = 'profiles/' + os.path.basename(f) + ' (rocprofv3 --pmc passes of this command)'
                break

    def rocprof_reference(kernel_tag, nbytes):
        """The committed rocprofv3 --kernel-trace --stats average of the same kernel on exactly this
        workload (profiles/<tag>_kernel_stats.csv + <tag>_bench_under_rocprof.log), for the reader who
        wants the bench line's event-based duration next to the profiler's: a file, labelled as such."""
        import csv
        import glob
        for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', '*_kernel_stats.csv')), reverse=True):
            log = f.replace('_kernel_stats.csv', '_bench_under_rocprof.log')
            try:
                if json.loads(open(log).read().strip().splitlines()[-1])['config']['workload'] != workload:
                    continue
                for r in csv.DictReader(open(f)):
                    if kernel_tag in r['Name']:
                        us = float(r['AverageNs']) / 1e3
                        return {'kernel_avg_us': round(us, 3), 'frac': round(nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                'source': 'profiles/' + os.path.basename(f)}
            except (OSError, ValueError, KeyError, IndexError):
                continue
        return None

    stream_kernel = (C % 1024 == 0 and args.dtype == 'f32') or (C == 2048)
    return {
        'roofline': {
            'bound': 'hbm',
            'kernel': 'm1s_bwd_main_kernel' if stream_kernel else 'm1_bwd_main_kernel',
            'achieved': round(achieved, 1),
            'peak': HBM_PEAK_GBS,
            'unit': 'GB/s',
            'frac': round(achieved / HBM_PEAK_GBS, 4),
            'traffic': traffic,
            'traffic_source': traffic_source,
            'alg_bytes_per_launch': alg_bytes,
            'kernel_avg_us': round(kb_avg_ms * 1e3, 3),
            'kernel_median_us': round(_median(kb) * 1e3, 3),
            'timer': 'hipExtLaunchKernel start/stop events around the dispatch, {} live steps, nothing '
                     'subtracted (reads ~1.2 us above rocprofv3\'s begin->end of the same kernel: '
                     'profiles/r03_summary.md)'.format(len(kb)),
            'rocprofv3': rocprof_reference('bwd_main', alg_bytes),
        },
        'roofline_fwd': {
            'bound': 'hbm',
            'kernel': 'm1s_pool_fwd_kernel' if stream_kernel else 'm1_pool_fwd_kernel',
            'achieved': round(fwd_achieved, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
            'frac': round(fwd_achieved / HBM_PEAK_GBS, 4), 'alg_bytes_per_launch': fwd_bytes,
            'kernel_avg_us': round(kf_avg_ms * 1e3, 3), 'kernel_median_us': round(_median(kf) * 1e3, 3),
            'rocprofv3': rocprof_reference('pool_fwd', fwd_bytes),
        },
    }


def main():
    args = parse_args()
    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` typed as is: become the launcher (one process per GPU, the same
        # command line the driver would use) and hand this process's stdout to rank 0's JSON line
        raise SystemExit(_self_launch(args.gpus))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit('bench.py --gpus {} started with WORLD_SIZE={}: the two must agree (one process per '
                         'GPU)'.format(args.gpus, world))
    if args.steps < 1:
        raise SystemExit('bench.py: --steps must be at least 1')
    real_stdout = _claim_stdout()
    assert torch.cuda.is_available(), 'bench.py needs an MI355X (no CPU fallback for the product path)'
    if args.comm == 'gloo':                      # ranks may share a GPU in this mode
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        if world == 1:
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('MASTER_PORT', '29531')
            os.environ.setdefault('RANK', '0')
            os.environ.setdefault('WORLD_SIZE', '1')
        if args.comm == 'torch':
            dist.init_process_group('nccl', device_id=dev)   # "nccl" == RCCL on ROCm
        else:
            os.environ.setdefault('GLOO_SOCKET_IFNAME', 'lo')   # single node: the hostname may not resolve
            dist.init_process_group('gloo')                  # bootstrap / barrier only; data goes over RCCL

    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    cof.load_library()

    N, H, C, K = args.batch, args.hw, args.channels, args.classes
    P = H * H
    if args.graph:
        args.rotate = 1

    # Data-parallel gradient sum (model_deploy.py:421-451).  dWt|dbt (99.7 % of the payload) are final
    # after the first kernel of the backward call: the library records `grad_ready` there and their
    # all-reduce starts on a side stream underneath the streaming pass; dWa|dba (8 KB) follow on the
    # main stream once the call is done.
    comm = comm_td = None
    comm_info = None
    bucket_numel = C + 1 + C * K + K
    if dist is not None and args.comm == 'rccl':
        from attentionalpoolingaction_amd import rccl
        ok = 1
        try:
            comm = rccl.RcclCommunicator(rank, max(world, 1), dev, group=None)
            comm.all_reduce_(torch.zeros(8, device=dev))      # first call builds the rings
            torch.cuda.synchronize()
        except Exception as e:                                 # noqa: BLE001 -- any failure -> fallback
            print('direct RCCL unavailable on rank {}: {}'.format(rank, e), file=sys.stderr)
            ok = 0
        flag = torch.tensor([ok], dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)            # every rank takes the same branch
        if int(flag.item()) == 0:                              # fall back to torch.distributed's RCCL
            if comm is not None:
                comm.close()
            comm = None
            args.comm = 'torch'
            dist.destroy_process_group()
            dist.init_process_group('nccl', device_id=dev)
        else:
            # What RCCL itself reports, and what the bucket's all-reduce costs on THIS node: the overlap decision is
            # taken from this measurement (every rank uses the slowest rank's figure), not from an estimate.
            if comm.count() != max(world, 1) or comm.user_rank() != rank:
                # fail fast and loudly: a communicator that does not span the launcher's ranks would time N private
                # one-rank "all-reduces" and print a scaling line that means nothing
                raise SystemExit('bench.py --gpus {}: RCCL reports {} rank(s) in the communicator and user rank {} for '
                                 'launcher rank {} -- ncclCommCount must equal WORLD_SIZE (one process per GPU, one '
                                 'communicator over all of them)'.format(args.gpus, comm.count(), comm.user_rank(),
                                                                         rank))
            ar_us = comm.measure_all_reduce_us(bucket_numel)
            t_ar = torch.tensor([ar_us], dtype=torch.float64)
            dist.all_reduce(t_ar, op=dist.ReduceOp.MAX)
            ar_us = float(t_ar.item())
            # --overlap auto: both schedules are built and a few steps of each are timed below (overlap_probe)
            want_overlap = args.overlap in ('on', 'auto') and not args.graph
            comm_info = {'ranks': comm.count(), 'user_rank': comm.user_rank(),
                         'allreduce_bucket_bytes': bucket_numel * 4, 'allreduce_us': round(ar_us, 2),
                         'overlap': 'on' if want_overlap else 'off',
                         'overlap_rule': '--overlap {}'.format(args.overlap)}
            if want_overlap:                                   # one communicator per stream
                comm_td = rccl.RcclCommunicator(rank, max(world, 1), dev, group=None)
                comm_td.all_reduce_(torch.zeros(8, device=dev))
                torch.cuda.synchronize()
    if dist is not None and comm is None:
        # torch.distributed transports (RCCL through torch, or gloo for the single-GPU functional check)
        buf = torch.zeros(bucket_numel, dtype=torch.float32, device=dev)
        for _ in range(3):
            dist.all_reduce(buf)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            dist.all_reduce(buf)
        torch.cuda.synchronize()
        t_ar = torch.tensor([(time.perf_counter() - t0) / 10 * 1e6], dtype=torch.float64,
                            device=dev if dist.get_backend() == 'nccl' else 'cpu')
        dist.all_reduce(t_ar, op=dist.ReduceOp.MAX)
        comm_info = {'ranks': dist.get_world_size(), 'user_rank': dist.get_rank(),
                     'allreduce_bucket_bytes': bucket_numel * 4, 'allreduce_us': round(float(t_ar.item()), 2),
                     'overlap': 'on' if args.overlap == 'on' and not args.graph else 'off',
                     'overlap_rule': 'torch.distributed transport: two async buckets only with --overlap on'}
        del buf

    # the overlapped schedule needs the bucket views before the workload exists: build the workload
    # first without hooks, then attach them to its steppers
    work = HeadWorkload(cof, args, dev, rank, world, N, args.rotate)
    bucket = work.bucket
    overlap = None
    bucket_att, bucket_td = bucket[:C + 1], bucket[C + 1:]
    if dist is not None and not args.graph and comm_td is not None:
        from attentionalpoolingaction_amd import deploy
        overlap = deploy.OverlappedGradientSum(bucket_att, bucket_td, comm, comm_td, dev)
        work.hooks = overlap.hooks
        for st in work.steppers:
            if st is not None:
                st.hooks = overlap.hooks
    torch_overlap = dist is not None and not args.graph and comm is None and args.overlap == 'on'

    def allreduce(t, stream=None, async_op=False):
        if comm is not None:
            comm.all_reduce_(t, stream)
            return None
        return dist.all_reduce(t, async_op=async_op)

    graph = None
    if args.graph:
        # the launches of a step are stream-ordered, allocation-free and argument-stable (the
        # dropout counter lives in HBM), so the whole step can be captured once in a hipGraph
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                work.compute()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            work.compute()

    def step(hooks=None):
        if graph is not None and hooks is None:
            graph.replay()
        else:
            work.compute(hooks)
        if overlap is not None:
            overlap.after_backward()
        elif torch_overlap:
            w_td = allreduce(bucket_td, async_op=True)
            w_att = allreduce(bucket_att, async_op=True)
            w_td.wait()                         # the main stream waits for both (no host block)
            w_att.wait()
        elif dist is not None:
            allreduce(bucket)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_max(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == 'nccl' else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    if overlap is not None and args.overlap == 'auto':
        # Which schedule is faster on THIS node is measured, not assumed (round 5; rounds 3-4 compared the measured
        # all-reduce with a constant from a one-rank run): 3 x 30 steps with the bucket reduced in-stream (no hooks)
        # against 3 x 30 steps of the two-stream schedule, median each, max over ranks; the faster one is kept.
        no_hooks = cof.make_hooks()
        from attentionalpoolingaction_amd import deploy as _deploy

        def _two():
            work.compute(None)
            overlap.after_backward()

        def _one():
            work.compute(no_hooks)
            allreduce(bucket)
        keep, us_two, us_one = _deploy.probe_overlap_schedule(_two, _one, barrier, reduce_max)
        comm_info['overlap'] = 'on' if keep else 'off'
        comm_info['overlap_rule'] = ('--overlap auto: probed at start-up, {:.1f} us/step with the two-stream schedule '
                                     'against {:.1f} us/step with the bucket reduced in-stream (30-step loops, median of 3, '
                                     'max over ranks); the faster one is kept'.format(us_two, us_one))
        comm_info['overlap_probe_us'] = {'two_streams': round(us_two, 2), 'in_stream': round(us_one, 2)}
        if not keep:
            overlap.close()
            overlap = None
            work.hooks = None
            for st in work.steppers:
                if st is not None:
                    st.hooks = None
    for _ in range(args.warmup):
        step()
    per, wall, enq = timed_steps(step, barrier, args.steps, args.repeats, reduce_max)
    sec = _median(per)
    print('host enqueue {:.1f} us/step, {:.1f} us/step (median of {} pieces, min {:.1f} max {:.1f}), {} steps in '
          '{:.3f} ms'.format(enq * 1e6, sec * 1e6, len(per), min(per) * 1e6, max(per) * 1e6, args.steps, wall * 1e3),
          file=sys.stderr)
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(work.last_outputs(), args.dump_outputs)

    esz = work.esz
    train = not args.eval_mode
    workload = ('cfg002 attentional-pooling head fwd + softmax-xent + bwd, per-GPU batch {} '
                'x {}x{}x{} {} features, K={}, M=1 (class-agnostic bottom-up map), {}; X/dX rotated over {} '
                'buffer sets ({:.0f} MB live)'.format(
                    N, H, H, C, args.dtype, K,
                    'dropout keep={}'.format(work.keep) if train else 'eval (no dropout)', work.rotate,
                    work.rotate * 2.0 * N * P * C * esz / 1e6))
    rooflines = None
    if args.full:
        rooflines = kernel_rooflines(args, cof, work, step, barrier, overlap.hooks if overlap is not None else None,
                                     workload)

    out = None
    if rank == 0:
        out = {
            'metric': 'images/sec attn-pool fwd+bwd, Nx14x14x2048, 393 classes',
            'value': round(N * world / sec, 1),
            'unit': 'images/sec',
            'n_gpus': world,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': round(sec * 1e3, 5),
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': None,
            'dtype': args.dtype,
            'data': 'synthetic',
            'timed_steps': args.steps,
            'repeats': len(per),
            'timed_ms_total': round(wall * 1e3, 3),
            'ms_per_step_min_max': [round(min(per) * 1e3, 5), round(max(per) * 1e3, 5)],
            'config': {
                'workload': workload,
                'global_batch': N * world,
                'parallelism': 'dp{}'.format(world),
                'softmax_att': bool(args.softmax_att),
                'hip_graph': graph is not None,
                'host_calls_per_step': 3 if args.per_op_calls else 1,
                'comm': None if dist is None else ('librccl ncclAllReduce, in-stream' if comm is not None
                                                   else 'torch.distributed ' + dist.get_backend()),
                'comm_detail': comm_info,
                'allreduce': ('none' if dist is None else
                              'dWt|dbt on a communication stream (own communicator) between the grad-ready and '
                              'td-weights-ready hooks; dWa|dba in-stream' if overlap is not None else
                              'two async buckets' if torch_overlap else 'one bucket, in-stream'),
            },
            'step_roofline_frac': round((3.0 * N * P * C * esz) / sec / 1e9 / HBM_PEAK_GBS, 4),
        }
        if rooflines is not None:
            out.update(rooflines)
        if dumped is not None:
            out['dump_outputs'] = {'dir': args.dump_outputs, 'arrays': dumped}

    # ---- --full: the other BASELINE configs, same process, same timing discipline (N = 1 only) ----
    if args.full and world == 1 and dist is None and not args.no_extra and out is not None:
        from tools import bench_dense as bd
        extra = {}
        del work
        torch.cuda.empty_cache()

        only = set(k for k in args.extra_only.split(',') if k)

        def run_extra(key, builder, **kw):
            if only and key not in only:
                return
            try:
                fn, info = builder(cof, dev, **kw)
                s, reps = bd.timed(fn, 50, 5, min_ms=args.min_ms, repeats=args.repeats)
                extra[key] = bd.report(info, s, reps)
            except Exception as e:                             # noqa: BLE001 -- report, do not lose the headline
                extra[key] = {'error': '{}: {}'.format(type(e).__name__, e)}
            torch.cuda.empty_cache()

        run_extra('cfg002_eval', bd.build_eval002, N=32, H=14, K=393, dtype='f32')
        run_extra('cfg003_bf16_train', bd.build_cfg003, N=32, H=14, K=393, dtype='bf16')
        run_extra('hmdb51_perclass_bf16_train', bd.build_perclass, N=32, H=14, K=51, dtype='bf16')
        run_extra('hmdb51_rank1_bf16_train', bd.build_rank1, N=32, H=14, K=51, dtype='bf16')
        # step + UPDATE: the optimiser launch that carries the relocated operand preparation, next to the plain launch
        # with per-step preparation, at TRAIN.ITER_SIZE 1 and 2 (src/train.py:90-94,529-566)
        for key, which in (('cfg003_bf16_update', 'cfg003'), ('hmdb51_perclass_update', 'perclass')):
            if only and key not in only:
                continue
            try:
                extra[key] = bd.run_update_pair(cof, dev, which, min_ms=args.min_ms, repeats=args.repeats)
            except Exception as e:                             # noqa: BLE001
                extra[key] = {'error': '{}: {}'.format(type(e).__name__, e)}
            torch.cuda.empty_cache()
        # the headline step far outside every cache: N = 512 (1.6 GB of features per pass).  TWO buffer sets since
        # round 6: the backward pass walks every block's pixels downwards and leaves their HEAD in the cache, which
        # a forward pass over the SAME map would meet first (measured: forward kernel 140 -> 134 us on one set) --
        # a training loop never re-reads a map, so the line must not either
        try:
            if only and 'cfg002_train_n512' not in only:
                raise KeyError('skipped')
            big = HeadWorkload(cof, args, dev, rank, world, 512, 2)
            for _ in range(3):
                big.compute()
            bper, _ = timed_loops(big.compute, torch.cuda.synchronize, 20, args.min_ms, args.repeats, lambda x: x)
            bf, bb = kernel_times(cof, big, big.compute, torch.cuda.synchronize, 20)
            bsec = _median(bper)
            bb_avg, bf_avg = sum(bb) / len(bb), sum(bf) / len(bf)
            extra['cfg002_train_n512'] = {
                'workload': 'the headline step at per-GPU batch 512 (1.6 GB of features per pass; X/dX alternate over 2 sets)',
                'images_per_sec': round(512 / bsec, 1), 'ms_per_step': round(bsec * 1e3, 5), 'repeats': len(bper),
                'step_roofline_frac': round(3.0 * 512 * P * C * esz / bsec / 1e9 / HBM_PEAK_GBS, 4),
                'roofline': {'bound': 'hbm', 'kernel': 'm1s_bwd_main_kernel', 'kernel_avg_us': round(bb_avg * 1e3, 2),
                             'achieved': round(2.0 * 512 * P * C * esz / (bb_avg * 1e-3) / 1e9, 1),
                             'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                             'frac': round(2.0 * 512 * P * C * esz / (bb_avg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
                'roofline_fwd': {'bound': 'hbm', 'kernel': 'm1s_pool_fwd_kernel', 'kernel_avg_us': round(bf_avg * 1e3, 2),
                                 'achieved': round(1.0 * 512 * P * C * esz / (bf_avg * 1e-3) / 1e9, 1),
                                 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                                 'frac': round(1.0 * 512 * P * C * esz / (bf_avg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}
            del big
        except KeyError:
            pass
        except Exception as e:                                 # noqa: BLE001
            extra['cfg002_train_n512'] = {'error': '{}: {}'.format(type(e).__name__, e)}
        torch.cuda.empty_cache()
        # the reference recipe's update: ITER_SIZE micro-batches of the headline step, side by side vs back to back
        if args.iter_size > 1 and not args.eval_mode and (not only or 'cfg002_train_iter_size' in only):
            try:
                it = IterSizeWorkload(cof, args, dev, N, args.iter_size)
                L = args.iter_size
                res = {}
                for name, fn in (('overlapped', it.run_overlapped), ('sequential', it.run_sequential)):
                    for _ in range(10):
                        fn()
                    p_, _ = timed_loops(fn, torch.cuda.synchronize, max(20, args.steps // L), args.min_ms, args.repeats,
                                        lambda x: x)
                    s_ = _median(p_)
                    res[name] = {'us_per_update': round(s_ * 1e6, 2), 'images_per_sec': round(L * N / s_, 1),
                                 'step_roofline_frac': round(L * 3.0 * N * P * C * esz / s_ / 1e9 / HBM_PEAK_GBS, 4),
                                 'repeats': len(p_)}
                it.sched.close()
                del it
                torch.cuda.empty_cache()
                # the same ITER_SIZE x N images as ONE call (per-GPU batch L*N, ITER_SIZE 1): what 288 GB of HBM allow
                one = HeadWorkload(cof, args, dev, rank, world, L * N, 0)
                for _ in range(10):
                    one.compute()
                p_, _ = timed_loops(one.compute, torch.cuda.synchronize, max(20, args.steps // L), args.min_ms,
                                    args.repeats, lambda x: x)
                s_ = _median(p_)
                res['one_pass'] = {'us_per_update': round(s_ * 1e6, 2), 'images_per_sec': round(L * N / s_, 1),
                                   'step_roofline_frac': round(L * 3.0 * N * P * C * esz / s_ / 1e9 / HBM_PEAK_GBS, 4),
                                   'repeats': len(p_)}
                del one
                extra['cfg002_train_iter_size'] = {
                    'workload': 'one UPDATE of the reference recipe (TRAIN.ITER_SIZE = {}: experiments/002...yaml, '
                                'src/train.py:529-566): {} micro-batches of the headline step (per-GPU batch {} each) + '
                                'gradient accumulation (one launch); overlapped = each micro-batch on its own HIP '
                                'stream, workspace, bucket and dropout counter (deploy.OverlappedMicroBatches); '
                                'sequential = back to back on one stream.  Same kernels, bit-identical gradients '
                                '(tests/test_head_gpu.py)'.format(L, L, N),
                    'iter_size': L, 'overlapped': res['overlapped'], 'sequential': res['sequential'],
                    'one_pass_batch_{}'.format(L * N): res['one_pass'],
                    'step_roofline_frac': res['overlapped']['step_roofline_frac'],
                    'note': 'step_roofline_frac = ITER_SIZE x 3 x N x P x C x 4 algorithmic bytes per update / time '
                            '/ 8 TB/s (the accumulation launch is inside the time, its 9.6 MB are not in the bytes); '
                            'one_pass = the same images as one call with ITER_SIZE 1 (mathematically the same update '
                            'for this head, not bit-identical: one reduction over all rows)'}
            except Exception as e:                             # noqa: BLE001
                extra['cfg002_train_iter_size'] = {'error': '{}: {}'.format(type(e).__name__, e)}
            torch.cuda.empty_cache()
        # BASELINE configs[1] / [2] END TO END: synthetic 448 x 448 images -> torch-ROCm ResNet-101 (channels-last)
        # -> HIP head -> loss (-> backward -> update): img/s of the real step and the head's share of it
        for key, which in (('cfg002_eval_e2e', 'eval002'), ('cfg003_train_e2e', 'train003')):
            if only and key not in only:
                continue
            try:
                from tools import bench_e2e
                extra[key] = bench_e2e.run(which, dev)
            except Exception as e:                             # noqa: BLE001
                extra[key] = {'error': '{}: {}'.format(type(e).__name__, e)}
            torch.cuda.empty_cache()
        out['extra'] = extra

    if rank == 0:
        if args.full and not args.no_cpu_baseline and world == 1:      # reported on rank 0 at N = 1 only
            out['cpu_baseline'] = cpu_baseline(args, args.cpu_seconds)
        print(json.dumps(out), file=real_stdout, flush=True)
    if dist is not None:
        torch.cuda.synchronize()
        if overlap is not None:
            overlap.close()
        for c in (comm, comm_td):
            if c is not None:
                c.close()
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
