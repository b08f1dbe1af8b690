"""Backward of the separable filter family at 4 x 160^3 x 1 and 4 x 160^3 x 3: GaussianBlur (sigma 1 and 3) forward + backward with
respect to x, one stride-2 pass, the tap gradient at sigma 3, minmax_norm forward + backward -- each next to torch autograd on the eager
expression of the same math in the same process (F.conv1d on the transposed tensor; amin / amax / where).  Every case runs RUNS
times, each run the mean of ITERS iterations between two events: min / median / max over the runs.  Also the stride-1 dx pass against
the forward pass of the same shape in the same run (the expectation: equal, they run on the same kernels), with the run-to-run spread.

    python tools/filter_bwd_bench.py [--out profiles/filter_bwd/filter_bwd_bench.jsonl] [--size 160] [--channels 1,3] [--append]

The eager expressions go through MIOpen, whose first call of every new convolution shape searches and compiles for minutes; the
product's own time of a case is printed before its eager twin starts.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neurite_amd as ne                      # noqa: E402
from neurite_amd import _lib                  # noqa: E402

RUNS, ITERS = 5, 5


def timeit(fn):
    """[min, median, max] ms over RUNS runs of ITERS iterations"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / ITERS)
    return [round(float(v), 4) for v in (np.min(out), np.median(out), np.max(out))]


def eager_pass(x, k, ax, stride=1):
    """one SAME pass along spatial axis `ax` of [B, *S, C] by F.conv1d on the transposed tensor"""
    n, W = x.shape[ax + 1], k.numel()
    o = -(-n // stride)
    total = max((o - 1) * stride + W - n, 0)
    rows = x.movedim(ax + 1, -1)
    lead = rows.shape[:-1]
    rows = TF.pad(rows.reshape(-1, 1, n), (total // 2, total - total // 2))
    return TF.conv1d(rows, k.reshape(1, 1, W), stride=stride).reshape(*lead, -1).movedim(-1, ax + 1)


def eager_minmax(x, axes):
    mn, mx = x.amin(axes, keepdim=True), x.amax(axes, keepdim=True)
    den = mx - mn
    return torch.where(den != 0, (x - mn) / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'filter_bwd', 'filter_bwd_bench.jsonl'))
    ap.add_argument('--size', type=int, default=160)
    ap.add_argument('--channels', default='1,3')
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    S, B = args.size, 4
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')

    def record(op, C, ours, eager, **extra):
        ours = timeit(ours) if callable(ours) else ours
        print('# %s C=%d: %s ms' % (op, C, ours), flush=True)
        eager = timeit(eager) if callable(eager) else eager
        row = dict(op=op, shape=[B, S, S, S, C], ms_min_med_max=ours, eager_ms_min_med_max=eager, runs=RUNS, iters=ITERS, **extra)
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + '\n')
        out.flush()

    for C in [int(c) for c in args.channels.split(',')]:
        x = torch.randn(B, S, S, S, C, device=dev, requires_grad=True)
        g = torch.randn(B, S, S, S, C, device=dev)
        for sigma in (1.0, 3.0):
            blur = ne.layers.GaussianBlur(sigma=sigma)
            taps = ne.utils.gaussian_kernel([sigma] * 3, separate=True)
            taps = [t.to(dev) for t in taps]

            def ours():
                torch.autograd.grad(blur(x), x, g)

            def eager():
                y = x
                for ax in range(3):
                    y = eager_pass(y, taps[ax], ax)
                torch.autograd.grad(y, x, g)
            record('GaussianBlur sigma=%g fwd+bwd(x) W=%d' % (sigma, taps[0].numel()), C, ours, eager)
        # the stride-1 dx pass against the forward pass of the same shape, per axis, through the C ABI (no allocation in the loop)
        k = ne.utils.gaussian_kernel([3.0], separate=True)
        k = (k[0] if isinstance(k, (list, tuple)) else k).to(dev)
        W = k.numel()
        xd, y = x.detach(), torch.empty_like(g)
        for ax, name in ((1, 'x'), (2, 'y'), (3, 'z')):
            outer, n, inner = int(np.prod(x.shape[:ax])), S, int(np.prod(x.shape[ax + 1:]))
            fwd = timeit(lambda: _lib.call(dev, 'nrt_conv1d_axis_f32', _lib.ptr(xd), _lib.ptr(k), _lib.ptr(y), outer, n, inner, n, W, 1, 1,
                                           (W - 1) // 2))
            bwd = timeit(lambda: _lib.call(dev, 'nrt_conv1d_axis_bwd_f32', _lib.ptr(g), _lib.ptr(k), _lib.ptr(y), outer, n, inner, n, W,
                                           1, 1, (W - 1) // 2))
            record('stride-1 dx pass %s sigma=3 vs forward pass' % name, C, bwd, None, forward_ms_min_med_max=fwd,
                   dx_over_forward_median=round(bwd[1] / fwd[1], 3), forward_spread=round(fwd[2] / fwd[0], 3),
                   dx_spread=round(bwd[2] / bwd[0], 3))
        k5 = torch.randn(5, device=dev)
        g2 = g[:, :, :S // 2].contiguous()
        record('one stride-2 pass (axis y, W=5) fwd+bwd(x)', C,
               lambda: torch.autograd.grad(ne.utils.separable_conv(x, k5, axis=1, batched=True, strides=2), x, g2),
               lambda: torch.autograd.grad(eager_pass(x, k5, 1, 2), x, g2))
        kg = k.clone().requires_grad_(True)
        record('tap gradient sigma=3 (axis y, W=%d) fwd+bwd(taps)' % W, C,
               lambda: torch.autograd.grad(ne.utils.separable_conv(xd, kg, axis=1, batched=True), kg, g),
               lambda: torch.autograd.grad(eager_pass(xd, kg, 1), kg, g))
        axes = (1, 2, 3, 4) if C == 1 else (1, 2, 3)
        record('minmax_norm axis=%s fwd+bwd' % (axes,), C,
               lambda: torch.autograd.grad(ne.utils.minmax_norm(x, axis=axes), x, g),
               lambda: torch.autograd.grad(eager_minmax(x, axes), x, g))
    out.close()


if __name__ == '__main__':
    main()
