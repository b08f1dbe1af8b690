"""
Timing of the dense kernels (csrc/dense.hip) against torch.matmul on the same tensors, at the shapes of the auto-encoder bottleneck.

    python tools/dense_bench.py [--reps 20] [--out profiles/dense/dense_bench.jsonl] [--cases NAME,...]
    python tools/dense_bench.py --dry       # CPU rehearsal: arguments, shapes, byte counts; measures nothing

Cases: 256 000 -> 512 (the encoder side of a five-level 160^3 network), 512 -> 256 000 (its decoder side), 32 768 -> 128 and
128 -> 32 768, each at batch 1, 4 and 16, forward and backward (gx, gw and gbias in one call).  The driver starts one child process
per case (`--case NAME`), each under a time limit of its own, and stops at the first child that fails or runs out of time.  A child
compares the kernel with torch first (relative error in the record), then times, with device events, the kernel and torch alternated
inside every repetition after a warm-up of both, and appends one JSON line: median / min / max ms of each, the share of the 8 TB/s HBM
peak that 4 * in * out bytes (W once; for the backward twice: read for gx, written as gw) over the median come to, the ratio
kernel / torch, and the library build id.  A time needs a GPU: without one the tool fails.
"""

import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurite_amd import _lib                                                                       # noqa: E402

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 120
SHAPES = [(256000, 512), (512, 256000), (32768, 128), (128, 32768)]
CASES = {'%s_%dto%d_b%d' % (d, i, o, b): (d, b, i, o) for i, o in SHAPES for b in (1, 4, 16) for d in ('fwd', 'bwd')}


def w_bytes(direction, cin, cout):
    return 4 * cin * cout * (1 if direction == 'fwd' else 2)


def run_case(name, reps):
    direction, B, cin, cout = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('dense_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    lib = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, cin), generator=g, device=dev)
    w = torch.randn((cin, cout), generator=g, device=dev) / cin ** 0.5
    bias = torch.randn((cout,), generator=g, device=dev)
    go = torch.randn((B, cout), generator=g, device=dev)
    n = lib.nrt_dense_workspace_bytes(B, cin, cout, 0)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    if direction == 'fwd':
        y = torch.empty((B, cout), device=dev)

        def kernel():
            _lib.check(lib.nrt_dense_f32(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), B, cin, cout, 0, 0, _lib.ptr(ws), n, st))
            return (y,)

        def eager():
            return (torch.addmm(bias, x, w),)
    else:
        gx, gw, gb = torch.empty_like(x), torch.empty_like(w), torch.empty_like(bias)

        def kernel():
            _lib.check(lib.nrt_dense_bwd_f32(_lib.ptr(go), _lib.ptr(x), _lib.ptr(w), _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), B, cin, cout,
                                             0, _lib.ptr(ws), n, st))
            return gx, gw, gb

        def eager():
            return torch.matmul(go, w.t()), torch.matmul(x.t(), go), go.sum(0)
    rel = 0.0
    for a, b in zip(kernel(), eager()):
        rel = max(rel, float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)))
    for _ in range(3):
        kernel()
        eager()
    torch.cuda.synchronize()
    times = {'kernel': [], 'torch': []}
    for _ in range(reps):
        for key, fn in (('kernel', kernel), ('torch', eager)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1))
    rec = {'case': name, 'direction': direction, 'batch': B, 'in': cin, 'out': cout, 'reps': reps, 'w_bytes': w_bytes(direction, cin, cout),
           'max_rel_diff_vs_torch': rel, 'build_id': lib.nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    for key, v in times.items():
        rec[key + '_ms'] = {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}
    rec['hbm_peak_share'] = rec['w_bytes'] / (rec['kernel_ms']['median'] * 1e-3) / HBM_PEAK
    rec['kernel_over_torch'] = rec['kernel_ms']['median'] / rec['torch_ms']['median']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dense', 'dense_bench.jsonl'))
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--case')
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case, args.reps)))
        return
    names = [c for c in args.cases.split(',') if c]
    for c in names:
        if c not in CASES:
            raise SystemExit('unknown case %s (known: %s)' % (c, ', '.join(CASES)))
    if args.dry:
        for c in names:
            d, B, cin, cout = CASES[c]
            print('%-28s batch %2d  %7d -> %7d  W traffic %8.1f MB  workspace %8.1f MB' % (
                c, B, cin, cout, w_bytes(d, cin, cout) / 1e6, _lib.lib().nrt_dense_workspace_bytes(B, cin, cout, 0) / 1e6))
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for c in names:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', c, '--reps', str(args.reps)], capture_output=True,
                               text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit('dense_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('dense_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        print('%-28s kernel %8.3f ms  torch %8.3f ms  %.2f of the HBM peak  kernel/torch %.2f' % (
            c, r['kernel_ms']['median'], r['torch_ms']['median'], r['hbm_peak_share'], r['kernel_over_torch']))


if __name__ == '__main__':
    main()
