"""
Timing of the global max kernels (csrc/globalmax.hip) against torch.amax and its autograd on the same tensors.

    python tools/global_max_bench.py [--reps 20] [--out profiles/global_max/global_max_bench.jsonl] [--cases NAME,...]
    python tools/global_max_bench.py --dry       # CPU rehearsal: arguments, shapes, byte counts; measures nothing

Cases: x [4, 160^3, C] for C = 2, 16 and 32, and the flattened [4, 160^3 * 16, 1] of design_dnn's lambda; each forward alone and
forward + backward.  The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at
the first child that fails or runs out of time.  A child compares the kernel with torch first (y must be equal; the gradients differ
where maxima tie, which random data does not do), then times, with device events, the kernel and torch alternated inside every
repetition after a warm-up of both, and then the soft Dice reduction (nrt_dice_soft_f32 through metrics.Dice) on two [4, 160^3, 16]
tensors in the same process, as the yardstick of a one-pass reduction on this device.  It appends one JSON line: median / min / max
ms of each, the bytes the algorithm needs (forward: x once; backward: x once more and gx once) over the kernel's median, the share
of the 8 TB/s HBM peak, the ratio to soft Dice's bytes/s, the ratio kernel / torch, and the library build id.  A time needs a GPU:
without one the tool fails.
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
import neurite_amd as ne                                                                           # noqa: E402
from neurite_amd import _lib                                                                       # noqa: E402
from neurite_amd import models                                                                     # noqa: E402

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 180
BATCH, VOX = 4, 160 ** 3
SHAPES = {'c2': (VOX, 2), 'c16': (VOX, 16), 'c32': (VOX, 32), 'flat16': (VOX * 16, 1)}
CASES = {'%s_%s' % (d, k): (d, v, c) for k, (v, c) in SHAPES.items() for d in ('fwd', 'fwdbwd')}


def needed_bytes(direction, v, c):
    return 4 * BATCH * v * c * (1 if direction == 'fwd' else 3)


def _time(fns, reps):
    times = {k: [] for k in fns}
    for _ in range(reps):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1))
    return {k: {'median': float(np.median(t)), 'min': float(np.min(t)), 'max': float(np.max(t))} for k, t in times.items()}


def run_case(name, reps):
    direction, v, c = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('global_max_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    lib = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((BATCH, v, c), generator=g, device=dev)
    go = torch.randn((BATCH, c), generator=g, device=dev)

    def kernel():
        if direction == 'fwd':
            with torch.no_grad():
                return (models._global_max(x),)
        xin = x.detach().requires_grad_(True)
        y = models._global_max(xin)
        return y.detach(), torch.autograd.grad(y, xin, go)[0]

    def eager():
        if direction == 'fwd':
            return (torch.amax(x, dim=1),)
        xin = x.detach().requires_grad_(True)
        y = torch.amax(xin, dim=1)
        return y.detach(), torch.autograd.grad(y, xin, go)[0]

    got, want = kernel(), eager()
    y_equal = bool(torch.equal(got[0], want[0]))
    gx_diff = float((got[1] - want[1]).abs().max()) if direction != 'fwd' else 0.0
    del got, want
    for _ in range(3):
        kernel()
        eager()
    torch.cuda.synchronize()
    ms = _time({'kernel': kernel, 'torch': eager}, reps)
    # the yardstick: soft Dice over two tensors of x's size (read once each), in this process
    a = torch.rand((BATCH, 160, 160, 160, 16), generator=g, device=dev)
    b = torch.rand(a.shape, generator=g, device=dev)
    dice = ne.metrics.Dice(check_input_limits=False)
    for _ in range(3):
        dice.dice(a, b)
    torch.cuda.synchronize()
    ms.update(_time({'dice': lambda: dice.dice(a, b)}, reps))
    rec = {'case': name, 'direction': direction, 'batch': BATCH, 'v': v, 'channels': c, 'reps': reps,
           'needed_bytes': needed_bytes(direction, v, c), 'y_equal_torch': y_equal, 'gx_max_abs_diff_vs_torch': gx_diff,
           'build_id': lib.nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    for k, t in ms.items():
        rec[k + '_ms'] = t
    rec['bytes_per_s'] = rec['needed_bytes'] / (rec['kernel_ms']['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    rec['dice_bytes_per_s'] = 2 * 4 * a.numel() / (rec['dice_ms']['median'] * 1e-3)
    rec['bytes_per_s_over_dice'] = rec['bytes_per_s'] / rec['dice_bytes_per_s']
    rec['kernel_over_torch'] = rec['kernel_ms']['median'] / rec['torch_ms']['median']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'global_max', 'global_max_bench.jsonl'))
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
            d, v, ch = CASES[c]
            print('%-16s [%d, %d, %d]  needed traffic %8.1f MB  workspace %6.1f KB' % (
                c, BATCH, v, ch, needed_bytes(d, v, ch) / 1e6, _lib.lib().nrt_global_max_workspace_bytes(BATCH, v, ch) / 1e3))
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for c in names:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', c, '--reps', str(args.reps)], capture_output=True,
                               text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit('global_max_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('global_max_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        print('%-16s kernel %8.3f ms  torch %8.3f ms  %.2f of the HBM peak  %.2f of soft Dice  kernel/torch %.2f' % (
            c, r['kernel_ms']['median'], r['torch_ms']['median'], r['hbm_peak_share'], r['bytes_per_s_over_dice'], r['kernel_over_torch']))


if __name__ == '__main__':
    main()
