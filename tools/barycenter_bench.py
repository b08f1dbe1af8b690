"""
Timing of utils.barycenter (csrc/barycenter.hip) against the torch-eager restatement of the reference's expression
(neurite/tf/utils/utils.py:540-573: move the axes to the end, materialise the coordinate grid and grid * x, reduce twice) on the same
tensors.

    python tools/barycenter_bench.py [--reps 10] [--out profiles/barycenter/barycenter_bench.jsonl] [--cases NAME,...]
    python tools/barycenter_bench.py --dry       # CPU rehearsal: arguments, shapes, byte counts; measures nothing

Cases, each forward and forward + backward: 4 x 160^3 x 32 float32 and 4 x 160^3 x 64 bfloat16 feature maps (channels-last, the inner
arm), 4 x 160^3 x 1 (the trailing arm) and 8 x 256^2 x 64 (2-D).  The driver starts one child process per case (`--case NAME`), each
under a time limit of its own, and stops at the first child that fails or runs out of time.  A child compares the kernel with eager
first (largest difference in the record), then times, with device events, the two alternated inside every repetition after a warm-up
of both, and appends one JSON line: median / min / max ms of each, the share of the 8 TB/s HBM peak that numel * itemsize algorithmic
bytes (x read once; doubled for forward + backward: gx written once) over the median come to, the ratio kernel / eager, and the library
build id.  The 4 x 160^3 x 32 float32 children also time, in the same process, Dice(check_input_limits=False).dice on two tensors of that
shape -- the kernel with the same access pattern, which reads two tensors where barycenter reads one -- and record its bytes / s and
barycenter's bytes / s over it.  A time needs a GPU: without one the tool fails.
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

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 240
# name: (shape, axes, dtype, time soft Dice as well)
SHAPES = {
    'f32_4x160x160x160x32': ((4, 160, 160, 160, 32), (1, 2, 3), torch.float32, True),
    'bf16_4x160x160x160x64': ((4, 160, 160, 160, 64), (1, 2, 3), torch.bfloat16, False),
    'f32_4x160x160x160x1': ((4, 160, 160, 160, 1), (1, 2, 3), torch.float32, False),
    'f32_8x256x256x64': ((8, 256, 256, 64), (1, 2), torch.float32, False),
}
CASES = {'%s_%s' % (d, n): (d,) + v for n, v in SHAPES.items() for d in ('fwd', 'fwdbwd')}


def algorithmic_bytes(direction, shape, dtype):
    return int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size() * (1 if direction == 'fwd' else 2)


def eager_barycenter(x, axes, normalize=False, shift_center=False):
    """the reference's expression, op for op, in torch"""
    x = x.to(torch.float32)
    nd = x.dim()
    kept = tuple(a for a in range(nd) if a not in axes)
    if kept:
        x = x.permute(*kept, *axes)
    vol = x.shape[-len(axes):]
    grids = []
    for v in vol:
        g = torch.arange(v, dtype=torch.float32, device=x.device)
        if shift_center:
            g = g - (v - 1) / 2
        if normalize:
            g = g / v
        grids.append(g)
    grid = torch.stack(torch.meshgrid(*grids, indexing='ij'), dim=-1)
    red = tuple(range(nd - len(axes), nd))
    x = x.unsqueeze(-1)
    num, den = (grid * x).sum(dim=red), x.sum(dim=red)
    return torch.where(den == 0, torch.zeros_like(num), num / den)


def timed(fns, reps):
    """median / min / max ms of each of `fns` (name -> callable), alternated inside every repetition"""
    times = {k: [] for k in fns}
    for _ in range(reps):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1))
    return {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()}


def run_case(name, reps):
    direction, shape, axes, dtype, with_dice = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('barycenter_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(shape, generator=g, device=dev).to(dtype)
    kw = dict(normalize=True, shift_center=True)
    k = len(axes)
    if direction == 'fwd':
        def kernel():
            return (ne.utils.barycenter(x, axes=axes, **kw),)

        def eager():
            return (eager_barycenter(x, axes, **kw),)
    else:
        x.requires_grad_(True)
        w = torch.randn((shape[0], shape[-1], k), generator=g, device=dev)

        def kernel():
            y = ne.utils.barycenter(x, axes=axes, **kw)
            return (y,) + torch.autograd.grad(y, x, w)

        def eager():
            y = eager_barycenter(x, axes, **kw)
            return (y,) + torch.autograd.grad(y, x, w)
    diff = []
    for a, b in zip(kernel(), eager()):
        diff.append(float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30)))
    for _ in range(2):
        kernel()
        eager()
    torch.cuda.synchronize()
    t = timed({'kernel': kernel, 'eager': eager}, reps)
    nbytes = algorithmic_bytes(direction, shape, dtype)
    rec = {'case': name, 'direction': direction, 'shape': list(shape), 'axes': list(axes), 'dtype': str(dtype).replace('torch.', ''),
           'reps': reps, 'algorithmic_bytes': nbytes, 'max_rel_diff_vs_eager': max(diff), 'kernel_ms': t['kernel'], 'eager_ms': t['eager'],
           'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    rec['bytes_per_s'] = nbytes / (t['kernel']['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    rec['kernel_over_eager'] = t['kernel']['median'] / t['eager']['median']
    if with_dice:
        x.requires_grad_(False)
        other = torch.rand(shape, generator=g, device=dev)
        dice = ne.metrics.Dice(check_input_limits=False)
        for _ in range(3):
            dice.dice(x, other)
        torch.cuda.synchronize()
        td = timed({'dice': lambda: dice.dice(x, other)}, reps)['dice']
        rec['dice_ms'] = td
        rec['dice_bytes_per_s'] = 2 * algorithmic_bytes('fwd', shape, dtype) / (td['median'] * 1e-3)
        rec['bytes_per_s_over_dice'] = rec['bytes_per_s'] / rec['dice_bytes_per_s']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'barycenter', 'barycenter_bench.jsonl'))
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
            d, shape, axes, dtype, _ = CASES[c]
            code = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16}[dtype]
            red = [shape[a] for a in axes]
            ws = _lib.lib().nrt_barycenter_workspace_bytes(code, shape[0], _lib.ints(red), len(red), shape[-1])
            print('%-36s %-22s axes %-10s %-9s %8.1f MB  workspace %6.2f MB' % (
                c, 'x'.join(map(str, shape)), axes, str(dtype).replace('torch.', ''), algorithmic_bytes(d, shape, dtype) / 1e6, ws / 1e6))
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for c in names:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', c, '--reps', str(args.reps)], capture_output=True,
                               text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit('barycenter_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('barycenter_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        print('%-36s kernel %8.3f ms  eager %8.3f ms  %.2f of the HBM peak  kernel/eager %.3f%s' % (
            c, r['kernel_ms']['median'], r['eager_ms']['median'], r['hbm_peak_share'], r['kernel_over_eager'],
            '  bytes/s over soft Dice %.2f' % r['bytes_per_s_over_dice'] if 'bytes_per_s_over_dice' in r else ''))


if __name__ == '__main__':
    main()
