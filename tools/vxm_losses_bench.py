"""
Timing of losses.NCC and losses.Grad (csrc/vxmloss.hip) against the torch-eager restatement of the same losses on the same tensors.

    python tools/vxm_losses_bench.py [--reps 10] [--out profiles/vxm_losses/vxm_losses_bench.jsonl] [--cases NAME,...]
    python tools/vxm_losses_bench.py --dry       # CPU rehearsal: arguments, shapes, byte counts, the eager side at a toy size; measures nothing

Cases: NCC forward and forward + backward at 4 x 160^3 x 1 with windows 9 and 5 and at 4 x 256^2 x 1 with window 9; Grad 'l1' and 'l2'
forward + backward at 4 x 160^3 x 3.  The eager side of NCC is five avg_pool{2,3}d(.., stride 1, count_include_pad=True) * prod(win) box
sums (channels first, one channel) plus the expression of DESIGN 8, with autograd for the backward; the eager side of Grad is slicing,
abs / square and mean.  The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at
the first child that fails or runs out of time.  A child compares the kernel with eager first (largest difference in the record), then
times, with device events, the two alternated inside every repetition after a warm-up of both, and appends one JSON line: median / min /
max ms of each, the ratio kernel / eager, the share of the 8 TB/s HBM peak that the algorithmic bytes over the kernel's median come to,
and the library build id.  Algorithmic bytes: NCC forward reads I and J once (the loss is B floats); forward + backward reads them
again and writes gI and gJ once (the five coefficient fields that travel through the workspace are the implementation's, not the
algorithm's); Grad forward + backward reads y twice and writes gy once.  A time needs a GPU: without one the tool fails.
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
EPS = 1e-5
# name: (loss, direction, shape, window or penalty)
CASES = {
    'ncc_fwd_4x160x160x160x1_w9': ('ncc', 'fwd', (4, 160, 160, 160, 1), 9),
    'ncc_fwdbwd_4x160x160x160x1_w9': ('ncc', 'fwdbwd', (4, 160, 160, 160, 1), 9),
    'ncc_fwd_4x160x160x160x1_w5': ('ncc', 'fwd', (4, 160, 160, 160, 1), 5),
    'ncc_fwdbwd_4x160x160x160x1_w5': ('ncc', 'fwdbwd', (4, 160, 160, 160, 1), 5),
    'ncc_fwd_4x256x256x1_w9': ('ncc', 'fwd', (4, 256, 256, 1), 9),
    'ncc_fwdbwd_4x256x256x1_w9': ('ncc', 'fwdbwd', (4, 256, 256, 1), 9),
    'grad_l1_fwdbwd_4x160x160x160x3': ('grad', 'fwdbwd', (4, 160, 160, 160, 3), 'l1'),
    'grad_l2_fwdbwd_4x160x160x160x3': ('grad', 'fwdbwd', (4, 160, 160, 160, 3), 'l2'),
}


def algorithmic_bytes(loss, direction, shape):
    n = int(np.prod(shape)) * 4
    if loss == 'ncc':
        return 2 * n if direction == 'fwd' else 6 * n            # I, J read; again for the backward, gI and gJ written
    return n if direction == 'fwd' else 3 * n                    # y read; again for the backward, gy written


def eager_ncc_loss(I, J, win, eps=EPS):
    """the torch restatement: [B, *S, 1] float32 -> -mean(cc) per batch entry, [B]"""
    nd = I.dim() - 2
    assert I.shape[-1] == 1
    pool = {2: torch.nn.functional.avg_pool2d, 3: torch.nn.functional.avg_pool3d}[nd]
    a, b = I.movedim(-1, 1), J.movedim(-1, 1)
    n = float(win ** nd)

    def box(x):
        return pool(x, win, stride=1, padding=(win - 1) // 2, count_include_pad=True) * n

    SI, SJ, SII, SJJ, SIJ = box(a), box(b), box(a * a), box(b * b), box(a * b)
    uI, uJ = SI / n, SJ / n
    cross = (((SIJ - uJ * SI) - uI * SJ) + (uI * uJ) * n).clamp(min=eps)
    Ivar = ((SII - (2 * uI) * SI) + (uI * uI) * n).clamp(min=eps)
    Jvar = ((SJJ - (2 * uJ) * SJ) + (uJ * uJ) * n).clamp(min=eps)
    cc = (cross / Ivar) * (cross / Jvar)
    return -cc.reshape(cc.shape[0], -1).mean(1)


def eager_grad_loss(y, penalty):
    total = None
    for ax in range(1, y.dim() - 1):
        d = y.narrow(ax, 1, y.shape[ax] - 1) - y.narrow(ax, 0, y.shape[ax] - 1)
        d = d.abs() if penalty == 'l1' else d * d
        m = d.reshape(d.shape[0], -1).mean(1)
        total = m if total is None else total + m
    return total / (y.dim() - 2)


def make_pair(case, dev, shape=None):
    """(kernel, eager): callables that return (loss, *gradients)"""
    loss, direction, full_shape, arg = CASES[case]
    shape = full_shape if shape is None else shape
    g = torch.Generator(device=dev).manual_seed(0)
    if loss == 'ncc':
        I = torch.rand(shape, generator=g, device=dev)
        J = 0.7 * I + 0.3 * torch.rand(shape, generator=g, device=dev)
        w = torch.rand((shape[0],), generator=g, device=dev) + 0.5
        ncc = ne.losses.NCC(win=arg)
        if direction == 'fwd':
            return (lambda: (ncc.loss(I, J),)), (lambda: (eager_ncc_loss(I, J, arg),))
        I.requires_grad_(True)
        J.requires_grad_(True)

        def kernel():
            out = ncc.loss(I, J)
            return (out,) + torch.autograd.grad(out, (I, J), w)

        def eager():
            out = eager_ncc_loss(I, J, arg)
            return (out,) + torch.autograd.grad(out, (I, J), w)
        return kernel, eager
    y = torch.randn(shape, generator=g, device=dev).requires_grad_(True)
    w = torch.rand((shape[0],), generator=g, device=dev) + 0.5
    grad = ne.losses.Grad(arg)

    def kernel():
        out = grad.loss(None, y)
        return (out,) + torch.autograd.grad(out, (y,), w)

    def eager():
        out = eager_grad_loss(y, arg)
        return (out,) + torch.autograd.grad(out, (y,), w)
    return kernel, eager


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
    loss, direction, shape, arg = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('vxm_losses_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    kernel, eager = make_pair(name, dev)
    diff = []
    for a, b in zip(kernel(), eager()):
        diff.append(float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30)))
    for _ in range(2):
        kernel()
        eager()
    torch.cuda.synchronize()
    t = timed({'kernel': kernel, 'eager': eager}, reps)
    nbytes = algorithmic_bytes(loss, direction, shape)
    rec = {'case': name, 'loss': loss, 'direction': direction, 'shape': list(shape), 'win' if loss == 'ncc' else 'penalty': arg,
           'reps': reps, 'algorithmic_bytes': nbytes, 'max_rel_diff_vs_eager': max(diff), 'kernel_ms': t['kernel'], 'eager_ms': t['eager'],
           'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    rec['bytes_per_s'] = nbytes / (t['kernel']['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    rec['kernel_over_eager'] = t['kernel']['median'] / t['eager']['median']
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases, their byte counts and workspaces, and the eager side at a toy size on the CPU"""
    for c in names:
        loss, direction, shape, arg = CASES[c]
        ws = 0
        if loss == 'ncc':
            nd = len(shape) - 2
            ws = _lib.lib().nrt_ncc_workspace_bytes(shape[0], _lib.ints([1] * (3 - nd) + list(shape[1:-1])), shape[-1],
                                                    _lib.ints([1] * (3 - nd) + [arg] * nd))
            toy = (2,) + (12,) * nd + (1,)
            I = torch.rand(toy, requires_grad=True)
            out = eager_ncc_loss(I, torch.rand(toy), arg)
        else:
            ws = shape[0] * 6144
            y = torch.randn((2, 6, 7, 8, 3), requires_grad=True)
            out = eager_grad_loss(y, arg)
        out.sum().backward()
        assert out.shape == (2,) and bool(torch.isfinite(out).all())
        print('%-34s %-18s %-4s %8.1f MB algorithmic  workspace %7.2f MB' % (
            c, 'x'.join(map(str, shape)), arg, algorithmic_bytes(loss, direction, shape) / 1e6, ws / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vxm_losses', 'vxm_losses_bench.jsonl'))
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
        dry(names)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for c in names:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', c, '--reps', str(args.reps)], capture_output=True,
                               text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit('vxm_losses_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('vxm_losses_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        print('%-34s kernel %8.3f ms  eager %8.3f ms  %.3f of the HBM peak  kernel/eager %.3f  diff %.2g' % (
            c, r['kernel_ms']['median'], r['eager_ms']['median'], r['hbm_peak_share'], r['kernel_over_eager'], r['max_rel_diff_vs_eager']))


if __name__ == '__main__':
    main()
