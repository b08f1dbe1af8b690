"""
Timing of the Jacobian determinant kernels (csrc/jacobian.hip) against the torch-eager restatement of the same quantities on the same
tensors, and against losses.Grad('l2') forward + backward -- the project's existing streaming pass over the same field -- timed in the
same process as the bytes-per-second yardstick.

    python tools/jacobian_bench.py [--reps 10] [--out profiles/jacobian/jacobian_bench.jsonl] [--cases NAME,...]
    python tools/jacobian_bench.py --dry       # CPU rehearsal: arguments, shapes, byte counts, the eager side at a toy size; measures nothing

Cases (fields [B, *S, D]): 4 x 160^3 x 3, 1 x 160^3 x 3, 4 x 256^2 x 2.  Modes at each: `map` (utils.jacobian_determinant), `stats`
(metrics.JacobianDeterminant.stats, no map written), `loss_fwd` and `loss_fwdbwd` (losses.NegJacobian).  The eager side is slicing,
concatenation and element-wise arithmetic on the three (two) channels with autograd for the backward: np.gradient's stencil and the
VoxelMorph expansion.  The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at
the first child that fails or runs out of time.  A child compares each kernel mode with eager first (largest relative difference in
the record), warms both up, sizes an inner loop so that a timed window holds about 20 ms of work, then times with device events, the
kernel, eager and Grad alternated inside every repetition, and appends one JSON line per mode: median / min / max ms per call of
each, the ratios kernel / eager and kernel / Grad, the kernel's algorithmic bytes per second, its share of the 8 TB/s HBM peak, the
same rate for Grad, and the library build id.  Algorithmic bytes per voxel in 3-D: 12 read + 4 written for the map, 12 read for stats
and the loss, 12 more read + 12 written for the backward (8 / 4 / 8 / 8 in 2-D); Grad forward + backward reads y twice and writes gy
once.  A time needs a GPU: without one the tool fails.
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
WINDOW_MS = 20.0
CASES = {
    '4x160x160x160x3': (4, 160, 160, 160, 3),
    '1x160x160x160x3': (1, 160, 160, 160, 3),
    '4x256x256x2': (4, 256, 256, 2),
}
MODES = ('map', 'stats', 'loss_fwd', 'loss_fwdbwd')


def algorithmic_bytes(mode, shape):
    field = int(np.prod(shape)) * 4
    voxels = int(np.prod(shape[:-1])) * 4
    return {'map': field + voxels, 'stats': field, 'loss_fwd': field, 'loss_fwdbwd': 3 * field, 'grad_fwdbwd': 3 * field}[mode]


def _diff(f, ax):
    n = f.shape[ax]
    first = f.narrow(ax, 1, 1) - f.narrow(ax, 0, 1)
    last = f.narrow(ax, n - 1, 1) - f.narrow(ax, n - 2, 1)
    if n == 2:
        return torch.cat([first, last], ax)
    return torch.cat([first, (f.narrow(ax, 2, n - 2) - f.narrow(ax, 0, n - 2)) * 0.5, last], ax)


def eager_det(disp):
    """the torch restatement: [B, *S, D] -> [B, *S]"""
    nd = disp.dim() - 2
    eye = torch.eye(nd, dtype=disp.dtype, device=disp.device)
    J = [_diff(disp, 1 + a) + eye[a] for a in range(nd)]
    if nd == 3:
        return (J[0][..., 0] * (J[1][..., 1] * J[2][..., 2] - J[1][..., 2] * J[2][..., 1])
                - J[0][..., 1] * (J[1][..., 0] * J[2][..., 2] - J[1][..., 2] * J[2][..., 0])
                + J[0][..., 2] * (J[1][..., 0] * J[2][..., 1] - J[1][..., 1] * J[2][..., 0]))
    return J[0][..., 0] * J[1][..., 1] - J[1][..., 0] * J[0][..., 1]


def eager_stats(disp):
    d = eager_det(disp).reshape(disp.shape[0], -1)
    return (d <= 0).sum(1), d.amin(1), d.amax(1), d.double().mean(1), d.double().std(1, unbiased=False)


def eager_loss(disp):
    return torch.relu(-eager_det(disp)).reshape(disp.shape[0], -1).mean(1)


def make_modes(shape, dev):
    """mode -> (kernel, eager): callables that return a tuple of tensors; plus the Grad yardstick"""
    g = torch.Generator(device=dev).manual_seed(0)
    y = (1.5 * torch.randn(shape, generator=g, device=dev)).requires_grad_(True)
    w = torch.rand((shape[0],), generator=g, device=dev) + 0.5
    yd = y.detach()
    metric, neg, grad = ne.metrics.JacobianDeterminant(), ne.losses.NegJacobian(), ne.losses.Grad('l2')

    def k_stats():
        s = metric.stats(yd)
        return s.folded_voxels, s.min, s.max, s.mean, s.std

    def fwdbwd(loss_fn):
        def run():
            out = loss_fn(y)
            return (out,) + torch.autograd.grad(out, (y,), w)
        return run

    modes = {
        'map': ((lambda: (ne.utils.jacobian_determinant(yd),)), (lambda: (eager_det(yd),))),
        'stats': (k_stats, (lambda: eager_stats(yd))),
        'loss_fwd': ((lambda: (neg.loss(None, yd),)), (lambda: (eager_loss(yd),))),
        'loss_fwdbwd': (fwdbwd(lambda t: neg.loss(None, t)), fwdbwd(eager_loss)),
    }
    return modes, fwdbwd(lambda t: grad.loss(None, t))


def timed(fns, reps, inner):
    """median / min / max ms per call of each of `fns` (name -> callable), alternated inside every repetition; a timed window runs
    inner[name] calls"""
    times = {k: [] for k in fns}
    for _ in range(reps):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner[key]):
                fn()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) / inner[key])
    return {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()}


def run_case(name, reps):
    shape = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('jacobian_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    modes, grad_fwdbwd = make_modes(shape, dev)
    recs = []
    for mode in MODES:
        kernel, eager = modes[mode]
        diff = []
        for a, b in zip(kernel(), eager()):
            a, b = a.double(), b.double()
            diff.append(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)))
        fns = {'kernel': kernel, 'eager': eager, 'grad': grad_fwdbwd}
        for fn in fns.values():
            fn()
            fn()
        torch.cuda.synchronize()
        once = timed(fns, 3, {k: 1 for k in fns})
        inner = {k: int(min(200, max(1, round(WINDOW_MS / max(once[k]['median'], 1e-3))))) for k in fns}
        t = timed(fns, reps, inner)
        nbytes, gbytes = algorithmic_bytes(mode, shape), algorithmic_bytes('grad_fwdbwd', shape)
        rec = {'case': name, 'mode': mode, 'shape': list(shape), 'reps': reps, 'calls_per_window': inner, 'algorithmic_bytes': nbytes,
               'max_rel_diff_vs_eager': max(diff), 'kernel_ms': t['kernel'], 'eager_ms': t['eager'], 'grad_l2_fwdbwd_ms': t['grad'],
               'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
        rec['bytes_per_s'] = nbytes / (t['kernel']['median'] * 1e-3)
        rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
        rec['grad_bytes_per_s'] = gbytes / (t['grad']['median'] * 1e-3)
        rec['kernel_over_eager'] = t['kernel']['median'] / t['eager']['median']
        rec['bytes_per_s_over_grad'] = rec['bytes_per_s'] / rec['grad_bytes_per_s']
        recs.append(rec)
    return recs


def dry(names):
    """what can be rehearsed without a device: the cases, their byte counts and workspaces, and the eager side at a toy size on the CPU"""
    for c in names:
        shape = CASES[c]
        nd = len(shape) - 2
        ws = _lib.lib().nrt_jacdet_workspace_bytes(shape[0], _lib.ints(shape[1:-1]), nd)
        toy = (2,) + (6, 7, 8)[:nd] + (nd,)
        y = torch.randn(toy, requires_grad=True)
        out = eager_loss(y)
        out.sum().backward()
        st = eager_stats(y.detach())
        assert out.shape == (2,) and bool(torch.isfinite(y.grad).all()) and all(t.shape == (2,) for t in st)
        print('%-18s %s  workspace %7.3f MB' % (c, '  '.join('%s %7.1f MB' % (m, algorithmic_bytes(m, shape) / 1e6) for m in MODES), ws / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jacobian', 'jacobian_bench.jsonl'))
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--case')
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    if args.case:
        for rec in run_case(args.case, args.reps):
            print(json.dumps(rec))
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
            raise SystemExit('jacobian_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('jacobian_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith('{')][-len(MODES):]
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
        for ln in lines:
            r = json.loads(ln)
            print('%-18s %-12s kernel %8.3f ms  eager %8.3f ms  Grad l2 fwd+bwd %7.3f ms  %.3f of the HBM peak  kernel/eager %.3f  '
                  'bytes/s over Grad %.2f  diff %.2g' % (c, r['mode'], r['kernel_ms']['median'], r['eager_ms']['median'],
                                                         r['grad_l2_fwdbwd_ms']['median'], r['hbm_peak_share'], r['kernel_over_eager'],
                                                         r['bytes_per_s_over_grad'], r['max_rel_diff_vs_eager']))


if __name__ == '__main__':
    main()
