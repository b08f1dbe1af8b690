"""
Timing of fused.affine_warp (csrc/affine_warp.hip) against the two-kernel path it replaces in SpatialTransformer, on the same tensors in
the same process.

    python tools/affine_warp_bench.py [--reps 10] [--out profiles/affine_warp/affine_warp_bench.jsonl] [--cases NAME,...]
    python tools/affine_warp_bench.py --dry      # CPU rehearsal: arguments, shapes, byte counts and workspaces; measures nothing

Cases: 4 x 160^3 at 1, 3, 4, 8, 16, 32 and 64 channels, 1 x 160^3 x 1 and 4 x 256^2 x 1; the forward with linear and with nearest interpolation, and
forward + backward wrt the matrix (linear); and the linear forward alone at 4 x 160^3 x 128 and 2 x 160^3 x 256.  The other side is the path of the parent commit: for the forward
utils.affine_to_dense_shift (one kernel writes the dense field) and SpatialTransformer on that field; for forward + backward the
route a matrix that needs a gradient took -- the field from torch ops (mesh grid, stack, matmul, transpose, subtract), the warp and its
backward wrt the field, and autograd back through the torch ops.  The matrix is a near-identity affine per batch entry (rotation-like
off-diagonal terms of a few percent and a translation of a few voxels), fill_value 0.  The driver starts one child process per case
(`--case NAME`), each under a time limit of its own, and stops at the first child that fails or runs out of time.  A child compares the
two sides first (largest difference in the record; the forwards must be equal bit for bit), then times, with device events, the two
alternated inside every repetition after a warm-up of both, and appends one JSON line: median / min / max ms of each, the ratio
fused / parent, the share of the 8 TB/s HBM peak that the algorithmic bytes over the fused median come to, and the library build id.
Algorithmic bytes of the forward: 4 C (V + V') per batch entry, the volume read once and the result written once (8 C per output voxel
when the shapes agree); forward + backward reads the volume again and the incoming gradient once.  A time needs a GPU: without one the
tool fails.
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
from neurite_amd import _lib, deferred, fused, utils                                               # noqa: E402

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 240
SHAPES = {
    '4x160x160x160x1': (4, 160, 160, 160, 1),
    '4x160x160x160x3': (4, 160, 160, 160, 3),
    '4x160x160x160x32': (4, 160, 160, 160, 32),
    '4x160x160x160x4': (4, 160, 160, 160, 4),                      # the channel counts between: where SpatialTransformer's route turns
    '4x160x160x160x8': (4, 160, 160, 160, 8),
    '4x160x160x160x16': (4, 160, 160, 160, 16),
    '4x160x160x160x64': (4, 160, 160, 160, 64),
    '1x160x160x160x1': (1, 160, 160, 160, 1),
    '4x256x256x1': (4, 256, 256, 1),
}
# name: (direction, method, shape)
CASES = {}
for _tag, _shape in SHAPES.items():
    CASES['fwd_linear_' + _tag] = ('fwd', 'linear', _shape)
    CASES['fwd_nearest_' + _tag] = ('fwd', 'nearest', _shape)
    CASES['fwdbwd_linear_' + _tag] = ('fwdbwd', 'linear', _shape)
# the linear forward alone at the widest rows SpatialTransformer keeps on the dense field
CASES['fwd_linear_4x160x160x160x128'] = ('fwd', 'linear', (4, 160, 160, 160, 128))
CASES['fwd_linear_2x160x160x160x256'] = ('fwd', 'linear', (2, 160, 160, 160, 256))


def algorithmic_bytes(direction, shape):
    n = int(np.prod(shape)) * 4                                   # S == S': the volume, the result and the gradient are one size
    return 2 * n if direction == 'fwd' else 4 * n


def matrices(batch, nd, seed=0):
    rng = np.random.default_rng(seed)
    M = np.eye(nd, nd + 1, dtype=np.float32)[None] + 0.03 * rng.standard_normal((batch, nd, nd + 1)).astype(np.float32)
    M[:, :, nd] = 3.0 * rng.standard_normal((batch, nd)).astype(np.float32)
    return M


def make_pair(case, dev, shape=None):
    """(fused, parent): callables that return a tuple of tensors"""
    direction, method, full_shape = CASES[case]
    shape = full_shape if shape is None else shape
    nd = len(shape) - 2
    S = list(shape[1:-1])
    g = torch.Generator(device=dev).manual_seed(0)
    vol = torch.rand(shape, generator=g, device=dev)
    M = torch.tensor(matrices(shape[0], nd), device=dev)
    st = ne.layers.SpatialTransformer(interp_method=method, fill_value=0.0)
    if direction == 'fwd':
        def fused_fn():
            return (fused.affine_warp(vol, M, interp_method=method, fill_value=0.0),)

        def parent_fn():
            with deferred.scope(False):
                return (st([vol, utils.affine_to_dense_shift(M, S)]),)
        return fused_fn, parent_fn
    w = torch.randn(shape, generator=g, device=dev)
    M.requires_grad_(True)

    def fused_fn():
        out = fused.affine_warp(vol, M, interp_method=method, fill_value=0.0)
        return (out.detach(),) + torch.autograd.grad(out, (M,), w)

    def parent_fn():
        with deferred.scope(False):
            out = st([vol, utils.affine_to_dense_shift(M, S)])      # a matrix that needs a gradient: the field comes from torch ops
        return (out.detach(),) + torch.autograd.grad(out, (M,), w)
    return fused_fn, parent_fn


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
    direction, method, shape = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('affine_warp_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    fused_fn, parent_fn = make_pair(name, dev)
    a, b = fused_fn(), parent_fn()
    fwd_equal = bool(torch.equal(a[0], b[0]))
    if direction == 'fwd' and not fwd_equal:
        raise SystemExit('affine_warp_bench: %s: the fused forward is not the parent path bit for bit' % name)
    diff = [float((x.float() - y.float()).abs().max() / y.float().abs().max().clamp_min(1e-30)) for x, y in zip(a, b)]
    del a, b
    for _ in range(2):
        fused_fn()
        parent_fn()
    torch.cuda.synchronize()
    t = timed({'fused': fused_fn, 'parent': parent_fn}, reps)
    nbytes = algorithmic_bytes(direction, shape)
    rec = {'case': name, 'direction': direction, 'method': method, 'shape': list(shape), 'reps': reps, 'algorithmic_bytes': nbytes,
           'forward_bit_equal': fwd_equal, 'max_rel_diff_vs_parent': max(diff), 'fused_ms': t['fused'], 'parent_ms': t['parent'],
           'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    rec['bytes_per_s'] = nbytes / (t['fused']['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    rec['fused_over_parent'] = t['fused']['median'] / t['parent']['median']
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases, their byte counts and workspaces"""
    for c in names:
        direction, method, shape = CASES[c]
        nd = len(shape) - 2
        ws = _lib.lib().nrt_affine_warp_workspace_bytes(nd, _lib.ints(shape[1:-1]), shape[-1], shape[0]) if direction == 'fwdbwd' else 0
        M = matrices(shape[0], nd)
        assert M.shape == (shape[0], nd, nd + 1) and (direction == 'fwd' or ws > 0)
        print('%-34s %-18s %-8s %8.1f MB algorithmic  field %7.1f MB  workspace %6.3f MB' % (
            c, 'x'.join(map(str, shape)), method, algorithmic_bytes(direction, shape) / 1e6,
            int(np.prod(shape[:-1])) * nd * 4 / 1e6, ws / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'affine_warp', 'affine_warp_bench.jsonl'))
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
            raise SystemExit('affine_warp_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('affine_warp_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        print('%-34s fused %8.3f ms  parent %8.3f ms  %.3f of the HBM peak  fused/parent %.3f  diff %.2g' % (
            c, r['fused_ms']['median'], r['parent_ms']['median'], r['hbm_peak_share'], r['fused_over_parent'], r['max_rel_diff_vs_parent']))


if __name__ == '__main__':
    main()
