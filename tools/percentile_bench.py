"""
Timing of utils.percentile and utils.percentile_norm (csrc/select.hip) against the path they replace, torch.quantile, on the same
tensors in the same process.

    python tools/percentile_bench.py [--reps 10] [--out profiles/percentile/percentile_bench.jsonl] [--cases NAME,...]
    python tools/percentile_bench.py --dry       # CPU rehearsal: the cases, their inputs at a toy size and the torch path; measures nothing

Cases: percentile(x, [0.5, 99.5]) and percentile_norm(x, 0, 99) of 1 x 160^3, 4 x 160^3 and 1 x 256^3 float32 volumes, each on a
smooth synthetic image, on an image that is 70 % exact zeros with a smooth positive rest (a skull-stripped brain: the hot-bin case of the
histogram kernels) and on a constant image (every increment to one counter); the masked percentile (a random mask at 0.3) and the
bfloat16 percentile at 4 x 160^3.  The torch side: torch.quantile(x.view(B, -1), q, dim=1) -- a sort of every volume -- and for the
normalisation the eager expression built on it, ((x - lo) / (hi - lo)).clamp(0, 1); for the mask, torch.quantile of x[b][mask[b]] entry
by entry (a boolean index: a host synchronisation per entry); for bfloat16, torch.quantile of x.float() (it takes no bfloat16).
All cases run in one process, one after the other.  Each warms up, sizes an inner loop so that a timed window holds about 20 ms of
work, and times both sides with device events (median of --reps windows, with min and max).  One JSON line per case: ms per call of
each, the ratio, the largest difference between the two results (torch interpolates in float32), the bytes the passes read (three
reads of x for float32, two for bfloat16, the mask with each; the normalisation reads x once more and writes float32) per second as a
share of the 8 TB/s HBM peak, and the library build id.  A case that torch.quantile refuses (it has an input size limit) carries the
error text instead of a torch time.  A time needs a GPU: without one the tool fails.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neurite_amd as ne                                                                           # noqa: E402
from neurite_amd import _lib                                                                       # noqa: E402

HBM_PEAK = 8.0e12
WINDOW_MS = 20.0
Q_PAIR = (0.5, 99.5)
NORM_PAIR = (0.0, 99.0)
GEOMETRIES = {'1x160^3': (1, 160), '4x160^3': (4, 160), '1x256^3': (1, 256)}
# name -> (kind, image, batch, size, dtype)
CASES = {}
for _geom, (_b, _s) in GEOMETRIES.items():
    for _image in ('smooth', 'zeros70', 'constant'):
        CASES['percentile_%s_%s' % (_image, _geom)] = ('percentile', _image, _b, _s, 'float32')
        CASES['norm_%s_%s' % (_image, _geom)] = ('norm', _image, _b, _s, 'float32')
CASES['masked_smooth_4x160^3'] = ('masked', 'smooth', 4, 160, 'float32')
CASES['masked_zeros70_4x160^3'] = ('masked', 'zeros70', 4, 160, 'float32')
CASES['bf16_smooth_4x160^3'] = ('percentile', 'smooth', 4, 160, 'bfloat16')
CASES['bf16_zeros70_4x160^3'] = ('percentile', 'zeros70', 4, 160, 'bfloat16')


def pass_bytes(kind, batch, size, dtype):
    """the bytes the kernels read and write, from the shapes"""
    n = batch * size ** 3
    item, passes = (4, 3) if dtype == 'float32' else (2, 2)
    total = passes * n * (item + (1 if kind == 'masked' else 0))
    if kind == 'norm':
        total += n * (item + 4)
    return total


def make_image(image, batch, size, dtype, dev):
    g = torch.Generator().manual_seed(0)
    if image == 'constant':
        x = torch.full((batch, size, size, size), 3.25)
    else:
        coarse = max(2, size // 8)
        x = torch.nn.functional.interpolate(torch.randn(batch, 1, coarse, coarse, coarse, generator=g), size=(size,) * 3, mode='trilinear',
                                            align_corners=False)[:, 0]
        x = x * 100.0 + torch.randn(x.shape, generator=g)                                         # (texture: few exact ties)
        if image == 'zeros70':
            flat = x.reshape(batch, -1)
            cut = flat.kthvalue(int(0.7 * flat.shape[1]), dim=1).values
            x = (x - cut.view(batch, 1, 1, 1)).clamp(min=0)
    return x.to(getattr(torch, dtype)).to(dev)


def make_calls(kind, image, batch, size, dtype, dev):
    """(device, torch): callables that return a tensor"""
    x = make_image(image, batch, size, dtype, dev)
    if kind == 'percentile':
        q = torch.tensor([v / 100.0 for v in Q_PAIR], device=dev)
        return (lambda: ne.utils.percentile(x, list(Q_PAIR), batched=True)), \
            (lambda: torch.quantile(x.view(batch, -1).float(), q, dim=1).t())
    if kind == 'masked':
        g = torch.Generator().manual_seed(1)
        mask = (torch.rand(x.shape, generator=g) < 0.3).to(dev)
        q = torch.tensor([v / 100.0 for v in Q_PAIR], device=dev)
        return (lambda: ne.utils.percentile(x, list(Q_PAIR), mask=mask, batched=True)), \
            (lambda: torch.stack([torch.quantile(x[b][mask[b]], q) for b in range(batch)]))
    q = torch.tensor([v / 100.0 for v in NORM_PAIR], device=dev)

    def eager():
        b = torch.quantile(x.view(batch, -1), q, dim=1)
        lo, hi = b[0].view(batch, 1, 1, 1), b[1].view(batch, 1, 1, 1)
        return ((x - lo) / (hi - lo)).clamp(0, 1)
    return (lambda: ne.utils.percentile_norm(x, NORM_PAIR[0], NORM_PAIR[1], batched=True)), eager


def _spread(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def timed(fn, reps, inner):
    """median / min / max ms per call over `reps` windows of `inner` calls, by device events"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return _spread(out)


def measure(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    once = timed(fn, 3, 1)
    inner = int(min(200, max(1, round(WINDOW_MS / max(once['median'], 1e-3)))))
    return timed(fn, reps, inner), inner


def run_case(name, reps):
    kind, image, batch, size, dtype = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('percentile_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    device, eager = make_calls(kind, image, batch, size, dtype, dev)
    got = device()
    rec = {'case': name, 'kind': kind, 'image': image, 'batch': batch, 'shape': [size] * 3, 'dtype': dtype, 'reps': reps,
           'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    t, inner = measure(device, reps)
    nbytes = pass_bytes(kind, batch, size, dtype)
    rec.update(calls_per_window=inner, pass_bytes=nbytes, device_ms=t)
    rec['bytes_per_s'] = nbytes / (t['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    try:
        want = eager()
        diff = (got.float() - want.float()).abs()
        rec['max_abs_diff_vs_torch'] = float(diff[~diff.isnan()].max()) if bool((~diff.isnan()).any()) else 0.0
        rec['torch_ms'], _ = measure(eager, reps)
        rec['device_over_torch'] = t['median'] / rec['torch_ms']['median']
    except RuntimeError as e:                                                                      # torch.quantile refuses the input
        rec['torch_error'] = str(e).splitlines()[0][:200]
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases, their images and the torch path at a toy size"""
    for image in ('smooth', 'zeros70', 'constant'):
        x = make_image(image, 2, 16, 'float32', 'cpu')
        assert x.shape == (2, 16, 16, 16)
        if image == 'zeros70':
            assert abs(float((x == 0).float().mean()) - 0.7) < 0.01
        q = torch.tensor([0.005, 0.995])
        assert torch.quantile(x.view(2, -1), q, dim=1).t().shape == (2, 2)
    for c in names:
        kind, image, batch, size, dtype = CASES[c]
        print('%-28s %-10s %-8s %d x %d^3 %-8s %8.1f MB read and written by the passes' % (c, kind, image, batch, size, dtype,
                                                                                          pass_bytes(kind, batch, size, dtype) / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'percentile', 'percentile_bench.jsonl'))
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    names = [c for c in args.cases.split(',') if c]
    for c in names:
        if c not in CASES:
            raise SystemExit('unknown case %s (known: %s)' % (c, ', '.join(CASES)))
    if args.dry:
        dry(names)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for c in names:
        r = run_case(c, args.reps)
        with open(args.out, 'a') as f:
            f.write(json.dumps(r) + '\n')
        other = r.get('torch_ms', {}).get('median')
        print('%-28s device %9.3f ms (%.3f - %.3f)  torch %s ms  %.4f of the HBM peak  device/torch %s' % (
            c, r['device_ms']['median'], r['device_ms']['min'], r['device_ms']['max'], '%9.3f' % other if other is not None else '        -',
            r['hbm_peak_share'], '%.4f' % r['device_over_torch'] if other is not None else '-'), flush=True)


if __name__ == '__main__':
    main()
