"""
Timing of utils.label_stats and metrics.LabelOverlap.confusion (csrc/labelstats.hip) against the two routes they replace, on the same
tensors in the same process.

    python tools/label_stats_bench.py [--reps 10] [--out profiles/label_stats/label_stats_bench.jsonl] [--cases NAME,...] [--no-host]
    python tools/label_stats_bench.py --dry      # CPU rehearsal: the cases, their inputs at a toy size and both other routes; measures nothing

Cases: label_stats with and without a one-channel float32 image at 1 x 160^3 and 4 x 160^3, on blob label maps (nearest-seed Voronoi
cells: a wave sees one to three ids) and on i.i.d. ids (every wave meets every label), 32 listed labels; 4 and 256 labels, a bfloat16
image and 4 x 256^2 at the batch of 4; the confusion matrix at 4 x 160^3 with 32 and 256 labels on blobs and on i.i.d. ids.
The routes it is timed against:
  eager   torch on the device: the id -> slot map by searchsorted, torch.bincount (with weights for the coordinate and intensity sums:
          float atomics, sums that change from run to run) and scatter_reduce amin / amax for the boxes and the extrema; for the
          confusion bincount(a * (L + 1) + b)
  host    what a user does today: device -> host, scipy.ndimage.sum / mean / center_of_mass / find_objects (the confusion:
          np.bincount), host -> device; three repetitions, if scipy imports
All cases run in one process, one after the other.  Each warms up, sizes an inner loop so that a timed window holds about 20 ms of
work, and times with device events (median of --reps windows, with min and max).  One JSON line per case: ms per call of each route, the
ratios, the algorithmic bytes (4 B per voxel of ids -- two maps for the confusion -- plus the image's bytes) per second as a share of
the 8 TB/s HBM peak and relative to soft Dice (metrics.Dice(check_input_limits=False).dice on two 4 x 160^3 x 32 float32 maps, timed
once in the same process), and the library build id.  A time needs a GPU: without one the tool fails.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neurite_amd as ne                                                                           # noqa: E402
from neurite_amd import _lib                                                                       # noqa: E402

HBM_PEAK = 8.0e12
WINDOW_MS = 20.0
HOST_REPS = 3
# name -> (kind, ids, batch, spatial shape, labels, image dtype or None)
CASES = {}
for _b in (1, 4):
    for _ids in ('blobs', 'iid'):
        for _image in (None, 'float32'):
            CASES['stats_%s_%s_%dx160^3_L32' % ('image' if _image else 'noimage', _ids, _b)] = ('stats', _ids, _b, (160,) * 3, 32, _image)
for _n in (4, 256):
    for _ids in ('blobs', 'iid'):
        CASES['stats_image_%s_4x160^3_L%d' % (_ids, _n)] = ('stats', _ids, 4, (160,) * 3, _n, 'float32')
CASES['stats_bf16_blobs_4x160^3_L32'] = ('stats', 'blobs', 4, (160,) * 3, 32, 'bfloat16')
CASES['stats_image_blobs_4x256^2_L32'] = ('stats', 'blobs', 4, (256, 256), 32, 'float32')
for _n in (32, 256):
    for _ids in ('blobs', 'iid'):
        CASES['confusion_%s_4x160^3_L%d' % (_ids, _n)] = ('confusion', _ids, 4, (160,) * 3, _n, None)


def label_list(n):
    """n distinct positive ids, unsorted (positive: scipy.ndimage.find_objects indexes with them)"""
    return [int(v) for v in 3 * np.random.default_rng(n).permutation(n) + 1]


def make_ids(kind, batch, spatial, labels, dev, seed=0):
    """int32 [B, *S]: i.i.d. listed ids, or nearest-seed Voronoi cells of 64 seeds per entry"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.tensor(labels, dtype=torch.int32)
    if kind == 'iid':
        return lab[torch.randint(len(labels), (batch,) + tuple(spatial), generator=g)].to(dev)
    grid = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device=dev) for s in spatial], indexing='ij'), -1)
    out = []
    for _ in range(batch):
        seeds = (torch.rand((64, len(spatial)), generator=g) * torch.tensor(spatial, dtype=torch.float32)).to(dev)
        owner = lab[torch.randint(len(labels), (64,), generator=g)].to(dev)
        best = torch.full(tuple(spatial), float('inf'), device=dev)
        ids = torch.zeros(tuple(spatial), dtype=torch.int32, device=dev)
        for k in range(64):
            d = ((grid - seeds[k]) ** 2).sum(-1)
            ids = torch.where(d < best, owner[k], ids)
            best = torch.minimum(best, d)
        out.append(ids)
    return torch.stack(out)


def make_image(batch, spatial, dtype, dev, seed=0):
    g = torch.Generator().manual_seed(seed + 1)
    return (100.0 + 30.0 * torch.randn((batch,) + tuple(spatial), generator=g)).to(getattr(torch, dtype)).to(dev)


def slots_of(ids, labels):
    """eager id -> slot: the position in `labels`, len(labels) for an id that is not listed"""
    lab = torch.tensor(labels, dtype=ids.dtype, device=ids.device)
    keys, perm = lab.sort()
    pos = torch.searchsorted(keys, ids.reshape(-1)).clamp_(max=len(labels) - 1)
    return torch.where(keys[pos] == ids.reshape(-1), perm[pos], len(labels)).view(ids.shape)


def eager_stats(ids, image, labels):
    """the torch-eager route: one bincount / scatter per quantity"""
    batch, spatial, n = ids.shape[0], ids.shape[1:], len(labels)
    slot = slots_of(ids, labels).reshape(batch, -1)
    index = (slot + (n + 1) * torch.arange(batch, device=ids.device).view(batch, 1)).reshape(-1)
    size = batch * (n + 1)
    out = {'count': torch.bincount(index, minlength=size)}
    grids = torch.meshgrid(*[torch.arange(s, device=ids.device) for s in spatial], indexing='ij')
    for a, g in enumerate(grids):
        coord = g.reshape(1, -1).expand(batch, -1).reshape(-1)
        out['coord_sum_%d' % a] = torch.bincount(index, weights=coord.double(), minlength=size)
        out['bbox_min_%d' % a] = torch.full((size,), spatial[a], dtype=coord.dtype, device=ids.device).scatter_reduce(0, index, coord, 'amin')
        out['bbox_max_%d' % a] = torch.full((size,), -1, dtype=coord.dtype, device=ids.device).scatter_reduce(0, index, coord, 'amax')
    if image is not None:
        x = image.reshape(-1).float()
        out['sum'] = torch.bincount(index, weights=x.double(), minlength=size)
        out['sumsq'] = torch.bincount(index, weights=(x * x).double(), minlength=size)
        out['min'] = torch.full((size,), float('inf'), device=ids.device).scatter_reduce(0, index, x, 'amin')
        out['max'] = torch.full((size,), float('-inf'), device=ids.device).scatter_reduce(0, index, x, 'amax')
    return {k: v.view(batch, n + 1)[:, :n] for k, v in out.items()}


def eager_confusion(a, b, labels):
    batch, n = a.shape[0], len(labels)
    code = slots_of(a, labels).reshape(batch, -1) * (n + 1) + slots_of(b, labels).reshape(batch, -1)
    code = code + (n + 1) ** 2 * torch.arange(batch, device=a.device).view(batch, 1)
    return torch.bincount(code.reshape(-1), minlength=batch * (n + 1) ** 2).view(batch, n + 1, n + 1)


def host_stats(ids, image, labels):
    """device -> host, scipy.ndimage per entry, host -> device"""
    with np.errstate(invalid='ignore', divide='ignore'):                                           # (a label that does not occur: 0 / 0)
        return _host_stats(ids, image, labels)


def _host_stats(ids, image, labels):
    from scipy import ndimage
    ids_h = ids.cpu().numpy()
    image_h = None if image is None else image.float().cpu().numpy()
    out = []
    for e in range(ids_h.shape[0]):
        ones = np.ones(ids_h.shape[1:], np.float32)
        row = [ndimage.sum(ones, ids_h[e], labels), np.asarray(ndimage.center_of_mass(ones, ids_h[e], labels))]
        boxes = ndimage.find_objects(ids_h[e], max_label=max(labels))
        row.append(np.asarray([[(s.start, s.stop - 1) for s in boxes[l - 1]] if boxes[l - 1] is not None else
                               [(0, -1)] * (ids_h.ndim - 1) for l in labels]))
        if image_h is not None:
            row += [ndimage.sum(image_h[e], ids_h[e], labels), ndimage.mean(image_h[e], ids_h[e], labels),
                    ndimage.standard_deviation(image_h[e], ids_h[e], labels), ndimage.minimum(image_h[e], ids_h[e], labels),
                    ndimage.maximum(image_h[e], ids_h[e], labels)]
        out.append(row)
    return [torch.from_numpy(np.stack([r[k] for r in out])).to(ids.device) for k in range(len(out[0]))]


def host_confusion(a, b, labels):
    a_h, b_h, n = a.cpu().numpy(), b.cpu().numpy(), len(labels)
    keys = np.sort(labels)
    perm = np.argsort(labels)

    def slots(x):
        pos = np.minimum(np.searchsorted(keys, x), n - 1)
        return np.where(keys[pos] == x, perm[pos], n)
    out = [np.bincount((slots(a_h[e]) * (n + 1) + slots(b_h[e])).reshape(-1), minlength=(n + 1) ** 2).reshape(n + 1, n + 1)
           for e in range(a_h.shape[0])]
    return torch.from_numpy(np.stack(out)).to(a.device)


def algorithmic_bytes(kind, batch, spatial, image):
    voxels = batch * int(np.prod(spatial))
    if kind == 'confusion':
        return 8 * voxels
    return voxels * (4 + (0 if image is None else 4 if image == 'float32' else 2))


def make_calls(name, dev, toy=False):
    """(device, eager, host): callables; host is None without scipy"""
    kind, ids_kind, batch, spatial, n, image_dtype = CASES[name]
    if toy:
        spatial = (12,) * len(spatial)
    labels = label_list(n)
    ids = make_ids(ids_kind, batch, spatial, labels, dev)
    try:
        import scipy.ndimage                                                                       # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    if kind == 'confusion':
        other = make_ids(ids_kind, batch, spatial, labels, dev, seed=5)
        keep = torch.rand(ids.shape, generator=torch.Generator(device=dev).manual_seed(9), device=dev) < 0.8
        other = torch.where(keep, ids, other)                                                      # (a prediction: mostly right)
        overlap = ne.metrics.LabelOverlap(labels) if dev.type == 'cuda' else None
        return (lambda: overlap.confusion(ids, other)), (lambda: eager_confusion(ids, other, labels)), \
            (lambda: host_confusion(ids, other, labels))
    image = None if image_dtype is None else make_image(batch, spatial, image_dtype, dev)
    return (lambda: ne.utils.label_stats(ids, image, labels, batched=True)), (lambda: eager_stats(ids, image, labels)), \
        ((lambda: host_stats(ids, image, labels)) if have_scipy else None)


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


def host_timed(fn, reps):
    """a route that ends on the host: wall clock around a call that starts and ends synchronised"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _spread(out)


_dice = {}


def dice_bytes_per_s(dev, reps):
    """soft Dice on two 4 x 160^3 x 32 float32 maps, timed once per process: the bytes it reads per second"""
    if not _dice:
        g = torch.Generator(device=dev).manual_seed(0)
        shape = (4, 160, 160, 160, 32)
        x, y = torch.rand(shape, generator=g, device=dev), torch.rand(shape, generator=g, device=dev)
        dice = ne.metrics.Dice(check_input_limits=False)
        t, _ = measure(lambda: dice.dice(x, y), reps)
        _dice.update(ms=t, bytes_per_s=2 * x.numel() * 4 / (t['median'] * 1e-3))
    return _dice


def run_case(name, reps, host):
    kind, ids_kind, batch, spatial, n, image_dtype = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('label_stats_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    dice = dice_bytes_per_s(dev, reps)
    device, eager, on_host = make_calls(name, dev)
    rec = {'case': name, 'kind': kind, 'ids': ids_kind, 'batch': batch, 'shape': list(spatial), 'labels': n, 'image': image_dtype,
           'reps': reps, 'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    got, want = device(), eager()
    if kind == 'confusion':
        rec['equals_eager'] = bool(torch.equal(got, want))
    else:
        rec['equals_eager'] = bool(torch.equal(got['count'], want['count']))
        if image_dtype is not None:
            rec['max_rel_diff_sum_vs_eager'] = float(((got['sum'][..., 0] - want['sum']).abs() / want['sum'].abs().clamp_min(1e-30)).max())
    t, inner = measure(device, reps)
    nbytes = algorithmic_bytes(kind, batch, spatial, image_dtype)
    rec.update(calls_per_window=inner, algorithmic_bytes=nbytes, device_ms=t)
    rec['bytes_per_s'] = nbytes / (t['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    rec['dice_ms'], rec['bytes_per_s_over_dice'] = dice['ms'], rec['bytes_per_s'] / dice['bytes_per_s']
    rec['eager_ms'], _ = measure(eager, reps)
    rec['device_over_eager'] = t['median'] / rec['eager_ms']['median']
    if host and on_host is not None:
        rec['host_ms'] = host_timed(on_host, HOST_REPS)
        rec['device_over_host'] = t['median'] / rec['host_ms']['median']
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases, their inputs at a toy size, the eager and the host route against each other"""
    cpu = torch.device('cpu')
    for c in names:
        kind, ids_kind, batch, spatial, n, image_dtype = CASES[c]
        _, eager, on_host = make_calls(c, cpu, toy=True)
        want = eager()
        if on_host is not None:
            got = on_host()
            if kind == 'confusion':
                assert torch.equal(got, want)
            else:
                assert torch.equal(got[0].long(), want['count'])
        print('%-36s %-9s %-5s %d x %s L=%-3d image %-8s %8.1f MB algorithmic' % (
            c, kind, ids_kind, batch, 'x'.join(map(str, spatial)), n, image_dtype, algorithmic_bytes(kind, batch, spatial, image_dtype) / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'label_stats', 'label_stats_bench.jsonl'))
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--no-host', action='store_true', help='skip the scipy route')
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
        r = run_case(c, args.reps, not args.no_host)
        with open(args.out, 'a') as f:
            f.write(json.dumps(r) + '\n')
        host = r.get('host_ms', {}).get('median')
        print('%-36s device %8.3f ms (%.3f - %.3f)  eager %8.3f ms  host %s ms  %.4f of the HBM peak  %.3f of soft Dice\'s bytes/s' % (
            c, r['device_ms']['median'], r['device_ms']['min'], r['device_ms']['max'], r['eager_ms']['median'],
            '%9.1f' % host if host is not None else '        -', r['hbm_peak_share'], r['bytes_per_s_over_dice']), flush=True)


if __name__ == '__main__':
    main()
