"""
Timing of the distance transforms and surface distances (csrc/edt.hip) against the two things they replace, on the same tensors:
  (i)  the torch-eager restatement: the separable squared transform as a min-plus product by broadcasting, one axis at a time,
       chunked so that a chunk's [rows, n, n] intermediate stays under 512 MB;
  (ii) the host path: device -> host copy, scipy.ndimage.distance_transform_edt (what VoxelMorph's dist_trf calls), host -> device copy.
       Left out of the record where scipy does not import.

    python tools/edt_bench.py [--reps 10] [--out profiles/edt/edt_bench.jsonl] [--cases NAME,...]
    python tools/edt_bench.py --dry       # CPU rehearsal: arguments, shapes, byte counts, both baselines at a toy size; measures nothing

Cases: dist_trf and signed_dist_trf of 1 x 160^3, 4 x 160^3 and 4 x 256^2 binary volumes (blob-shaped sets); label_dist_trf of a
4 x 160^3 map of 32 blob labels at 4 and at 32 labels; SurfaceDistance.distances of two such maps at 32 labels.  The driver starts one
child process per case (`--case NAME`), each under a time limit of its own, and stops at the first child that fails or runs out of
time.  A child compares the kernel with eager (and the host path) first, warms both up, sizes an inner loop so that a timed window
holds about 20 ms of work, then times kernel and eager with device events, alternated inside every repetition, and the host path with
a host clock around calls that end in a device synchronise (3 calls, 1 where a call takes more than 5 s).  One JSON line per case:
median / min / max ms per call of each, the ratios, the kernel's algorithmic bytes per second -- 1 B (a binary voxel) or 4 B (an id)
read and 4 L B written per voxel; 8 B read per voxel for the surface distances -- its share of the 8 TB/s HBM peak, and the library
build id.  The eager side of the surface distances is the two transforms from the surfaces and masked max / sum reductions, without
the percentile; its host side is binary_erosion + two transforms per label and the NumPy reductions.  A time needs a GPU: without one
the tool fails.
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neurite_amd as ne                                                                           # noqa: E402
from neurite_amd import _lib, synth                                                                # noqa: E402

try:
    import scipy.ndimage as ndi
except ImportError:                                                                                # the record then has no host line
    ndi = None

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 400
WINDOW_MS = 20.0
CHUNK_BYTES = 512 << 20
# name -> (kind, batch, spatial shape, labels)
CASES = {
    'dist_1x160^3': ('dist', 1, (160, 160, 160), 1),
    'signed_1x160^3': ('signed', 1, (160, 160, 160), 1),
    'dist_4x160^3': ('dist', 4, (160, 160, 160), 1),
    'signed_4x160^3': ('signed', 4, (160, 160, 160), 1),
    'labels4_4x160^3': ('labels', 4, (160, 160, 160), 4),
    'labels32_4x160^3': ('labels', 4, (160, 160, 160), 32),
    'surface32_4x160^3': ('surface', 4, (160, 160, 160), 32),
    'dist_4x256^2': ('dist', 4, (256, 256), 1),
    'signed_4x256^2': ('signed', 4, (256, 256), 1),
}


def algorithmic_bytes(kind, batch, shape, labels):
    voxels = batch * int(np.prod(shape))
    if kind == 'surface':
        return 8 * voxels
    return voxels * ((1 if kind in ('dist', 'signed') else 4) + 4 * labels)


# ---- (i) torch eager ----------------------------------------------------------------------------------------------------------------
def eager_sq_edt(feat):
    """feat: bool [B, *S, L] -> squared distance to the nearest True voxel along the spatial axes, float32 (+inf without one)"""
    g = torch.where(feat, 0.0, float('inf')).to(torch.float32)
    for ax in range(1, feat.dim() - 1):
        n = g.shape[ax]
        idx = torch.arange(n, device=g.device, dtype=torch.float32)
        cost = (idx[:, None] - idx[None, :]) ** 2                                                  # [i, j]
        rows = g.movedim(ax, -1).reshape(-1, n)
        out = torch.empty_like(rows)
        step = max(1, CHUNK_BYTES // (4 * n * n))
        for beg in range(0, rows.shape[0], step):
            out[beg:beg + step] = (rows[beg:beg + step, None, :] + cost[None]).amin(-1)
        g = out.reshape(g.movedim(ax, -1).shape).movedim(-1, ax)
    return g.contiguous()


def eager_dist(feat, signed):
    pos = eager_sq_edt(feat)
    if not signed:
        return pos.sqrt()
    return torch.where(feat, -eager_sq_edt(~feat).sqrt(), pos.sqrt())


def eager_surface(mask):
    """mask: bool [B, *S, L] -> its voxels with a face neighbour outside it (zero border)"""
    inside = mask.clone()
    for ax in range(1, mask.dim() - 1):
        n = mask.shape[ax]
        pad = torch.zeros_like(mask.narrow(ax, 0, 1))
        inside &= torch.cat([pad, mask.narrow(ax, 0, n - 1)], ax) & torch.cat([mask.narrow(ax, 1, n - 1), pad], ax)
    return mask & ~inside


def eager_surface_distances(t, p, labels):
    st, sp = eager_surface(t[..., None] == labels), eager_surface(p[..., None] == labels)
    out = []
    for a, b in ((st, sp), (sp, st)):
        d = eager_sq_edt(b).sqrt()
        d = torch.where(a, d, torch.zeros_like(d)).flatten(1, -2)
        out += [a.flatten(1, -2).sum(1), d.amax(1), d.double().sum(1)]
    return out


# ---- (ii) the host path ---------------------------------------------------------------------------------------------------------------
def host_dist(vol, signed):
    m = vol.cpu().numpy().astype(bool)
    out = np.empty(m.shape, np.float32)
    for b in range(m.shape[0]):
        pos = ndi.distance_transform_edt(~m[b])
        out[b] = pos * ~m[b] - ndi.distance_transform_edt(m[b]) * m[b] if signed else pos
    return torch.from_numpy(out).to(vol.device)


def host_labels(ids, labels):
    a = ids.cpu().numpy()
    out = np.empty(a.shape + (len(labels),), np.float32)
    for b in range(a.shape[0]):
        for k, lab in enumerate(labels):
            m = a[b] == lab
            out[b, ..., k] = ndi.distance_transform_edt(~m) if m.any() else np.inf
    return torch.from_numpy(out).to(ids.device)


def host_surface_distances(t, p, labels):
    a, b = t.cpu().numpy(), p.cpu().numpy()
    out = np.full((6, a.shape[0], len(labels)), np.nan)
    for e in range(a.shape[0]):
        for k, lab in enumerate(labels):
            ma, mb = a[e] == lab, b[e] == lab
            sa, sb = ma & ~ndi.binary_erosion(ma), mb & ~ndi.binary_erosion(mb)
            if not sa.any() or not sb.any():
                continue
            dab, dba = ndi.distance_transform_edt(~sb)[sa], ndi.distance_transform_edt(~sa)[sb]
            out[:, e, k] = dab.size, dab.max(), dab.sum(), dba.size, dba.max(), dba.sum()
    return torch.from_numpy(out).to(t.device)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def make_inputs(kind, batch, shape, labels, dev):
    """(ids [B, *S] int32 of 32 blob labels or None, second map or None, bool volume or None)"""
    if len(shape) == 2:
        g = torch.Generator().manual_seed(0)
        field = torch.nn.functional.interpolate(torch.randn(batch, 1, 16, 16, generator=g), size=shape, mode='bilinear', align_corners=False)
        return None, None, (field[:, 0] > 0.3).to(dev)
    size = shape[0]
    ids = torch.stack([synth.blob_labels(1 + b, size=size, nb_labels=32, coarse=max(2, size // 16), device=dev) for b in range(batch)], 0)
    ids = ids.to(torch.int32)
    if kind == 'surface':
        return ids, torch.roll(ids, (2, 1, 1), (1, 2, 3)), None
    if kind == 'labels':
        return ids, None, None
    return None, None, ids < 8                                                                     # a quarter of the blobs


def make_calls(kind, batch, shape, labels, dev):
    """(kernel, eager, host or None): callables that return a tuple of tensors"""
    ids, other, vol = make_inputs(kind, batch, shape, labels, dev)
    lab_list = list(range(labels))
    if kind in ('dist', 'signed'):
        signed = kind == 'signed'
        fn = ne.utils.signed_dist_trf if signed else ne.utils.dist_trf
        host = (lambda: (host_dist(vol, signed),)) if ndi is not None else None
        return (lambda: (fn(vol, batched=True),)), (lambda: (eager_dist(vol[..., None], signed)[..., 0],)), host
    lab_t = torch.tensor(lab_list, dtype=torch.int32, device=dev)
    if kind == 'labels':
        host = (lambda: (host_labels(ids, lab_list),)) if ndi is not None else None
        return (lambda: (ne.utils.label_dist_trf(ids, lab_list),)), (lambda: (eager_dist(ids[..., None] == lab_t, False),)), host
    sd = ne.metrics.SurfaceDistance(lab_list)

    def kernel():
        d = sd.distances(ids, other)
        return (d['count_t'], d['max_tp'], d['mean_tp'] * d['count_t'], d['count_p'], d['max_pt'], d['mean_pt'] * d['count_p'], d['hd_percentile'])

    host = (lambda: tuple(host_surface_distances(ids, other, lab_list))) if ndi is not None else None
    return kernel, (lambda: tuple(eager_surface_distances(ids, other, lab_t))), host


def max_rel_diff(a, b):
    """largest |a - b| / max |b| over the tensors both sides return (the kernel's extra outputs are not compared); inf == inf"""
    worst = 0.0
    for x, y in zip(a, b):
        x, y = x.double(), y.double()
        same = (x == y) | (x.isnan() & y.isnan())
        d = torch.where(same, torch.zeros_like(x), (x - y).abs())
        scale = torch.where(y.isfinite(), y.abs(), torch.zeros_like(y)).max().clamp_min(1e-30)
        worst = max(worst, float(d.max() / scale))
    return worst


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
    return {k: _spread(v) for k, v in times.items()}


def _spread(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def host_timed(fn):
    """a host clock around calls that end in a device synchronise: 3 calls, 1 if the first takes more than 5 s; and the first result"""
    out, first = [], None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        first = res if first is None else first
        if out[0] > 5000.0:
            break
    return dict(_spread(out), calls=len(out)), first


def run_case(name, reps):
    kind, batch, shape, labels = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('edt_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    kernel, eager, host = make_calls(kind, batch, shape, labels, dev)
    got = kernel()
    rec = {'case': name, 'kind': kind, 'batch': batch, 'shape': list(shape), 'labels': labels, 'reps': reps,
           'max_rel_diff_vs_eager': max_rel_diff(got, eager()), 'build_id': _lib.lib().nrt_build_id().decode(),
           'device': torch.cuda.get_device_name(dev)}
    fns = {'kernel': kernel, 'eager': eager}
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    once = timed(fns, 3, {k: 1 for k in fns})
    inner = {k: int(min(200, max(1, round(WINDOW_MS / max(once[k]['median'], 1e-3))))) for k in fns}
    t = timed(fns, reps, inner)
    nbytes = algorithmic_bytes(kind, batch, shape, labels)
    rec.update(calls_per_window=inner, algorithmic_bytes=nbytes, kernel_ms=t['kernel'], eager_ms=t['eager'])
    rec['bytes_per_s'] = nbytes / (t['kernel']['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    rec['kernel_over_eager'] = t['kernel']['median'] / t['eager']['median']
    if host is not None:
        rec['host_ms'], first = host_timed(host)
        rec['max_rel_diff_vs_host'] = max_rel_diff(got, first)
        rec['kernel_over_host'] = t['kernel']['median'] / rec['host_ms']['median']
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases and their byte counts, and both baselines against each other at a toy size"""
    g = torch.Generator().manual_seed(0)
    for nd in (2, 3):
        ids = torch.randint(0, 4, (2,) + (6, 7, 8)[:nd], generator=g, dtype=torch.int32)
        vol = ids < 2
        for signed in (False, True):
            e = eager_dist(vol[..., None], signed)[..., 0]
            if ndi is not None:
                assert max_rel_diff((e,), (host_dist(vol, signed),)) < 1e-6
        e = eager_dist(ids[..., None] == torch.arange(5, dtype=torch.int32), False)
        assert bool(torch.isposinf(e[..., 4]).all())
        if ndi is not None:
            assert max_rel_diff((e,), (host_labels(ids, list(range(5))),)) < 1e-6
            other = torch.roll(ids, 1, 1)
            es = eager_surface_distances(ids, other, torch.arange(4, dtype=torch.int32))
            hs = host_surface_distances(ids, other, list(range(4)))
            assert max_rel_diff(es, tuple(hs)) < 1e-6
    for c in names:
        kind, batch, shape, labels = CASES[c]
        print('%-20s %-8s %d x %s x %2d labels  %8.1f MB algorithmic' % (c, kind, batch, 'x'.join(map(str, shape)), labels,
                                                                        algorithmic_bytes(kind, batch, shape, labels) / 1e6))
    print('scipy %s' % ('imports: the host path is part of the record' if ndi is not None else 'does not import: no host line'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'edt', 'edt_bench.jsonl'))
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
            raise SystemExit('edt_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('edt_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = [ln for ln in p.stdout.strip().splitlines() if ln.startswith('{')][-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        host = r.get('host_ms', {}).get('median')
        print('%-20s kernel %9.3f ms  eager %10.3f ms  host %s ms  %.4f of the HBM peak  kernel/eager %.4f  diff %.2g' % (
            c, r['kernel_ms']['median'], r['eager_ms']['median'], '%11.1f' % host if host is not None else '          -',
            r['hbm_peak_share'], r['kernel_over_eager'], r['max_rel_diff_vs_eager']), flush=True)


if __name__ == '__main__':
    main()
