"""
Timing of connected-component labelling and the mask clean-up (csrc/ccl.hip) against the host path they replace, on the same tensors in
the same process: device -> host copy, scipy.ndimage.label / binary_fill_holes, host -> device copy.

    python tools/ccl_bench.py [--reps 10] [--out profiles/ccl/ccl_bench.jsonl] [--cases NAME,...]
    python tools/ccl_bench.py --dry       # CPU rehearsal: the cases, their inputs at a toy size and the host path; measures nothing

Cases: connected_components of 1 x 160^3 and 4 x 160^3 blob masks (and the first at connectivity 3), of a 1 x 160^3 map of 32 blob labels (synth.blob_labels, all 32
listed: one pass on the device, 32 scipy calls and a renumbering on the host), of a random mask at the site-percolation density of the
6-neighbourhood (0.3116: components wind through the whole volume -- the adversarial case for a union-find) and of 4 x 256^2 blob masks;
fill_holes of a 1 x 160^3 blob mask; and the post-processing of SynthStrip.brain_mask alone (largest_component, then fill_holes, of a
1 x 160^3 thresholded smooth field).  The driver starts one child process per case (`--case NAME`), each under a time limit of its own,
and stops at the first child that fails or runs out of time.  A child compares the device result with the host's first (they must be
EQUAL), warms up, sizes an inner loop so that a timed window holds about 20 ms of work, times the device call with device events
(median of --reps windows, with min and max) and the host path with a host clock around calls that end in a device synchronise
(3 calls).  One JSON line per case: ms per call of each, the ratio, the call's algorithmic bytes per second (input read once, output
written once) as a share of the 8 TB/s HBM peak, and the library build id.  A time needs a GPU: without one the tool fails.
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
PERCOLATION_DENSITY = 0.3116
# name -> (kind, batch, spatial shape, connectivity)
CASES = {
    'label_1x160^3': ('label', 1, (160, 160, 160), 1),
    'label_4x160^3': ('label', 4, (160, 160, 160), 1),
    'label26_1x160^3': ('label', 1, (160, 160, 160), 3),
    'labels32_1x160^3': ('labels32', 1, (160, 160, 160), 1),
    'percolation_1x160^3': ('percolation', 1, (160, 160, 160), 1),
    'label_4x256^2': ('label', 4, (256, 256), 1),
    'fill_holes_1x160^3': ('fill_holes', 1, (160, 160, 160), 1),
    'brain_mask_post_1x160^3': ('brain_mask_post', 1, (160, 160, 160), 1),
}


def algorithmic_bytes(kind, batch, shape):
    voxels = batch * int(np.prod(shape))
    if kind == 'labels32':
        return voxels * (4 + 4)
    if kind in ('fill_holes', 'brain_mask_post'):
        return voxels * (1 + 1) * (2 if kind == 'brain_mask_post' else 1)
    return voxels * (1 + 4)


# ---- the host path --------------------------------------------------------------------------------------------------------------------
def host_label(x, connectivity):
    a = x.cpu().numpy()
    st = ndi.generate_binary_structure(a.ndim - 1, connectivity)
    comp = np.empty(a.shape, np.int32)
    count = np.empty(a.shape[0], np.int32)
    for b in range(a.shape[0]):
        comp[b], count[b] = ndi.label(a[b], st, output=np.int32)
    return torch.from_numpy(comp).to(x.device), torch.from_numpy(count).to(x.device)


def host_label_ids(ids, labels, connectivity):
    """every label's mask through scipy, then one renumbering by first voxel"""
    a = ids.cpu().numpy()
    st = ndi.generate_binary_structure(a.ndim - 1, connectivity)
    comp = np.zeros(a.shape, np.int32)
    count = np.zeros(a.shape[0], np.int32)
    for b in range(a.shape[0]):
        for lab in labels:
            c, n = ndi.label(a[b] == lab, st, output=np.int32)
            comp[b] += np.where(c > 0, c + count[b], 0).astype(np.int32)
            count[b] += n
        flat = comp[b].reshape(-1)
        idx = np.flatnonzero(flat)
        _, first = np.unique(flat[idx], return_index=True)                                         # first voxel of each provisional number
        order = np.argsort(idx[first], kind='stable')
        lut = np.zeros(count[b] + 1, np.int32)
        lut[1 + order] = np.arange(1, count[b] + 1, dtype=np.int32)
        comp[b] = lut[comp[b]]
    return torch.from_numpy(comp).to(ids.device), torch.from_numpy(count).to(ids.device)


def host_fill_holes(x, connectivity):
    a = x.cpu().numpy()
    st = ndi.generate_binary_structure(a.ndim - 1, connectivity)
    return (torch.from_numpy(np.stack([ndi.binary_fill_holes(a[b], st) for b in range(a.shape[0])])).to(x.device),)


def host_brain_mask_post(x, connectivity):
    a = x.cpu().numpy()
    st = ndi.generate_binary_structure(a.ndim - 1, connectivity)
    out = np.zeros(a.shape, bool)
    for b in range(a.shape[0]):
        c, n = ndi.label(a[b], st)
        if n:
            sizes = np.bincount(c.reshape(-1))
            sizes[0] = 0
            out[b] = ndi.binary_fill_holes(c == np.argmax(sizes), st)
    return (torch.from_numpy(out).to(x.device),)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def make_calls(kind, batch, shape, connectivity, dev):
    """(device, host or None): callables that return a tuple of tensors"""
    if kind == 'percolation':
        g = torch.Generator().manual_seed(0)
        x = (torch.rand((batch,) + tuple(shape), generator=g) < PERCOLATION_DENSITY).to(dev)
    elif len(shape) == 2:
        g = torch.Generator().manual_seed(0)
        field = torch.nn.functional.interpolate(torch.randn(batch, 1, 16, 16, generator=g), size=shape, mode='bilinear', align_corners=False)
        x = (field[:, 0] > 0.3).to(dev)
    else:
        size = shape[0]
        ids = torch.stack([synth.blob_labels(1 + b, size=size, nb_labels=32, coarse=max(2, size // 16), device=dev) for b in range(batch)], 0)
        ids = ids.to(torch.int32)
        x = ids < 8                                                                                # a quarter of the blobs
    if kind in ('label', 'percolation'):
        return (lambda: ne.utils.connected_components(x, connectivity, batched=True)), \
            ((lambda: host_label(x, connectivity)) if ndi is not None else None)
    if kind == 'labels32':
        labels = list(range(32))
        return (lambda: ne.utils.connected_components(ids, connectivity, labels=labels, batched=True)), \
            ((lambda: host_label_ids(ids, labels, connectivity)) if ndi is not None else None)
    if kind == 'fill_holes':
        return (lambda: (ne.utils.fill_holes(x, connectivity, batched=True),)), \
            ((lambda: host_fill_holes(x, connectivity)) if ndi is not None else None)
    return (lambda: (ne.utils.fill_holes(ne.utils.largest_component(x, connectivity, batched=True), connectivity, batched=True),)), \
        ((lambda: host_brain_mask_post(x, connectivity)) if ndi is not None else None)


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


def host_timed(fn):
    """a host clock around calls that end in a device synchronise: 3 calls; and the first result"""
    out, first = [], None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        first = res if first is None else first
    return dict(_spread(out), calls=len(out)), first


def run_case(name, reps):
    kind, batch, shape, connectivity = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('ccl_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    device, host = make_calls(kind, batch, shape, connectivity, dev)
    got = device()
    rec = {'case': name, 'kind': kind, 'batch': batch, 'shape': list(shape), 'connectivity': connectivity, 'reps': reps,
           'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    if kind in ('label', 'labels32', 'percolation'):
        rec['components'] = [int(v) for v in got[1].cpu()]
    device()
    device()
    torch.cuda.synchronize()
    once = timed(device, 3, 1)
    inner = int(min(200, max(1, round(WINDOW_MS / max(once['median'], 1e-3)))))
    t = timed(device, reps, inner)
    nbytes = algorithmic_bytes(kind, batch, shape)
    rec.update(calls_per_window=inner, algorithmic_bytes=nbytes, device_ms=t)
    rec['bytes_per_s'] = nbytes / (t['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    if host is not None:
        rec['host_ms'], first = host_timed(host)
        rec['equal_to_host'] = all(torch.equal(a.to(b.dtype), b) for a, b in zip(got, first))
        rec['device_over_host'] = t['median'] / rec['host_ms']['median']
        if not rec['equal_to_host']:
            raise SystemExit('ccl_bench: case %s: the device result differs from the host path' % name)
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases, and the host path against itself at a toy size"""
    if ndi is not None:
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(0, 3, (2, 6, 7, 8), generator=g, dtype=torch.int32)
        comp, count = host_label_ids(ids, [1], 1)
        one, n1 = host_label(ids == 1, 1)
        assert torch.equal(comp, one) and torch.equal(count, n1)                                   # one label: scipy's own numbering
        comp, count = host_label_ids(ids, [1, 2], 2)
        assert bool(((comp > 0) == (ids > 0)).all()) and int(comp.max()) == int(count.max())
        firsts = [int((comp[0].reshape(-1) == k).nonzero()[0]) for k in range(1, int(count[0]) + 1)]
        assert firsts == sorted(firsts)                                                            # numbered by first voxel
        assert bool((host_fill_holes(ids > 0, 1)[0] >= (ids > 0)).all())
        host_brain_mask_post(ids > 0, 1)
    for c in names:
        kind, batch, shape, connectivity = CASES[c]
        print('%-26s %-16s %d x %s  connectivity %d  %8.1f MB algorithmic' % (c, kind, batch, 'x'.join(map(str, shape)), connectivity,
                                                                              algorithmic_bytes(kind, batch, shape) / 1e6))
    print('scipy %s' % ('imports: the host path is part of the record' if ndi is not None else 'does not import: no host line'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ccl', 'ccl_bench.jsonl'))
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
            raise SystemExit('ccl_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('ccl_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = [ln for ln in p.stdout.strip().splitlines() if ln.startswith('{')][-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        host = r.get('host_ms', {}).get('median')
        print('%-26s device %9.3f ms (%.3f - %.3f)  host %s ms  %.4f of the HBM peak  device/host %s' % (
            c, r['device_ms']['median'], r['device_ms']['min'], r['device_ms']['max'], '%9.1f' % host if host is not None else '        -',
            r['hbm_peak_share'], '%.5f' % r['device_over_host'] if host is not None else '-'), flush=True)


if __name__ == '__main__':
    main()
