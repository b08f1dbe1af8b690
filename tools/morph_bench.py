"""
Timing of the binary morphology, the box minimum / maximum filters and the box median (csrc/morph.hip) against the two routes they
replace, on the same tensors in the same process.

    python tools/morph_bench.py [--reps 10] [--out profiles/morphology/morph_bench.jsonl] [--cases NAME,...] [--no-host] [--host-cases NAME,...]
    python tools/morph_bench.py --dry      # CPU rehearsal: the cases, the eager and the host route at a toy size; measures nothing

Cases, each at 1 x 160^3, 4 x 160^3 and 4 x 256^2: binary_erosion / dilation / opening / closing of a blob mask (thresholded smoothed
noise, half set, bool) at connectivity 1 and the full box, 1, 3 and 8 iterations, border_value 0; minimum_filter and maximum_filter of
a smooth float32 image at sizes 3, 9 and 31 (mode 'nearest'); median_filter at 3 x 3 x 3 and 1 x 5 x 5 (3 x 3 and 5 x 5 in 2-D).
`steps_*`: 8 dilations at 4 x 160^3 as 8 calls of 1 iteration, 4 of 2 and 2 of 4 -- the launches a kernel limited to 1, 2 or 4 steps
per launch would make, with the tile that goes with each (how the steps per launch were chosen).
The routes it is timed against:
  eager   torch on the device: max_pool3d / max_pool2d for the box dilation and the maximum filter (the minimum by negation; its
          padding is -inf, so the edges differ from 'nearest': equality is checked on the interior), conv3d / conv2d with the structure
          and a threshold for the other binary cases (zero padding is border_value 0: checked everywhere), replicate-pad + unfold +
          kthvalue for the median (checked everywhere)
  host    what a user does today: device -> host, scipy.ndimage, host -> device; one repetition, if scipy imports
Each route warms up, sizes an inner loop so that a timed window holds about 20 ms of work, and times with device events (median of
--reps windows, with min and max).  One JSON line per case: ms per call of each route, the ratios, the algorithmic bytes (every voxel
read once and written once: 1 + 1 B for a bool mask, 4 + 4 B for an image) per second as a share of the 8 TB/s HBM peak, and the
library build id.  A time needs a GPU: without one the tool fails.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neurite_amd as ne                                                                           # noqa: E402
from neurite_amd import _lib                                                                       # noqa: E402

HBM_PEAK = 8.0e12
WINDOW_MS = 20.0
SHAPES = {'1x160^3': (1, 160, 160, 160), '4x160^3': (4, 160, 160, 160), '4x256^2': (4, 256, 256)}
# name -> (family, shape name, op, parameter, iterations)
CASES = {}
for _s in SHAPES:
    for _op in ('erosion', 'dilation', 'opening', 'closing'):
        for _c in ('conn1', 'box'):
            for _n in (1, 3, 8):
                CASES['binary_%s_%s_n%d_%s' % (_op, _c, _n, _s)] = ('binary', _s, _op, _c, _n)
    for _op in ('minimum', 'maximum'):
        for _k in (3, 9, 31):
            CASES['%s_%d_%s' % (_op, _k, _s)] = ('minmax', _s, _op, _k, 1)
    for _k in ('3', '5x5'):
        CASES['median_%s_%s' % (_k, _s)] = ('median', _s, 'median', _k, 1)
for _k in (1, 2, 4):
    CASES['steps_%d_4x160^3' % _k] = ('steps', '4x160^3', 'dilation', 'conn1', _k)
STAGES = {'erosion': (0,), 'dilation': (1,), 'opening': (0, 1), 'closing': (1, 0)}


def smooth_noise(shape, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g).to(dev).unsqueeze(1)
    pool = F.avg_pool3d if len(shape) == 4 else F.avg_pool2d
    for _ in range(2):
        x = pool(x, 5, 1, 2, count_include_pad=False)
    return x.squeeze(1).contiguous()


def structure(kind, nd):
    conn = 1 if kind == 'conn1' else nd
    return torch.from_numpy((np.abs(np.indices((3,) * nd) - 1).sum(0) <= conn).astype(np.float32))


def median_size(kind, nd):
    return ((3,) * nd) if kind == '3' else ((1, 5, 5) if nd == 3 else (5, 5))


def eager_binary(m, st, stages, iterations, box):
    """m bool [B, *S]; border_value 0"""
    nd = m.dim() - 1
    conv, pool = (F.conv3d, F.max_pool3d) if nd == 3 else (F.conv2d, F.max_pool2d)
    x = m.unsqueeze(1).float()
    w = st.to(m.device).view((1, 1) + (3,) * nd)
    count = float(st.sum())
    for dilate in stages:
        for _ in range(iterations):
            if dilate and box:
                x = pool(x, 3, 1, 1)
            elif dilate:
                x = (conv(x, w.flip(tuple(range(2, 2 + nd))), padding=1) > 0.5).float()
            else:
                x = (conv(x, w, padding=1) > count - 0.5).float()
    return x.squeeze(1) > 0.5


def eager_minmax(x, size, want_max):
    pool = F.max_pool3d if x.dim() == 4 else F.max_pool2d
    y = x.unsqueeze(1)
    return (pool(y, size, 1, size // 2) if want_max else -pool(-y, size, 1, size // 2)).squeeze(1)


def eager_median(x, sizes):
    nd = x.dim() - 1
    pad = []
    for s in reversed(sizes):
        pad += [s // 2, s // 2]
    y = F.pad(x.unsqueeze(1), pad, mode='replicate').squeeze(1)
    for a, s in enumerate(sizes):
        y = y.unfold(1 + a, s, 1)
    n = int(np.prod(sizes))
    return y.reshape(x.shape + (n,)).kthvalue(n // 2 + 1, dim=-1).values


def host_call(family, x, op, param, iterations):
    from scipy import ndimage
    h = x.cpu().numpy()
    nd = h.ndim - 1
    if family == 'binary':
        fn = getattr(ndimage, 'binary_' + op)
        st = ndimage.generate_binary_structure(nd, 1 if param == 'conn1' else nd)
        out = np.stack([fn(v, structure=st, iterations=iterations) for v in h])
    elif family == 'minmax':
        fn = ndimage.minimum_filter if op == 'minimum' else ndimage.maximum_filter
        out = np.stack([fn(v, size=param, mode='nearest') for v in h])
    else:
        out = np.stack([ndimage.median_filter(v, size=median_size(param, nd), mode='nearest') for v in h])
    return torch.from_numpy(out).to(x.device)


def make_calls(name, dev, toy=False):
    """(device, eager, host, input, how to compare): callables"""
    family, shape_name, op, param, iterations = CASES[name]
    shape = SHAPES[shape_name]
    if toy:
        shape = shape[:1] + (12,) * (len(shape) - 1)
    nd = len(shape) - 1
    field = smooth_noise(shape, dev)
    if family in ('binary', 'steps'):
        m = field > field.median()
        st = structure(param, nd)
        device = None
        if dev.type == 'cuda':
            fn = getattr(ne.utils, 'binary_' + op)
            arg = 1 if param == 'conn1' else nd
            if family == 'steps':
                per = iterations

                def device():
                    out = m
                    for _ in range(8 // per):
                        out = fn(out, arg, per, batched=True)
                    return out
            else:
                def device():
                    return fn(m, arg, iterations, batched=True)
        total = 8 if family == 'steps' else iterations
        return device, (lambda: eager_binary(m, st, STAGES[op], total, param == 'box')), \
            (lambda: host_call('binary', m, op, param, total)), m, 'all'
    if family == 'minmax':
        size = min(param, 11) if toy else param
        fn = getattr(ne.utils, op + '_filter') if dev.type == 'cuda' else None
        return (lambda: fn(field, size, 'nearest', batched=True)), (lambda: eager_minmax(field, size, op == 'maximum')), \
            (lambda: host_call('minmax', field, op, size, 1)), field, size // 2
    sizes = median_size(param, nd)
    fn = ne.utils.median_filter if dev.type == 'cuda' else None
    return (lambda: fn(field, sizes, 'nearest', batched=True)), (lambda: eager_median(field, sizes)), \
        (lambda: host_call('median', field, op, param, 1)), field, 'all'


def same(a, b, how):
    if how != 'all' and how > 0:                                                               # the interior: the paddings differ
        cut = (slice(None),) + (slice(how, -how),) * (a.dim() - 1)
        a, b = a[cut], b[cut]
    return bool(torch.equal(a, b))


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


def host_timed(fn):
    """a route that ends on the host: wall clock around a call that starts and ends synchronised"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run_case(name, reps, host):
    family, shape_name, op, param, iterations = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('morph_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    device, eager, on_host, x, how = make_calls(name, dev)
    rec = {'case': name, 'family': family, 'shape': list(SHAPES[shape_name]), 'op': op, 'param': param, 'iterations': iterations,
           'reps': reps, 'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    got = device()
    rec['equals_eager'] = same(got, eager(), how)
    t, inner = measure(device, reps)
    nbytes = 2 * x.numel() * x.element_size()
    rec.update(calls_per_window=inner, algorithmic_bytes=nbytes, device_ms=t)
    rec['bytes_per_s'] = nbytes / (t['median'] * 1e-3)
    rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    rec['eager_ms'], _ = measure(eager, reps)
    rec['device_over_eager'] = t['median'] / rec['eager_ms']['median']
    have_scipy = True
    try:
        import scipy.ndimage                                                                       # noqa: F401
    except ImportError:
        have_scipy = False
    if host and have_scipy and family != 'steps':
        ms, out = host_timed(on_host)
        rec['host_ms'] = ms
        rec['equals_host'] = bool(torch.equal(got, out))
        rec['device_over_host'] = t['median'] / ms
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases, their inputs at a toy size, the eager and the host route against each other"""
    cpu = torch.device('cpu')
    for c in names:
        _, eager, on_host, x, how = make_calls(c, cpu, toy=True)
        want = eager()
        try:
            ok = same(on_host(), want, how)
        except ImportError:
            ok = None
        print('%-40s eager == host at a toy size: %s   %8.1f MB algorithmic' % (
            c, ok, 2 * int(np.prod(SHAPES[CASES[c][1]])) * x.element_size() / 1e6))
        assert ok is not False, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'morphology', 'morph_bench.jsonl'))
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--no-host', action='store_true', help='skip the scipy route')
    ap.add_argument('--host-cases', default=None, help='the scipy route for these cases only (default: every case)')
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
        r = run_case(c, args.reps, not args.no_host and (args.host_cases is None or c in args.host_cases.split(',')))
        with open(args.out, 'a') as f:
            f.write(json.dumps(r) + '\n')
        host = r.get('host_ms')
        print('%-40s device %8.3f ms (%.3f - %.3f)  eager %8.3f ms  host %s ms  %.4f of the HBM peak  == eager %s  == host %s' % (
            c, r['device_ms']['median'], r['device_ms']['min'], r['device_ms']['max'], r['eager_ms']['median'],
            '%9.1f' % host if host is not None else '        -', r['hbm_peak_share'], r['equals_eager'], r.get('equals_host')), flush=True)


if __name__ == '__main__':
    main()
