"""
Timing of the two kernels a 2x2x2 'same' convolution can run on -- conv3d_direct (variant 1, what such a layer ran on before the
2x2x2 matrix-core arm existed) and conv3d_mfma_k2 (variant 6) -- on the same tensors, at the shapes of design_dnn's stride-1
"strided" convolution: 16 -> 16, 32 -> 32 and 64 -> 64 channels at 4 x 160^3, 4 x 80^3 and 4 x 40^3, forward (zero padding 0 before /
1 after, ELU epilogue) and input gradient (the transposed layer: 1 before / 0 after, no epilogue), both through nrt_conv3d_pad_f32.

    python tools/conv_even_bench.py [--reps 10] [--out profiles/conv_even/conv_even_bench.jsonl] [--cases NAME,...]
    python tools/conv_even_bench.py --dry       # CPU rehearsal: arguments, shapes, flop and byte counts; measures nothing

The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at the first child that
fails or runs out of time.  A child compares the two outputs first (largest difference over the largest magnitude, in the record),
then times, with device events, the two kernels alternated inside every repetition after a warm-up of both, and appends one JSON
line: median / min / max ms of each, each kernel's run-to-run spread (max - min) / median, the flops 2 * voxels * 8 * cin * cout over
the median, and `k2_faster`: whether the arm's median is below the direct kernel's by more than the larger of the two spreads --
the condition csrc/conv.hip: k2_auto() may rest on.  A time needs a GPU: without one the tool fails.
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
from neurite_amd import _lib                                                                       # noqa: E402

CASE_TIMEOUT_S = 240
BATCH = 4
CASES = {'%s_c%d_s%d' % (d, c, s): (d, c, s) for s in (160, 80, 40) for c in (16, 32, 64) for d in ('fwd', 'dgrad')}


def flops(c, s):
    return 2.0 * BATCH * s ** 3 * 8 * c * c


def run_case(name, reps):
    direction, c, s = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('conv_even_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    lib = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((BATCH, s, s, s, c), generator=g, device=dev)
    w = torch.randn((2, 2, 2, c, c), generator=g, device=dev) / (8 * c) ** 0.5
    bias = torch.randn((c,), generator=g, device=dev) * 0.1
    k3, S = _lib.ints([2, 2, 2]), _lib.ints([s, s, s])
    n = lib.nrt_conv3d_packed_weight_floats(k3, c, c)
    packed = torch.empty(int(n), device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(lib.nrt_conv3d_pack_weights_f32(_lib.ptr(w), k3, c, c, _lib.ptr(packed), st))
    pad = _lib.ints([0, 0, 0] if direction == 'fwd' else [1, 1, 1])
    act = 1 if direction == 'fwd' else 0
    outs = {v: torch.empty_like(x) for v in (1, 6)}

    def run(variant):
        _lib.check(lib.nrt_conv3d_pad_f32(_lib.ptr(x), c, None, 0, None, _lib.ptr(w), _lib.ptr(packed),
                                          _lib.ptr(bias) if direction == 'fwd' else None, _lib.ptr(outs[variant]), BATCH, S, k3, c, 1, pad,
                                          act, variant, st), 'variant %d' % variant)

    for v in (1, 6):
        run(v)
    torch.cuda.synchronize()
    diff = float((outs[1] - outs[6]).abs().max() / outs[1].abs().max())
    for _ in range(2):
        run(1)
        run(6)
    torch.cuda.synchronize()
    times = {1: [], 6: []}
    for _ in range(reps):
        for v in (1, 6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(v)
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1))
    rec = {'case': name, 'direction': direction, 'batch': BATCH, 'size': s, 'channels': c, 'reps': reps, 'flops': flops(c, s),
           'max_diff_over_scale': diff, 'build_id': lib.nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    for key, v in (('direct', 1), ('k2', 6)):
        t = times[v]
        rec[key + '_ms'] = {'median': float(np.median(t)), 'min': float(np.min(t)), 'max': float(np.max(t))}
        rec[key + '_spread'] = (rec[key + '_ms']['max'] - rec[key + '_ms']['min']) / rec[key + '_ms']['median']
        rec[key + '_tflops'] = rec['flops'] / (rec[key + '_ms']['median'] * 1e-3) / 1e12
    rec['k2_over_direct'] = rec['k2_ms']['median'] / rec['direct_ms']['median']
    rec['k2_faster'] = bool(rec['k2_ms']['median'] * (1.0 + max(rec['k2_spread'], rec['direct_spread'])) < rec['direct_ms']['median'])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_even', 'conv_even_bench.jsonl'))
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
            d, ch, s = CASES[c]
            print('%-20s %d x %d^3  %2d -> %2d  %8.2f GFLOP  tensors 2 x %7.1f MB' % (c, BATCH, s, ch, ch, flops(ch, s) / 1e9,
                                                                                BATCH * s ** 3 * ch * 4 / 1e6))
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for c in names:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', c, '--reps', str(args.reps)], capture_output=True,
                               text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit('conv_even_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('conv_even_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        print('%-20s direct %9.3f ms (spread %.2f)  k2 %9.3f ms (spread %.2f)  k2/direct %.2f  faster: %s' % (
            c, r['direct_ms']['median'], r['direct_spread'], r['k2_ms']['median'], r['k2_spread'], r['k2_over_direct'], r['k2_faster']))


if __name__ == '__main__':
    main()
