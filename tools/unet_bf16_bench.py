#!/usr/bin/env python3
"""BASELINE config 3 forward in float32 and in bfloat16 (models.ConvNet bf16 path), one JSON line.

    python tools/unet_bf16_bench.py [--reps 20] [--warmup 5] [--kernel-stats STATS.csv] [--out FILE]
    python tools/unet_bf16_bench.py --trace N      # N bf16 forwards only: run under rocprofv3 --kernel-trace --stats

Config 3 with the SURVEY 8(d) seeds (weights N(0, glorot) seed 5 in Keras layout, biases N(0, 0.01), input N(0, 1) seed 4);
the bf16 model is the float32 one converted with .bfloat16().  The fp32 and bf16 forwards alternate in one process; each is
timed with device events, median of `reps` runs after `warmup` warm-ups.  Per layer: the layer's own kernel(s) timed the same
way on the tensors of one bf16 forward, with TFLOP/s against the dense bf16 MFMA peak (2.5 PFLOP/s) for the convolutions and
bytes/s against 8 TB/s for the HBM-bound layers (first convolution, pooling, head).  Agreement of the bf16 prediction with the
float32 one: argmax agreement (all voxels, and where float32's top-two margin exceeds 0.05) and max |dp|.
With --kernel-stats, the per-kernel averages of a rocprofv3 --stats CSV of a --trace run are attached.
"""
import argparse
import contextlib
import copy
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import neurite_amd as ne                      # noqa: E402
from neurite_amd import models as nm          # noqa: E402

BF16_PEAK_TFLOPS = 2500.0
HBM_TBS = 8.0
S = 160


def build(dev):
    with contextlib.redirect_stdout(sys.stderr):
        model = ne.models.unet(16, (S, S, S, 1), 3, 3, 32, feat_mult=2)
    rng = np.random.default_rng(5)
    with torch.no_grad():
        for name in model.layer_names:
            m = model.layers_by_name[name] if name in model.layers_by_name else None
            if isinstance(m, nm._Conv):
                k = m.kernel.shape
                fan_in, fan_out = int(np.prod(k[:-1])), int(np.prod(k[:-2])) * k[-1]
                m.kernel.copy_(torch.from_numpy((rng.standard_normal(k) * np.sqrt(2.0 / (fan_in + fan_out))).astype(np.float32)))
                m.bias.copy_(torch.from_numpy((rng.standard_normal(k[-1]) * 0.01).astype(np.float32)))
    model = model.to(dev).eval()
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((1, S, S, S, 1)).astype(np.float32)).to(dev)
    return model, x


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def layer_table(m16, x16, reps, warmup):
    """each layer's kernel(s) on the tensors of one bf16 forward"""
    names = ['unet_input', 'unet_conv_downarm_0_0', 'unet_maxpool_0', 'unet_conv_downarm_1_0', 'unet_maxpool_1',
             'unet_conv_downarm_2_0', 'unet_conv_uparm_3_0', 'unet_conv_uparm_4_0']
    with torch.no_grad():
        t = m16(x16, return_tensors=names)
    L = m16.layers_by_name
    V = float(S ** 3)
    rows = []

    def conv(name, src, lo=None, up=None, hbm=False):
        m = L[name]
        vout = float(np.prod(src.shape[1:4]))
        gflop = 2 * vout * m.cin * m.cout * int(np.prod(m.ksize3)) / 1e9
        nbytes = 2 * (src.numel() + (0 if lo is None else lo.numel()) + vout * m.cout)
        with torch.no_grad():
            ms = float(np.median(timed(lambda: m.run_bf16(src, lo, up), reps, warmup)))
        r = {'layer': name, 'ms': round(ms, 4), 'gflop': round(gflop, 2), 'tflops': round(gflop / ms, 1),
             'of_bf16_mfma_peak': round(gflop / ms / BF16_PEAK_TFLOPS, 4)}
        if hbm:
            r.update({'gbytes': round(nbytes / 1e9, 4), 'tbytes_per_s': round(nbytes / ms / 1e9, 3),
                      'of_8tbs': round(nbytes / ms / 1e9 / HBM_TBS, 4)})
        rows.append(r)

    def mem(name, fn, nbytes):
        with torch.no_grad():
            ms = float(np.median(timed(fn, reps, warmup)))
        rows.append({'layer': name, 'ms': round(ms, 4), 'gbytes': round(nbytes / 1e9, 4), 'tbytes_per_s': round(nbytes / ms / 1e9, 3),
                     'of_8tbs': round(nbytes / ms / 1e9 / HBM_TBS, 4)})

    conv('unet_conv_downarm_0_0', t['unet_input'], hbm=True)
    a = t['unet_conv_downarm_0_0']
    mem('unet_maxpool_0', lambda: nm._maxpool(a, (2, 2, 2), 'same'), 2 * (a.numel() + a.numel() / 8))
    conv('unet_conv_downarm_1_0', t['unet_maxpool_0'])
    b = t['unet_conv_downarm_1_0']
    mem('unet_maxpool_1', lambda: nm._maxpool(b, (2, 2, 2), 'same'), 2 * (b.numel() + b.numel() / 8))
    conv('unet_conv_downarm_2_0', t['unet_maxpool_1'])
    conv('unet_conv_uparm_3_0', t['unet_conv_downarm_1_0'], t['unet_conv_downarm_2_0'], (2, 2, 2))
    conv('unet_conv_uparm_4_0', t['unet_conv_downarm_0_0'], t['unet_conv_uparm_3_0'], (2, 2, 2))
    h, f = L['unet_likelihood'], t['unet_conv_uparm_4_0']
    mem('unet_likelihood+prediction', lambda: nm._conv1x1_softmax(f, h.kernel, h.bias, True), 2 * (f.numel() + V * h.cout))
    return rows


def kernel_stats(path):
    out = {}
    for r in csv.DictReader(open(path)):
        k = r['Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        out[k] = {'calls': int(r['Calls']), 'avg_ms': round(float(r['AverageNs']) * 1e-6, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trace', type=int, default=0)
    ap.add_argument('--kernel-stats')
    ap.add_argument('--out')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    m32, x = build(dev)
    m16 = copy.deepcopy(m32).bfloat16().eval()
    if args.trace:
        with torch.no_grad():
            for _ in range(args.trace):
                m16(x)
        torch.cuda.synchronize()
        return
    with torch.no_grad():
        for _ in range(args.warmup):
            m32(x)
            m16(x)
        t32, t16 = [], []
        for _ in range(args.reps):                     # alternating
            t32 += timed(lambda: m32(x), 1, 0)
            t16 += timed(lambda: m16(x), 1, 0)
        p32 = m32(x)
        p16 = m16(x).float()
    top2 = torch.topk(p32, 2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) > 0.05
    same = p32.argmax(-1) == p16.argmax(-1)
    res = {'workload': 'BASELINE config 3 forward: unet(16, (160,160,160,1), 3, 3, 32, feat_mult=2), batch 1, float32 vs bfloat16 models',
           'fwd_ms_f32': round(float(np.median(t32)), 4), 'fwd_ms_bf16': round(float(np.median(t16)), 4),
           'speedup': round(float(np.median(t32)) / float(np.median(t16)), 3), 'reps': args.reps, 'warmup': args.warmup,
           'agreement': {'argmax_all': round(float(same.float().mean()), 6),
                         'argmax_margin_gt_0.05': round(float(same[sure].float().mean()), 6), 'voxels_margin_gt_0.05': int(sure.sum()),
                         'max_abs_dp': round(float((p16 - p32).abs().max()), 6)},
           'floors_ms': {'compute_283.8_gflop_at_2.5_pflops': 0.114, 'memory_1.15_gb_at_8_tbs': 0.144},
           'layers': layer_table(m16, x, args.reps, args.warmup),
           'build_id': ne._lib.lib().nrt_build_id().decode()}
    res['layers_ms_sum'] = round(sum(r['ms'] for r in res['layers']), 4)
    if args.kernel_stats and os.path.exists(args.kernel_stats):
        res['kernel_stats_rocprofv3'] = kernel_stats(args.kernel_stats)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
