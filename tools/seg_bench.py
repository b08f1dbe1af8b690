"""
Timing of neurite_amd.seg (csrc/seg.hip) against torch restatements on the same tensors, in the same process.

    python tools/seg_bench.py [--reps 10] [--out profiles/seg/seg_bench.jsonl] [--cases NAME,...]
    python tools/seg_bench.py --dry       # CPU rehearsal: case names, shapes, byte counts; measures nothing

Cases:
    argmax_{f32,bf16}[_prob]   the arg-max of a 4 x 160^3 x 32 probability map into int32 labels, without and with the probability of
                               the arg-max in the same pass, against torch.argmax(x, -1) (with: + gather / sum / divide in torch).  The
                               float32 ones also time soft Dice on two maps of that shape and record its bytes / s.
    quilt_{mean,median}        343 int32 label patches of 64^3 at stride 32 into 256^3, against a torch restatement of the mean (a sum
                               and a count volume, one slice-add of each per patch, then a divide).
    predict_volume_{mean,median}   predict_volume on a 256^3 x 1 scan with the BASELINE config 3 unet (16 features, 3 levels, 32 labels,
                               feat_mult 2) on 64^3 patches at stride 32, batch 7, against the same loop built from torch slicing,
                               torch.argmax and the torch quilt (a mean, whichever reducer the kernel side runs).

The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at the first child that
fails or runs out of time.  A child checks the kernel against the restatement first, then times, with device events around the whole
Python call, the two alternated inside every repetition after a warm-up of both, and appends one JSON line: median / min / max ms of
each, the share of the 8 TB/s HBM peak that the algorithmic bytes (every input read once, every output written once) over the median
come to, the ratio kernel / torch and the library build id.  A time needs a GPU: without one the tool fails.
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
from neurite_amd import _lib, seg                                                                  # noqa: E402

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 240
MAP = (4, 160, 160, 160, 32)
SCAN, PATCH, STRIDE, GRID, LABELS, BATCH = (256, 256, 256), (64, 64, 64), (32, 32, 32), (7, 7, 7), 32, 7
CASES = ['argmax_f32', 'argmax_f32_prob', 'argmax_bf16', 'argmax_bf16_prob', 'quilt_mean', 'quilt_median', 'predict_volume_mean',
         'predict_volume_median']


def algorithmic_bytes(name):
    if name.startswith('argmax'):
        nvox = int(np.prod(MAP[:-1]))
        return nvox * MAP[-1] * (2 if 'bf16' in name else 4) + nvox * 4 * (2 if name.endswith('prob') else 1)
    if name.startswith('quilt'):
        return (int(np.prod(GRID)) * int(np.prod(PATCH)) + int(np.prod(SCAN))) * 4
    return None                                                     # predict_volume: the network dominates, no byte count


def torch_quilt_mean(patches, patch, grid, stride):
    """[N, *patch] -> the mean over the covering patches: a sum and a count volume, one slice-add per patch"""
    shape = tuple((g - 1) * s + p for g, s, p in zip(grid, stride, patch))
    total = torch.zeros(shape, dtype=torch.float32, device=patches.device)
    count = torch.zeros(shape, dtype=torch.float32, device=patches.device)
    for n in range(patches.shape[0]):
        idx = np.unravel_index(n, grid)
        win = tuple(slice(int(i) * s, int(i) * s + p) for i, s, p in zip(idx, stride, patch))
        total[win] += patches[n].reshape(patch)
        count[win] += 1
    return total / count


def torch_predict_volume(model, vol, patch, stride, batch_size):
    shape = tuple(vol.shape[:-1])
    grid = tuple((v - p) // s + 1 for v, p, s in zip(shape, patch, stride))
    N = int(np.prod(grid))
    labels = torch.empty((N,) + tuple(patch), dtype=torch.float32, device=vol.device)
    for start in range(0, N, batch_size):
        wins = []
        for n in range(start, min(start + batch_size, N)):
            idx = np.unravel_index(n, grid)
            wins.append(vol[tuple(slice(int(i) * s, int(i) * s + p) for i, s, p in zip(idx, stride, patch))])
        with torch.no_grad():
            pred = model(torch.stack(wins))
        labels[start:start + len(wins)] = torch.argmax(pred, -1)
    return torch_quilt_mean(labels, patch, grid, stride).to(torch.int64)


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
    if not torch.cuda.is_available():
        raise SystemExit('seg_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rec = {'case': name, 'reps': reps, 'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    extra = {}
    if name.startswith('argmax'):
        dtype = torch.bfloat16 if 'bf16' in name else torch.float32
        with_prob = name.endswith('prob')
        x = (torch.rand(MAP, generator=g, device=dev) + 0.01).to(dtype)
        labels = torch.empty(MAP[:-1], dtype=torch.int32, device=dev)
        prob = torch.empty(MAP[:-1], dtype=torch.float32, device=dev) if with_prob else None

        def kernel():
            seg._argmax(x, labels=labels, prob=prob)
            return labels, prob

        def eager():
            idx = torch.argmax(x, -1)
            if not with_prob:
                return idx, None
            xf = x.float()
            return idx, xf.gather(-1, idx[..., None])[..., 0] / xf.sum(-1)
        lab_k, prob_k = kernel()
        lab_e, prob_e = eager()
        rec['labels_equal'] = bool(torch.equal(lab_k.long(), lab_e))
        if with_prob:
            rec['max_rel_diff_vs_torch'] = float(((prob_k - prob_e).abs() / prob_e).max())
        rec.update(shape=list(MAP), dtype=str(dtype).replace('torch.', ''))
        if dtype == torch.float32 and not with_prob:
            other = torch.rand(MAP, generator=g, device=dev)
            dice = ne.metrics.Dice(check_input_limits=False)
            extra['dice'] = lambda: dice.dice(x, other)
    elif name.startswith('quilt'):
        N = int(np.prod(GRID))
        patches = torch.randint(0, LABELS, (N,) + PATCH, generator=g, device=dev, dtype=torch.int32)
        func = name.split('_')[1]

        def kernel():
            return seg.quilt(patches, PATCH, GRID, STRIDE, nan_func=func)

        def eager():
            return torch_quilt_mean(patches, PATCH, GRID, STRIDE)
        if func == 'mean':
            rec['max_abs_diff_vs_torch'] = float((kernel() - eager()).abs().max())
        rec.update(patches=[N] + list(PATCH), volume=list(SCAN), dtype='int32')
    else:
        func = name.split('_')[2]
        torch.manual_seed(5)
        net = ne.models.unet(16, PATCH + (1,), 3, 3, LABELS, feat_mult=2).to(dev)
        vol = torch.randn(SCAN + (1,), generator=g, device=dev)

        def kernel():
            return seg.predict_volume(net, vol, PATCH, STRIDE, batch_size=BATCH, nan_func=func)

        def eager():
            return torch_predict_volume(net, vol, PATCH, STRIDE, BATCH)
        if func == 'mean':
            rec['labels_equal_share'] = float((kernel() == eager()).float().mean())
        rec.update(scan=list(SCAN), patch=list(PATCH), stride=list(STRIDE), batch_size=BATCH, nb_labels=LABELS)
    fns = dict(kernel=kernel, eager=eager, **extra)
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = timed(fns, reps)
    rec.update(kernel_ms=t['kernel'], torch_ms=t['eager'], kernel_over_torch=t['kernel']['median'] / t['eager']['median'])
    nbytes = algorithmic_bytes(name)
    if nbytes:
        rec.update(algorithmic_bytes=nbytes, bytes_per_s=nbytes / (t['kernel']['median'] * 1e-3))
        rec['hbm_peak_share'] = rec['bytes_per_s'] / HBM_PEAK
    if 'dice' in t:
        rec['dice_ms'] = t['dice']
        rec['dice_bytes_per_s'] = 2 * int(np.prod(MAP)) * 4 / (t['dice']['median'] * 1e-3)
        rec['bytes_per_s_over_dice'] = rec['bytes_per_s'] / rec['dice_bytes_per_s']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seg', 'seg_bench.jsonl'))
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
            b = algorithmic_bytes(c)
            print('%-24s %s' % (c, '%10.1f MB' % (b / 1e6) if b else 'scan %s, patches %s at stride %s' % (SCAN, PATCH, STRIDE)))
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for c in names:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', c, '--reps', str(args.reps)], capture_output=True,
                               text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit('seg_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('seg_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        print('%-24s kernel %9.3f ms  torch %9.3f ms  kernel/torch %.3f%s%s' % (
            c, r['kernel_ms']['median'], r['torch_ms']['median'], r['kernel_over_torch'],
            '  %.2f of the HBM peak' % r['hbm_peak_share'] if 'hbm_peak_share' in r else '',
            '  bytes/s over soft Dice %.2f' % r['bytes_per_s_over_dice'] if 'bytes_per_s_over_dice' in r else ''))


if __name__ == '__main__':
    main()
