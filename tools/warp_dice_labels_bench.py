"""
Timing of fused.warp_dice_labels (csrc/warp_labels.hip) against fused.warp_dice on the one-hot maps of the same label maps.

    python tools/warp_dice_labels_bench.py [--reps 10] [--out profiles/warp_dice_labels/warp_dice_labels_bench.jsonl] [--cases NAME,...]
    python tools/warp_dice_labels_bench.py --dry     # CPU rehearsal: cases, byte counts, workspaces, the inputs at a toy size; measures nothing

Cases: the bench field (synth.cfg2_batch: blob labels = arg-max of its one-hot maps, smooth displacement) at 4 x 160^3 and 1 x 160^3 with
32 labels and at 4 x 160^3 with 4, 33 and 100 labels; synth.rough_displacement at 4 x 160^3 x 32; i.i.d. label ids (the worst case for
the loop over the distinct ids of a wave) at 4 x 160^3 x 32.  Each case is timed forward and forward + backward (gradient wrt the field).
Alternatives, in the same process on the same inputs, alternated inside every repetition after a warm-up of all of them, device events:
    labels        warp_dice_labels on the int32 label maps
    onehot_f32    warp_dice on float32 one-hot maps built beforehand     (33 labels: SpatialTransformer -> Dice, there is no fused form)
    onehot_bf16   the same on bfloat16 maps                              (forward only: the bfloat16 form has no backward)
    build_f32     building the two float32 one-hot maps from the label maps, then onehot_f32
The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at the first child that fails
or runs out of time.  A child compares `labels` with `onehot_f32` first (largest relative difference of dice and of the gradient in the
record), then times and appends one JSON line: median / min / max ms of every alternative, the ratio labels / alternative, the share of
the 8 TB/s HBM peak that the algorithmic bytes (20 B per voxel forward: 12 B of field, 4 B of fixed id and 4 B of moving id; 32 B per voxel
forward + backward: 12 B of gradient on top) over the median of `labels` come to, and the library build id.
`not_slower_than_onehot_f32` is the condition the op is held to on the bench field at 32 labels.  A time needs a GPU: without one the tool
fails.
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
from neurite_amd import _lib, synth                                                                # noqa: E402

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 240
BYTES_PER_VOXEL = {'fwd': 20, 'fwdbwd': 32}
# name: (batch, size, labels, input kind)
CASES = {
    'bench_4x160_L32': (4, 160, 32, 'bench'),
    'bench_1x160_L32': (1, 160, 32, 'bench'),
    'bench_4x160_L4': (4, 160, 4, 'bench'),
    'bench_4x160_L33': (4, 160, 33, 'bench'),
    'bench_4x160_L100': (4, 160, 100, 'bench'),
    'rough_4x160_L32': (4, 160, 32, 'rough'),
    'iid_4x160_L32': (4, 160, 32, 'iid'),
}


def make_inputs(batch, size, L, kind, dev):
    """int32 label maps [B, S, S, S] and the field [B, S, S, S, 3]"""
    if kind == 'iid':
        g = torch.Generator(device=dev).manual_seed(0)
        mov = torch.randint(0, L, (batch, size, size, size), generator=g, device=dev, dtype=torch.int32)
        fix = torch.randint(0, L, (batch, size, size, size), generator=g, device=dev, dtype=torch.int32)
        trf = torch.stack([synth.smooth_displacement(102 + 3 * b, size, device=dev) for b in range(batch)])
        return mov, fix, trf
    M, Fx, trf = synth.cfg2_batch(batch, size, L, device=dev, rough=(kind == 'rough'))
    return M.argmax(-1).to(torch.int32), Fx.argmax(-1).to(torch.int32), trf


def one_hot(lab, L, dtype=torch.float32):
    out = torch.zeros(tuple(lab.shape) + (L,), dtype=dtype, device=lab.device)
    out.scatter_(-1, lab.long().unsqueeze(-1), 1.0)
    return out


def make_alternatives(mov, fix, trf, L):
    """{direction: {name: callable}}; the callables return (dice,) or (dice, gradient)"""
    M, Fx = one_hot(mov, L), one_hot(fix, L)
    fused = L % 4 == 0
    w = torch.rand((mov.shape[0], L), generator=torch.Generator(device=mov.device).manual_seed(1), device=mov.device) + 0.5

    def labels(t):
        return ne.fused.warp_dice_labels(mov, t, fix, L)

    def onehot(t, m=M, f=Fx):
        if fused:
            return ne.fused.warp_dice(m, t, f)
        with ne.deferred.scope(False):
            return ne.metrics.Dice(check_input_limits=False).dice(f, ne.layers.SpatialTransformer()([m, t]))

    def build(t):
        return onehot(t, one_hot(mov, L), one_hot(fix, L))

    tg = trf.clone().requires_grad_(True)

    def bwd(fn):
        def run():
            d = fn(tg)
            return d, torch.autograd.grad(d, (tg,), w)[0]
        return run

    fwd = {'labels': lambda: (labels(trf),), 'onehot_f32': lambda: (onehot(trf),), 'build_f32': lambda: (build(trf),)}
    if fused:
        M16, F16 = M.bfloat16(), Fx.bfloat16()
        fwd['onehot_bf16'] = lambda: (ne.fused.warp_dice(M16, trf, F16),)
    return {'fwd': fwd, 'fwdbwd': {'labels': bwd(labels), 'onehot_f32': bwd(onehot), 'build_f32': bwd(build)}}


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
    batch, size, L, kind = CASES[name]
    if not torch.cuda.is_available():
        raise SystemExit('warp_dice_labels_bench: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    mov, fix, trf = make_inputs(batch, size, L, kind, dev)
    alts = make_alternatives(mov, fix, trf, L)
    nvox = batch * size ** 3
    rec = {'case': name, 'batch': batch, 'size': size, 'labels': L, 'inputs': kind, 'reps': reps, 'voxels': nvox,
           'baseline': 'fused.warp_dice' if L % 4 == 0 else 'SpatialTransformer -> Dice',
           'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    got, want = alts['fwdbwd']['labels'](), alts['fwdbwd']['onehot_f32']()
    rec['max_rel_diff_vs_onehot_f32'] = [float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(got, want)]
    del got, want
    for direction, fns in alts.items():
        for _ in range(2):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = timed(fns, reps)
        nbytes = BYTES_PER_VOXEL[direction] * nvox
        rec[direction] = {'ms': t, 'algorithmic_bytes': nbytes,
                          'labels_over': {k: t['labels']['median'] / v['median'] for k, v in t.items() if k != 'labels'},
                          'hbm_peak_share': nbytes / (t['labels']['median'] * 1e-3) / HBM_PEAK,
                          'not_slower_than_onehot_f32': t['labels']['median'] <= t['onehot_f32']['median']}
    return rec


def dry(names):
    """what can be rehearsed without a device: the cases, their byte counts and workspaces, and the inputs at a toy size on the CPU"""
    for c in names:
        batch, size, L, kind = CASES[c]
        ws = _lib.lib().nrt_warp_dice_labels_workspace_bytes(_lib.ints([size] * 3), L, batch)
        ws_oh = _lib.lib().nrt_warp_dice_workspace_bytes(_lib.ints([size] * 3), L, batch, 0) if L % 4 == 0 else 0
        mov, fix, trf = make_inputs(2, 12, L, kind, 'cpu')
        M = one_hot(mov, L)
        assert mov.dtype == torch.int32 and mov.shape == (2, 12, 12, 12) and trf.shape == (2, 12, 12, 12, 3) and fix.shape == mov.shape
        assert M.shape == (2, 12, 12, 12, L) and bool((M.sum(-1) == 1).all()) and bool((M.argmax(-1) == mov).all())
        nvox = batch * size ** 3
        print('%-18s %d x %d^3 x %-3d %-6s labels %6.1f MB  one-hot f32 %8.1f MB  algorithmic fwd %6.1f MB fwd+bwd %6.1f MB  workspace %6.2f MB '
              '(one-hot form %6.2f MB)' % (c, batch, size, L, kind, 2 * nvox * 4 / 1e6, 2 * nvox * L * 4 / 1e6, BYTES_PER_VOXEL['fwd'] * nvox / 1e6,
                                          BYTES_PER_VOXEL['fwdbwd'] * nvox / 1e6, ws / 1e6, ws_oh / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'warp_dice_labels', 'warp_dice_labels_bench.jsonl'))
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
            raise SystemExit('warp_dice_labels_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('warp_dice_labels_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        for direction in ('fwd', 'fwdbwd'):
            d = r[direction]
            print('%-18s %-6s ' % (c, direction) + '  '.join('%s %.3f ms' % (k, v['median']) for k, v in d['ms'].items()) +
                  '  labels/onehot_f32 %.3f  %.3f of the HBM peak  diff %.2g' % (d['labels_over']['onehot_f32'], d['hbm_peak_share'],
                                                                               max(r['max_rel_diff_vs_onehot_f32'])))


if __name__ == '__main__':
    main()
