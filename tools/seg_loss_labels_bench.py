"""
Timing of the segmentation loss pair on an integer label map (fused.seg_loss_labels, csrc/segloss_labels.hip) against the same pair on the
float32 one-hot map of that label map (metrics._SegLossFn, csrc/segloss.hip).

    python tools/seg_loss_labels_bench.py [--reps 10] [--out profiles/seg_loss_labels/seg_loss_labels_bench.jsonl] [--cases NAME,...]
    python tools/seg_loss_labels_bench.py --dry     # CPU rehearsal: cases, byte counts, workspaces, the inputs at a toy size; measures nothing

Cases: blob labels (synth.cfg2_batch: the arg-max of its one-hot maps, as tools/warp_dice_labels_bench.py takes them) and y_pred = the
soft-max of seeded noise, at 4 x 160^3 and 1 x 160^3 with 32 labels and at 4 x 160^3 with 4, 24 and 33 labels; and one training step of the
BASELINE config 3 unet (1 x 160^3 x 32) with either target.  Each loss case is timed forward and forward + backward (gradient wrt y_pred, a leaf).
Alternatives, in the same process on the same inputs, alternated inside every repetition after a warm-up of all of them, device events:
    labels    seg_loss_labels on the int32 label map
    onehot    _SegLossFn on a float32 one-hot map built beforehand  (24 and 33 labels: the two separate losses, there is no joint one-hot kernel)
    build     building the float32 one-hot map from the label map on the device, then onehot
The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at the first child that fails
or runs out of time.  A child compares `labels` with `onehot` first (largest relative difference of the CCE sum, of dice and of the
gradient in the record), then times and appends one JSON line: median / min / max ms of every alternative, the ratio labels / alternative,
the share of the 8 TB/s HBM peak that the algorithmic bytes (4 L + 4 B per voxel forward: one row of y_pred and one id; 8 L + 4 B forward +
backward: the row again and the gradient row) over the median of `labels` come to, the time of the pinned-host -> device copy of the ids and
of the one-hot map, and the library build id.  `not_slower_than_onehot` is the condition the op is held to.  The unet case records the step
time and torch.cuda.max_memory_allocated of a step with either target (the one-hot target resident on the device, as bench.py holds it).
A time needs a GPU: without one the tool fails.
"""

import argparse
import contextlib
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
from neurite_amd import metrics as MT                                                              # noqa: E402

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 240
# name: (batch, size, labels, kind)
CASES = {
    'blobs_4x160_L32': (4, 160, 32, 'loss'),
    'blobs_1x160_L32': (1, 160, 32, 'loss'),
    'blobs_4x160_L4': (4, 160, 4, 'loss'),
    'blobs_4x160_L24': (4, 160, 24, 'loss'),
    'blobs_4x160_L33': (4, 160, 33, 'loss'),
    'unet_step_1x160_L32': (1, 160, 32, 'unet'),
}


def bytes_per_voxel(L):
    return {'fwd': 4 * L + 4, 'fwdbwd': 8 * L + 4}


def make_inputs(batch, size, L, dev):
    """int32 blob labels [B, S, S, S] and y_pred [B, S, S, S, L] = soft-max of seeded noise"""
    _, Fx, _ = synth.cfg2_batch(batch, size, L, device=dev)
    ids = Fx.argmax(-1).to(torch.int32)
    del Fx
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.softmax(torch.randn((batch, size, size, size, L), generator=g, device=dev) * 2, -1)
    return ids, p


def one_hot(ids, L):
    out = torch.zeros(tuple(ids.shape) + (L,), dtype=torch.float32, device=ids.device)
    out.scatter_(-1, ids.long().unsqueeze(-1), 1.0)
    return out


def make_alternatives(ids, p, L):
    """{direction: {name: callable}}; the callables return (cce_sum, dice) or (cce_sum, dice, gradient)"""
    T = one_hot(ids, L)
    joint = bool(_lib.lib().nrt_seg_loss_supported(L))
    dev = p.device
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.rand((L,), generator=gen, device=dev) + 0.5
    gd = torch.rand((p.shape[0], L), generator=gen, device=dev) + 0.5
    n = p.numel() // L

    def labels(y):
        return ne.fused.seg_loss_labels(ids, y, w, check_input_limits=False)

    def onehot(y, t=T):
        if joint:
            return MT._SegLossFn.apply(t, y, w, (0.0, 0.0, False), None)
        return MT._WcceFn.apply(t, y, w, False, 0.0, False), MT._SoftDiceFn.apply(t, y, 0.0, False, False)

    def build(y):
        return onehot(y, one_hot(ids, L))

    pg = p.clone().requires_grad_(True)

    def bwd(fn):
        def run():
            c, d = fn(pg)
            return c, d, torch.autograd.grad(c[0] / n + (gd * d).sum(), (pg,))[0]
        return run

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(p)
        return run

    return {'fwd': {'labels': fwd(labels), 'onehot': fwd(onehot), 'build': fwd(build)},
            'fwdbwd': {'labels': bwd(labels), 'onehot': bwd(onehot), 'build': bwd(build)}}


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


def upload_ms(ids, L, reps):
    """median ms of the pinned-host -> device copy of the ids and of their float32 one-hot map"""
    out = {}
    for name, host in (('ids', ids.cpu().pin_memory()), ('onehot_f32', one_hot(ids, L).cpu().pin_memory())):
        dst = torch.empty_like(host, device=ids.device)
        fns = {name: lambda: dst.copy_(host, non_blocking=True)}
        fns[name]()
        torch.cuda.synchronize()
        out[name] = dict(timed(fns, reps)[name], bytes=host.numel() * host.element_size())
        del dst, host
    return out


def run_loss_case(name, reps):
    batch, size, L, _ = CASES[name]
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    ids, p = make_inputs(batch, size, L, dev)
    nvox = batch * size ** 3
    rec = {'case': name, 'batch': batch, 'size': size, 'labels': L, 'inputs': 'blob labels, soft-max of seeded noise', 'reps': reps,
           'voxels': nvox, 'baseline': '_SegLossFn (csrc/segloss.hip)' if _lib.lib().nrt_seg_loss_supported(L) else '_WcceFn + _SoftDiceFn',
           'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    rec['upload_ms'] = upload_ms(ids, L, reps)
    alts = make_alternatives(ids, p, L)
    got, want = alts['fwdbwd']['labels'](), alts['fwdbwd']['onehot']()
    rec['max_rel_diff_vs_onehot'] = [float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(got, want)]
    del got, want
    bpv = bytes_per_voxel(L)
    for direction, fns in alts.items():
        for _ in range(2):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = timed(fns, reps)
        nbytes = bpv[direction] * nvox
        rec[direction] = {'ms': t, 'algorithmic_bytes': nbytes,
                          'labels_over': {k: t['labels']['median'] / v['median'] for k, v in t.items() if k != 'labels'},
                          'hbm_peak_share': nbytes / (t['labels']['median'] * 1e-3) / HBM_PEAK,
                          'not_slower_than_onehot': t['labels']['median'] <= t['onehot']['median']}
    return rec


def run_unet_case(name, reps):
    """one training step of the BASELINE config 3 unet (bench.py: unet_train_bench) with an ids target and with the one-hot target"""
    batch, size, L, _ = CASES[name]
    dev = torch.device('cuda:0')
    _lib.init_device(dev)
    with contextlib.redirect_stdout(sys.stderr):
        net = ne.models.unet(16, (size, size, size, 1), 3, 3, L, feat_mult=2).to(dev)
    net.train()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((batch, size, size, size, 1), generator=g, device=dev)
    ids = torch.randint(0, L, (batch, size, size, size), generator=g, device=dev, dtype=torch.int32)
    cce, dice = ne.losses.CategoricalCrossentropy(), ne.losses.Dice(check_input_limits=False)
    seg_loss = ne.losses.multiple_losses_decorator([cce.loss, dice.loss])
    params = list(net.parameters())

    def step_with(t):
        def step():
            for q in params:
                q.grad = None
            seg_loss(t, net(x)).mean().backward()
            with torch.no_grad():
                torch._foreach_add_(params, [q.grad for q in params], alpha=-1e-4)
        return step

    rec = {'case': name, 'batch': batch, 'size': size, 'labels': L, 'reps': reps, 'what': 'BASELINE config 3 unet, forward + joint loss + '
           'backward + SGD, eager', 'build_id': _lib.lib().nrt_build_id().decode(), 'device': torch.cuda.get_device_name(dev)}
    # peak memory first, with one target alive at a time (the 16 MB of ids stay resident under the one-hot step too)
    mem, target_bytes = {}, {}
    for k in ('labels', 'onehot'):
        t = ids if k == 'labels' else one_hot(ids, L)
        target_bytes[k] = t.numel() * t.element_size()
        step = step_with(t)
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        step()
        torch.cuda.synchronize()
        mem[k] = int(torch.cuda.max_memory_allocated(dev))
        del t, step
        for q in params:
            q.grad = None
    rec['target_bytes'] = target_bytes
    rec['max_memory_allocated'] = mem
    steps = {'labels': step_with(ids), 'onehot': step_with(one_hot(ids, L))}
    for step in steps.values():
        step()
    torch.cuda.synchronize()
    t = timed(steps, reps)
    rec['step'] = {'ms': t, 'labels_over': {'onehot': t['labels']['median'] / t['onehot']['median']},
                   'not_slower_than_onehot': t['labels']['median'] <= t['onehot']['median']}
    return rec


def run_case(name, reps):
    if not torch.cuda.is_available():
        raise SystemExit('seg_loss_labels_bench: no ROCm device')
    return run_unet_case(name, reps) if CASES[name][3] == 'unet' else run_loss_case(name, reps)


def dry(names):
    """what can be rehearsed without a device: the cases, their byte counts and workspaces, and the inputs at a toy size on the CPU"""
    for c in names:
        batch, size, L, kind = CASES[c]
        nvox = batch * size ** 3
        ws = _lib.lib().nrt_seg_loss_labels_workspace_bytes(size ** 3, L, batch)
        ws_oh = _lib.lib().nrt_seg_loss_workspace_bytes(size ** 3, L, batch) if _lib.lib().nrt_seg_loss_supported(L) else 0
        ids, p = make_inputs(2, 12, L, 'cpu')
        T = one_hot(ids, L)
        assert ids.dtype == torch.int32 and ids.shape == (2, 12, 12, 12) and p.shape == (2, 12, 12, 12, L) and p.dtype == torch.float32
        assert bool((T.sum(-1) == 1).all()) and bool((T.argmax(-1) == ids).all()) and bool(((p.sum(-1) - 1).abs() < 1e-5).all())
        assert bool(torch.equal(T, MT._one_hot_ids(ids, L)))
        bpv = bytes_per_voxel(L)
        print('%-20s %-4s %d x %d^3 x %-3d ids %6.1f MB  one-hot f32 %8.1f MB  algorithmic fwd %7.1f MB fwd+bwd %7.1f MB  workspace %6.2f MB '
              '(one-hot form %6.2f MB)' % (c, kind, batch, size, L, nvox * 4 / 1e6, nvox * L * 4 / 1e6, bpv['fwd'] * nvox / 1e6,
                                          bpv['fwdbwd'] * nvox / 1e6, ws / 1e6, ws_oh / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seg_loss_labels', 'seg_loss_labels_bench.jsonl'))
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--case')
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    if args.reps < 10 and not args.dry:
        raise SystemExit('seg_loss_labels_bench: at least 10 repetitions')
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
            raise SystemExit('seg_loss_labels_bench: case %s ran past %d s; stopping' % (c, CASE_TIMEOUT_S))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit('seg_loss_labels_bench: case %s failed (exit %d); stopping' % (c, p.returncode))
        line = p.stdout.strip().splitlines()[-1]
        with open(args.out, 'a') as f:
            f.write(line + '\n')
        r = json.loads(line)
        if 'step' in r:
            print('%-20s step   ' % c + '  '.join('%s %.3f ms' % (k, v['median']) for k, v in r['step']['ms'].items()) +
                  '  peak memory ' + '  '.join('%s %.0f MB' % (k, v / 1e6) for k, v in r['max_memory_allocated'].items()))
            continue
        for direction in ('fwd', 'fwdbwd'):
            d = r[direction]
            print('%-20s %-6s ' % (c, direction) + '  '.join('%s %.3f ms' % (k, v['median']) for k, v in d['ms'].items()) +
                  '  labels/onehot %.3f  %.3f of the HBM peak  diff %.2g' % (d['labels_over']['onehot'], d['hbm_peak_share'],
                                                                           max(r['max_rel_diff_vs_onehot'])))
        print('%-20s upload ' % c + '  '.join('%s %.3f ms' % (k, v['median']) for k, v in r['upload_ms'].items()))


if __name__ == '__main__':
    main()
