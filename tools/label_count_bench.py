"""Fused warp + Dice at label counts that are multiples of 4 but not 4 * 2^k (warp_dice_tile_pad / warp_dice_bwd_rows_pad), against
the unfused pipeline and against the power-of-two count each one pads to.  Inputs synth.cfg2_batch(4, 160, L).

    python tools/label_count_bench.py [--reps R] [--iters N] [--labels 12,24,...]

Every case is an A / B pair timed in one process with device events: both arms warmed up, then R alternating samples of N calls each;
one JSON line per case with the median and the [min, max] of the samples (ms per call) and the ratio of the medians.
  pipeline  Dice().dice(fixed, SpatialTransformer()([moving, trf])): deferred (fused kernel) vs `with deferred.scope(False)` (eager)
  storage   fused.warp_dice on float32 maps vs the same maps stored as bfloat16
  backward  forward + backward wrt the field: fused.warp_dice vs SpatialTransformer -> Dice
  padded    fused.warp_dice at L vs at the power of two it pads to (same register kernel: _tune = 1 << 30), per voxel
"""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neurite_amd as ne                 # noqa: E402
from neurite_amd import synth            # noqa: E402

S, B = 160, 4
NO_WC = 1 << 30


def sample(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def ab(fa, fb, reps, n):
    for f in (fa, fb, fa, fb):
        f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(sample(fa, n))
        tb.append(sample(fb, n))
    return ta, tb


def emit(case, L, names, ta, tb, **extra):
    ma, mb = statistics.median(ta), statistics.median(tb)
    row = {'case': case, 'L': L, 'a': names[0], 'b': names[1],
           'a_ms': round(ma, 4), 'a_spread': [round(min(ta), 4), round(max(ta), 4)],
           'b_ms': round(mb, 4), 'b_spread': [round(min(tb), 4), round(max(tb), 4)], 'b_over_a': round(mb / ma, 3)}
    row.update(extra)
    print(json.dumps(row), flush=True)


def kernel(L, tune=0):
    n = ne._lib.ints([S] * 3)
    return ne._lib.lib().nrt_warp_dice_kernel_name(n, n, L, B, 1, 0, 0, 0, tune).decode()


def pow2_of(L):
    g = 1
    while g < L // 4:
        g <<= 1
    return 4 * g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--labels', default='12,16,20,24,28,32,36,48,64')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    labels = [int(v) for v in args.labels.split(',')]
    D = ne.metrics.Dice(check_input_limits=False)
    st = ne.layers.SpatialTransformer()
    nvox = B * S ** 3
    for L in labels:
        mov, fix, trf = synth.cfg2_batch(B, S, L, device=dev, seed0=1)

        def pipeline():
            return D.dice(fix, st([mov, trf]))

        def pipeline_eager():
            with ne.deferred.scope(False):
                return D.dice(fix, st([mov, trf]))
        assert isinstance(st([mov, trf]), ne.deferred.DeferredWarp), L
        ta, tb = ab(pipeline, pipeline_eager, args.reps, args.iters)
        emit('pipeline', L, ('deferred', 'eager'), ta, tb, kernel=kernel(L))

        mb, fb = mov.bfloat16(), fix.bfloat16()
        ta, tb = ab(lambda: ne.fused.warp_dice(mov, trf, fix), lambda: ne.fused.warp_dice(mb, trf, fb), args.reps, args.iters)
        emit('storage', L, ('float32', 'bfloat16'), ta, tb)
        del mb, fb

        tg = trf.clone().requires_grad_()

        def fused_step():
            tg.grad = None
            ne.fused.warp_dice(mov, tg, fix).sum().backward()

        def unfused_step():
            tg.grad = None
            D.dice(fix, st([mov, tg])).sum().backward()
        ta, tb = ab(fused_step, unfused_step, args.reps, max(1, args.iters // 2))
        emit('backward', L, ('fused', 'unfused'), ta, tb)
        del tg

        P = pow2_of(L)
        if P != L and P in labels:
            mp, fp, tp = synth.cfg2_batch(B, S, P, device=dev, seed0=1)
            ta, tb = ab(lambda: ne.fused.warp_dice(mov, trf, fix, _tune=NO_WC), lambda: ne.fused.warp_dice(mp, tp, fp, _tune=NO_WC),
                        args.reps, args.iters)
            emit('padded', L, ('L=%d' % L, 'L=%d' % P), ta, tb, ns_per_voxel=[round(statistics.median(ta) * 1e6 / nvox, 4),
                                                                              round(statistics.median(tb) * 1e6 / nvox, 4)],
                 kernels=[kernel(L, NO_WC), kernel(P, NO_WC)])
            del mp, fp, tp
        del mov, fix, trf
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
