"""
Every dispatch arm of the convolution forward kernels (csrc/conv.hip, conv_p27.h, conv_up2.h: conv3d_mfma<NT, FAST, FOLD, HYPER>,
conv3d_p27_mfma<NT, POOL, HYPER>, conv3d_up2_mfma<NT, 0>, conv3d_mfma_k2<NT>, conv3d_direct<HYPER>, space_to_depth2 and the weight-pack
kernels), each under an id that starts with the kernel instance the dispatcher takes, the gridDim.z of the N split (`z`), the most
tiles one block walks (`t`) and, for the generic conv3d_mfma instance, its inner path.  `plan` of oracle/conv_fwd_oracle.py restates the
host dispatch; tests/test_conv_fwd_oracle.py checks this table against it at 256 compute units and against the instances the compiler
emitted, every test here asserts the same for the device's own CU count before it launches, and a kernel trace of this file with
tools/arm_coverage.py --families conv_fwd confirms it on the device (profiles/dispatch_arms/README.md).  These kernels also produce
every input gradient (transposed weights, nrt_conv3d_s2d_taps_f32, nrt_conv3d_pad_f32).

The dispatchers choose by tile count against the CU count, so the batch size of the large-grid cases is derived from
torch.cuda.get_device_properties(dev).multi_processor_count (conv_fwd_oracle.batch_for): the volumes stay small, the batch carries the
tile count.  At 256 CUs: (5, 9, 17) x 43 = 516 tiles (>= 2 CUs: no N split), x 22 = 264 tiles (the split-by-2 of cout 49 .. 64),
(9, 9, 33) x 24 = 648 tiles (conv3d_p27_mfma blocks walk 2 or 3 tiles; 27 tiles per entry, one of them interior), (8, 8, 32) x 82 for
the pooled form (whole tiles), (10, 10, 34) x 48 = 1296 tiles (conv3d_up2_mfma blocks walk 2 or 3).  The small grid: (1, 1, 1) x 1 --
everything is halo; (4, 4, 16) x 1 -- exactly one tile; (5, 9, 17) x 2 -- 12 tiles per entry, the last of each axis partial, 12 no multiple
of the 8 XCDs; with dilation 2 also (3, 2, 5) x 1, every extent below the halo.

The C ABI is called directly on guarded buffers (tests/arm_buffers.py): every pointer is 16-byte aligned, every output (the packed
weights included) is checked for writes outside it.  The weights go through the library's own pack kernels (nrt_conv3d_pack_weights_f32,
nrt_conv3d_up2_pack_weights_f32, nrt_hyperconv3d_pack_weights_f32 with and without transpose_flip), and the matrix-core variants get
packed weights ONLY, so a silent detour over the direct kernel is an error.

Every case is checked twice on the same shapes against the float64 reference of oracle/conv_fwd_oracle.py:

  exact     x, x_lo, w, bias from the integers -3 .. 3.  9 taps (c0 + c1) + 3 < 2^24 (asserted), so every product, every partial sum in
            any order, the pre-summed taps of the folded decoder kernel and every matrix-core result is an integer float32 holds: the
            output must equal the reference BIT FOR BIT, every element, with activation none and relu.  One dropped, doubled or
            misplaced tap, channel, voxel or N-tile fails it.
  Gaussian  standard normal inputs, |got - ref| <= 8 x 2^-24 x S (+ 3e-6 with ELU) element-wise, S = |bias| + sum |x| |w|: close_conv of
            tests/test_gpu_unet.py.  With ELU and with none.  Each id prints its worst err / bound in a BOUND line
            (profiles/dispatch_arms/conv_fwd_bounds.txt is the record of one run).

Per-entry (HYPER) cases carry different weights and bias per entry, one entry whose weights are all zero (its output must be exactly
act(bias)) and one more run with bias = NULL.

The float64 reference is computed once per shape and input kind and shared by the activations, the bias = NULL run and the variant 0
launch.  The whole file takes 19 s on an MI355X, the slowest id 1.7 s.
"""

import collections
import zlib

import numpy as np
import pytest
import torch

from arm_buffers import Buf, call
from neurite_amd import _lib
from oracle import conv_fwd_oracle as cfo

pytestmark = pytest.mark.gpu
F = np.float32
K1, K2, K3 = (1, 1, 1), (2, 2, 2), (3, 3, 3)
ACT = {None: 0, 'elu': 1, 'relu': 2}
REF_CUS = 256                     # the ids are written for the MI355X; on another CU count the batch sizes follow batch_for

# shape, batch rule (an integer, or a name batch_for turns into one from the CU count)
SMALL = (((1, 1, 1), 1), ((4, 4, 16), 1), ((5, 9, 17), 2))
SMALL_PE = (((1, 1, 1), 1), ((4, 4, 16), 1), ((5, 9, 17), 3))          # per entry: three entries, the middle one with zero weights
SMALL_DIL2 = SMALL + (((3, 2, 5), 1),)
SMALL_UP = {(2, 2, 2): (((2, 2, 2), 1), ((4, 4, 16), 1), ((6, 10, 18), 2)), (2, 1, 4): (((2, 1, 4), 1), ((4, 4, 16), 1), ((6, 9, 20), 2)),
            (3, 1, 2): (((3, 1, 2), 1), ((3, 4, 16), 1), ((6, 9, 18), 2))}
UNSPLIT, SPLIT2 = (((5, 9, 17), 'unsplit'),), (((5, 9, 17), 'split2'),)
UNSPLIT_UP = (((6, 10, 18), 'unsplit'),)
P27_MULTI, POOL_MULTI, UP2_MULTI = (((9, 9, 33), 'p27'),), (((8, 8, 32), 'pool'),), (((10, 10, 34), 'up2'),)
VALID_SHAPES = (((3, 3, 3), 1), ((6, 6, 18), 1), ((7, 11, 19), 2))       # 'valid' 3x3x3: outputs (1,1,1), one tile, (5,9,17)

Case = collections.namedtuple('Case', 'label entry c0 cout shapes c1 up k dil same pad variant group pack also0')


def C(label, entry, c0, cout, shapes, c1=0, up=None, k=K3, dil=1, same=True, pad=None, variant=2, group=0, pack='plain', also0=False):
    """pack: 'plain' (nrt_conv3d_pack_weights_f32, or the batched kernel per entry), 'flip' (nrt_hyperconv3d_pack_weights_f32 with
    transpose_flip on the flipped and transposed kernel: the same packed set), 'keras' (no packing: the direct kernel).
    also0: variant 0 must take the same arm and return the same bits."""
    if entry == 'up2':
        up = (2, 2, 2)
    return Case(label, entry, c0, cout, shapes, c1, up, k, dil, same, pad, variant, group, pack, also0)


def case_plan(c, cus, shape, rule):
    out = shape if c.same else tuple(s - (kk - 1) * c.dil for s, kk in zip(shape, c.k))
    B = cfo.batch_for(rule, cus, cfo.tiles_per_entry(out))
    return B, cfo.plan(c.entry, cus, shape, B, c.c0, c.cout, c1=c.c1, up=c.up, ksize=c.k, dilation=c.dil, same=c.same, pad_before=c.pad,
                       variant=c.variant, group=c.group, packed=c.pack != 'keras', weights=c.pack == 'keras')


def case_id(c, cus=REF_CUS):
    """the id: what `plan` derives for the case's last (largest) shape, and the case's label"""
    return cfo.plan_id(case_plan(c, cus, *c.shapes[-1])[1]) + ' ' + c.label


def _x(t):
    return 'x'.join(str(v) for v in t)


def _mfma(entry, shapes_small, shapes_big):
    """conv3d_mfma through variant 2 of nrt_conv3d_f32 ('conv3d') or nrt_hyperconv3d_f32 ('hyperconv3d')"""
    pe = entry == 'hyperconv3d'
    cases = [
        # FAST, no N split: NT = 1 .. 4, cin 16 / 24 (a partial last chunk) / 48
        C('16->16 unsplit', entry, 16, 16, shapes_big), C('24->32 unsplit', entry, 24, 32, shapes_big, pack='flip'),
        C('48->48 unsplit', entry, 48, 48, shapes_big), C('16->64 unsplit', entry, 16, 64, shapes_big),
        # FAST on the small grid: a partial N-tile, gridDim.z 2, 3 and 4 of NT = 1, the split-by-2 of NT = 2
        C('16->5 small', entry, 16, 5, shapes_small), C('16->32 small', entry, 16, 32, shapes_small),
        C('24->40 small', entry, 24, 40, shapes_small, pack='flip'), C('16->64 small', entry, 16, 64, shapes_small),
        C('16->64 split-by-2', entry, 16, 64, SPLIT2),
        # generic with register prefetch, one reason for leaving FAST per NT, no N split
        C('16->16 k 1x3x3 unsplit', entry, 16, 16, shapes_big, k=(1, 3, 3)), C('16->32 k 3x1x3 unsplit', entry, 16, 32, shapes_big, k=(3, 1, 3)),
        C('16->48 k 1x1x1 unsplit', entry, 16, 48, shapes_big, k=K1, pack='flip'), C('10->64 scalar loader unsplit', entry, 10, 64, shapes_big),
        # generic without prefetch and with more than 64 KB of LDS: dilation 2, per NT
        C('16->16 dil 2 unsplit', entry, 16, 16, shapes_big, dil=2), C('16->32 dil 2 unsplit', entry, 16, 32, shapes_big, dil=2),
        C('16->40 dil 2 unsplit', entry, 16, 40, shapes_big, dil=2), C('16->64 dil 2 unsplit', entry, 16, 64, shapes_big, dil=2),
        # generic on the small grid
        C('16->16 dil 2 small', entry, 16, 16, SMALL_DIL2[:2] + shapes_small[2:] + SMALL_DIL2[3:], dil=2),
        C('10->5 scalar loader small', entry, 10, 5, shapes_small), C('16->32 k 1x1x1 small', entry, 16, 32, shapes_small, k=K1),
    ]
    if not pe:
        cases += [
            # two sources, FAST: the boundary on a chunk (16 | 32), a factor per axis, the first chunk straddling both sources (4 | 12)
            C('16+32->16 up 2x2x2 small', entry, 16, 16, SMALL_UP[(2, 2, 2)], c1=32, up=(2, 2, 2)),
            C('16+16->32 up 2x1x4 small', entry, 16, 32, SMALL_UP[(2, 1, 4)], c1=16, up=(2, 1, 4)),
            C('4+12->16 up 2x2x2 small', entry, 4, 16, SMALL_UP[(2, 2, 2)], c1=12, up=(2, 2, 2)),
            C('16+32->32 up 2x2x2 unsplit', entry, 16, 32, UNSPLIT_UP, c1=32, up=(2, 2, 2)),
            # two sources, generic: the second source loaded as scalars (c1 % 4 != 0), a factor that is no power of two
            C('4+6->16 up 2x2x2 small', entry, 4, 16, SMALL_UP[(2, 2, 2)], c1=6, up=(2, 2, 2)),
            C('8+8->32 up 3x1x2 small', entry, 8, 32, SMALL_UP[(3, 1, 2)], c1=8, up=(3, 1, 2)),
        ]
    return cases


CASES = _mfma('conv3d', SMALL, UNSPLIT) + _mfma('hyperconv3d', SMALL_PE, UNSPLIT) + [
    # conv3d_mfma<NT, true, true, false>: nrt_conv3d_s2d_taps_f32, c0 = 8 group, on low-resolution shapes
    C('group 16 ->16 unsplit', 's2d_taps', 128, 16, UNSPLIT, group=16), C('group 16 ->32 unsplit', 's2d_taps', 128, 32, UNSPLIT, group=16),
    C('group 16 ->48 unsplit', 's2d_taps', 128, 48, UNSPLIT, group=16), C('group 16 ->64 unsplit', 's2d_taps', 128, 64, UNSPLIT, group=16),
    C('group 32 ->32 small', 's2d_taps', 256, 32, SMALL, group=32), C('group 16 ->64 small', 's2d_taps', 128, 64, SMALL, group=16),
    C('group 32 ->64 split-by-2', 's2d_taps', 256, 64, SPLIT2, group=32),
    # conv3d_p27_mfma<NT, false, false>: variant 5.  cout 16: deferred stores and T.full; cout 8: NT = 1 with full = 0
    C('16->16 small', 'conv3d', 16, 16, SMALL, variant=5), C('32->8 small', 'conv3d', 32, 8, SMALL, variant=5),
    C('32->32 small', 'conv3d', 32, 32, SMALL, variant=5), C('16->40 small', 'conv3d', 16, 40, SMALL, variant=5, pack='flip'),
    C('48->64 small', 'conv3d', 48, 64, SMALL, variant=5),
    C('16->16 multi-tile', 'conv3d', 16, 16, P27_MULTI, variant=5, also0=True), C('32->8 multi-tile', 'conv3d', 32, 8, P27_MULTI, variant=5, also0=True),
    C('32->32 multi-tile', 'conv3d', 32, 32, P27_MULTI, variant=5, also0=True),
    C('16->40 multi-tile', 'conv3d', 16, 40, P27_MULTI, variant=5, also0=True, pack='flip'),
    C('48->64 multi-tile', 'conv3d', 48, 64, P27_MULTI, variant=5, also0=True),
    # conv3d_p27_mfma<NT, true, false>: nrt_conv3d_pool_f32, both outputs
    C('16->32 pooled multi-tile', 'pool', 16, 32, POOL_MULTI), C('32->48 pooled multi-tile', 'pool', 32, 48, POOL_MULTI),
    C('16->64 pooled multi-tile', 'pool', 16, 64, POOL_MULTI),
    # conv3d_p27_mfma<NT, false, true>: per entry, blocks cross entries
    C('16->16 multi-tile', 'hyperconv3d', 16, 16, P27_MULTI, variant=5, also0=True), C('32->24 multi-tile', 'hyperconv3d', 32, 24, P27_MULTI, variant=5),
    C('16->48 multi-tile', 'hyperconv3d', 16, 48, P27_MULTI, variant=5, pack='flip'), C('16->64 multi-tile', 'hyperconv3d', 16, 64, P27_MULTI, variant=5),
    C('16->16 small', 'hyperconv3d', 16, 16, SMALL_PE, variant=5),
    # conv3d_up2_mfma<NT, 0>: nrt_conv3d_up2_f32
    C('16+16->5 small', 'up2', 16, 5, SMALL_UP[(2, 2, 2)], c1=16), C('16+32->16 small', 'up2', 16, 16, SMALL_UP[(2, 2, 2)], c1=32),
    C('32+16->32 small', 'up2', 32, 32, SMALL_UP[(2, 2, 2)], c1=16), C('16+16->48 small', 'up2', 16, 48, SMALL_UP[(2, 2, 2)], c1=16),
    C('16+32->64 small', 'up2', 16, 64, SMALL_UP[(2, 2, 2)], c1=32),
    C('16+32->16 multi-tile', 'up2', 16, 16, UP2_MULTI, c1=32), C('32+16->32 multi-tile', 'up2', 32, 32, UP2_MULTI, c1=16),
    C('16+16->48 multi-tile', 'up2', 16, 48, UP2_MULTI, c1=16), C('16+16->64 multi-tile', 'up2', 16, 64, UP2_MULTI, c1=16),
] + [
    # conv3d_mfma_k2<NT>: 'same' (pad 0) through nrt_conv3d_f32, pad_before through nrt_conv3d_pad_f32, variant 6
    C('%d->%d %s' % (cin, cout, 'same' if pad is None else 'pad ' + _x(pad)), 'conv3d' if pad is None else 'conv3d_pad', cin, cout, SMALL,
      k=K2, pad=pad, variant=6)
    for cin, cout, pad in ((8, 16, None), (16, 16, (1, 1, 1)), (24, 16, (1, 0, 1)), (16, 32, None), (24, 32, (1, 1, 1)), (8, 32, (1, 0, 1)),
                           (24, 40, None), (8, 48, (1, 1, 1)), (16, 48, (1, 0, 1)), (16, 64, None), (24, 64, (1, 1, 1)), (8, 64, (0, 1, 0)))
] + [
    C('8+8->32 up 2x2x2 pad 1x0x1', 'conv3d_pad', 8, 32, SMALL_UP[(2, 2, 2)], c1=8, up=(2, 2, 2), k=K2, pad=(1, 0, 1), variant=6),
    C('16->16 auto', 'conv3d', 16, 16, (((40, 40, 40), 4),), k=K2, variant=6, also0=True),
    # conv3d_direct<false>: variant 1 on Keras-layout weights
    C('3->70 valid', 'conv3d', 3, 70, VALID_SHAPES, same=False, variant=1, pack='keras'),
    C('8->16 dil 4', 'conv3d', 8, 16, SMALL, dil=4, variant=1, pack='keras'),
    C('3+5->7 up 3x1x2', 'conv3d', 3, 7, SMALL_UP[(3, 1, 2)], c1=5, up=(3, 1, 2), variant=1, pack='keras'),
    C('5->6 k 4x4x4 pad 2x1x0', 'conv3d_pad', 5, 6, SMALL, k=(4, 4, 4), pad=(2, 1, 0), variant=1, pack='keras'),
    C('1->1 k 1x1x3 grid-stride', 'conv3d', 1, 1, (((1, 1, 8192 * 256 + 1), 1),), k=(1, 1, 3), variant=1, pack='keras'),
    # conv3d_direct<true>
    C('3->70 valid', 'hyperconv3d', 3, 70, VALID_SHAPES[:2] + (((7, 11, 19), 3),), same=False, variant=1, pack='keras'),
    C('8->16 dil 4', 'hyperconv3d', 8, 16, SMALL_PE, dil=4, variant=1, pack='keras'),
    C('5->6 k 4x4x4 pad 2x1x0', 'hyperconv3d_pad', 5, 6, SMALL_PE, k=(4, 4, 4), pad=(2, 1, 0), variant=1, pack='keras'),
]
IDS = [case_id(c) for c in CASES]


# ------------------------------------------------------------------------------------------------------------------------------
# packing, the launch, the comparison
# ------------------------------------------------------------------------------------------------------------------------------

def draw(rng, shape, kind):
    return cfo.integers(rng, shape) if kind == 'exact' else rng.standard_normal(shape).astype(F)


def pack(dev, c, w, B):
    """the packed weights of case c on the device (a guarded buffer whose guards have been checked), or the Keras-layout ones"""
    pe = c.entry.startswith('hyperconv3d')
    cin = c.c0 + c.c1
    if c.pack == 'keras':
        return Buf(dev, w.size, 0, w)
    wb = Buf(dev, w.size, 0, w)
    if c.entry == 'up2':
        pb = Buf(dev, int(_lib.lib().nrt_conv3d_up2_packed_weight_floats(c.c0, c.c1, c.cout)))
        call(dev, 'nrt_conv3d_up2_pack_weights_f32', wb.p, c.c0, c.c1, c.cout, pb.p)
    else:
        n = int(_lib.lib().nrt_conv3d_packed_weight_floats(_lib.ints(c.k), cin, c.cout))
        nb = B if pe else 1
        pb = Buf(dev, nb * n)
        if c.pack == 'flip':
            # the kernel flipped in space and transposed in its channel axes, [.., cout, cin]: transpose_flip packs w itself from it
            wt = np.ascontiguousarray(np.flip(w.reshape((nb,) + c.k + (cin, c.cout)), (1, 2, 3)).transpose(0, 1, 2, 3, 5, 4))
            wb = Buf(dev, wt.size, 0, wt)
            call(dev, 'nrt_hyperconv3d_pack_weights_f32', wb.p, nb, _lib.ints(c.k), c.cout, cin, 1, pb.p)
        elif pe:
            call(dev, 'nrt_hyperconv3d_pack_weights_f32', wb.p, nb, _lib.ints(c.k), cin, c.cout, 0, pb.p)
        else:
            call(dev, 'nrt_conv3d_pack_weights_f32', wb.p, _lib.ints(c.k), cin, c.cout, pb.p)
    pb.get()
    return pb


def launch(dev, c, S, B, xb, lb, wb, bb, act, variant, out_shape):
    """one call of the case's entry point on a fresh guarded output: the output (and the pooled one of 'pool')"""
    ob = Buf(dev, B * int(np.prod(out_shape)) * c.cout)
    keras = c.pack == 'keras'
    wk, wp = (wb.p, None) if keras else (None, wb.p)
    bp, lp, up = (bb.p if bb is not None else None), (lb.p if lb is not None else None), (_lib.ints(c.up) if c.c1 else None)
    pool = None
    if c.entry == 'conv3d':
        call(dev, 'nrt_conv3d_f32', xb.p, c.c0, lp, c.c1, up, wk, wp, bp, ob.p, B, _lib.ints(S), _lib.ints(c.k), c.cout, c.dil, int(c.same),
             ACT[act], variant)
    elif c.entry == 'conv3d_pad':
        call(dev, 'nrt_conv3d_pad_f32', xb.p, c.c0, lp, c.c1, up, wk, wp, bp, ob.p, B, _lib.ints(S), _lib.ints(c.k), c.cout, c.dil,
             _lib.ints(c.pad), ACT[act], variant)
    elif c.entry == 'hyperconv3d':
        call(dev, 'nrt_hyperconv3d_f32', xb.p, c.c0, wk, wp, bp, ob.p, B, _lib.ints(S), _lib.ints(c.k), c.cout, c.dil, int(c.same), ACT[act], variant)
    elif c.entry == 'hyperconv3d_pad':
        call(dev, 'nrt_hyperconv3d_pad_f32', xb.p, c.c0, wk, wp, bp, ob.p, B, _lib.ints(S), _lib.ints(c.k), c.cout, c.dil, _lib.ints(c.pad),
             ACT[act], variant)
    elif c.entry == 'up2':
        call(dev, 'nrt_conv3d_up2_f32', xb.p, c.c0, lp, c.c1, wp, bp, ob.p, B, _lib.ints(S), c.cout, ACT[act])
    elif c.entry == 'pool':
        pool = Buf(dev, B * int(np.prod(out_shape)) // 8 * c.cout)
        call(dev, 'nrt_conv3d_pool_f32', xb.p, c.c0, wp, bp, ob.p, pool.p, B, _lib.ints(S), c.cout, ACT[act])
        pool = pool.get((B,) + tuple(s // 2 for s in out_shape) + (c.cout,))
    else:
        assert c.entry == 's2d_taps' and bb is None and act is None
        call(dev, 'nrt_conv3d_s2d_taps_f32', xb.p, c.group, wp, ob.p, B, _lib.ints(S), c.cout)
    return ob.get((B,) + tuple(out_shape) + (c.cout,)), pool


def compare(worst, kind, got, ref, bnd, what):
    """bit for bit, or within the bound (exactly the reference where the bound is 0); returns the running worst err / bound"""
    if kind == 'exact':
        cfo.check_exact(got, ref, what)
        return worst
    r = cfo.ratio(got, ref, bnd)
    assert r <= 1.0, '%s: worst err / bound = %.3g' % (what, r)
    return max(worst, r)


def run_case(dev, cid, c):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    pe = c.entry.startswith('hyperconv3d')
    ntap = c.k[0] * c.k[1] * c.k[2]
    cin = c.c0 + c.c1
    worst = 0.0
    for S, rule in c.shapes:
        B, p = case_plan(c, cus, S, rule)
        assert cfo.plan_id(p) + ' ' + c.label == cid, (cid, S, B, p)
        if c.also0:
            assert cfo.plan(c.entry, cus, S, B, c.c0, c.cout, ksize=c.k, variant=0).name == p.name
        zero = 1 if pe and B >= 3 else None                     # the entry whose weights are all zero
        for kind in ('exact', 'gauss'):
            rng = np.random.default_rng(zlib.crc32(('%s %s %d %s' % (cid, S, B, kind)).encode()))
            x = draw(rng, (B,) + S + (c.c0,), kind)
            lo = draw(rng, (B,) + tuple(s // u for s, u in zip(S, c.up)) + (c.c1,), kind) if c.c1 else None
            w = draw(rng, ((B,) if pe else ()) + c.k + (cin, c.cout), kind)
            b = None if c.entry == 's2d_taps' else draw(rng, ((B,) if pe else ()) + (c.cout,), kind)
            if zero is not None:
                w[zero] = 0
            what = '%s %s x %d %s' % (cid, S, B, kind)
            if kind == 'exact':
                cfo.exact_condition(ntap, cin)
            if c.entry == 's2d_taps':
                assert np.abs(w).reshape(27, -1).sum(1).min() > 0          # a kernel that reads a dead tap reads a non-zero weight
                pre, S_abs, _ = cfo.s2d_taps(x, w, c.group, with_abs=kind == 'gauss')
            else:
                pre, S_abs, _ = cfo.conv(x, w, b, c.dil, 'same' if c.same else 'valid', lo, c.up, c.pad, pe, with_abs=kind == 'gauss')
            out_shape = pre.shape[1:4]
            xb, lb = Buf(dev, x.size, 0, x), (Buf(dev, lo.size, 0, lo) if c.c1 else None)
            bb = Buf(dev, b.size, 0, b) if b is not None else None
            wb = pack(dev, c, w, B)
            acts = (None,) if c.entry == 's2d_taps' else (None, 'relu') if kind == 'exact' else ('elu', None)
            for act in acts:
                ref = cfo.activate(pre, act)
                bnd = cfo.bound(S_abs, act) if kind == 'gauss' else None
                got, pool = launch(dev, c, S, B, xb, lb, wb, bb, act, c.variant, out_shape)
                worst = compare(worst, kind, got, ref, bnd, '%s act %s' % (what, act))
                if pool is not None:
                    # MaxPooling3D(2) of the activated output: of the output the kernel wrote, bit for bit, hence of the reference too
                    assert np.array_equal(pool, cfo.maxpool2(got)), what + ': pool_out is not the 2x2x2 max of out'
                    if kind == 'exact':
                        cfo.check_exact(pool, cfo.maxpool2(ref), what + ' pool_out')
                if zero is not None and act != 'elu':
                    want = cfo.activate(np.asarray(b[zero], np.float64), act).astype(F)
                    assert np.array_equal(got[zero], np.broadcast_to(want, got[zero].shape)), what + ': zero weights, the output is not act(bias)'
                if c.also0:
                    got0, _ = launch(dev, c, S, B, xb, lb, wb, bb, act, 0, out_shape)
                    assert np.array_equal(got0.view(np.uint32), got.view(np.uint32)), what + ': variant 0 differs from variant %d' % c.variant
            if pe:                                              # bias = NULL, the reference without its bias term
                b64 = np.asarray(b, np.float64).reshape(B, 1, 1, 1, c.cout)
                got, _ = launch(dev, c, S, B, xb, lb, wb, None, None, c.variant, out_shape)
                worst = compare(worst, kind, got, pre - b64, cfo.bound(S_abs - np.abs(b64)) if kind == 'gauss' else None, what + ' no bias')
                if zero is not None:
                    assert not got[zero].any(), what + ': zero weights and no bias, the output is not zero'
    print('BOUND %-96s worst err / bound: %.3g' % (cid, worst))


@pytest.mark.parametrize('cid,case', list(zip(IDS, CASES)), ids=IDS)
def test_arm(dev, cid, case):
    run_case(dev, cid, case)


# ------------------------------------------------------------------------------------------------------------------------------
# space_to_depth2: nrt_space_to_depth2_f32, a permutation
# ------------------------------------------------------------------------------------------------------------------------------

S2D = (((2, 2, 2), 4, 2), ((2, 2, 2), 20, 2), ((4, 6, 10), 4, 2), ((4, 6, 10), 20, 2), ((256, 256, 258), 4, 1))
S2D_IDS = ['space_to_depth2 %s x %d channels %d' % (_x(s), b, ch) for s, ch, b in S2D]


@pytest.mark.parametrize('arm,case', list(zip(S2D_IDS, S2D)), ids=S2D_IDS)
def test_space_to_depth2(dev, arm, case):
    """y[b][q][P C + c] = x[b][2 q + p][c] on distinct 32-bit patterns (compared as integers: the kernel moves bits).  The last shape
    has more than 65536 x 256 float4 per entry: the grid is capped at 65536 blocks and the grid-stride loop runs a second pass."""
    S, ch, B = case
    n4 = int(np.prod(S)) * ch // 4
    assert (S == (256, 256, 258)) == (n4 > 65536 * 256)
    bits = np.arange(B * n4 * 4, dtype=np.int32).reshape((B,) + S + (ch,))
    xb, yb = Buf(dev, bits.size, 0, bits.view(F)), Buf(dev, bits.size)
    call(dev, 'nrt_space_to_depth2_f32', xb.p, yb.p, B, _lib.ints(S), ch)
    got = yb.get((B,) + tuple(s // 2 for s in S) + (8 * ch,)).view(np.int32)
    assert np.array_equal(got, cfo.space_to_depth2(bits)), arm
