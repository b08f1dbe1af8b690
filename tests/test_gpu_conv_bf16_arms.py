"""
Every dispatch arm of the bfloat16 inference kernels (csrc/conv_bf16.hip: conv3d_bf16<NT>, conv3d_pack_bf16<T>, conv1x1_bf16<CO_MAX>,
softmax_lastdim_bf16<V8>, maxpool3d_bf16<V>, upsample_concat_bf16<V>, add_act_affine_bf16<V>: 17 instances behind 7 entry points),
each under an id that starts with what `plan` of oracle/conv_bf16_oracle.py, a restatement of the host code, derives for the call.  For
the convolution that is the instance, gridDim.z of the N split (`z`) and the live N-tiles of its last split (`live`), the loader (vec /
scalar / dense), the staged channel groups per chunk, the chunks and the groups of the last chunk (`cg`, `chunks`, `last`; dense: the
k-steps, `ks`), whether the LDS exceeds 64 KB and the epilogue's store; for the glue kernels the instance, its run-time path, the grid
(`b`) and the grid-stride passes (`p`).  tests/test_conv_bf16_oracle.py checks this table against `plan` at 256 compute units and
against the instances the compiler emitted, every test here asserts the same for the device's own CU count before it launches, and a
kernel trace of this file with tools/arm_coverage.py --families conv_bf16 confirms it on the device (profiles/dispatch_arms/README.md).

nrt_conv3d_bf16 takes all N-tiles in one block only from two tiles per CU on, so the large-grid cases derive their batch from
torch.cuda.get_device_properties(dev).multi_processor_count (batch_for 'unsplit': (5, 9, 17) x 43 = 516 tiles at 256 CUs): the volumes
stay small, the batch carries the tile count.  The small grid: (1, 1, 1) x 1 -- everything is halo; (4, 4, 16) x 1 -- exactly one tile;
(5, 9, 17) x 2 -- 12 tiles per entry, the last of each axis partial, 12 no multiple of the 8 XCDs; from dilation 2 on also (3, 2, 5) x 1,
every extent below the halo.

The C ABI is called directly on guarded byte buffers (arm_buffers.Raw): the payloads are bf16 bit patterns, byte offsets set the
alignment of a pointer exactly, every output (the packed weights included) is checked for writes outside it, and a refused call must
leave its output without one byte written.  Weights always go through nrt_conv3d_pack_weights_bf16 (from float32 storage for the
integer data, from bf16 storage for the Gaussian data).

Every id is checked on the same shapes against float64 references in which nothing of the kernels' tiles, groups or chunks appears
(conv of oracle/conv_fwd_oracle.py, the glue references of oracle/conv_bf16_oracle.py):

  exact     inputs and weights from the integers -3 .. 3, an integer bias.  9 taps cin + 1000 < 2^24 (asserted), so the float32 value
            before the final rounding is an integer, exact in any order and on the matrix cores: the bf16 output must equal
            rne_bf16(reference) BIT FOR BIT, every element, with activation none and relu.
  rounding  the same with bias magnitudes from the integers 257 .. 1000, signs alternating over the channels (add / affine: a, b from
            -100 .. 100, or -30 .. 30 with ACT_MUL_B, an odd integer scale, shift as that bias).  Before any GPU result is looked at the
            reference of the id (all its shapes together) must have, with activation none, at least 50 % of its outputs not
            representable in bf16, 8 % exact ties that round up in magnitude, 8 % that round down and 25 % non-ties; half of each
            with relu.  An add id without a shift stays inside the range bf16 holds exactly (|a + b| <= 200) and a multiply id leaves
            it with few of its values; they run the same data bit for bit without that premise.
  Gaussian  standard-normal values rounded to bf16 (a float32 bias, scale and shift), within the suite's own bounds
            (tests/test_gpu_unet_bf16.py): convolutions 2^-8 |act(ref)| + 9 x 2^-24 x S (+ 3e-6 with ELU), the 1x1 softmax and the
            last-axis softmax 2^-8 p + 1e-6, the element-wise kernels 2^-8 |ref| + 4e-7 (1 + |ref|).  Each id prints its worst
            err / bound in a BOUND line (profiles/dispatch_arms/conv_bf16_bounds.txt is the record of one run).

The last-axis softmax has no integer form (Gaussian only, at scale 1 and 4); max-pooling and up-sample + concatenate are copies of
bits, checked bit for bit on Gaussian bf16 data.

The float64 reference of a convolution is computed once per shape and input kind, without its bias, and shared by the exact and the
rounding check, the activations and the bias = NULL run; the rows of the second-pass 1x1 and add / affine ids repeat a block of PERIOD
rows.  The whole file takes 5.3 s on an MI355X (87 tests), the slowest id 0.8 s.
"""

import collections
import zlib

import numpy as np
import pytest
import torch

from arm_buffers import Raw
from neurite_amd import _lib
from oracle import conv_bf16_oracle as cbo

pytestmark = pytest.mark.gpu
F, F64 = np.float32, np.float64
K1, K2, K3 = (1, 1, 1), (2, 2, 2), (3, 3, 3)
ACT = {None: 0, 'elu': 1, 'relu': 2, 'sigmoid': 3}
ACT_MUL_B = 0x100
REF_CUS = 256                     # the ids are written for the MI355X; on another CU count the batch sizes follow batch_for

SMALL = (((1, 1, 1), 1), ((4, 4, 16), 1), ((5, 9, 17), 2))
SMALL_DIL = SMALL + (((3, 2, 5), 1),)
SMALL_UP = {(2, 2, 2): (((2, 2, 2), 1), ((4, 4, 16), 1), ((6, 10, 18), 2)), (1, 2, 3): (((1, 2, 3), 1), ((4, 4, 15), 1), ((5, 10, 18), 2))}
LARGE = (((5, 9, 17), 'unsplit'),)
ONE_TILE = (((4, 4, 16), 1),)


def valid_shapes(k, dil=1):
    """input shapes whose VALID outputs are the small grid"""
    return tuple((tuple(s + (kk - 1) * dil for s, kk in zip(S, k)), B) for S, B in SMALL)


# ------------------------------------------------------------------------------------------------------------------------------
# buffers and calls
# ------------------------------------------------------------------------------------------------------------------------------

def rc_of(dev, name, *args):
    with torch.cuda.device(dev):
        return getattr(_lib.lib(), name)(*args, _lib.stream_ptr(dev))


def call(dev, name, *args):
    _lib.check(rc_of(dev, name, *args), name)


def bf(dev, a, off=0):
    """a guarded buffer with the bf16 bits of the float32 array a (which holds bf16 values), `off` bytes past a 16-byte boundary"""
    bits = cbo.to_bits(a)
    return Raw(dev, 2 * bits.size, off, bits)


def f32(dev, a):
    a = np.ascontiguousarray(a, F)
    return Raw(dev, 4 * a.size, 0, a)


def p_of(buf):
    return buf.p if buf is not None else None


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint16, (got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %r (0x%04x), want %r (0x%04x)' % (
            what, len(bad), want.size, i, float(cbo.from_bits(got[i])), int(got[i]), float(cbo.from_bits(want[i])), int(want[i])))


def within(worst, bits, ref, bnd, what):
    """the bf16 output within the bound of the float64 reference; returns the running worst err / bound"""
    r = cbo.ratio(cbo.from_bits(bits), ref, np.broadcast_to(bnd, ref.shape))
    assert r <= 1.0, '%s: worst err / bound = %.3g' % (what, r)
    return max(worst, r)


def seeded(*key):
    return np.random.default_rng(zlib.crc32(' '.join(str(k) for k in key).encode()))


def report(cid, worst):
    print('BOUND %-112s worst err / bound: %.3g' % (cid, worst))


def _x(t):
    return 'x'.join(str(v) for v in t)


# ------------------------------------------------------------------------------------------------------------------------------
# conv3d_bf16<NT> and conv3d_pack_bf16<T>
# ------------------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple('Case', 'label c0 cout shapes c1 up k dil same off0 ooff nobias')


def C(label, c0, cout, shapes=SMALL, c1=0, up=None, k=K3, dil=1, same=True, off0=0, ooff=0, nobias=False):
    """off0 / ooff: the byte offset of src0 / out from a 16-byte boundary; nobias: one more run with bias = NULL"""
    return Case(label, c0, cout, shapes, c1, up, k, dil, same, off0, ooff, nobias)


def case_plan(c, cus, shape, rule):
    B = cbo.batch_for(rule, cus, cbo.tiles_per_entry(cbo.out_shape(shape, c.k, c.dil, c.same)))
    return B, cbo.plan(cus, shape, B, c.c0, c.cout, c1=c.c1, ksize=c.k, dilation=c.dil, same=c.same, src0_off=c.off0, out_off=c.ooff)


def case_id(c, cus=REF_CUS):
    return cbo.plan_id(case_plan(c, cus, *c.shapes[-1])[1]) + ' ' + c.label


CASES = [
    # the small grid, NT = 1: gridDim.z 1 .. 4; a partial N-tile with the scalar store (5, 7) and with the packed store (12)
    C('16->16 small', 16, 16, nobias=True), C('16->32 small', 16, 32), C('16->40 small', 16, 40), C('16->64 small', 16, 64),
    C('16->5 small', 16, 5), C('16->7 small', 16, 7), C('16->12 small', 16, 12),
    # the large grid: all N-tiles in one block, NT = 2, 3 (whole and with a partial last tile), 4; cin 16 and 24 (three groups of four)
    C('16->32 large', 16, 32, LARGE), C('24->32 large', 24, 32, LARGE), C('16->40 large', 16, 40, LARGE), C('24->40 large', 24, 40, LARGE),
    C('16->33 large', 16, 33, LARGE), C('16->64 large', 16, 64, LARGE), C('24->64 large', 24, 64, LARGE),
    # more than four N-tiles: NT = 4 split over z, the last split with one live tile of four (80: 5 tiles, 130: 9 tiles, the last partial)
    C('16->80 small', 16, 80), C('16->130 small', 16, 130),
    # the scalar loader: through a source 2 bytes off a 16-byte boundary, through channel counts (12: a partial group; 20: a partial last)
    C('16->16 src 2 bytes off', 16, 16, off0=2), C('12->16 small', 12, 16, nobias=True), C('20->16 small', 20, 16),
    # the dense K order: cin 1 (one k-step), 3, 7 (K = 189: 6 k-steps), two sources
    C('1->16 small', 1, 16), C('3->16 small', 3, 16, nobias=True), C('7->16 small', 7, 16),
    C('2+4->16 up 2x2x2', 2, 16, SMALL_UP[(2, 2, 2)], c1=4, up=(2, 2, 2)),
    # two sources, 8-channel groups: vec with the boundary on a group, a factor per axis; scalar with the boundary inside a group
    C('16+32->16 up 2x2x2', 16, 16, SMALL_UP[(2, 2, 2)], c1=32, up=(2, 2, 2)), C('16+32->16 up 1x2x3', 16, 16, SMALL_UP[(1, 2, 3)], c1=32, up=(1, 2, 3)),
    C('4+12->16 up 2x2x2', 4, 16, SMALL_UP[(2, 2, 2)], c1=12, up=(2, 2, 2)),
    # staging: CG = 4 with a second chunk of one group; more than 64 KB of LDS; CG = 2 (dilation 3), CG = 1 (dilation 4)
    C('40->16 small', 40, 16), C('16->16 dil 2', 16, 16, SMALL_DIL, dil=2), C('16->16 dil 3', 16, 16, SMALL_DIL, dil=3),
    C('40->16 dil 3', 40, 16, SMALL_DIL, dil=3), C('24->16 dil 4', 24, 16, SMALL_DIL, dil=4),
    # no CG fits: refused, nothing written; the same dilation on the dense path fits
    C('16->16 dil 6', 16, 16, SMALL_DIL, dil=6), C('4->16 dil 6', 4, 16, SMALL_DIL, dil=6),
    # kernels: 1x1x1 (three padded taps), 2x2x2 (no pad tap), 1x3x5; VALID
    C('16->16 k 1x1x1', 16, 16, k=K1), C('16->16 k 2x2x2', 16, 16, k=K2), C('16->16 k 1x3x5', 16, 16, k=(1, 3, 5)),
    C('16->16 valid', 16, 16, valid_shapes(K3), same=False), C('3->5 valid', 3, 5, valid_shapes(K3), same=False),
    C('16->12 k 2x2x2 valid', 16, 12, valid_shapes(K2), k=K2, same=False), C('12->16 dil 2 valid', 12, 16, valid_shapes(K3, 2), dil=2, same=False),
    # refused: out 2 bytes off its 8-byte alignment
    C('16->16 out 2 bytes off', 16, 16, ooff=2),
    # the pack kernel past its 4096 x 256 grid: 1 146 880 packed elements, all of them consumed by the convolution
    C('256->160 one tile', 256, 160, ONE_TILE),
]
IDS = [case_id(c) for c in CASES]
ROUND_AMAX = 1000


def conv_prepare(cid, c, S, B):
    """the inputs of one shape and their float64 references WITHOUT the bias: {'int': ..., 'gauss': ...}; the bias of each kind"""
    cin, ntap = c.c0 + c.c1, c.k[0] * c.k[1] * c.k[2]
    lo_shape = (B,) + tuple(s // u for s, u in zip(S, c.up)) + (c.c1,) if c.c1 else None
    assert 9 * ntap * cin + ROUND_AMAX < 2 ** 24
    cbo.exact_condition(ntap, cin)
    d = {}
    rng = seeded(cid, S, B, 'int')
    x, lo = cbo.integers(rng, (B,) + S + (c.c0,)), (cbo.integers(rng, lo_shape) if c.c1 else None)
    w = cbo.integers(rng, c.k + (cin, c.cout))
    pre, _, _ = cbo.conv(x, w, None, c.dil, 'same' if c.same else 'valid', lo, c.up, with_abs=False)
    d['int'] = dict(x=x, lo=lo, w=w, pre=pre, S_abs=None, b={'exact': cbo.integers(rng, (c.cout,)), 'rounding': cbo.rounding_bias(rng, c.cout)})
    rng = seeded(cid, S, B, 'gauss')
    x, lo = cbo.gaussian_bf16(rng, (B,) + S + (c.c0,)), (cbo.gaussian_bf16(rng, lo_shape) if c.c1 else None)
    w = cbo.gaussian_bf16(rng, c.k + (cin, c.cout))
    pre, S_abs, _ = cbo.conv(x, w, None, c.dil, 'same' if c.same else 'valid', lo, c.up)
    d['gauss'] = dict(x=x, lo=lo, w=w, pre=pre, S_abs=S_abs, b={'gauss': rng.standard_normal(c.cout).astype(F)})
    return d


def rounding_premise(refs):
    """(activation none, relu): the shares of `rounding_shares`, asserted on the reference alone"""
    return cbo.check_shares(refs), cbo.check_shares([cbo.activate(r, 'relu') for r in refs], 'relu')


def conv_pack(dev, c, w, bf16_storage):
    cin = c.c0 + c.c1
    n = int(_lib.lib().nrt_conv3d_packed_weight_bytes_bf16(_lib.ints(c.k), cin, c.cout))
    assert n == cbo.packed_weight_bytes(c.k, cin, c.cout)
    wb, pb = (bf(dev, w) if bf16_storage else f32(dev, w)), Raw(dev, n)
    call(dev, 'nrt_conv3d_pack_weights_bf16', wb.p, _lib.DT_BF16 if bf16_storage else _lib.DT_F32, _lib.ints(c.k), cin, c.cout, pb.p)
    pb.get(np.uint16)                                               # the guards of the packed buffer
    return pb


def conv_launch(dev, c, S, B, xb, lb, pb, bb, act, oshape):
    ob = Raw(dev, 2 * B * int(np.prod(oshape)) * c.cout, c.ooff)
    rc = rc_of(dev, 'nrt_conv3d_bf16', xb.p, c.c0, p_of(lb), c.c1, _lib.ints(c.up) if c.c1 else None, pb.p, p_of(bb), ob.p, B, _lib.ints(S),
               _lib.ints(c.k), c.cout, c.dil, int(c.same), ACT[act])
    return rc, ob


def run_conv(dev, cid, c):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    todo = []
    for S, rule in c.shapes:
        B, p = case_plan(c, cus, S, rule)
        assert cbo.plan_id(p) + ' ' + c.label == cid, (cid, S, B, p)
        todo.append((S, B, p, conv_prepare(cid, c, S, B)))
    refused = not todo[0][2].name.startswith('conv3d_bf16')
    if not refused:
        rounding_premise([d['int']['pre'] + d['int']['b']['rounding'].astype(F64) for _, _, _, d in todo])
    worst = 0.0
    for S, B, p, data in todo:
        oshape = cbo.out_shape(S, c.k, c.dil, c.same)
        for src in ('int', 'gauss'):
            d = data[src]
            xb, lb = bf(dev, d['x'], c.off0), (bf(dev, d['lo']) if c.c1 else None)
            pb = conv_pack(dev, c, d['w'], src == 'gauss')
            for kind, b in d['b'].items():
                bb = f32(dev, b)
                what = '%s %s x %d %s' % (cid, S, B, kind)
                if refused:
                    rc, ob = conv_launch(dev, c, S, B, xb, lb, pb, bb, None, oshape)
                    want = _lib.NRT_ERR_INVALID_ARG if p.name.startswith('invalid') else _lib.NRT_ERR_UNSUPPORTED
                    assert rc == want and ob.untouched(), '%s: status %d, expected %d with not one byte written' % (what, rc, want)
                    continue
                pre = d['pre'] + b.astype(F64)
                runs = [(act, bb, pre) for act in ((None, 'relu') if src == 'int' else ('elu', None))]
                if c.nobias:
                    runs.append((None, None, d['pre']))
                for act, bbuf, pr in runs:
                    rc, ob = conv_launch(dev, c, S, B, xb, lb, pb, bbuf, act, oshape)
                    _lib.check(rc, 'nrt_conv3d_bf16')
                    got = ob.get(np.uint16, (B,) + oshape + (c.cout,))
                    ref = cbo.activate(pr, act)
                    tag = '%s act %s%s' % (what, act, '' if bbuf is not None else ' no bias')
                    if src == 'int':
                        same_bits(got, cbo.expected_bits(ref), tag)
                    else:
                        S_abs = d['S_abs'] + (np.abs(b.astype(F64)) if bbuf is not None else 0.0)
                        worst = within(worst, got, ref, cbo.bound_conv(ref, S_abs, act), tag)
    report(cid, worst)


@pytest.mark.parametrize('cid,case', list(zip(IDS, CASES)), ids=IDS)
def test_conv(dev, cid, case):
    run_conv(dev, cid, case)


PACK_SHAPE = (K3, 20, 40)             # ksize, cin, cout
PACK_ID = '%s + %s same bytes 20->40' % (cbo.plan_id(cbo.plan_pack(*PACK_SHAPE, dtype='float')),
                                         cbo.plan_id(cbo.plan_pack(*PACK_SHAPE, dtype='unsigned short')))


@pytest.mark.parametrize('cid', [PACK_ID], ids=[PACK_ID])
def test_pack_from_both_storages(dev, cid):
    """float32 weights that are NOT bf16 values, and their round-to-nearest-even bf16 bits: the two packed buffers are byte-identical,
    every real weight appears in them once and everything else is zero"""
    k, cin, cout = PACK_SHAPE
    w = seeded(cid).standard_normal(k + (cin, cout)).astype(F)
    wr = cbo.rne_bf16(w)
    assert (wr != w).mean() > 0.9 and (wr != 0).all()
    n = cbo.packed_weight_bytes(k, cin, cout)
    got = []
    for src, dt in ((f32(dev, w), _lib.DT_F32), (bf(dev, wr), _lib.DT_BF16)):
        pb = Raw(dev, n)
        call(dev, 'nrt_conv3d_pack_weights_bf16', src.p, dt, _lib.ints(k), cin, cout, pb.p)
        got.append(pb.get(np.uint16))
    assert np.array_equal(got[0], got[1]), 'packed from float32 and from bf16 storage differ'
    assert np.array_equal(np.sort(got[0][got[0] != 0]), np.sort(cbo.to_bits(wr).reshape(-1)))
    report(cid, 0.0)


# ------------------------------------------------------------------------------------------------------------------------------
# conv1x1_bf16<16|32|64>
# ------------------------------------------------------------------------------------------------------------------------------

SECOND_4096 = 4096 * 256 + 300          # items past the 4096-block cap: the busiest threads take a second grid-stride pass
# the rows of a second-pass id repeat a block of PERIOD rows, so that the float64 reference costs what a small id costs.  PERIOD is a
# prime: the row a thread takes in its second pass and the row it took in its first (4096 x 256 or 8192 x 256 x 8 / C rows earlier) are
# different rows of the block, as are any two rows a power of two apart.
PERIOD = 65521
C1 = [('16->16', 16, 16, 700, 0), ('16->32', 16, 32, 700, 0), ('16->64', 16, 64, 700, 0), ('16->4', 16, 4, 700, 0), ('7->50', 7, 50, 700, 0),
      ('16->16 x 2 bytes off', 16, 16, 700, 2), ('16->16 second pass', 16, 16, SECOND_4096, 0)]
C1_IDS = ['%s %s nvox %d' % (cbo.plan_id(cbo.plan_conv1x1(nvox, cin, cout, xoff)), label, nvox) for label, cin, cout, nvox, xoff in C1]


@pytest.mark.parametrize('cid,case', list(zip(C1_IDS, C1)), ids=C1_IDS)
def test_conv1x1(dev, cid, case):
    label, cin, cout, nvox, xoff = case
    assert cid.startswith(cbo.plan_id(cbo.plan_conv1x1(nvox, cin, cout, xoff)) + ' ')
    assert ('second pass' in label) == (' p2 ' in cid)
    worst, per = 0.0, min(nvox, PERIOD)

    def full(a):
        return cbo.tile_rows(a, nvox)

    def launch(xb, wb, bb, softmax, act):
        ob = Raw(dev, 2 * nvox * cout)
        call(dev, 'nrt_conv1x1_softmax_bf16', xb.p, wb.p, p_of(bb), ob.p, nvox, cin, cout, int(softmax), ACT[act])
        return ob.get(np.uint16, (nvox, cout))

    rng = seeded(cid, 'int')
    x, w = cbo.integers(rng, (per, cin)), cbo.integers(rng, (cin, cout))
    bias = {'exact': cbo.integers(rng, (cout,)), 'rounding': cbo.rounding_bias(rng, cout)}
    pre0, _ = cbo.conv1x1(x, w)
    rounding_premise([pre0 + bias['rounding'].astype(F64)])
    xb, wb = bf(dev, full(x), xoff), bf(dev, w)
    for kind, b in bias.items():
        bb = f32(dev, b)
        for act in (None, 'relu'):
            want = cbo.expected_bits(cbo.activate(pre0 + b.astype(F64), act))
            same_bits(launch(xb, wb, bb, False, act), full(want), '%s %s act %s' % (cid, kind, act))
    same_bits(launch(xb, wb, None, False, None), full(cbo.expected_bits(pre0)), cid + ' exact no bias')

    rng = seeded(cid, 'gauss')
    x, w, b = cbo.gaussian_bf16(rng, (per, cin)), cbo.gaussian_bf16(rng, (cin, cout)), rng.standard_normal(cout).astype(F)
    pre, S_abs = cbo.conv1x1(x, w, b)
    xb, wb, bb = bf(dev, full(x), xoff), bf(dev, w), f32(dev, b)
    for act in (None, 'elu'):
        ref = cbo.activate(pre, act)
        worst = within(worst, launch(xb, wb, bb, False, act), full(ref), full(cbo.bound_conv(ref, S_abs, act)), '%s gauss act %s' % (cid, act))
    p = cbo.softmax_lastdim(pre)
    worst = within(worst, launch(xb, wb, bb, True, None), full(p), full(cbo.bound_prob(p)), cid + ' gauss softmax')
    report(cid, worst)


# ------------------------------------------------------------------------------------------------------------------------------
# softmax_lastdim_bf16<true|false>
# ------------------------------------------------------------------------------------------------------------------------------

SM = [('C 8', 700, 8, 0), ('C 16', 700, 16, 0), ('C 33', 700, 33, 0), ('C 8 x 2 bytes off', 700, 8, 2), ('C 8 second pass', SECOND_4096, 8, 0),
      ('C 3 second pass', SECOND_4096, 3, 0)]
SM_IDS = ['%s %s n %d' % (cbo.plan_id(cbo.plan_softmax(n, ch, xoff)), label, n) for label, n, ch, xoff in SM]


@pytest.mark.parametrize('cid,case', list(zip(SM_IDS, SM)), ids=SM_IDS)
def test_softmax(dev, cid, case):
    label, n, ch, xoff = case
    assert cid.startswith(cbo.plan_id(cbo.plan_softmax(n, ch, xoff)) + ' ') and ('second pass' in label) == (' p2 ' in cid)
    worst = 0.0
    for scale in (1.0, 4.0):
        x = cbo.gaussian_bf16(seeded(cid, scale), (n, ch), scale)
        xb, ob = bf(dev, x, xoff), Raw(dev, 2 * n * ch)
        call(dev, 'nrt_softmax_lastdim_bf16', xb.p, ob.p, n, ch)
        p = cbo.softmax_lastdim(x)
        worst = within(worst, ob.get(np.uint16, (n, ch)), p, cbo.bound_prob(p), '%s scale %g' % (cid, scale))
    report(cid, worst)


# ------------------------------------------------------------------------------------------------------------------------------
# maxpool3d_bf16<8|1>, upsample_concat_bf16<8|1>: copies of bits
# ------------------------------------------------------------------------------------------------------------------------------

MP = [('C %d pool %s %s' % (ch, _x(pool), 'same' if same else 'valid'), (9, 8, 7), 2, ch, pool, same)
      for ch in (16, 5) for pool in ((2, 2, 2), (3, 1, 2), (1, 2, 4)) for same in (True, False)] + [
    # just over 8192 x 256 items per entry
    ('C 16 pool 1x1x2 second pass', (129, 128, 128), 1, 16, (1, 1, 2), True), ('C 5 pool 1x1x2 second pass', (5, 128, 1311), 1, 5, (1, 1, 2), True)]
MP_IDS = ['%s %s %s x %d' % (cbo.plan_id(cbo.plan_maxpool(S, ch, pool, same)), label, _x(S), B) for label, S, B, ch, pool, same in MP]


@pytest.mark.parametrize('cid,case', list(zip(MP_IDS, MP)), ids=MP_IDS)
def test_maxpool(dev, cid, case):
    label, S, B, ch, pool, same = case
    assert cid.startswith(cbo.plan_id(cbo.plan_maxpool(S, ch, pool, same)) + ' ') and ('second pass' in label) == (' p2 ' in cid)
    x = cbo.gaussian_bf16(seeded(cid), (B,) + S + (ch,))
    o = cbo.pooled_shape(S, pool, same)
    xb, ob = bf(dev, x), Raw(dev, 2 * B * int(np.prod(o)) * ch)
    call(dev, 'nrt_maxpool3d_bf16', xb.p, ob.p, B, _lib.ints(S), ch, _lib.ints(pool), int(same))
    same_bits(ob.get(np.uint16, (B,) + o + (ch,)), cbo.to_bits(cbo.maxpool(x, pool, same)), cid)
    report(cid, 0.0)


# label, low-resolution shape, batch, c0, c1, up, byte offset of lo
UC = [('16+32 up 2x2x2', (3, 4, 2), 2, 16, 32, (2, 2, 2), 0), ('3+5 up 1x2x3', (3, 4, 2), 2, 3, 5, (1, 2, 3), 0),
      ('0+8 skip NULL up 2x1x2', (3, 4, 2), 2, 0, 8, (2, 1, 2), 0), ('8+8 lo 2 bytes off up 2x2x2', (3, 4, 2), 2, 8, 8, (2, 2, 2), 2),
      ('8+8 up 1x1x2 second pass', (129, 128, 32), 1, 8, 8, (1, 1, 2), 0), ('3+5 up 1x2x2 second pass', (65, 32, 32), 1, 3, 5, (1, 2, 2), 0)]


def _uc_shape(L, up):
    return tuple(s * u for s, u in zip(L, up))


UC_IDS = ['%s %s %s x %d' % (cbo.plan_id(cbo.plan_upsample(_uc_shape(L, up), c0, c1, lo_off=off)), label, _x(_uc_shape(L, up)), B)
          for label, L, B, c0, c1, up, off in UC]


@pytest.mark.parametrize('cid,case', list(zip(UC_IDS, UC)), ids=UC_IDS)
def test_upsample_concat(dev, cid, case):
    label, L, B, c0, c1, up, off = case
    S = _uc_shape(L, up)
    assert cid.startswith(cbo.plan_id(cbo.plan_upsample(S, c0, c1, lo_off=off)) + ' ') and ('second pass' in label) == (' p2 ' in cid)
    rng = seeded(cid)
    lo = cbo.gaussian_bf16(rng, (B,) + L + (c1,))
    skip = cbo.gaussian_bf16(rng, (B,) + S + (c0,)) if c0 else None
    lb, sb, ob = bf(dev, lo, off), (bf(dev, skip) if c0 else None), Raw(dev, 2 * B * int(np.prod(S)) * (c0 + c1))
    call(dev, 'nrt_upsample_concat_bf16', p_of(sb), c0, lb.p, c1, ob.p, B, _lib.ints(S), _lib.ints(up))
    same_bits(ob.get(np.uint16, (B,) + S + (c0 + c1,)), cbo.to_bits(cbo.upsample_concat(skip, lo, up)), cid)
    report(cid, 0.0)


# ------------------------------------------------------------------------------------------------------------------------------
# add_act_affine_bf16<8|1>
# ------------------------------------------------------------------------------------------------------------------------------

SECOND_8192 = 8192 * 256 + 300
# label, rows, channels, with b, with scale and shift, ACT_MUL_B, byte offset of a
AA = [('a + b', 200, 16, True, False, False, 0), ('a', 200, 16, False, False, False, 0), ('(a + b) scale + shift', 200, 16, True, True, False, 0),
      ('a scale + shift', 200, 16, False, True, False, 0), ('a b', 200, 16, True, False, True, 0), ('a b scale + shift', 200, 16, True, True, True, 0),
      ('a + b n % 8 != 0', 201, 5, True, False, False, 0), ('(a + b) scale + shift C 6', 64, 6, True, True, False, 0),
      ('a + b a 2 bytes off', 200, 16, True, False, False, 2),
      ('(a + b) scale + shift second pass', SECOND_8192 // 2, 16, True, True, False, 0), ('a scale + shift second pass', SECOND_8192 // 5 + 1, 5, False, True, False, 0)]
AA_IDS = ['%s %s n %d C %d' % (cbo.plan_id(cbo.plan_add(rows * ch, ch, hb, hs, a_off=off)), label, rows * ch, ch) for label, rows, ch, hb, hs, mul, off in AA]


@pytest.mark.parametrize('cid,case', list(zip(AA_IDS, AA)), ids=AA_IDS)
def test_add_act_affine(dev, cid, case):
    label, rows, ch, hb, hs, mul, off = case
    n = rows * ch
    assert cid.startswith(cbo.plan_id(cbo.plan_add(n, ch, hb, hs, a_off=off)) + ' ') and ('second pass' in label) == (' p2 ' in cid)
    assert (label == '(a + b) scale + shift C 6') == (n % 8 == 0 and hs and ch % 8 != 0)
    worst, per = 0.0, min(rows, PERIOD)

    def full(v):
        return cbo.tile_rows(v, rows)

    def launch(ab, bb, sb, hb_, act):
        ob = Raw(dev, 2 * n)
        call(dev, 'nrt_add_act_affine_bf16', ab.p, p_of(bb), p_of(sb), p_of(hb_), ob.p, n, ch, ACT[act] | (ACT_MUL_B if mul else 0))
        return ob.get(np.uint16, (rows, ch))

    for kind, amax in (('exact', 3), ('rounding', 30 if mul else 100)):
        rng = seeded(cid, kind)
        a, b = cbo.integers(rng, (per, ch), amax), (cbo.integers(rng, (per, ch), amax) if hb else None)
        scale = rng.choice((-3, -1, 1, 3), size=ch).astype(F) if hs else None
        shift = (cbo.integers(rng, (ch,)) if kind == 'exact' else cbo.rounding_bias(rng, ch)) if hs else None
        assert (amax * amax if mul else 2 * amax) * 3 + ROUND_AMAX < 2 ** 24
        refs = {act: cbo.add_act_affine(a, b, scale, shift, act, mul) for act in (None, 'relu')}
        if kind == 'rounding' and hs:
            cbo.check_shares([refs[None]])
            cbo.check_shares([refs['relu']], 'relu')
        ab, bb, sb, hb_ = bf(dev, full(a), off), (bf(dev, full(b)) if hb else None), (f32(dev, scale) if hs else None), (f32(dev, shift) if hs else None)
        for act, ref in refs.items():
            same_bits(launch(ab, bb, sb, hb_, act), full(cbo.expected_bits(ref)), '%s %s act %s' % (cid, kind, act))

    rng = seeded(cid, 'gauss')
    a, b = cbo.gaussian_bf16(rng, (per, ch)), (cbo.gaussian_bf16(rng, (per, ch)) if hb else None)
    scale, shift = (rng.standard_normal(ch).astype(F), rng.standard_normal(ch).astype(F)) if hs else (None, None)
    ab, bb, sb, hb_ = bf(dev, full(a), off), (bf(dev, full(b)) if hb else None), (f32(dev, scale) if hs else None), (f32(dev, shift) if hs else None)
    for act in (None, 'elu', 'sigmoid'):
        ref = cbo.add_act_affine(a, b, scale, shift, act, mul)
        worst = within(worst, launch(ab, bb, sb, hb_, act), full(ref), full(cbo.bound_elementwise(ref)), '%s gauss act %s' % (cid, act))
    report(cid, worst)


ALL_IDS = IDS + [PACK_ID] + C1_IDS + SM_IDS + MP_IDS + UC_IDS + AA_IDS
