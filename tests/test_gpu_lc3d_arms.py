"""
Every dispatch arm of the LocallyConnected3D kernels (csrc/lc3d.hip: lc3d_fwd<T, NB, MAXIT, STAGED, SPLIT>, lc3d_bwd<T, MAXIT, NB,
HAS_DX, SPLIT>, lc3d_fwd_mfma<T, CPL, S, NCMAX, NPC>, lc3d_fwd_mfma_blk, lc3d_generic<T>, pad3d_rows<U>), each under an id that starts
with the kernel instances the dispatcher launches for the call (`nb3` = a launch with a dead batch entry, ` + ` = the next batch chunk).
`plan_fwd` / `plan_bwd` / `plan_pad` of oracle/lc3d_arms_oracle.py restate the host dispatch; tests/test_lc3d_arms_oracle.py checks
this table against them and against the instances the compiler emitted, every test here asserts the same before it launches, and a
kernel trace of this file with tools/arm_coverage.py --families lc3d confirms it on the device (profiles/dispatch_arms/README.md).

The C ABI is called directly on guarded buffers (tests/arm_buffers.py: Raw, compared byte for byte, bfloat16 as bits): the alignment
of every pointer is exact and every output is checked for writes outside it.  Output grids have a few positions: (2, 3, 2) with
strides (1, 2, 1) and (2, 1, 2), and a single position (the input is the kernel size); the channel counts carry the arm
(nit = ceil(F / RPW), RPW = 64 / (Cout / VEC)).  Batches 1, 2, 3, 6 and 9: NB 1; NB 2; NB 4 with a dead entry; NB 4 then NB 2 at
b0 = 4; three chunks, the last NB 1 at b0 = 8 (the matrix-core forward takes chunks of 8: S 1 with a dead entry; S 2; S 2 then S 1).

Every id is checked twice against the float64 references of oracle/lc3d_arms_oracle.py:

  exact     x, K, bias, g from the integers -3 .. 3, activation none and relu (the backward reads the y the GPU forward stored).
            Every sum of absolute terms is below 2^24 and every bfloat16 output an integer of magnitude <= 256 (asserted on the
            reference; the bfloat16 shapes keep F <= 216 for that), so y, dK, dbias and dx must equal the reference BIT FOR BIT.
  Gaussian  standard normal inputs (rounded to bfloat16 first for that type), activation none and elu, element-wise:
            float32 (n + 3) 2^-24 A (+ 3e-6 for the ELU forward); bfloat16 forward 2^-8 |want| + (n + 3) 2^-24 A; bfloat16 dK and
            dbias ceil(B / 4) 2^-8 A + (n + 3) 2^-24 A; dx is float32 at the ABI.  Exactly 0 where A = 0.  Each id prints its worst
            err / bound in a BOUND line (profiles/dispatch_arms/lc3d_bounds.txt is the record of one run).

Backward ids run with all three outputs, with grad_x NULL (HAS_DX = false), with grad_kernel NULL and with grad_bias NULL.

The float64 reference of a geometry and input kind is computed once and shared by its activations and output sets.  The whole file
takes 6 s on an MI355X (291 tests), the slowest id (grid-stride, 42 M weights) 0.7 s.
"""

import collections
import zlib

import numpy as np
import pytest
import torch

import neurite_amd as ne
from arm_buffers import Raw, call
from neurite_amd import _lib
from oracle import grad_oracle as go
from oracle import lc3d_arms_oracle as lco

pytestmark = pytest.mark.gpu
F, F64 = np.float32, np.float64
F32, BF16 = 'float32', 'bfloat16'
DT = {F32: _lib.DT_F32, BF16: _lib.DT_BF16}
ACT = {None: 0, 'elu': 1, 'relu': 2}
K1, K2, K3 = (1, 1, 1), (2, 2, 2), (3, 3, 3)
# (output grid, strides); the input shape follows from the kernel size
GEOMS = (((2, 3, 2), (1, 2, 1)), ((2, 3, 2), (2, 1, 2)), ((1, 1, 1), (1, 1, 1)))
BATCHES = (1, 2, 3, 6, 9)

Case = collections.namedtuple('Case', 'label dtype cout k cin B geoms x_off k_off mfma variant')


def C(label, dtype, cout, k, cin, B, geoms=GEOMS, x_off=0, k_off=0, mfma=True, variant=0):
    """x_off / k_off: elements by which x / the kernel miss 16-byte alignment; mfma False: under NRT_LC_MFMA=0"""
    return Case(label, dtype, cout, k, cin, B, geoms, x_off, k_off, mfma, variant)


def in_shape(c, geom):
    return tuple((o - 1) * s + k for o, s, k in zip(geom[0], geom[1], c.k))


def fwd_plan(c, geom):
    return lco.plan_fwd(c.dtype, c.B, in_shape(c, geom), c.cin, c.k, geom[1], c.cout, variant=c.variant, x_aligned=c.x_off == 0,
                        k_aligned=c.k_off == 0, mfma=c.mfma)


def bwd_plan(c, geom, has_dx=True):
    return lco.plan_bwd(c.dtype, c.B, in_shape(c, geom), c.cin, c.k, geom[1], c.cout, has_dx=has_dx)


def _x(t):
    return 'x'.join(str(v) for v in t)


def label(c):
    s = '%s %s k%s %d->%d x %d' % (c.label, c.dtype, _x(c.k), c.cin, c.cout, c.B)
    return s + (' x off' if c.x_off else '') + (' K off' if c.k_off else '') + ('' if c.mfma else ' NRT_LC_MFMA=0') + \
        (' variant %d' % c.variant if c.variant else '')


def fwd_id(c):
    return lco.plan_id(fwd_plan(c, c.geoms[-1])) + ' ' + label(c)


def bwd_id(c):
    return lco.plan_id(bwd_plan(c, c.geoms[-1])) + ' ' + label(c)


# the vector kernels: (label, cout, k, cin) per type.  Unstaged: the voxel row is no multiple of 16 bytes.
VEC_F32 = [('MAXIT 8 ragged', 4, K3, 3), ('MAXIT 14 ragged', 16, K3, 7), ('MAXIT 16', 16, K3, 9), ('SPLIT 2 one live group', 32, K3, 5),
           ('SPLIT 4', 32, K3, 10), ('LPR 64', 256, (1, 2, 2), 3)]
STAGED_F32 = [('MAXIT 8 staged', 4, K2, 4), ('MAXIT 14 staged', 32, K2, 12), ('MAXIT 16 staged', 64, K2, 8), ('SPLIT 2 full staged', 32, K2, 32),
              ('SPLIT 4 full staged', 64, K2, 32)]
# bfloat16: F <= 216, so that the integer outputs stay within 256 (4 sqrt(F) is their standard deviation)
VEC_BF16 = [('MAXIT 8 ragged', 8, K3, 3), ('MAXIT 14 ragged', 64, K3, 4), ('MAXIT 16 ragged', 64, (3, 3, 1), 13),
            ('SPLIT 2 one live group', 64, K3, 5), ('SPLIT 4', 128, K3, 5), ('LPR 64', 512, (1, 2, 2), 3)]
STAGED_BF16 = [('MAXIT 8 staged', 8, K3, 8), ('MAXIT 14 staged', 64, (1, 2, 2), 24), ('MAXIT 16 staged', 64, K2, 16),
               ('SPLIT 2 full staged', 128, K2, 16), ('SPLIT 4 full staged', 256, K2, 16)]
G_BLK = (((2, 3, 5), (1, 2, 1)),)            # z extent 5: the second group of four z-positions has one live wave
G_S2 = (GEOMS[1],)                           # z stride 2: not the block-staged form
# the matrix-core forward: (label, dtype, cout, k, cin, geoms)
MFMA = [('blk', F32, 16, (1, 2, 3), 16, G_BLK), ('blk full ring', F32, 16, K3, 16, G_BLK), ('NPC 1', F32, 16, K2, 8, GEOMS[:1]),
        ('NPC 2', F32, 16, K3, 16, G_S2), ('blk', F32, 8, (2, 1, 3), 16, G_BLK), ('blk full ring', F32, 8, K3, 16, G_BLK),
        ('NPC 1', F32, 8, K2, 8, GEOMS[:1]), ('NPC 2', F32, 8, K3, 16, G_S2),
        ('blk', BF16, 16, (1, 2, 3), 16, G_BLK), ('NPC 1', BF16, 16, K2, 8, GEOMS[:1]), ('blk', BF16, 32, (2, 1, 3), 16, G_BLK),
        ('NPC 1', BF16, 32, K2, 8, GEOMS[:1])]

FWD_CASES = []
for _dt, _vec, _staged in ((F32, VEC_F32, STAGED_F32), (BF16, VEC_BF16, STAGED_BF16)):
    FWD_CASES += [C(l, _dt, co, k, ci, B) for l, co, k, ci in _vec + _staged for B in BATCHES]
    FWD_CASES += [C(l.replace('staged', 'unstaged partner'), _dt, co, k, ci, 6, x_off=1) for l, co, k, ci in _staged]
FWD_CASES += [C(l, dt, co, k, ci, B, geoms=g) for l, dt, co, k, ci, g in MFMA for B in (3, 6, 9)]
FWD_CASES += [C(l, dt, co, k, ci, 6, geoms=g, mfma=False) for l, dt, co, k, ci, g in MFMA]
FWD_CASES += [
    # lc3d_generic: asked for, Cout no multiple of the vector, and the silent fallbacks: nit > 64, a misaligned kernel pointer
    C('generic odd Cout', F32, 5, (2, 3, 2), 3, 2), C('generic odd Cout', BF16, 12, (2, 3, 2), 3, 2),
    C('generic LPR 3', F32, 12, K2, 3, 2), C('generic nit 108', F32, 64, K3, 16, 2), C('generic nit 81', BF16, 512, K3, 3, 2),
    C('generic', F32, 4, K3, 3, 2, k_off=1), C('generic', BF16, 8, K3, 3, 2, k_off=1),
    C('generic asked for', F32, 16, K3, 7, 2, variant=1), C('generic asked for', BF16, 8, K3, 8, 2, variant=1),
]
FWD_IDS = [fwd_id(c) for c in FWD_CASES]

BWD_CASES = []
for _dt, _vec, _staged in ((F32, VEC_F32, STAGED_F32), (BF16, VEC_BF16, STAGED_BF16)):
    BWD_CASES += [C(l.replace(' staged', ''), _dt, co, k, ci, B) for l, co, k, ci in _vec + _staged[3:] for B in BATCHES]
BWD_IDS = [bwd_id(c) for c in BWD_CASES]


# ------------------------------------------------------------------------------------------------------------------------------
# buffers, the launches, the comparison
# ------------------------------------------------------------------------------------------------------------------------------

def draw(rng, shape, kind, dtype):
    if kind == 'exact':
        return lco.integers(rng, shape)
    v = rng.standard_normal(shape).astype(F)
    return lco.bf16_value(lco.bf16_bits(v)) if dtype == BF16 else v


def put(dev, dtype, a, off=0):
    """the float32 values `a` (representable in `dtype`) on the device, `off` elements past 16-byte alignment"""
    data = np.ascontiguousarray(a, F) if dtype == F32 else lco.bf16_bits(a)
    return Raw(dev, data.nbytes, off * lco.ITEM[dtype], data)


def out(dev, dtype, n, off=0):
    return Raw(dev, n * lco.ITEM[dtype], off * lco.ITEM[dtype])


def read(buf, dtype, shape):
    return buf.get(F, shape) if dtype == F32 else lco.bf16_value(buf.get(np.uint16, shape))


def run_forward(dev, c, S, st, xb, kb, bb, act, osh):
    yb = out(dev, c.dtype, c.B * int(np.prod(osh)) * c.cout)
    call(dev, 'nrt_lc3d_f', xb.p, kb.p, bb.p if bb is not None else None, yb.p, DT[c.dtype], c.B, _lib.ints(S), c.cin, _lib.ints(c.k),
         _lib.ints(st), c.cout, ACT[act], c.variant)
    return yb


def compare(worst, kind, got, ref, bnd, what, bf16):
    """bit for bit, or within the bound (exactly the reference where the bound is 0); returns the running worst err / bound"""
    if kind == 'exact':
        lco.exact_range(ref, bf16, what)
        lco.check_exact(got, ref, what)
        return worst
    r = lco.ratio(got, ref, bnd)
    assert r <= 1.0, '%s: worst err / bound = %.3g' % (what, r)
    return max(worst, r)


def inputs(cid, c, geom, kind):
    S, osh = in_shape(c, geom), geom[0]
    O, Fd = int(np.prod(osh)), int(np.prod(c.k)) * c.cin
    rng = np.random.default_rng(zlib.crc32(('%s %s %s %s' % (label(c), geom, c.B, kind)).encode()))
    x = draw(rng, (c.B,) + S + (c.cin,), kind, c.dtype)
    K = draw(rng, (O, Fd, c.cout), kind, c.dtype)
    bias = draw(rng, osh + (c.cout,), kind, c.dtype)
    g = draw(rng, (c.B, O, c.cout), kind, c.dtype)
    return S, osh, O, Fd, x, K, bias, g


def forward_checks(c, geom, kind, x, K, bias):
    """the reference of one geometry and input kind: [(act, with bias, want, bound or None)]"""
    pre, A, n = lco.forward(x.astype(F64), K.astype(F64), bias.astype(F64), c.k, geom[1])
    acts = (None, 'relu') if kind == 'exact' else (None, 'elu')
    rows = []
    for act in acts:
        want = lco.activate(pre, act)
        bnd = None if kind == 'exact' else lco.bound_f32(A, n, act == 'elu') if c.dtype == F32 else lco.bound_bf16_fwd(want, A, n)
        rows.append((act, True, want, bnd))
    if kind == 'exact':
        assert A.max() < 2 ** 24
        pre0, _, _ = lco.forward(x.astype(F64), K.astype(F64), None, c.k, geom[1])
        rows.append((None, False, pre0, None))                     # bias = NULL
    return rows


def run_fwd_case(dev, cid, c):
    worst = 0.0
    for geom in c.geoms:
        p = fwd_plan(c, geom)
        assert lco.plan_id(p) + ' ' + label(c) == cid, (cid, geom, p)
        for kind in ('exact', 'gauss'):
            S, osh, O, Fd, x, K, bias, _ = inputs(cid, c, geom, kind)
            xb, kb, bb = put(dev, c.dtype, x, c.x_off), put(dev, c.dtype, K, c.k_off), put(dev, c.dtype, bias)
            for act, with_bias, want, bnd in forward_checks(c, geom, kind, x, K, bias):
                got = read(run_forward(dev, c, S, geom[1], xb, kb, bb if with_bias else None, act, osh), c.dtype, (c.B, O, c.cout))
                worst = compare(worst, kind, got, want, bnd, '%s %s %s act %s bias %s' % (cid, geom, kind, act, with_bias), c.dtype == BF16)
    print('BOUND %-120s worst err / bound: %.3g' % (cid, worst))


@pytest.mark.parametrize('cid,case', list(zip(FWD_IDS, FWD_CASES)), ids=FWD_IDS)
def test_fwd_arm(dev, cid, case, monkeypatch):
    if not case.mfma:
        monkeypatch.setenv('NRT_LC_MFMA', '0')
    run_fwd_case(dev, cid, case)


OUTPUTS = ((True, True, True), (True, True, False), (False, True, True), (True, False, True))       # grad_kernel, grad_bias, grad_x


def run_backward(dev, c, S, st, xb, kb, yb, gb, act, want_k, want_b, want_x, O, Fd):
    dkb = out(dev, c.dtype, O * Fd * c.cout) if want_k else None
    dbb = out(dev, c.dtype, O * c.cout) if want_b else None
    dxb = Raw(dev, c.B * int(np.prod(S)) * c.cin * 4).zero() if want_x else None          # float32, zero-filled by the caller
    call(dev, 'nrt_lc3d_bwd_f', xb.p, kb.p, yb.p if yb is not None else None, gb.p, dkb.p if dkb else None, dbb.p if dbb else None,
         dxb.p if dxb else None, DT[c.dtype], c.B, _lib.ints(S), c.cin, _lib.ints(c.k), _lib.ints(st), c.cout, ACT[act])
    return dkb, dbb, dxb


def run_bwd_case(dev, cid, c):
    worst = 0.0
    bf = c.dtype == BF16
    for geom in c.geoms:
        for has_dx in (True, False):
            p = bwd_plan(c, geom, has_dx)
            assert lco.plan_id(p) == lco.plan_id(bwd_plan(c, c.geoms[-1], has_dx)) and (not has_dx or lco.plan_id(p) + ' ' + label(c) == cid)
        for kind in ('exact', 'gauss'):
            S, osh, O, Fd, x, K, bias, g = inputs(cid, c, geom, kind)
            xb, kb, bb, gb = put(dev, c.dtype, x), put(dev, c.dtype, K), put(dev, c.dtype, bias), put(dev, c.dtype, g)
            for act in (None, 'relu') if kind == 'exact' else (None, 'elu'):
                yb = run_forward(dev, c, S, geom[1], xb, kb, bb, act, osh) if act else None
                y = read(yb, c.dtype, (c.B, O, c.cout)).astype(F64) if act else None
                r = lco.backward(x, K, y, g, c.k, geom[1], act)
                if kind == 'exact':
                    assert max(r.A_dK.max(), r.A_dbias.max(), r.A_dx.max()) < 2 ** 24
                    bk = bb_ = bx = None
                elif bf:
                    bk, bb_, bx = lco.bound_bf16_sum(r.A_dK, r.n_b, c.B), lco.bound_bf16_sum(r.A_dbias, r.n_b, c.B), lco.bound_f32(r.A_dx, r.n_dx)
                else:
                    bk, bb_, bx = lco.bound_f32(r.A_dK, r.n_b), lco.bound_f32(r.A_dbias, r.n_b), lco.bound_f32(r.A_dx, r.n_dx)
                for want_k, want_b, want_x in OUTPUTS:
                    what = '%s %s %s act %s outputs %d%d%d' % (cid, geom, kind, act, want_k, want_b, want_x)
                    dkb, dbb, dxb = run_backward(dev, c, S, geom[1], xb, kb, yb, gb, act, want_k, want_b, want_x, O, Fd)
                    if want_k:
                        worst = compare(worst, kind, read(dkb, c.dtype, (O, Fd, c.cout)), r.dK, bk, what + ' dK', bf)
                    if want_b:
                        worst = compare(worst, kind, read(dbb, c.dtype, (O, c.cout)), r.dbias, bb_, what + ' dbias', bf)
                    if want_x:
                        worst = compare(worst, kind, dxb.get(F, x.shape), r.dx, bx, what + ' dx', False)
    print('BOUND %-120s worst err / bound: %.3g' % (cid, worst))


@pytest.mark.parametrize('cid,case', list(zip(BWD_IDS, BWD_CASES)), ids=BWD_IDS)
def test_bwd_arm(dev, cid, case):
    run_bwd_case(dev, cid, case)


# ------------------------------------------------------------------------------------------------------------------------------
# grid-stride: more positions than waves, one case per SPLIT, forward and backward.  Integer inputs; the reference in float32 numpy,
# exact by the same argument.  Smallest F Cout that reaches the arm: nit > 16 needs F Cout > 4096, nit > 32 F Cout > 8192.
# ------------------------------------------------------------------------------------------------------------------------------

STRIDE = [C('grid-stride', F32, 4, (1, 1, 2), 1, 2, geoms=(((1, 1, 20489), K1),)), C('grid-stride', F32, 32, K1, 129, 2, geoms=(((1, 1, 10250), K1),)),
          C('grid-stride', F32, 32, K1, 257, 2, geoms=(((1, 1, 5130), K1),))]


def stride_id(c):
    O = int(np.prod(c.geoms[0][0]))
    pf, pb = fwd_plan(c, c.geoms[0]), bwd_plan(c, c.geoms[0])
    return '%s walks %d | %s walks %d %s' % (lco.plan_id(pf), lco.walks(pf, O), lco.plan_id(pb), lco.walks(pb, O), label(c))


STRIDE_IDS = [stride_id(c) for c in STRIDE]


@pytest.mark.parametrize('cid,c', list(zip(STRIDE_IDS, STRIDE)), ids=STRIDE_IDS)
def test_grid_stride(dev, cid, c):
    geom = c.geoms[0]
    assert stride_id(c) == cid and ' walks 2 | ' in cid and cid.split(' | ')[1].split(' walks ')[1].startswith('2 ')
    S, osh, O, Fd, x, K, bias, g = inputs(cid, c, geom, 'exact')
    assert 9 * Fd + 3 < 2 ** 24 and 9 * c.B < 2 ** 24 and 9 * c.cout * int(np.prod(c.k)) < 2 ** 24          # every sum of absolute terms
    P = lco.patches(x, c.k, geom[1], F)
    pre = np.einsum('bof,ofc->boc', P, K) + bias.reshape(1, O, c.cout)
    xb, kb, bb, gb = put(dev, c.dtype, x), put(dev, c.dtype, K), put(dev, c.dtype, bias), put(dev, c.dtype, g)
    y = None
    for act in (None, 'relu'):
        yb = run_forward(dev, c, S, geom[1], xb, kb, bb, act, osh)
        y = read(yb, c.dtype, (c.B, O, c.cout))
        lco.check_exact(y, lco.activate(pre, act).astype(F64), '%s forward act %s' % (cid, act))
    r = lco.backward(x, K, y, g, c.k, geom[1], 'relu', dt=F, with_abs=False)
    dkb, dbb, dxb = run_backward(dev, c, S, geom[1], xb, kb, yb, gb, 'relu', True, True, True, O, Fd)
    lco.check_exact(read(dkb, c.dtype, (O, Fd, c.cout)), r.dK.astype(F64), cid + ' dK')
    lco.check_exact(read(dbb, c.dtype, (O, c.cout)), r.dbias.astype(F64), cid + ' dbias')
    lco.check_exact(dxb.get(F, x.shape), r.dx.astype(F64), cid + ' dx')


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: the layer has no generic backward
# ------------------------------------------------------------------------------------------------------------------------------

# label, dtype, cout, k, cin, which pointer is 4 (float32) / 2 (bfloat16) bytes off alignment
REFUSALS = [('Cout 5', F32, 5, K2, 3, None), ('Cout 12 LPR 3', F32, 12, K2, 3, None), ('Cout 12', BF16, 12, K2, 3, None), ('nit 108', F32, 64, K3, 16, None),
            ('kernel off', F32, 8, K2, 3, 'kernel'), ('grad_out off', F32, 8, K2, 3, 'grad_out'), ('y off', F32, 8, K2, 3, 'y'),
            ('grad_kernel off', F32, 8, K2, 3, 'grad_kernel'), ('kernel off', BF16, 8, K2, 3, 'kernel'), ('grad_kernel off', BF16, 8, K2, 3, 'grad_kernel')]
REFUSAL_IDS = ['unsupported %s %s' % (r[1], r[0]) for r in REFUSALS]


@pytest.mark.parametrize('rid,case', list(zip(REFUSAL_IDS, REFUSALS)), ids=REFUSAL_IDS)
def test_bwd_refusal(dev, rid, case):
    """nrt_lc3d_bwd_f returns NRT_ERR_UNSUPPORTED before any launch: not one byte of the three output buffers is written"""
    lab, dtype, cout, k, cin, off = case
    c = C(lab, dtype, cout, k, cin, 2)
    geom = GEOMS[0]
    S, osh, O, Fd, x, K, bias, g = inputs(rid, c, geom, 'exact')
    assert lco.plan_bwd(dtype, c.B, S, cin, k, geom[1], cout, aligned=off is None) == 'unsupported'
    assert off is None or lco.plan_bwd(dtype, c.B, S, cin, k, geom[1], cout) != 'unsupported'
    o = {name: int(name == off) for name in ('kernel', 'grad_out', 'y', 'grad_kernel')}
    xb, kb, gb, yb = put(dev, dtype, x), put(dev, dtype, K, o['kernel']), put(dev, dtype, g, o['grad_out']), put(dev, dtype, g, o['y'])
    dkb, dbb = out(dev, dtype, O * Fd * cout, o['grad_kernel']), out(dev, dtype, O * cout)
    dxb = Raw(dev, x.size * 4)
    for act in (None, 'relu'):
        with torch.cuda.device(dev):
            rc = _lib.lib().nrt_lc3d_bwd_f(xb.p, kb.p, yb.p, gb.p, dkb.p, dbb.p, dxb.p, DT[dtype], c.B, _lib.ints(S), cin, _lib.ints(k),
                                           _lib.ints(geom[1]), cout, ACT[act], _lib.stream_ptr(dev))
        torch.cuda.synchronize(dev)
        assert rc == _lib.NRT_ERR_UNSUPPORTED, rc
        assert dkb.untouched() and dbb.untouched() and dxb.untouched()


@pytest.mark.parametrize('dtype,cout,k,cin', [(F32, 5, K2, 3), (F32, 12, K2, 3), (BF16, 12, K2, 3), (F32, 64, K3, 16)])
def test_layer_raises_where_the_backward_is_unsupported(dev, dtype, cout, k, cin):
    """LocallyConnected3D computes these forwards on lc3d_generic; asked for a gradient it raises rather than return numbers"""
    tdt = getattr(torch, dtype)
    S = in_shape(C('', dtype, cout, k, cin, 2), GEOMS[0])
    assert lco.plan_bwd(dtype, 2, S, cin, k, GEOMS[0][1], cout) == 'unsupported'
    x = torch.randn((2,) + S + (cin,), device=dev).to(tdt).requires_grad_()
    layer = ne.layers.LocallyConnected3D(cout, k, strides=GEOMS[0][1])
    layer(x.detach().float())
    layer.to(tdt)
    y = layer(x)
    with pytest.raises(ne._lib.NeuriteAmdError, match='nrt_lc3d_bwd_f'):
        y.float().sum().backward()
    assert x.grad is None and layer.kernel.grad is None and layer.bias.grad is None


def test_fwd_variant_2_refusal(dev):
    """variant 2 where the vector kernels cannot run: NRT_ERR_UNSUPPORTED, nothing written"""
    c = C('', F32, 5, K2, 3, 2, variant=2)
    assert fwd_plan(c, GEOMS[0]) == 'unsupported'
    S, osh, O, Fd, x, K, bias, g = inputs('variant 2', c, GEOMS[0], 'exact')
    xb, kb, yb = put(dev, F32, x), put(dev, F32, K), out(dev, F32, c.B * O * c.cout)
    with torch.cuda.device(dev):
        rc = _lib.lib().nrt_lc3d_f(xb.p, kb.p, None, yb.p, DT[F32], c.B, _lib.ints(S), c.cin, _lib.ints(c.k), _lib.ints(GEOMS[0][1]), c.cout, 0, 2,
                                   _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc == _lib.NRT_ERR_UNSUPPORTED and yb.untouched()


# ------------------------------------------------------------------------------------------------------------------------------
# nrt_pad3d
# ------------------------------------------------------------------------------------------------------------------------------

# row_bytes, byte offset of both pointers from 16-byte alignment
PAD_ROWS = ((2, 0), (6, 0), (8, 0), (12, 4), (8, 2), (64, 0), (62, 0))
PAD_GEOMS = (((3, 2, 4), (0, 0, 0), (3, 2, 4)), ((3, 2, 4), (1, 0, 2), (5, 3, 7)), ((3, 2, 4), (0, 0, 0), (4, 4, 5)), ((1, 1, 1), (2, 1, 1), (3, 2, 2)))
PAD_CASES = [(rb, off, crop) for rb, off in PAD_ROWS for crop in (0, 1)]
PAD_IDS = ['%s row_bytes %d pointers +%d %s' % (lco.plan_pad(rb, off, off), rb, off, 'crop' if crop else 'pad') for rb, off, crop in PAD_CASES]


@pytest.mark.parametrize('pid,case', list(zip(PAD_IDS, PAD_CASES)), ids=PAD_IDS)
def test_pad3d(dev, pid, case):
    """zero padding and its gradient, the crop, on distinct bit patterns against numpy slicing: pad_before zero and non-zero, padding
    after the volume, batch 2; 16-bit units for an odd bfloat16 channel count and for pointers aligned to 2 bytes only"""
    rb, off, crop = case
    ut = np.uint32 if pid.startswith('pad3d_rows<unsignedint>') else np.uint16
    assert (ut == np.uint32) == (rb % 4 == 0 and off % 4 == 0)
    units = rb // 2                                             # the reference works on 16-bit units throughout
    B = 2
    for S, before, padded in PAD_GEOMS:
        small, big = (B,) + S + (units,), (B,) + padded + (units,)
        box = (slice(None),) + tuple(slice(p, p + s) for p, s in zip(before, S))
        src_shape = big if crop else small
        src = (np.arange(int(np.prod(src_shape)), dtype=np.uint32) % 65521 + 1).astype(np.uint16).reshape(src_shape)
        if crop:
            want = src[box]
        else:
            want = np.zeros(big, np.uint16)
            want[box] = src
        ib = Raw(dev, src.nbytes, off, src)
        ob = Raw(dev, want.nbytes, off)
        assert lco.plan_pad(rb, ib.t.data_ptr(), ob.t.data_ptr()) + ' ' == pid[:pid.index(' ') + 1]
        call(dev, 'nrt_pad3d', ib.p, ob.p, B, _lib.ints(S), _lib.ints(before), _lib.ints(padded), rb, crop)
        assert np.array_equal(ob.get(np.uint16, want.shape), want), (pid, S, before, padded)


# ------------------------------------------------------------------------------------------------------------------------------
# through the layer: a SPLIT shape at batch 9 (three batch chunks), the input without a gradient (grad_x NULL), then the kernel frozen
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype,cout,cin', [(F32, 32, 5), (BF16, 32, 10)])
def test_layer_split_batch_9(dev, dtype, cout, cin):
    """gradients of layers.LocallyConnected3D against float64 autograd of oracle/grad_oracle.lc3d within the element-wise bounds of
    the Gaussian check (linear activation: the bounds are those of the sums alone)"""
    tdt = getattr(torch, dtype)
    B, (osh, st) = 9, GEOMS[0]
    c = C('layer', dtype, cout, K3, cin, B)
    S = in_shape(c, GEOMS[0])
    assert 'true,2> nb1' in lco.plan_id(bwd_plan(c, GEOMS[0])) and 'false,2> nb1' in lco.plan_id(bwd_plan(c, GEOMS[0], False))
    _, _, O, Fd, x, K, bias, g = inputs('layer', c, GEOMS[0], 'gauss')
    layer = ne.layers.LocallyConnected3D(cout, K3, strides=st)
    xt = torch.from_numpy(x).to(dev).to(tdt)
    layer(xt.float())
    layer.to(tdt)
    with torch.no_grad():
        layer.kernel.copy_(torch.from_numpy(K).to(tdt))
        layer.bias.copy_(torch.from_numpy(bias).to(tdt))
    gt = torch.from_numpy(g.reshape((B,) + osh + (cout,))).to(dev)
    xo = torch.from_numpy(x).double()
    ko, bo = torch.from_numpy(K).double().requires_grad_(), torch.from_numpy(bias).double().requires_grad_()
    (go.lc3d(xo, ko, bo, K3, st) * gt.cpu().double()).sum().backward()
    r = lco.backward(x, K, None, g, K3, st)
    assert np.abs(r.dK - ko.grad.numpy()).max() <= 1e-12 * np.abs(r.dK).max()
    bound = (lambda A: lco.bound_f32(A, B)) if dtype == F32 else (lambda A: lco.bound_bf16_sum(A, B, B))
    for frozen in (False, True):
        layer.kernel.requires_grad_(not frozen)
        layer.kernel.grad = layer.bias.grad = None
        y = layer(xt)
        (y.float() * gt).sum().backward()
        assert (layer.kernel.grad is None) == frozen and layer.bias.grad.dtype == tdt
        rb = lco.ratio(layer.bias.grad.float().cpu().numpy().reshape(O, cout), bo.grad.numpy().reshape(O, cout), bound(r.A_dbias))
        rk = 0.0 if frozen else lco.ratio(layer.kernel.grad.float().cpu().numpy(), ko.grad.numpy(), bound(r.A_dK))
        print('BOUND layer %s kernel frozen %s: worst err / bound dK %.3g dbias %.3g' % (dtype, frozen, rk, rb))
        assert rb <= 1.0 and rk <= 1.0
