"""
TEST INFRASTRUCTURE ONLY -- the host dispatch of neurite_amd/csrc/lc3d.hip restated (nrt_lc3d_f: launch_any, launch_mfma, launch_vec;
nrt_lc3d_bwd_f: launch_bwd, launch_bwd_it; nrt_pad3d), and plain float64 numpy references of the LocallyConnected3D forward and
backward with the sum of absolute terms A and the number of terms n of every output element (CPU, no GPU import).

    y[b, o, c]     = act(bias[o, c] + sum_f patch[b, o, f] K[o, f, c])          patch flattened (kr, kc, kz, cin), positions row-major
    dpre           = g * slope(y)                                              slope through the STORED output (csrc/activations.h)
    dK[o, f, c]    = sum_b patch[b, o, f] dpre[b, o, c]
    dbias[o, c]    = sum_b dpre[b, o, c]
    dx[b, voxel]   = sum over the (o, f) that read the voxel, sum_c K[o, f, c] dpre[b, o, c]

Bounds (derived, not measured; profiles/dispatch_arms/README.md): a float32 result of n terms accumulated in float32 in any order is
within (n + 3) 2^-24 A of the exact one (n roundings of partial sums bounded by A, the bias add and the two roundings of dpre); a
bfloat16 forward adds one rounding of the result, 2^-8 |want|; bfloat16 dK / dbias are rounded once per batch chunk of 4 entries
(the read-modify-write of launch_bwd_it), each at most 2^-8 of a partial sum bounded by A.

With x, K, bias and g from the integers -3 .. 3 every product and partial sum is an integer below 2^24, and every bfloat16 output an
integer of magnitude <= 256 (asserted on the reference), so float32 accumulation, atomics in any order, the per-chunk
read-modify-write and the single bfloat16 rounding are exact: the outputs equal the reference bit for bit.

`plan_fwd` / `plan_bwd` / `plan_pad` name the kernel instances a call launches, in the spelling of tools/arm_coverage.norm.
tests/test_lc3d_arms_oracle.py checks the case table of tests/test_gpu_lc3d_arms.py against them and against the instances the
compiler emitted (profiles/dispatch_arms/lc3d_kernels.txt).

Only tests/ may import this module.
"""

import collections

import numpy as np

from oracle import np_oracle as npo
from oracle.conv_wgrad_oracle import check_exact, integers, ratio                        # noqa: F401 (re-exported)

F, F64 = np.float32, np.float64
U = 2.0 ** -24
TNAME = {'float32': 'float', 'bfloat16': 'unsignedshort'}
ITEM = {'float32': 4, 'bfloat16': 2}
FWD_CAP, BWD_CAP, GENERIC_CAP = 256 * 20, 256 * 16, 256 * 16
NXCD = 8

Launch = collections.namedtuple('Launch', 'name blocks nb b0')


# ------------------------------------------------------------------------------------------------------------------------------
# bfloat16 as bits
# ------------------------------------------------------------------------------------------------------------------------------

def bf16_bits(a):
    """float32 -> bfloat16 bits, round to nearest even (finite values)"""
    u = np.ascontiguousarray(a, F).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(F)


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch
# ------------------------------------------------------------------------------------------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def _b(v):
    return 'true' if v else 'false'


def out_shape(in_shape, ksize, strides):
    return tuple((s - k) // st + 1 for s, k, st in zip(in_shape, ksize, strides))


def _geom(dtype, in_shape, cin, ksize, cout):
    item = ITEM[dtype]
    vec = 16 // item
    Fd = ksize[0] * ksize[1] * ksize[2] * cin
    lpr = cout // vec if cout % vec == 0 else 0
    ok = lpr >= 1 and lpr <= 64 and (lpr & (lpr - 1)) == 0
    nit = _cdiv(Fd, 64 // lpr) if ok else 0
    vol_bytes = in_shape[0] * in_shape[1] * in_shape[2] * cin * item
    return item, Fd, lpr, ok, nit, vol_bytes


def _ladder(nit):
    """(MAXIT, SPLIT) of launch_any / launch_bwd"""
    return (8, 1) if nit <= 8 else (14, 1) if nit <= 14 else (16, 1) if nit <= 16 else (16, 2) if nit <= 32 else (16, 4)


def _nbt(nb):
    return 1 if nb == 1 else 2 if nb == 2 else 4


def stage_chunks(dtype, cin, ksize, x_aligned=True):
    """launch_any: the patch is kr * kc runs of kz * Cin elements; staged when run and voxel are whole 16-byte pieces"""
    item = ITEM[dtype]
    runb = ksize[2] * cin * item
    chunks = runb // 16 * ksize[0] * ksize[1]
    ok = runb % 16 == 0 and (cin * item) % 16 == 0 and chunks <= 128 and x_aligned and chunks * 16 * 4 * 4 <= 48 * 1024
    return chunks if ok else 0


def plan_fwd(dtype, B, in_shape, cin, ksize, strides, cout, variant=0, x_aligned=True, k_aligned=True, y_aligned=True, bias_aligned=True,
             mfma=True, cus=256, mfma_blocks_per_cu=2):
    """nrt_lc3d_f: the launches [(instance, blocks, nb, b0)], or 'unsupported'.  mfma: NRT_LC_MFMA is not 0.  The matrix-core grids
    are capped at the resident blocks (an occupancy query times the CU count); `mfma_blocks_per_cu` stands for the query."""
    item, Fd, lpr, ok, nit, vol_bytes = _geom(dtype, in_shape, cin, ksize, cout)
    T = TNAME[dtype]
    osh = out_shape(in_shape, ksize, strides)
    O = osh[0] * osh[1] * osh[2]
    vec_ok = ok and k_aligned and nit <= 64 and vol_bytes < 2 ** 31 and Fd * cout * item < 2 ** 31
    if variant == 0:
        variant = 2 if vec_ok else 1
    if variant != 2:
        return [Launch('lc3d_generic<%s>' % T, min(_cdiv(O * cout, 256), GENERIC_CAP), B, 0)]
    if not vec_ok:
        return 'unsupported'
    sc = stage_chunks(dtype, cin, ksize, x_aligned)
    cpl = cout // 4
    if (dtype == 'bfloat16' and cout in (16, 32)) or (dtype == 'float32' and cout in (16, 8)):
        ncmax = 27 if cpl * item == 8 else 28
        elig = (mfma and B >= 3 and Fd % 16 == 0 and Fd // 16 <= ncmax and 1 <= sc <= 128 and sc * 16 == Fd * item
                and k_aligned and y_aligned and bias_aligned and vol_bytes * 8 < 2 ** 31)
        if elig:
            two = sc > 64
            blk_ok = ksize[2] == 3 and cin == 16 and strides[2] == 1 and ksize[0] * ksize[1] <= 9 and x_aligned
            cinb = 16 * item
            cap = NXCD * _cdiv(mfma_blocks_per_cu * cus, NXCD)
            out = []
            for b0 in range(0, B, 8):
                nb = min(8, B - b0)
                S = 1 if nb <= 4 else 2
                if blk_ok:
                    npt = _cdiv(4 * S * 9 * 6 * cinb // 16, 256)
                    blocks = min(NXCD * _cdiv(osh[0] * osh[1] * _cdiv(osh[2], 4), NXCD), cap)
                    out.append(Launch('lc3d_fwd_mfma_blk<%s,%d,%d,%d,%d>' % (T, cpl, S, ncmax, npt), blocks, nb, b0))
                else:
                    blocks = min(NXCD * _cdiv(_cdiv(O, 4), NXCD), cap)
                    out.append(Launch('lc3d_fwd_mfma<%s,%d,%d,%d,%d>' % (T, cpl, S, ncmax, 2 if two else 1), blocks, nb, b0))
            return out
    maxit, split = _ladder(nit)
    blocks = min(_cdiv(O, 4 // split), FWD_CAP)
    return [Launch('lc3d_fwd<%s,%d,%d,%s,%d>' % (T, _nbt(min(4, B - b0)), maxit, _b(sc > 0), split), blocks, min(4, B - b0), b0)
            for b0 in range(0, B, 4)]


def plan_bwd(dtype, B, in_shape, cin, ksize, strides, cout, has_dx=True, aligned=True):
    """nrt_lc3d_bwd_f: the launches, or 'unsupported' (NRT_ERR_UNSUPPORTED, returned before any launch).  aligned: kernel, grad_out,
    y and grad_kernel are all 16-byte aligned (NULL counts as aligned)."""
    item, Fd, lpr, ok, nit, vol_bytes = _geom(dtype, in_shape, cin, ksize, cout)
    if not ok or nit > 64 or Fd * cout * item >= 2 ** 31 or not aligned or vol_bytes >= 2 ** 31:
        return 'unsupported'
    osh = out_shape(in_shape, ksize, strides)
    O = osh[0] * osh[1] * osh[2]
    maxit, split = _ladder(nit)
    blocks = min(BWD_CAP, _cdiv(O, 4 // split))
    return [Launch('lc3d_bwd<%s,%d,%d,%s,%d>' % (TNAME[dtype], maxit, _nbt(min(4, B - b0)), _b(has_dx), split), blocks, min(4, B - b0), b0)
            for b0 in range(0, B, 4)]


def plan_pad(row_bytes, in_ptr=0, out_ptr=0):
    """nrt_pad3d: 32-bit units when the voxel row is whole words and both pointers are word aligned, 16-bit units otherwise"""
    wide = row_bytes % 4 == 0 and ((in_ptr | out_ptr) & 3) == 0
    return 'pad3d_rows<unsignedint>' if wide else 'pad3d_rows<unsignedshort>'


def plan_id(p):
    """the launches of a call as the head of a test id: the instances joined by ' + ', each with ' nbN' (its live batch entries) when
    the call has several launches or the launch carries dead entries (N is not 1, 2 or 4)"""
    if isinstance(p, str):
        return p
    return ' + '.join('%s nb%d' % (l.name, l.nb) if len(p) > 1 or l.nb != _nbt(l.nb) else l.name for l in p)


def walks(p, O):
    """the most positions (groups of four for the block-staged kernel) one wave of the first launch walks"""
    l = p[0]
    split = int(l.name.rsplit(',', 1)[1][:-1]) if l.name.startswith(('lc3d_fwd<', 'lc3d_bwd<')) else 1
    return _cdiv(O, l.blocks * (4 // split))


# ------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------

def slope(y, act):
    """d act / d pre through the output y: nrt_activate_slope of csrc/activations.h"""
    if act == 'elu':
        return np.where(y > 0, 1.0, y + 1.0)
    if act == 'relu':
        return np.where(y > 0, 1.0, 0.0)
    assert act is None, act
    return np.ones_like(y)


def activate(v, act):
    if act == 'elu':
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    if act == 'relu':
        return np.maximum(v, 0)
    assert act is None, act
    return v


def forward(x, K, bias, ksize, strides, dt=F64):
    """(pre-activation [B, O, Cout], A, n): np_oracle.lc3d, and the same sum over absolute values"""
    B = x.shape[0]
    cout = K.shape[-1]
    pre = npo.lc3d(x, K, bias, ksize, strides, accumulate=dt)
    A = npo.lc3d(np.abs(x), np.abs(K), None if bias is None else np.abs(bias), ksize, strides, accumulate=dt)
    return pre.reshape(B, -1, cout), A.reshape(B, -1, cout), K.shape[1] + (bias is not None)


def patches(x, ksize, strides, dt=F64):
    """[B, O, F]: the patch of every output position, flattened (kr, kc, kz, cin)"""
    B, R, C, Z, cin = x.shape
    osh = out_shape((R, C, Z), ksize, strides)
    P = np.empty((B,) + osh + tuple(ksize) + (cin,), dt)
    for dr in range(ksize[0]):
        for dc in range(ksize[1]):
            for dz in range(ksize[2]):
                P[:, :, :, :, dr, dc, dz, :] = x[:, dr:dr + strides[0] * osh[0]:strides[0], dc:dc + strides[1] * osh[1]:strides[1],
                                                 dz:dz + strides[2] * osh[2]:strides[2], :]
    return P.reshape(B, osh[0] * osh[1] * osh[2], -1)


def _scatter(contrib, shape, ksize, strides, osh):
    """adds contrib[b, o, f] onto the voxel that element f of the patch of position o is"""
    B, cin = shape[0], shape[-1]
    dx = np.zeros(shape, contrib.dtype)
    c = contrib.reshape((B,) + osh + tuple(ksize) + (cin,))
    for dr in range(ksize[0]):
        for dc in range(ksize[1]):
            for dz in range(ksize[2]):
                dx[:, dr:dr + strides[0] * osh[0]:strides[0], dc:dc + strides[1] * osh[1]:strides[1],
                   dz:dz + strides[2] * osh[2]:strides[2], :] += c[:, :, :, :, dr, dc, dz, :]
    return dx


Grads = collections.namedtuple('Grads', 'dK A_dK dbias A_dbias n_b dx A_dx n_dx')


def backward(x, K, y, g, ksize, strides, act=None, dt=F64, with_abs=True):
    """the gradients from x [B, R, C, Z, Cin], K [O, F, Cout], the stored output y and g (both [B, O, Cout]), each with its sum of
    absolute terms and its number of terms (n_b = B for dK and dbias; n_dx per voxel)"""
    x, K, g = np.asarray(x, dt), np.asarray(K, dt), np.asarray(g, dt)
    B = x.shape[0]
    cout = K.shape[-1]
    osh = out_shape(x.shape[1:4], ksize, strides)
    dpre = g if act is None else g * slope(np.asarray(y, dt), act).astype(dt)
    P = patches(x, ksize, strides, dt)
    dK = np.einsum('bof,boc->ofc', P, dpre)
    dbias = dpre.sum(0)
    dx = _scatter(np.einsum('boc,ofc->bof', dpre, K), x.shape, ksize, strides, osh)
    if not with_abs:
        return Grads(dK, None, dbias, None, B, dx, None, None)
    aP, ad = np.abs(P), np.abs(dpre)
    A_dx = _scatter(np.einsum('boc,ofc->bof', ad, np.abs(K)), x.shape, ksize, strides, osh)
    n_dx = _scatter(np.full(P.shape, float(cout), dt), x.shape, ksize, strides, osh)
    return Grads(dK, np.einsum('bof,boc->ofc', aP, ad), dbias, ad.sum(0), B, dx, A_dx, n_dx)


def bound_f32(A, n, elu=False):
    return (n + 3) * U * A + (3e-6 if elu else 0.0)


def bound_bf16_fwd(want, A, n):
    return 2.0 ** -8 * np.abs(want) + (n + 3) * U * A


def bound_bf16_sum(A, n, B):
    """bfloat16 dK / dbias: one rounding per batch chunk of 4 entries"""
    return _cdiv(B, 4) * 2.0 ** -8 * A + (n + 3) * U * A


def exact_range(ref, bf16, what=''):
    """the exact check's premise, on the reference alone: integers below 2^24; a bfloat16 output of magnitude <= 256"""
    assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max(initial=0.0) < 2 ** 24, what + ': not in the exact range'
    if bf16:
        assert np.abs(ref).max(initial=0.0) <= 256, what + ': a bfloat16 output above 256 (%g)' % np.abs(ref).max()
