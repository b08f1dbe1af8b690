"""
TEST INFRASTRUCTURE ONLY -- references and the restated host dispatch of the bfloat16 inference kernels (neurite_amd/csrc/conv_bf16.hip:
nrt_conv3d_bf16, nrt_conv3d_pack_weights_bf16, nrt_conv1x1_softmax_bf16, nrt_softmax_lastdim_bf16, nrt_maxpool3d_bf16,
nrt_upsample_concat_bf16, nrt_add_act_affine_bf16).  CPU, numpy, no GPU import.

The contract of the family: tensors are stored as bf16, a kernel computes in float32 from the stored values and rounds its result to
bf16 ONCE, to nearest, ties to even.  `rne_bf16` is that rounding in integer arithmetic on the float32 bit pattern, independent of
torch's conversion (tests/test_conv_bf16_oracle.py compares the two).  With integer inputs the float32 value before the rounding is an
integer below 2^24, exact in any order and on the matrix cores, so the bf16 output must equal `rne_bf16(reference)` BIT FOR BIT;
`rounding_shares` says how many of a reference's values are not representable, are ties that round up / down in magnitude, or are
non-ties, so that a test can require that its data exercises the rounding before it looks at a GPU result.

The convolution reference is `conv` of oracle/conv_fwd_oracle.py (float64, with the sum of absolute terms S); nothing of the kernel's
4 x 4 x 16 tiles, 8-channel groups, staged chunks or N split is in it.  The glue references below are a few lines of float64 each.

`plan` restates the host code of nrt_conv3d_bf16, the glue plans that of the other entry points; `cus` (the device's compute units) is
an argument.  tests/test_conv_bf16_oracle.py checks the case table of tests/test_gpu_conv_bf16_arms.py against them and against the
instances the compiler emitted; a kernel trace of that file confirms it on the device (profiles/dispatch_arms/README.md).

Only tests/ may import this module.
"""

import collections

import numpy as np

from oracle.conv_fwd_oracle import F, F64, U, NXCD, TILE, activate, batch_for, conv, exact_condition, integers, ratio, tiles_per_entry  # noqa: F401

U16, U32 = np.uint16, np.uint32


# ------------------------------------------------------------------------------------------------------------------------------
# bfloat16
# ------------------------------------------------------------------------------------------------------------------------------

def rne_bf16(a):
    """float32 array -> float32 array of the nearest bf16 values, ties to even (finite values)"""
    bits = np.ascontiguousarray(a, F).view(U32)                     # finite values: the sum below stays within 32 bits
    r = ((bits + U32(0x7FFF) + ((bits >> U32(16)) & U32(1))) >> U32(16)) << U32(16)
    return r.view(F).reshape(np.shape(a))


def to_bits(a):
    """the 16-bit patterns of a float32 array that holds bf16 values exactly"""
    bits = np.ascontiguousarray(a, F).view(U32)
    assert not (bits & 0xFFFF).any(), 'not a bf16 value'
    return (bits >> 16).astype(U16).reshape(np.shape(a))


def from_bits(b):
    return (np.ascontiguousarray(b, U16).astype(U32) << 16).view(F).reshape(np.shape(b))


def gaussian_bf16(rng, shape, scale=1.0):
    """standard-normal values (x scale) rounded to bf16, as float32"""
    v = rng.standard_normal(shape, dtype=F)
    if scale != 1.0:
        v *= F(scale)
    return rne_bf16(v)


def tile_rows(block, rows):
    """`rows` rows that repeat the rows of `block` cyclically"""
    block = np.asarray(block)
    return block if len(block) == rows else np.tile(block, (-(-rows // len(block)),) + (1,) * (block.ndim - 1))[:rows]


def expected_bits(ref):
    """the bf16 bits of a float64 reference that float32 holds exactly (integers below 2^24): one rounding to nearest even.  The sign of
    a zero counts: -3 x 0 is -0 in float32 as in float64, while a sum that starts from a +0 accumulator is +0."""
    r = np.asarray(ref, F64)
    f = r.astype(F)
    assert np.array_equal(f.astype(F64), r), 'the reference is not exact in float32'
    return to_bits(rne_bf16(f))


Shares = collections.namedtuple('Shares', 'inexact up down nontie')


def rounding_shares(ref):
    """of the values of a reference exact in float32: the share not representable in bf16, the share of exact ties that round up in
    magnitude, of exact ties that round down in magnitude, and of non-ties"""
    bits = np.asarray(ref, F64).astype(F).reshape(-1).view(U32)
    low, odd = bits & 0xFFFF, ((bits >> 16) & 1) == 1
    n = float(max(bits.size, 1))
    tie = low == 0x8000
    return Shares((low != 0).sum() / n, (tie & odd).sum() / n, (tie & ~odd).sum() / n, ((low != 0) & ~tie).sum() / n)


def check_shares(refs, act=None):
    """the premise of a rounding check, on the reference alone: at least 50 % of the outputs not representable, 8 % ties in each
    direction and 25 % non-ties with activation none, half of each with relu"""
    s = rounding_shares(np.concatenate([np.asarray(r, F64).reshape(-1) for r in refs]))
    f = 0.5 if act == 'relu' else 1.0
    assert s.inexact >= 0.50 * f and s.up >= 0.08 * f and s.down >= 0.08 * f and s.nontie >= 0.25 * f, (act, s)
    return s


def rounding_bias(rng, n):
    """n per-channel values with magnitudes from the integers 257 .. 1000 and signs alternating over the channels.  A layer may have as
    few as 4 channels, so the magnitudes are stratified: channel i draws from the (n - 1 - i)-th of n equal parts of the range, which
    puts channels on both sides of 512 (below it every odd integer is a tie, above it every second one is a non-tie) whatever the
    draw.  The even channels are the positive ones: with an odd channel count relu keeps the larger half, and with 4 or 5 channels it
    keeps parts above 512 (815 .. 1000 and 443 .. 628; 852 .. 1000, 554 .. 702 and 257 .. 405), where the non-ties are."""
    i = np.arange(n)
    mag = 257 + np.floor((n - 1 - i + rng.random(n)) * 744 / n).astype(np.int64)
    assert mag.min() >= 257 and mag.max() <= 1000
    return (mag * np.where(i % 2, -1, 1)).astype(F)


def bound_conv(ref, S_abs, act=None):
    """check_layer of tests/test_gpu_unet_bf16.py: 2^-8 |act(ref)| + 9 x 2^-24 x S (+ 3e-6 with ELU)"""
    return 2.0 ** -8 * np.abs(ref) + 9 * U * np.asarray(S_abs, F64) + (3e-6 if act == 'elu' else 0.0)


def bound_prob(p):
    """the softmax criterion of tests/test_gpu_unet_bf16.py: 2^-8 p + 1e-6"""
    return 2.0 ** -8 * np.asarray(p, F64) + 1e-6


def bound_elementwise(ref):
    """the element-wise criterion of tests/test_gpu_unet_bf16.py: 2^-8 |ref| + 4e-7 (1 + |ref|)"""
    return 2.0 ** -8 * np.abs(ref) + 4e-7 * (1 + np.abs(ref))


# ------------------------------------------------------------------------------------------------------------------------------
# the glue operations, float64
# ------------------------------------------------------------------------------------------------------------------------------

def softmax_lastdim(x):
    x = np.asarray(x, F64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def conv1x1(x, w, b=None):
    """x [n, cin], w [cin, cout], b [cout] or None -> (pre, S): pre = x w + b and the sum of its absolute terms"""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    pre, S = 0.0 + x @ w, np.abs(x) @ np.abs(w)                    # a sum: +0 where every product is a zero of either sign
    if b is not None:
        pre, S = pre + np.asarray(b, F64), S + np.abs(np.asarray(b, F64))
    return pre, S


def pooled_shape(shape, pool, same):
    return tuple(-(-s // p) if same else s // p for s, p in zip(shape, pool))


def maxpool(x, pool, same):
    """MaxPooling3D with stride = pool size of [B, X, Y, Z, C]: SAME keeps the partial windows at the far end, VALID drops them"""
    x = np.asarray(x)
    B, C = x.shape[0], x.shape[-1]
    o = pooled_shape(x.shape[1:4], pool, same)
    full = [oo * p for oo, p in zip(o, pool)]
    if same:
        x = np.pad(x, [(0, 0)] + [(0, f - s) for f, s in zip(full, x.shape[1:4])] + [(0, 0)], constant_values=-np.inf)
    else:
        x = x[:, :full[0], :full[1], :full[2]]
    return x.reshape(B, o[0], pool[0], o[1], pool[1], o[2], pool[2], C).max((2, 4, 6))


def upsample_concat(skip, lo, up):
    """concat(skip, nearest up-sampling of lo [B, X/ux, Y/uy, Z/uz, c1]); skip None: the up-sampling alone"""
    lo = np.asarray(lo)
    for d, u in enumerate(up):
        lo = np.repeat(lo, u, axis=1 + d)
    return lo if skip is None else np.concatenate([np.asarray(skip), lo], -1)


def act64(v, act):
    if act == 'sigmoid':
        return 1 / (1 + np.exp(-v))
    return activate(v, act)


def add_act_affine(a, b=None, scale=None, shift=None, act=None, mul=False):
    """act(a + b) * scale + shift, or act(a) * b [* scale + shift] with mul; the channel is the last axis"""
    u = np.asarray(a, F64)
    if mul:
        u = act64(u, act) * np.asarray(b, F64)
    else:
        if b is not None:
            u = u + np.asarray(b, F64)
        u = act64(u, act)
    if scale is not None:
        u = u * np.asarray(scale, F64) + np.asarray(shift, F64)
    return u


# ------------------------------------------------------------------------------------------------------------------------------
# the host dispatch, restated
# ------------------------------------------------------------------------------------------------------------------------------

LDS_MAX = 160 * 1024
ConvPlan = collections.namedtuple('ConvPlan', 'name nsplit live_last loader CG nchunk last nks lds attr store blocks')
ConvPlan.__doc__ = """name: the kernel instance as tools/arm_coverage.py normalises it (or 'unsupported: ...' / 'invalid: ...');
nsplit: gridDim.z; live_last: the live N-tiles of the last split; loader: 'vec', 'scalar' or 'dense'; CG, nchunk, last: the staged
channel groups per chunk, the chunks and the groups of the last chunk (dense: 1, 1, 1); nks: k-steps in all; lds: dynamic LDS bytes;
attr: the launch goes through hipFuncSetAttribute (more than 64 KB); store: 'pack' (8 bytes a lane) or 'scalar'; blocks: gridDim.x"""
GluePlan = collections.namedtuple('GluePlan', 'name path blocks passes')
GluePlan.__doc__ = """name: the kernel instance; path: what the instance does at run time ('' if nothing to choose); blocks: gridDim.x;
passes: the grid-stride passes of the busiest thread"""


def _cdiv(a, b):
    return -(-a // b)


def _al16(off):
    return off % 16 == 0


def conv_geometry(ksize, cin, cout):
    """(ntap, ntap4, nks, ntt, dense) of conv_bf16.hip"""
    ntap = ksize[0] * ksize[1] * ksize[2]
    ntap4 = (ntap + 3) & ~3
    dense = cin < 8
    nks = _cdiv(ntap * cin, 32) if dense else _cdiv(cin, 8) * (ntap4 // 4)
    return ntap, ntap4, nks, _cdiv(cout, 16), dense


def packed_weight_bytes(ksize, cin, cout):
    _, _, nks, ntt, _ = conv_geometry(ksize, cin, cout)
    return nks * ntt * 64 * 8 * 2


def conv_lds_bytes(ksize, dil, dense, CG, nks, ntap4):
    rows = 1
    for t, k in zip(TILE, ksize):
        rows *= t + (k - 1) * dil
    return rows * (8 if dense else 8 * CG + 8) * 2 + (nks * 32 if dense else ntap4) * 4


def out_shape(shape, ksize, dil, same):
    return tuple(shape) if same else tuple(s - (k - 1) * dil for s, k in zip(shape, ksize))


def plan(cus, shape, batch, c0, cout, c1=0, ksize=(3, 3, 3), dilation=1, same=True, src0_off=0, src1_off=0, out_off=0):
    """nrt_conv3d_bf16.  *_off: the byte offset of the pointer from a 16-byte boundary."""
    cin = c0 + c1
    ntap, ntap4, nks, ntt, dense = conv_geometry(ksize, cin, cout)
    vec = (not dense) and c0 % 8 == 0 and c1 % 8 == 0 and _al16(src0_off) and (c1 == 0 or _al16(src1_off))
    none = (0,) * 11
    if out_off % 8:
        return ConvPlan('invalid: out is not 8-byte aligned', *none)
    CG = 0
    for cg in (4, 2, 1):
        if conv_lds_bytes(ksize, dilation, dense, cg, nks, ntap4) <= LDS_MAX:
            CG = cg
            break
    if not CG:
        return ConvPlan('unsupported: no halo tile fits the LDS', *none)
    if dense:
        CG = 1
    out = out_shape(shape, ksize, dilation, same)
    tiles = batch * tiles_per_entry(out)
    NT = min(ntt, 4)
    if tiles < 2 * cus and 1 < ntt <= 4:
        NT = 1
    nsplit = _cdiv(ntt, NT)
    ng = _cdiv(cin, 8)
    nchunk = 1 if dense else _cdiv(ng, CG)
    last = 1 if dense else ng - (nchunk - 1) * CG
    lds = conv_lds_bytes(ksize, dilation, dense, CG, nks, ntap4)
    return ConvPlan('conv3d_bf16<%d>' % NT, nsplit, ntt - (nsplit - 1) * NT, 'dense' if dense else 'vec' if vec else 'scalar', CG, nchunk, last,
                    nks, lds, lds > 64 * 1024, 'pack' if cout % 4 == 0 else 'scalar', NXCD * _cdiv(tiles_per_entry(out), NXCD))


def _grid_for(items, cap):
    return min(max(_cdiv(items, 256), 1), cap)


def _glue(name, path, items, cap):
    blocks = _grid_for(items, cap)
    return GluePlan(name, path, blocks, _cdiv(items, blocks * 256))


def plan_pack(ksize, cin, cout, dtype='float'):
    """nrt_conv3d_pack_weights_bf16; dtype 'float' or 'unsigned short' (bf16 storage)"""
    assert dtype in ('float', 'unsigned short')
    return _glue('conv3d_pack_bf16<%s>' % dtype.replace(' ', ''), '', packed_weight_bytes(ksize, cin, cout) // 2, 4096)


def plan_conv1x1(nvox, cin, cout, x_off=0, y_off=0):
    if cout > 64 or (cin + 1) * cout * 4 > 64 * 1024:
        return GluePlan('unsupported: conv1x1', '', 0, 0)
    vec = cin % 8 == 0 and _al16(x_off) and _al16(y_off)
    path = ('vec,store16' if cout % 8 == 0 else 'vec,store2') if vec else 'scalar'
    return _glue('conv1x1_bf16<%d>' % (16 if cout <= 16 else 32 if cout <= 32 else 64), path, nvox, 4096)


def plan_softmax(n, C, x_off=0, y_off=0):
    return _glue('softmax_lastdim_bf16<%s>' % ('true' if C % 8 == 0 and _al16(x_off) and _al16(y_off) else 'false'), '', n, 4096)


def plan_maxpool(shape, C, pool, same, x_off=0, y_off=0):
    total = int(np.prod(pooled_shape(shape, pool, same))) * C
    v8 = C % 8 == 0 and _al16(x_off) and _al16(y_off)
    return _glue('maxpool3d_bf16<%d>' % (8 if v8 else 1), '', total // 8 if v8 else total, 8192)


def plan_upsample(shape, c0, c1, skip_off=0, lo_off=0, y_off=0):
    total = int(np.prod(shape)) * (c0 + c1)
    v8 = c0 % 8 == 0 and c1 % 8 == 0 and (c0 == 0 or _al16(skip_off)) and _al16(lo_off) and _al16(y_off)
    return _glue('upsample_concat_bf16<%d>' % (8 if v8 else 1), '', total // 8 if v8 else total, 8192)


def plan_add(n, C, has_b, has_scale, a_off=0, b_off=0, y_off=0):
    v8 = n % 8 == 0 and (not has_scale or C % 8 == 0) and _al16(a_off) and (not has_b or _al16(b_off)) and _al16(y_off)
    return _glue('add_act_affine_bf16<%d>' % (8 if v8 else 1), '', n // 8 if v8 else n, 8192)


def plan_id(p):
    """what a pytest id of tests/test_gpu_conv_bf16_arms.py starts with"""
    if isinstance(p, GluePlan):
        return '%s%s b%d p%d' % (p.name, ' ' + p.path if p.path else '', p.blocks, p.passes)
    if not p.name.startswith('conv3d_bf16'):
        return p.name
    stage = 'dense ks%d' % p.nks if p.loader == 'dense' else '%s cg%d chunks%d last%d' % (p.loader, p.CG, p.nchunk, p.last)
    return '%s z%d live%d %s %s %s-store' % (p.name, p.nsplit, p.live_last, stage, 'lds>64K' if p.attr else 'lds<=64K', p.store)
