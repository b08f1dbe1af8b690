"""
TEST INFRASTRUCTURE ONLY -- float64 reference of the convolution forward entry points (neurite_amd/csrc/conv.hip, conv_p27.h,
conv_up2.h: nrt_conv3d_f32, nrt_conv3d_pad_f32, nrt_hyperconv3d_f32, nrt_hyperconv3d_pad_f32, nrt_conv3d_pool_f32, nrt_conv3d_up2_f32,
nrt_conv3d_s2d_taps_f32, nrt_space_to_depth2_f32), and a restatement of their host dispatch (CPU, numpy float64, no GPU import).

`conv` is the formula of include/neurite_amd.h, one tap at a time over the whole zero-padded volume; nothing of the kernels' 4 x 4 x 16
voxel tiles, 16-channel chunks, N split or persistent schedules is in it:

    pre[b, v, co] = bias[co] + sum_{t, ci} xin[b, v + t dil - pad, ci] W[t, ci, co]           (zero outside the volume)
    xin           = concat(x, repeat(x_lo, up)) when a second source is given
    pad           = floor((k - 1) dil / 2) ('same'), 0 ('valid': the output shrinks by (k - 1) dil), or `pad_before` (output = input shape)
    per entry     : W [B, ...], bias [B, cout]
    out           = act(pre), act in none / elu / relu

It returns the pre-activation value, the sum of the absolute terms S = |bias| + sum |xin| |W| of every output (the S of close_conv in
tests/test_gpu_unet.py) and the activated value.  `bound` is that test's element-wise criterion, 8 x 2^-24 x S (+ 3e-6 with ELU, the
hardware exponential of the epilogue); nothing in it is tuned on the kernels.

With x, x_lo, W and bias drawn from the integers -3 .. 3 and 9 taps (c0 + c1) + 3 < 2^24 (`exact_condition`) every product, every
partial sum in any order, the pre-summed taps of the folded decoder kernel and the result of v_mfma_f32_16x16x4_f32 are integers that
float32 holds exactly, so a float32 output must equal this reference BIT FOR BIT (check_exact of oracle/conv_wgrad_oracle.py), with
activation none and relu.

`plan` restates which kernel instance the host code launches for a call, with which grid; `cus` (the device's compute units) is an
argument.  tests/test_conv_fwd_oracle.py checks the case table of tests/test_gpu_conv_fwd_arms.py against it and against the instances
the compiler emitted; a kernel trace of that file confirms it on the device (profiles/dispatch_arms/README.md).

Only tests/ may import this module.
"""

import collections

import numpy as np

from oracle.conv_wgrad_oracle import F, F64, U, check_exact, integers, layer_input, ratio, space_to_depth2      # noqa: F401 (re-exported)
from oracle.conv_wgrad_oracle import pad_before as same_pad_before


# ------------------------------------------------------------------------------------------------------------------------------
# the operations
# ------------------------------------------------------------------------------------------------------------------------------

def activate(v, act):
    if act == 'elu':
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    if act == 'relu':
        return np.maximum(v, 0)
    assert act is None, act
    return v


def _geometry(S, k, dilation, padding, pad_before):
    """(padding before, output shape, padding after) per axis"""
    ext = [(kk - 1) * dilation for kk in k]
    if pad_before is not None:
        pb, out = [int(p) for p in pad_before], list(S)
        assert all(0 <= p <= e for p, e in zip(pb, ext))
    elif padding == 'same':
        pb, out = [same_pad_before(kk, dilation) for kk in k], list(S)
    else:
        assert padding == 'valid', padding
        pb, out = [0, 0, 0], [s - e for s, e in zip(S, ext)]
        assert min(out) >= 1
    return pb, out, [o + e - p - s for o, e, p, s in zip(out, ext, pb, S)]


def _add_tap(acc, xp, wt, offs, out, chans, per_entry):
    """acc[b, v, :] += xp[b, v + offs, chans] @ wt[chans, :]   (wt [cin, cout], or [B, cin, cout] per entry)"""
    B = xp.shape[0]
    s = xp[:, offs[0]:offs[0] + out[0], offs[1]:offs[1] + out[1], offs[2]:offs[2] + out[2], chans]
    ci = s.shape[-1]
    if per_entry:
        acc += np.matmul(s.reshape(B, -1, ci), wt[:, chans, :]).reshape(acc.shape)
    else:
        acc += (s.reshape(-1, ci) @ wt[chans, :]).reshape(acc.shape)


def conv(x, w, b, dilation=1, padding='same', x_lo=None, up=None, pad_before=None, per_entry=False, act=None, with_abs=True, taps=None):
    """x [B, X, Y, Z, c0] (+ x_lo [B, X/ux, Y/uy, Z/uz, c1], up), w [kx, ky, kz, c0 + c1, cout] and b [cout] or None (a leading B axis on
    both with per_entry) -> (ref_pre, abs_sum, ref), float64 [B, OX, OY, OZ, cout]; abs_sum is None without with_abs.
    taps: {(tx, ty, tz): channel slice} -- only these taps and channels are read (s2d_taps); None: all of them."""
    xin = layer_input(x, x_lo, up)
    w = np.asarray(w, F64)
    B, S, cin = xin.shape[0], xin.shape[1:4], xin.shape[-1]
    k, cout = w.shape[-5:-2], w.shape[-1]
    assert w.shape == ((B,) if per_entry else ()) + tuple(k) + (cin, cout), (w.shape, xin.shape)
    pb, out, pa = _geometry(S, k, dilation, padding, pad_before)
    xp = np.pad(xin, [(0, 0)] + list(zip(pb, pa)) + [(0, 0)])
    pre = np.zeros((B,) + tuple(out) + (cout,), F64)
    S_abs = np.zeros_like(pre) if with_abs else None
    xa, wa = (np.abs(xp), np.abs(w)) if with_abs else (None, None)
    for tx in range(k[0]):
        for ty in range(k[1]):
            for tz in range(k[2]):
                todo = [slice(None)] if taps is None else taps.get((tx, ty, tz), [])
                offs = (tx * dilation, ty * dilation, tz * dilation)
                for chans in todo:
                    _add_tap(pre, xp, w[..., tx, ty, tz, :, :], offs, out, chans, per_entry)
                    if with_abs:
                        _add_tap(S_abs, xa, wa[..., tx, ty, tz, :, :], offs, out, chans, per_entry)
    if b is not None:
        bb = np.asarray(b, F64)
        assert bb.shape == ((B, cout) if per_entry else (cout,)), bb.shape
        bb = bb.reshape(B, 1, 1, 1, cout) if per_entry else bb
        pre += bb
        if with_abs:
            S_abs += np.abs(bb)
    return pre, S_abs, activate(pre, act)


def s2d_taps(x, w, group, with_abs=True):
    """nrt_conv3d_s2d_taps_f32: the 3x3x3 'same' convolution of x [B, X, Y, Z, 8 group] with w [3, 3, 3, 8 group, cout] in which the
    channels of parity group P = (px 2 + py) 2 + pz only use the taps e = (p ? 1 : 2) - t, t in {0, 1}, per axis; every other weight
    is treated as zero, whatever w holds there.  No bias, no activation."""
    assert np.asarray(x).shape[-1] == 8 * group and np.asarray(w).shape[:4] == (3, 3, 3, 8 * group)
    taps = collections.defaultdict(list)
    for P in range(8):
        p = ((P >> 2) & 1, (P >> 1) & 1, P & 1)
        for t in range(8):
            e = tuple((1 if p[d] else 2) - ((t >> (2 - d)) & 1) for d in range(3))
            taps[e].append(slice(P * group, (P + 1) * group))
    return conv(x, w, None, with_abs=with_abs, taps=taps)


def maxpool2(y):
    """MaxPooling3D(2) of [B, X, Y, Z, C] with even X, Y, Z"""
    B, X, Y, Z, C = y.shape
    return y.reshape(B, X // 2, 2, Y // 2, 2, Z // 2, 2, C).max((2, 4, 6))


def bound(abs_sum, act=None, ulps=8.0):
    """close_conv of tests/test_gpu_unet.py: ulps x 2^-24 x S element-wise; elu adds the 3e-6 of the epilogue's hardware exponential"""
    return ulps * U * np.asarray(abs_sum, F64) + (3e-6 if act == 'elu' else 0.0)


def exact_condition(taps, cin, amax=3):
    """integers of magnitude <= amax: |bias| + every partial sum of the taps x cin products stays below 2^24"""
    assert amax * amax * taps * cin + amax < 2 ** 24, 'integer sums may leave the exact range of float32'


# ------------------------------------------------------------------------------------------------------------------------------
# the host dispatch, restated
# ------------------------------------------------------------------------------------------------------------------------------

NXCD = 8
TILE = (4, 4, 16)
Plan = collections.namedtuple('Plan', 'name blocks grid_z tiles_per_block path')
Plan.__doc__ = """name: the kernel instance as tools/arm_coverage.py normalises it (or 'not conv_fwd: ...' / 'unsupported: ...');
blocks: gridDim.x; grid_z: gridDim.z; tiles_per_block: the most tiles (direct kernel: grid-stride passes) one block walks;
path: the inner path of the generic conv3d_mfma instance ('prefetch' or 'no-prefetch,lds>64K'), else ''"""


def plan_id(p):
    """what a pytest id of tests/test_gpu_conv_fwd_arms.py starts with"""
    return '%s z%d t%d%s' % (p.name, p.grid_z, p.tiles_per_block, ' ' + p.path if p.path else '')


def _cdiv(a, b):
    return -(-a // b)


def tiles_per_entry(out):
    return _cdiv(out[0], TILE[0]) * _cdiv(out[1], TILE[1]) * _cdiv(out[2], TILE[2])


def _pow2(v):
    return v & (v - 1) == 0


def _b(v):
    return 'true' if v else 'false'


def _persistent(name, ntiles, per_xcd):
    """launch_p27 / launch_up2: XCD k owns the k-th share of T8 tiles, its J blocks walk it with stride J"""
    T8 = _cdiv(ntiles, NXCD)
    J = min(T8, per_xcd)
    return Plan(name, NXCD * J, 1, _cdiv(T8, J), '')


def _direct(hyper, out):
    nvox = out[0] * out[1] * out[2]
    blocks = min(_cdiv(nvox, 256), 256 * 32)
    return Plan('conv3d_direct<%s>' % _b(hyper), blocks, 1, _cdiv(nvox, blocks * 256), '')


def plan(entry, cus, shape, batch, c0, cout, c1=0, up=None, ksize=(3, 3, 3), dilation=1, same=True, pad_before=None, variant=0,
         group=0, packed=True, weights=True):
    """entry: 'conv3d' (nrt_conv3d_f32), 'conv3d_pad', 'hyperconv3d', 'hyperconv3d_pad', 'pool' (nrt_conv3d_pool_f32), 'up2'
    (nrt_conv3d_up2_f32) or 's2d_taps' (c0 is 8 group there).  packed / weights: whether the call passes packed_weights / weights.
    Every pointer is taken as 16-byte aligned."""
    assert entry in ('conv3d', 'conv3d_pad', 'hyperconv3d', 'hyperconv3d_pad', 'pool', 'up2', 's2d_taps'), entry
    hyper = entry.startswith('hyperconv3d')
    k, dil = tuple(ksize), dilation
    if entry in ('pool', 'up2', 's2d_taps', 'conv3d_pad', 'hyperconv3d_pad'):
        same = True
    if entry == 'up2':
        up = (2, 2, 2)
    if entry == 's2d_taps':
        assert group >= 16 and group % 16 == 0 and c0 == 8 * group and c1 == 0
    ux, uy, uz = up if c1 else (1, 1, 1)
    X, Y, Z = shape
    cin = c0 + c1
    # conv_args
    if same:
        p = [same_pad_before(kk, dil) for kk in k]
        out = (X, Y, Z)
    else:
        p = [0, 0, 0]
        out = tuple(s - (kk - 1) * dil for s, kk in zip(shape, k))
    tiles = batch * tiles_per_entry(out)

    def mfma_ok():
        return (same and all(kk in (1, 3) for kk in k) and dil <= 2 and cout <= 64 and cin >= 8 and not (c1 > 0 and c0 % 4))

    def k2_ok():
        return (k == (2, 2, 2) and dil == 1 and out == (X, Y, Z) and cout <= 64 and cin >= 8 and not (c1 > 0 and c0 % 4) and not group)

    def k2_auto():
        return cin >= 16 and cout >= 16 and batch * out[0] * out[1] * out[2] >= 4 * 40 * 40 * 40

    def launch_k2():
        return Plan('conv3d_mfma_k2<%d>' % min(_cdiv(cout, 16), 4), NXCD * _cdiv(tiles_per_entry(out), NXCD), 1, 1, '')

    def p27_ok():
        return (same and k == (3, 3, 3) and dil == 1 and c1 == 0 and c0 >= 16 and c0 % 16 == 0 and cout <= 64 and not group and
                X * Y * Z * c0 < 2 ** 30 and batch * X * Y * Z * cout < 2 ** 30)

    def launch_p27(pool):
        return _persistent('conv3d_p27_mfma<%d,%s,%s>' % (min(_cdiv(cout, 16), 4), _b(pool), _b(hyper)), tiles, cus // NXCD)

    def dispatch_mfma():
        ntt = _cdiv(cout, 16)
        want, split = 2 * cus, 1
        if ntt > 1 and tiles < want:
            split = (2 if tiles * 2 >= want else 4) if ntt == 4 else ntt
        nt = ntt // split if ntt // split in (1, 2, 3) else 4
        # launch_mfma
        pow2 = c1 == 0 or (_pow2(ux) and _pow2(uy) and _pow2(uz))
        fast = (k == (3, 3, 3) and dil == 1 and c0 % 4 == 0 and c1 % 4 == 0 and pow2 and X * Y * Z * c0 < 2 ** 31 and
                Y * Z * max(c0, c1) < 2 ** 24)
        if group:
            if not fast or c1 or group % 16 or hyper:
                return Plan('unsupported: fold', 0, 0, 0, '')
            name, path = 'conv3d_mfma<%d,true,true,false>' % nt, ''
        elif fast:
            name, path = 'conv3d_mfma<%d,true,false,%s>' % (nt, _b(hyper)), ''
        else:
            h = [dil if kk > 1 else 0 for kk in k]
            nrows = (4 + 2 * h[0]) * (4 + 2 * h[1]) * (16 + 2 * h[2])
            path = ('prefetch' if nrows <= 64 * 11 else 'no-prefetch') + (',lds>64K' if nrows * 20 * 4 > 64 * 1024 else '')
            name = 'conv3d_mfma<%d,false,false,%s>' % (nt, _b(hyper))
        return Plan(name, NXCD * _cdiv(tiles_per_entry(out), NXCD), split, 1, path)

    def conv3d_dispatch(variant):
        if variant == 6 or (variant == 0 and not hyper and packed and k2_ok() and k2_auto()):
            if hyper or not packed or not k2_ok():
                return Plan('unsupported: variant 6', 0, 0, 0, '')
            return launch_k2()
        can_mfma = mfma_ok() and packed
        wstride = 0
        if hyper:
            wstride = _cdiv(c0, 16) * k[0] * k[1] * k[2] * _cdiv(cout, 16) * 256
        can_p27 = can_mfma and p27_ok() and (not hyper or batch * wstride * 4 < 2 ** 31)
        if variant == 0 and can_p27 and tiles >= 2 * cus:
            variant = 5
        if variant == 5:
            return launch_p27(False) if can_p27 else Plan('unsupported: variant 5', 0, 0, 0, '')
        if variant == 0:
            variant = 2 if can_mfma else 1
        if variant == 2:
            return dispatch_mfma() if can_mfma else Plan('unsupported: variant 2', 0, 0, 0, '')
        if variant not in (1, 3) or not weights:
            return Plan('unsupported: variant %d' % variant, 0, 0, 0, '')
        c1_ok = c0 == 1 and c1 == 0 and same and cout % 4 == 0 and cout // 4 in (1, 2, 4, 8, 16)
        if variant == 3 and not c1_ok:
            return Plan('unsupported: variant 3', 0, 0, 0, '')
        if variant == 1 and c0 == 1 and c1 == 0 and same and k == (3, 3, 3) and dil == 1 and cout % 16 == 0 and cout <= 64:
            return Plan('not conv_fwd: conv3d_c1_mfma', 0, 0, 0, '')
        if c1_ok:
            return Plan('not conv_fwd: conv3d_c1_vec', 0, 0, 0, '')
        return _direct(hyper, out)

    if entry == 's2d_taps':
        return dispatch_mfma() if mfma_ok() else Plan('unsupported: s2d_taps', 0, 0, 0, '')
    if entry == 'up2':
        ok = (c1 >= 16 and c0 >= 16 and c0 % 16 == 0 and c1 % 16 == 0 and cin // 16 <= 32 and cout <= 64 and X * Y * Z * c0 < 2 ** 30 and
              X * Y * Z * cout < 2 ** 30 and batch * X * Y * Z * cout < 2 ** 30)
        return _persistent('conv3d_up2_mfma<%d,0>' % min(_cdiv(cout, 16), 4), tiles, 2 * cus // NXCD) if ok else Plan('unsupported: up2', 0, 0, 0, '')
    if entry == 'pool':
        ok = mfma_ok() and p27_ok() and cout >= 32 and cout % 16 == 0 and X % 4 == 0 and Y % 4 == 0 and Z % 16 == 0
        return launch_p27(True) if ok else Plan('unsupported: pool', 0, 0, 0, '')
    if entry in ('conv3d_pad', 'hyperconv3d_pad'):
        # conv_pad_before
        pb = tuple(pad_before)
        assert all(0 <= q <= (kk - 1) * dil for q, kk in zip(pb, k))
        if list(pb) == p:
            return conv3d_dispatch(variant)
        if not hyper and (variant == 6 or (variant == 0 and packed and k2_ok() and k2_auto())):
            return launch_k2() if packed and k2_ok() else Plan('unsupported: variant 6', 0, 0, 0, '')
        if variant not in (0, 1) or not weights:
            return Plan('unsupported: variant %d with pad_before' % variant, 0, 0, 0, '')
        return _direct(hyper, out)
    assert pad_before is None
    return conv3d_dispatch(variant)


def batch_for(rule, cus, per_entry_tiles):
    """the batch size of a large-grid case from the CU count.  'unsplit': tiles >= 2 CUs, where dispatch_mfma stops splitting (and
    variant 0 turns persistent); 'split2': CUs <= tiles < 2 CUs, the split-by-2 of cout 49 .. 64; 'p27': 2.5 tiles per block of the
    CUs-block persistent grid; 'pool': the tile count of 'p27' on its (9, 9, 33) volume of 27 tiles, in whole-tile entries, and one entry more; 'up2': the same
    for the 2 CUs-block grid of conv3d_up2_mfma.  An integer is itself."""
    if isinstance(rule, int):
        return rule
    if rule == 'pool':
        return _cdiv(27 * _cdiv((5 * cus + 1) // 2, 27), per_entry_tiles) + 1
    n = {'unsplit': 2 * cus, 'split2': cus, 'p27': (5 * cus + 1) // 2, 'up2': 5 * cus}[rule]
    return _cdiv(n, per_entry_tiles)
