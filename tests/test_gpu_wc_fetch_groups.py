"""
The fetch list of the wave-cache gather (csrc/fused_wc.h: wc_item) travels in groups of eight entries: one row load and one 1 KB LDS
store per group.  Only the groups that hold an entry are stored (and, past the fixed groups, loaded), so the kernel can go wrong exactly
where a group is skipped that held an entry, or where a skipped group's stale LDS row is read.  These tests pin every group count.

Before anything is launched a NumPy restatement of the slot hash and the claim rule (M1a - M1c of fused_wc.h; tools/wc_sim.py:
histogram does the same for the bench field) counts the fetch-list length n of every wave and pass of the chosen inputs, and asserts
that every value of ceil(n / 8) from 0 to 8 occurs and that the more-than-16-orphans fallback occurs.  Two rows of one pass that miss
in the same slot are claimed by whichever lane's tag store lands last, which the hardware decides: the restatement is run with the
highest and with the lowest lane winning, and the cap must hold under both.

Forward (two pass states), per input, fill in {None, 0.25}, whole columns and columns cut into x segments: warped volume bit-equal to
the oracle and to the register kernel, Dice within RTOL of the oracle, sums equal to the register kernel's up to the order of the
additions (rtol 2e-5, atol 1e-4: the figures of test_gpu_dice_cce.py::test_fused_wave_cache_kernel), a second call bit-equal to the first.
Three pass states (the stand-alone warp, nrt_interpn_f32 variant 10, and both backward forms): marches of 3 k, 3 k + 1 and 3 k + 2 planes
at (X, 8, 8), X in {18, 19, 20}, with 256 batch entries (the x-march schedule wants 512 patch columns) that cycle through the same
seven fields -- the warp bit-equal to the oracle, d loc of both backward forms bit-equal to the register-pipelined warp_dice_bwd_xm
(NRT_BWD_WC=0), which shares their arithmetic and its order (tests/test_gpu_backward.py compares them the same way).
"""

import functools

import numpy as np
import pytest
import torch

import neurite_amd as ne
from conftest import bits_equal
from neurite_amd import synth
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu
F = np.float32
RTOL = 1e-5
NO_WC, WC = 1 << 30, 1 << 29
XM = 3 | (2 << 4) | (3 << 8) | (1 << 14) | WC                  # x-march, 4 x 8 patches, whole columns
TUNES = (XM, XM | (3 << 16) | (1 << 24) | (1 << 27))           # ... and x cut into three segments, 2 x 2 regions
SHAPES = ((2, (21, 18, 29), (21, 18, 29)), (1, (40, 33, 47), (37, 30, 41)))
FIELDS = ('zero', 'const0.5', 'smooth2', 'smooth4', 'iid0.7', 'iid3', 'incoherent')
XS = (18, 19, 20)
B3 = 256                                                        # 2 x 1 patch columns per entry: 512 columns


def field(name, rng, B, S, So):
    if name == 'zero':
        return np.zeros((B,) + So + (3,), F)
    if name == 'const0.5':
        return np.full((B,) + So + (3,), 0.5, F)
    if name in ('smooth2', 'smooth4'):
        sigma, coarse = (2.0, 4) if name == 'smooth2' else (4.0, max(2, max(So) // 4))
        return np.ascontiguousarray(np.stack([synth.smooth_displacement((11 if name == 'smooth2' else 31) + b, max(So), sigma=sigma, coarse=coarse,
                                                                       device='cpu').numpy()[:So[0], :So[1], :So[2]] for b in range(B)]), F)
    if name == 'iid0.7':
        return rng.normal(0, 0.7, (B,) + So + (3,)).astype(F)
    if name == 'iid3':
        return rng.normal(0, 3.0, (B,) + So + (3,)).astype(F)
    return rng.uniform(-max(S), max(S), (B,) + So + (3,)).astype(F)


# ----------------------------------------------------------------------------------------------------------------------------------
# the restatement: n of every wave and pass
# ----------------------------------------------------------------------------------------------------------------------------------

def fetch_list_lengths(trf, S, highest_lane_wins=True):
    """n per (wave, pass) of a whole-column march over the SHIFT field trf [B, *So, 3] into a source of shape S, and whether the pass
    took the fallback.  A wave owns a 2 x 4 (y, z) sub-patch; lane = 8 g + p: voxel g (z offsets 0, 2, 3, 1 for g & 3), corner p."""
    B, So = trf.shape[0], trf.shape[1:4]
    g, p = np.arange(64) >> 3, np.arange(64) & 7
    dz = np.array([0, 2, 3, 1])[g & 3]
    ys, zs = np.arange(0, So[1], 2), np.arange(0, So[2], 4)
    b_, y_, z_ = [a.ravel() for a in np.meshgrid(np.arange(B), ys, zs, indexing='ij')]
    W = b_.size
    yc = np.minimum(y_[:, None] + (g >> 2)[None], So[1] - 1)
    zc = np.minimum(z_[:, None] + dz[None], So[2] - 1)
    tags = np.full((W, 129), -1, np.int64)                     # row id << 6 | lane; entry 128: where the hits store
    wi = np.repeat(np.arange(W), 64).reshape(W, 64)
    lane = np.broadcast_to(np.arange(64), (W, 64))
    order = slice(None) if highest_lane_wins else (slice(None), slice(None, None, -1))
    ns, fallback = [], []
    for x in range(So[0]):
        d = trf[b_[:, None], x, yc, zc]                        # [W, 64, 3]
        idx = []
        for ax, (q, hi) in enumerate(((F(x), p & 4), (yc.astype(F), p & 2), (zc.astype(F), p & 1))):
            mx = F(S[ax] - 1)
            l0 = np.floor(np.clip((q + d[..., ax]).astype(F), F(0), mx))
            idx.append(np.where(hi != 0, np.minimum(l0 + 1, mx), l0).astype(np.int64))
        ix, iy, iz = idx
        rid = (ix * S[1] + iy) * S[2] + iz
        slot = ((ix & 3) << 5) | ((iy & 3) << 3) | (iz & 7)
        mytag = (rid << 6) | lane
        miss = (tags[wi, slot] >> 6) != rid
        dst = np.where(miss, slot, 128)
        # (a repeated index keeps the last value assigned; flat copies, so that the order is the one written here)
        tags[wi[order].ravel(), dst[order].ravel()] = mytag[order].ravel()
        t2 = tags[wi, slot]
        orphan = (t2 >> 6) != rid
        loader = miss & (t2 == mytag)
        n = (loader | orphan).sum(1)
        fb = orphan.sum(1) > 16
        tags[fb, :128] = -1
        ns.append(np.where(fb, 64, n))
        fallback.append(fb)
    return np.stack(ns, 1), np.stack(fallback, 1)


@functools.lru_cache(maxsize=None)
def forward_case(si, name):
    """inputs and oracle results of one forward case, computed once and shared (never modified)"""
    B, S, So = SHAPES[si]
    rng = np.random.default_rng(4040 + 17 * si + FIELDS.index(name))
    mov = rng.random((B,) + S + (32,)).astype(F)               # (positive maps: no cancellation in the Dice sums)
    fix = rng.random((B,) + So + (32,)).astype(F)
    trf = field(name, rng, B, S, So)
    ref = {}
    for fill in (None, 0.25):
        w = npo.spatial_transformer(mov, trf, fill_value=fill)
        ref[fill] = (w, npo.dice(fix, w, check_input_limits=False))
    return mov, fix, trf, ref


@functools.lru_cache(maxsize=None)
def three_state_case(X):
    """256 entries of (X, 8, 8) cycling through the seven fields"""
    S = (X, 8, 8)
    rng = np.random.default_rng(7070 + X)
    mov = rng.random((B3,) + S + (32,)).astype(F)
    fix = rng.random((B3,) + S + (32,)).astype(F)
    per = -(-B3 // len(FIELDS))
    trf = np.stack([field(name, rng, per, S, S) for name in FIELDS], 1)                    # [per, 7, X, 8, 8, 3]
    trf = np.ascontiguousarray(trf.reshape((-1,) + trf.shape[2:])[:B3])
    return mov, fix, trf


@pytest.fixture(scope='module')
def cap():
    """the coverage cap, on the reference alone, before anything is launched"""
    for highest in (True, False):
        buckets, nofb8, fb = np.zeros(9, np.int64), 0, 0
        for si, (B, S, So) in enumerate(SHAPES):
            for name in FIELDS:
                n, f = fetch_list_lengths(forward_case(si, name)[2], S, highest)
                buckets += np.bincount(-(-n.ravel() // 8), minlength=9)
                fb += int(f.sum())
                nofb8 += int(((n > 56) & ~f).sum())
        print('CAP forward, %s lane wins: passes with ceil(n / 8) = 0 .. 8: %s, fallback passes %d, n > 56 without the fallback %d'
              % ('highest' if highest else 'lowest', buckets.tolist(), fb, nofb8))
        assert (buckets > 0).all() and fb > 0, (highest, buckets.tolist(), fb)
        for X in XS:
            n, f = fetch_list_lengths(three_state_case(X)[2], (X, 8, 8), highest)
            b3 = np.bincount(-(-n.ravel() // 8), minlength=9)
            print('CAP three states X = %d: %s, fallback passes %d' % (X, b3.tolist(), int(f.sum())))
            assert (b3 > 0).all() and f.any(), (highest, X, b3.tolist())
    return True


def G(a, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_() if grad else t


def N(t):
    return t.detach().cpu().numpy()


def assert_kernels(B, S, So, fill, tune):
    """the forced tune does select the wave-cache kernel at this shape, and bit 30 the register kernel: the comparison below is between
    two kernels (the library names the instantiation it launches)"""
    from neurite_amd import _lib
    for store in (0, 1):
        for minmax in (0, 1):
            args = (_lib.ints(So), _lib.ints(S), 32, B, _lib.LOC_SHIFT, int(fill is not None), store, minmax)
            assert _lib.lib().nrt_warp_dice_kernel_name(*args, tune).startswith(b'warp_dice_wc<'), (S, fill, tune, store, minmax)
            assert _lib.lib().nrt_warp_dice_kernel_name(*args, (tune & ~WC) | NO_WC).startswith(b'warp_dice_tile<'), (S, fill, tune, store, minmax)


# ----------------------------------------------------------------------------------------------------------------------------------
# the fused forward: two pass states
# ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', FIELDS)
@pytest.mark.parametrize('si', range(len(SHAPES)), ids=['21x18x29', '40x33x47-37x30x41'])
def test_fused_forward_every_group_count(dev, cap, si, name):
    mov, fix, trf, ref = forward_case(si, name)
    m, t, f = G(mov, dev), G(trf, dev), G(fix, dev)
    for fill in (None, 0.25):
        w_ref, d_ref = ref[fill]
        for tune in TUNES:
            what = str((SHAPES[si][1], name, fill, tune))
            assert_kernels(*SHAPES[si], fill, tune)
            d, w, s = ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, _tune=tune)
            assert bits_equal(N(w), w_ref), what
            np.testing.assert_allclose(N(d), d_ref, rtol=RTOL, err_msg=what)
            d2, w2, s2 = ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, _tune=tune)
            assert bits_equal(N(w2), N(w)) and bits_equal(N(d2), N(d)) and bits_equal(N(s2), N(s)), what
            # the register kernel on the same schedule: same warped bits, same sums up to the order of the additions
            d0, w0, s0 = ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, _tune=(tune & ~WC) | NO_WC)
            assert bits_equal(N(w0), N(w)), what
            np.testing.assert_allclose(N(s0), N(s), rtol=2e-5, atol=1e-4, err_msg=what)


# ----------------------------------------------------------------------------------------------------------------------------------
# three pass states: the stand-alone warp and the backward forms
# ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('X', XS)
def test_fused_forward_short_columns(dev, cap, X):
    """the forward on the three-state inputs: 2 k and 2 k + 1 planes per column, one patch column wide"""
    mov, fix, trf = three_state_case(X)
    m, t, f = G(mov, dev), G(trf, dev), G(fix, dev)
    for fill in (None, 0.25):
        w_ref = npo.spatial_transformer(mov, trf, fill_value=fill)
        for tune in TUNES:
            assert_kernels(B3, (X, 8, 8), (X, 8, 8), fill, tune)
            d, w, s = ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, _tune=tune)
            assert bits_equal(N(w), w_ref), (X, fill, tune)
            d0, w0, s0 = ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, _tune=(tune & ~WC) | NO_WC)
            assert bits_equal(N(w0), N(w)), (X, fill, tune)
            np.testing.assert_allclose(N(s0), N(s), rtol=2e-5, atol=1e-4, err_msg=str((X, fill, tune)))


@pytest.mark.parametrize('X', XS)
def test_standalone_warp_every_group_count(dev, cap, X):
    mov, _, trf = three_state_case(X)
    m, t = G(mov, dev), G(trf, dev)
    for fill in (None, 0.25):
        st = ne.layers.SpatialTransformer(fill_value=fill)
        st._variant = 10
        got = N(st([m, t]))
        assert bits_equal(got, npo.spatial_transformer(mov, trf, fill_value=fill)), (X, fill)
        assert bits_equal(N(st([m, t])), got), (X, fill)


@pytest.mark.parametrize('X', XS)
def test_backward_forms_every_group_count(dev, cap, X, monkeypatch):
    mov, fix, trf = three_state_case(X)
    rng = np.random.default_rng(9090 + X)
    wgt = rng.standard_normal(mov.shape).astype(F)
    m, f, w = G(mov, dev), G(fix, dev), G(wgt, dev)
    for fill in (None, 0.25):
        got = {}
        for wc in ('1', '0'):
            monkeypatch.setenv('NRT_BWD_WC', wc)
            t1 = G(trf, dev, True)
            (-ne.fused.warp_dice(m, t1, f, fill_value=fill, laplace_smoothing=0.05).mean()).backward()
            t2 = G(trf, dev, True)
            (ne.layers.SpatialTransformer(fill_value=fill)([m, t2]) * w).sum().backward()
            got[wc] = (N(t1.grad), N(t2.grad))
        assert np.isfinite(got['1'][0]).all() and np.abs(got['1'][0]).max() > 0 and np.abs(got['1'][1]).max() > 0
        assert bits_equal(got['1'][0], got['0'][0]), 'fused, X %d fill %r: %g' % (X, fill, np.abs(got['1'][0] - got['0'][0]).max())
        assert bits_equal(got['1'][1], got['0'][1]), 'plain, X %d fill %r: %g' % (X, fill, np.abs(got['1'][1] - got['0'][1]).max())
