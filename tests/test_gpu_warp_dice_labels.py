"""
ne.fused.warp_dice_labels (csrc/warp_labels.hip): SpatialTransformer('linear') + soft Dice on the one-hot maps of two integer label
maps, without the one-hot maps, and its backward wrt the field.  The one-hot references are built on the host as
(lab[..., None] == arange(L)), so ids outside [0, L) give zero rows.  Helpers and tolerances are those of
tests/test_gpu_fused_label_counts.py: warped bit-identical, sums 1e-6, dice 1e-5 against the numpy oracle, dice 1e-6 against the HIP
pipelines on the one-hot tensors, gradients 1e-4 of their scale against the float64 oracle.  sum t^2 is a voxel count: exact.
"""

import numpy as np
import pytest
import torch

import neurite_amd as ne
from conftest import bits_equal
from neurite_amd import synth
from oracle import c_oracle as co
from oracle import grad_oracle as go
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu
F = np.float32
RTOL = 1e-5
TOL = 1e-4


def G(a, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_() if grad else t


def N(t):
    return t.detach().cpu().numpy()


def D64(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).double()
    return t.requires_grad_() if grad else t


def close(got, want, what=''):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max()) / scale
    assert got.shape == want.shape and err < TOL, '%s: max err / scale = %.3g' % (what, err)


def eager(fn):
    with ne.deferred.scope(False):
        return fn()


def one_hot(lab, L):
    return (np.asarray(lab)[..., None] == np.arange(L)).astype(F)


def _shift_oracle(vol, shift, fill=None):
    """float32 location (grid + shift, one rounding) like the kernel, then float64 interpolation"""
    O = shift.shape[:-1]
    grid = np.stack(np.meshgrid(*[np.arange(s, dtype=F) for s in O], indexing='ij'), -1)
    lo = D64((grid + shift).astype(F), True)
    return go.interpn(D64(vol, True), lo, fill), lo


def _unfused_dice(mov, trf, fix, **kw):
    st_kw = {k: kw[k] for k in ('fill_value', 'single_transform', 'indexing') if k in kw}
    w = eager(lambda: ne.layers.SpatialTransformer(**st_kw)([mov, trf]))
    return w, ne.metrics.Dice(check_input_limits=False, laplace_smoothing=kw.get('laplace_smoothing', 0.)).dice(fix, w)


def check_forward(dev, mov, fix, trf, L, fills=(None, 0.0), epss=(0.25, 0.0)):
    """every forward assertion of this file for one (moving ids, fixed ids, field); returns {(fill, eps): dice}"""
    M, Fx = one_hot(mov, L), one_hot(fix, L)
    m, f, t = G(mov.astype(np.int32), dev), G(fix.astype(np.int32), dev), G(trf, dev)
    counts = Fx.reshape(Fx.shape[0], -1, L).sum(1, dtype=np.float64).astype(F)
    out = {}
    for fill in fills:
        w_ref = npo.spatial_transformer(M, trf, fill_value=fill)
        sums_ref = np.stack(npo.dice_sums(Fx, w_ref), 1)
        for eps in epss:
            d, w, s = ne.fused.warp_dice_labels(m, t, f, L, fill_value=fill, laplace_smoothing=eps, return_warped=True, return_sums=True)
            assert bits_equal(N(w), w_ref), (L, fill, eps)
            assert bits_equal(N(s)[:, 1], counts), (L, fill, eps)
            np.testing.assert_allclose(N(s), sums_ref, rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(N(d), npo.dice(Fx, w_ref, laplace_smoothing=eps, check_input_limits=False), rtol=RTOL)
            d2, s2 = ne.fused.warp_dice_labels(m, t, f, L, fill_value=fill, laplace_smoothing=eps, return_sums=True)
            assert bits_equal(N(d2), N(d)) and bits_equal(N(s2), N(s)), (L, fill, eps)       # with / without writing `warped`
            out[(fill, eps)] = N(d)
    return out


@pytest.mark.parametrize('L', [1, 2, 5, 32, 33, 100, 256])
def test_forward_against_oracle(dev, L):
    """i.i.d. ids from [-1, L + 1]: up to 8 distinct labels per voxel, many per wave, out-of-range ids on both sides"""
    rng = np.random.default_rng(300 + L)
    shapes = ((2, (19, 14, 27), (19, 14, 27)), (1, (9, 8, 12), (7, 11, 5)))
    if L > 64:
        shapes = ((2, (9, 7, 11), (9, 7, 11)), (1, (6, 8, 5), (7, 5, 9)))
    for B, S, So in shapes:
        mov = rng.integers(-1, L + 2, (B,) + S)
        fix = rng.integers(-1, L + 2, (B,) + So)
        trf = rng.normal(0, 2.5, (B,) + So + (3,)).astype(F)
        check_forward(dev, mov, fix, trf, L)
        M, Fx = one_hot(mov, L), one_hot(fix, L)
        m, f, t = G(mov.astype(np.int32), dev), G(fix.astype(np.int32), dev), G(trf, dev)
        if L == 32:                                     # the fused kernel on the one-hot tensors
            for fill in (None, 0.0):
                d = ne.fused.warp_dice_labels(m, t, f, L, fill_value=fill, laplace_smoothing=0.25)
                d_oh = ne.fused.warp_dice(G(M, dev), t, G(Fx, dev), fill_value=fill, laplace_smoothing=0.25)
                np.testing.assert_allclose(N(d), N(d_oh), rtol=1e-6)
        # a single transform and cartesian indexing, against the unfused pipeline on the one-hot tensors
        for kw in ({'single_transform': True}, {'indexing': 'xy'}, {'single_transform': True, 'indexing': 'xy'}):
            tt = t[:1] if kw.get('single_transform') else t
            d, w = ne.fused.warp_dice_labels(m, tt, f, L, return_warped=True, **kw)
            w_hip, d_hip = _unfused_dice(G(M, dev), tt, G(Fx, dev), **kw)
            w_ref = npo.spatial_transformer(M, N(tt), indexing=kw.get('indexing', 'ij'), single_transform=kw.get('single_transform', False))
            assert bits_equal(N(w), w_ref) and bits_equal(N(w_hip), w_ref), (L, kw)
            np.testing.assert_allclose(N(d), N(d_hip), rtol=1e-6)


def test_blob_labels(dev):
    """synth.blob_labels: structures with an interior (eight equal corners), several ids per wave at their borders"""
    rng = np.random.default_rng(41)
    L, size = 5, 22
    mov = np.stack([N(synth.blob_labels(s, size, L, coarse=3)) for s in (1, 2)])
    fix = np.stack([N(synth.blob_labels(s, size, L, coarse=3)) for s in (3, 4)])
    trf = rng.normal(0, 2.5, (2, size, size, size, 3)).astype(F)
    check_forward(dev, mov, fix, trf, L)
    trf = np.stack([N(synth.smooth_displacement(s, size, coarse=4)) for s in (5, 6)])
    check_forward(dev, mov, fix, trf, L, fills=(0.0,), epss=(0.0,))


def test_slabs_and_constant_volume(dev):
    """whole waves of one id (the accumulators that stay in registers), the id changing between steps, an out-of-range slab, and
    one constant volume"""
    rng = np.random.default_rng(42)
    L, S = 6, (19, 14, 27)
    mov = np.zeros((2,) + S, np.int64)
    mov[0, :6], mov[0, 6:11], mov[0, 11:15], mov[0, 15:] = 3, 1, L + 1, 3
    mov[0, 8, 5, 9] = 4                                           # one voxel of another id inside a slab
    mov[1] = 2                                                    # constant
    fix = np.zeros((2,) + S, np.int64)
    fix[0, :, :7], fix[0, :, 7:] = 3, 1
    fix[1] = rng.integers(0, L, S)
    for sigma in (0.4, 2.5):
        trf = rng.normal(0, sigma, (2,) + S + (3,)).astype(F)
        check_forward(dev, mov, fix, trf, L)
    # zero flow: integer locations, every p is exactly 0 or 1
    d = check_forward(dev, mov, mov, np.zeros((2,) + S + (3,), F), L, fills=(None,), epss=(0.0,))[(None, 0.0)]
    assert np.array_equal(d[0], np.array([0, 1, 0, 1, 1, 0], F)) and np.array_equal(d[1], np.array([0, 0, 1, 0, 0, 0], F))


@pytest.mark.parametrize('S,So', [((9, 8, 1), (7, 6, 3)), ((6, 7, 2), (5, 9, 4)), ((1, 1, 5), (3, 2, 6)), ((1, 1, 1), (2, 2, 2))])
def test_thin_volumes(dev, S, So):
    """extents of 1 and 2: the z-neighbours of a row are fetched as a pair where the volume has two of them, one by one where not"""
    rng = np.random.default_rng(46)
    L = 4
    mov = rng.integers(-1, L + 1, (2,) + S)
    fix = rng.integers(-1, L + 1, (2,) + So)
    trf = rng.normal(0, 1.5, (2,) + So + (3,)).astype(F)
    check_forward(dev, mov, fix, trf, L, epss=(0.25,))
    f = G(trf, dev, True)
    ne.fused.warp_dice_labels(G(mov.astype(np.int32), dev), f, G(fix.astype(np.int32), dev), L, laplace_smoothing=0.25).sum().backward()
    f2 = G(trf, dev, True)
    warped = ne.layers.SpatialTransformer()([G(one_hot(mov, L), dev), f2])
    ne.metrics.Dice(check_input_limits=False, laplace_smoothing=0.25).dice(G(one_hot(fix, L), dev), warped).sum().backward()
    close(N(f.grad), N(f2.grad), 'thin volume')


def test_empty_labels(dev):
    """ids from [0, L - 3): the last labels are empty, dice = 0 at eps = 0 and 1 at eps > 0"""
    rng = np.random.default_rng(43)
    L, S = 8, (9, 8, 12)
    mov = rng.integers(0, L - 3, (2,) + S)
    fix = rng.integers(0, L - 3, (2,) + S)
    trf = rng.normal(0, 2.5, (2,) + S + (3,)).astype(F)
    out = check_forward(dev, mov, fix, trf, L)
    for fill in (None, 0.0):
        assert np.all(out[(fill, 0.0)][:, L - 3:] == 0.0) and np.all(out[(fill, 0.25)][:, L - 3:] == 1.0)
        assert np.all(out[(fill, 0.0)][:, :L - 3] > 0.0)


def test_integer_dtypes_and_trailing_axis(dev):
    rng = np.random.default_rng(44)
    L, S = 7, (9, 8, 12)
    mov = rng.integers(0, L + 2, (2,) + S)
    fix = rng.integers(0, L + 2, (2,) + S)
    t = G(rng.normal(0, 2.5, (2,) + S + (3,)).astype(F), dev)
    ref = None
    for dt in (torch.int32, torch.uint8, torch.int16, torch.int64):
        m, f = G(mov, dev).to(dt), G(fix, dev).to(dt)
        for mm, ff in ((m, f), (m.unsqueeze(-1), f.unsqueeze(-1))):
            got = [N(x) for x in ne.fused.warp_dice_labels(mm, t, ff, L, laplace_smoothing=0.1, return_warped=True, return_sums=True)]
            ref = ref or got
            assert all(bits_equal(a, b) for a, b in zip(got, ref)), dt
    # an int64 id beyond int32 is out of range, not wrapped into [0, L)
    big = G(mov, dev).clone()
    big[G(mov == L + 1, dev)] = (1 << 32) + 1
    got = [N(x) for x in ne.fused.warp_dice_labels(big, t, G(fix, dev), L, laplace_smoothing=0.1, return_warped=True, return_sums=True)]
    assert all(bits_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize('L,fill,eps', [(5, None, 0.), (32, 0.0, 0.1), (33, None, 0.)])
def test_backward(dev, L, fill, eps):
    """backward == ne.fused.warp_dice's / SpatialTransformer -> Dice's on the one-hot tensors == float64 oracle; deterministic"""
    rng = np.random.default_rng(23 + L)
    B, S = 2, (14, 12, 10)
    mov_l = rng.integers(-1, L + 1, (B,) + S)
    fix_l = rng.integers(-1, L + 1, (B,) + S)
    mov, fix = one_hot(mov_l, L), one_hot(fix_l, L)
    m, fx = G(mov_l.astype(np.int32), dev), G(fix_l.astype(np.int32), dev)
    flow = (rng.standard_normal((B,) + S + (3,)) * 2.0).astype(F)
    flow[1, :2] = 0
    wl = rng.uniform(0.5, 1.5, (B, L)).astype(F)
    grads = []
    for _ in range(2):
        f = G(flow, dev, True)
        d = ne.fused.warp_dice_labels(m, f, fx, L, fill_value=fill, laplace_smoothing=eps)
        (-(d * G(wl, dev)).mean()).backward()
        grads.append(N(f.grad))
    assert bits_equal(grads[0], grads[1])
    f2 = G(flow, dev, True)
    if L == 32:
        d2 = ne.fused.warp_dice(G(mov, dev), f2, G(fix, dev), fill_value=fill, laplace_smoothing=eps)
    else:
        warped = ne.layers.SpatialTransformer(fill_value=fill)([G(mov, dev), f2])
        d2 = ne.metrics.Dice(check_input_limits=False, laplace_smoothing=eps).dice(G(fix, dev), warped)
    (-(d2 * G(wl, dev)).mean()).backward()
    close(grads[0], N(f2.grad), 'labels vs one-hot')
    for b in range(B):
        ref, lo = _shift_oracle(mov[b], flow[b], fill)
        dd = go.soft_dice(D64(fix[b:b + 1]), ref[None], eps)
        (-(dd * D64(wl[b:b + 1])).sum() / (B * L)).backward()
        close(N(d[b]), dd.detach().numpy()[0], 'dice')
        close(grads[0][b], lo.grad.numpy(), 'grad_flow b%d' % b)
    # single transform and 'xy' indexing
    f1 = G(flow[:1], dev, True)
    ne.fused.warp_dice_labels(m, f1, fx, L, single_transform=True, indexing='xy').sum().backward()
    f3 = G(flow[:1], dev, True)
    warped = ne.layers.SpatialTransformer(single_transform=True, indexing='xy')([G(mov, dev), f3])
    ne.metrics.Dice(check_input_limits=False).dice(G(fix, dev), warped).sum().backward()
    close(N(f1.grad), N(f3.grad), 'single/xy')


def test_deterministic(dev):
    rng = np.random.default_rng(45)
    L, S = 32, (19, 14, 27)
    m = G(rng.integers(-1, L + 2, (2,) + S).astype(np.int32), dev)
    f = G(rng.integers(-1, L + 2, (2,) + S).astype(np.int32), dev)
    t = G(rng.normal(0, 2.5, (2,) + S + (3,)).astype(F), dev)
    d1, s1 = ne.fused.warp_dice_labels(m, t, f, L, return_sums=True)
    d1, s1 = N(d1), N(s1)
    d2, s2 = ne.fused.warp_dice_labels(m, t, f, L, return_sums=True)
    assert bits_equal(N(d2), d1) and bits_equal(N(s2), s1)


def test_graph_capture_recomputes(dev):
    L, size = 32, 32
    mov = torch.stack([synth.blob_labels(s, size, L, device=dev) for s in (31, 32)]).to(torch.int32)
    fix = torch.stack([synth.blob_labels(s, size, L, device=dev) for s in (33, 34)]).to(torch.int32)
    trf = torch.stack([synth.smooth_displacement(s, size, device=dev) for s in (35, 36)])
    mov_a, mov_b = mov.clone(), torch.roll(mov, 3, dims=1).contiguous()
    trf_a, trf_b = trf.clone(), (trf * 0.5).contiguous()

    def fn():
        return ne.fused.warp_dice_labels(mov, trf, fix, L)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    seen = []
    for msrc, tsrc in ((mov_a, trf_a), (mov_b, trf_a), (mov_b, trf_b), (mov_a, trf_a)):
        mov.copy_(msrc)
        trf.copy_(tsrc)
        g.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert torch.equal(got, fn())
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and torch.equal(seen[0], seen[3])


def test_many_blocks(dev):
    """2 x 64^3, 32 labels: 256 blocks per volume, four groups of rows in the second stage; against the float64 sums"""
    L, size = 32, 64
    mov = torch.stack([synth.blob_labels(s, size, L, device=dev) for s in (51, 52)])
    fix = torch.stack([synth.blob_labels(s, size, L, device=dev) for s in (53, 54)])
    trf = torch.stack([synth.smooth_displacement(s, size, device=dev) for s in (55, 56)])
    d, s = ne.fused.warp_dice_labels(mov, trf, fix, L, return_sums=True)
    M = torch.nn.functional.one_hot(mov, L).float()
    Fx = torch.nn.functional.one_hot(fix, L).float()
    w = eager(lambda: ne.layers.SpatialTransformer()([M, trf]))
    sums, _ = co.dice_sums(N(Fx), N(w))
    assert bits_equal(N(s)[:, 1], sums[:, 1].astype(F))
    np.testing.assert_allclose(N(s), sums, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(N(d), co.dice_from_sums(sums), rtol=RTOL)
    np.testing.assert_allclose(N(d), N(ne.fused.warp_dice(M, trf, Fx)), rtol=1e-6)
