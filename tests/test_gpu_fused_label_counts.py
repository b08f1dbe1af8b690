"""
Fused warp + Dice (csrc/fused.hip, entry point warp_dice_tile_pad) and its backward wrt the field (csrc/backward.hip, entry point
warp_dice_bwd_rows_pad) for label counts that are multiples of 4 but not 4 * 2^k: lane groups of the next power of two, the lanes
past L / 4 idle.  Each is the PAD = true instance of the one kernel body it shares with the 4 * 2^k entry point.
Tolerances as tests/test_gpu_dice_cce.py (warped bit-identical, sums / dice 1e-6 against the unfused HIP pipeline) and
tests/test_gpu_backward.py (gradients 1e-4 of their scale against the float64 oracle).
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
TILES = (3 | (3 << 4) | (4 << 8), 1 | (1 << 4) | (3 << 8) | (1 << 12))      # 8 x 8 x 16 tiles; 2 x 2 x 8, z outermost


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


@pytest.mark.parametrize('L', [12, 20, 24, 28, 36, 44, 60, 100, 252])
def test_forward_against_oracle(dev, L):
    rng = np.random.default_rng(100 + L)
    shapes = ((2, (19, 14, 27), (19, 14, 27)), (1, (9, 8, 12), (7, 11, 5)))
    if L > 64:
        shapes = ((2, (9, 7, 11), (9, 7, 11)), (1, (6, 8, 5), (7, 5, 9)))
    for B, S, So in shapes:
        mov = rng.random((B,) + S + (L,)).astype(F)
        fix = rng.random((B,) + So + (L,)).astype(F)
        trf = rng.normal(0, 2.5, (B,) + So + (3,)).astype(F)
        m, f, t = G(mov, dev), G(fix, dev), G(trf, dev)
        for fill in (None, 0.0):
            w_ref = npo.spatial_transformer(mov, trf, fill_value=fill)
            sums_ref = np.stack(npo.dice_sums(fix, w_ref), 1)
            w_hip, d_hip = _unfused_dice(m, t, f, fill_value=fill, laplace_smoothing=0.25)
            assert bits_equal(N(w_hip), w_ref), (L, S, fill)
            for tune in (0,) + TILES:
                d, w, s = ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, laplace_smoothing=0.25,
                                             _tune=tune)
                assert bits_equal(N(w), w_ref), (L, S, fill, tune)
                np.testing.assert_allclose(N(s), sums_ref, rtol=1e-6, atol=1e-6)
                np.testing.assert_allclose(N(d), npo.dice(fix, w_ref, laplace_smoothing=0.25, check_input_limits=False), rtol=RTOL)
                np.testing.assert_allclose(N(d), N(d_hip), rtol=1e-6)
                d2 = ne.fused.warp_dice(m, t, f, fill_value=fill, laplace_smoothing=0.25, _tune=tune)
                assert bits_equal(N(d2), N(d)), (L, S, fill, tune)            # with / without writing `warped`
        # a single transform and cartesian indexing
        for kw in ({'single_transform': True}, {'indexing': 'xy'}, {'single_transform': True, 'indexing': 'xy'}):
            tt = t[:1] if kw.get('single_transform') else t
            d, w = ne.fused.warp_dice(m, tt, f, return_warped=True, **kw)
            w_hip, d_hip = _unfused_dice(m, tt, f, **kw)
            trf_np = N(tt)
            w_ref = npo.spatial_transformer(mov, trf_np, indexing=kw.get('indexing', 'ij'),
                                            single_transform=kw.get('single_transform', False))
            assert bits_equal(N(w), w_ref) and bits_equal(N(w_hip), w_ref), (L, kw)
            np.testing.assert_allclose(N(d), N(d_hip), rtol=1e-6)


def test_x_march_schedule_at_24_labels(dev):
    """24 labels = lane groups of 8 lanes: fused_geom takes the x-march block schedule by default (13 x 8 patches x 6 volumes >= 512);
    ragged patches, regions and segments as tests/test_gpu_dice_cce.py::test_fused_x_march_schedule_ragged"""
    lib = ne._lib.lib()
    rng = np.random.default_rng(78)
    B, S, L = 6, (36, 50, 61), 24
    assert lib.nrt_warp_dice_kernel_name(ne._lib.ints(S), ne._lib.ints(S), L, B, 1, 1, 1, 0, 0) == \
        b'warp_dice_tile_pad<8, 1, true, 3, float>'
    mov = rng.random((B,) + S + (L,)).astype(F)
    fix = rng.random((B,) + S + (L,)).astype(F)
    trf = rng.normal(0, 2.0, (B,) + S + (3,)).astype(F)
    w_ref = npo.spatial_transformer(mov, trf, fill_value=0.0)
    d_ref = npo.dice(fix, w_ref, check_input_limits=False)
    xm = 3 | (2 << 4) | (3 << 8) | (1 << 14)
    tunes = (0, 3 | (3 << 4) | (4 << 8), xm, xm | (3 << 16), xm | (5 << 16) | (2 << 24) | (1 << 27),
             3 | (3 << 4) | (3 << 8) | (1 << 14) | (1 << 24) | (3 << 27))
    m, f, t = G(mov, dev), G(fix, dev), G(trf, dev)
    for tune in tunes:
        d, w = ne.fused.warp_dice(m, t, f, fill_value=0.0, return_warped=True, _tune=tune)
        assert bits_equal(N(w), w_ref), tune
        np.testing.assert_allclose(N(d), d_ref, rtol=RTOL, err_msg=str(tune))
        d2 = ne.fused.warp_dice(m, t, f, fill_value=0.0, _tune=tune)
        assert bits_equal(N(d2), N(d)), tune


@pytest.mark.parametrize('L', [24, 36])
def test_bf16_storage(dev, L):
    mov, fix, trf = synth.cfg2_batch(2, 48, L, device=dev, seed0=5)
    rng = np.random.default_rng(L)
    soft = torch.from_numpy(rng.random((2, 48, 48, 48, L)).astype(F)).to(dev).bfloat16()
    for m, f in ((mov.bfloat16(), fix.bfloat16()), (soft, fix.bfloat16()), (mov.bfloat16(), soft)):
        for tune in (0, TILES[0]):
            for fill in (None, 0.0):
                d16, s16 = ne.fused.warp_dice(m, trf, f, fill_value=fill, return_sums=True, _tune=tune)
                d32, s32 = ne.fused.warp_dice(m.float(), trf, f.float(), fill_value=fill, return_sums=True, _tune=tune)
                assert bits_equal(N(s16), N(s32)) and bits_equal(N(d16), N(d32)), (tune, fill)
    # one-hot maps are exact in bfloat16
    assert bits_equal(N(ne.fused.warp_dice(mov.bfloat16(), trf, fix.bfloat16())), N(ne.fused.warp_dice(mov, trf, fix)))


@pytest.mark.parametrize('L', [12, 24, 36])
def test_range_asserts(dev, L):
    """check_input_limits=True / 'deferred' raise exactly when the eager pipeline does"""
    mov, fix, trf = synth.cfg2_batch(2, 24, L, device=dev, seed0=13)
    for m, f in ((mov, fix), (mov * 0.5, fix * 0.5), (mov, fix * 1.5)):
        try:
            eager(lambda: ne.metrics.Dice().dice(f, ne.layers.SpatialTransformer()([m, trf])).cpu())
            want = False
        except ne.errors.InvalidArgumentError:
            want = True
        try:
            ne.fused.warp_dice(m, trf, f, check_input_limits=True)
            got = False
        except ne.errors.InvalidArgumentError:
            got = True
        assert got == want
        try:
            ne.fused.warp_dice(m, trf, f, check_input_limits='deferred').cpu()
            got = False
        except ne.errors.InvalidArgumentError:
            got = True
        assert got == want
    with pytest.raises(NotImplementedError):
        ne.fused.warp_dice(mov[..., :10].contiguous(), trf, fix[..., :10].contiguous())


@pytest.mark.parametrize('L,fill,eps', [(12, None, 0.), (24, 0.0, 0.1), (36, None, 0.)])
def test_backward(dev, L, fill, eps):
    """ne.fused.warp_dice backward == SpatialTransformer -> Dice backward == float64 oracle; deterministic"""
    rng = np.random.default_rng(23 + L)
    B, S = 2, (14, 12, 10)
    mov = np.eye(L, dtype=F)[rng.integers(0, L, (B,) + S)]
    fix = np.eye(L, dtype=F)[rng.integers(0, L, (B,) + S)]
    flow = (rng.standard_normal((B,) + S + (3,)) * 2.0).astype(F)
    flow[1, :2] = 0
    wl = rng.uniform(0.5, 1.5, (B, L)).astype(F)
    grads = []
    for _ in range(2):
        f = G(flow, dev, True)
        d = ne.fused.warp_dice(G(mov, dev), f, G(fix, dev), fill_value=fill, laplace_smoothing=eps)
        (-(d * G(wl, dev)).mean()).backward()
        grads.append(N(f.grad))
    assert bits_equal(grads[0], grads[1])
    f2 = G(flow, dev, True)
    warped = ne.layers.SpatialTransformer(fill_value=fill)([G(mov, dev), f2])
    d2 = ne.metrics.Dice(check_input_limits=False, laplace_smoothing=eps).dice(G(fix, dev), warped)
    (-(d2 * G(wl, dev)).mean()).backward()
    close(grads[0], N(f2.grad), 'fused vs unfused')
    for b in range(B):
        ref, lo = _shift_oracle(mov[b], flow[b], fill)
        dd = go.soft_dice(D64(fix[b:b + 1]), ref[None], eps)
        (-(dd * D64(wl[b:b + 1])).sum() / (B * L)).backward()
        close(N(d[b]), dd.detach().numpy()[0], 'dice')
        close(grads[0][b], lo.grad.numpy(), 'grad_flow b%d' % b)
    # single transform and 'xy' indexing
    f1 = G(flow[:1], dev, True)
    ne.fused.warp_dice(G(mov, dev), f1, G(fix, dev), single_transform=True, indexing='xy').sum().backward()
    f3 = G(flow[:1], dev, True)
    warped = ne.layers.SpatialTransformer(single_transform=True, indexing='xy')([G(mov, dev), f3])
    ne.metrics.Dice(check_input_limits=False).dice(G(fix, dev), warped).sum().backward()
    close(N(f1.grad), N(f3.grad), 'single/xy')


def test_backward_x_march_at_24_labels(dev):
    """lane groups of 8: the backward takes the forward's x-march block schedule on a ragged shape (6 volumes)"""
    rng = np.random.default_rng(32)
    B, S, L = 6, (20, 50, 61), 24
    mov = rng.random((B,) + S + (L,)).astype(F)
    fix = rng.random((B,) + S + (L,)).astype(F)
    flow = (rng.standard_normal((B,) + S + (3,)) * 2.0).astype(F)
    wl = rng.uniform(0.5, 1.5, (B, L)).astype(F)
    grads = []
    for _ in range(2):
        f = G(flow, dev, True)
        (-(ne.fused.warp_dice(G(mov, dev), f, G(fix, dev)) * G(wl, dev)).mean()).backward()
        grads.append(N(f.grad))
    assert bits_equal(grads[0], grads[1])
    f2 = G(flow, dev, True)
    warped = ne.layers.SpatialTransformer()([G(mov, dev), f2])
    (-(ne.metrics.Dice(check_input_limits=False).dice(G(fix, dev), warped) * G(wl, dev)).mean()).backward()
    close(grads[0], N(f2.grad), 'fused vs unfused')
    for b in (0, B - 1):
        ref, lo = _shift_oracle(mov[b], flow[b])
        dd = go.soft_dice(D64(fix[b:b + 1]), ref[None])
        (-(dd * D64(wl[b:b + 1])).sum() / (B * L)).backward()
        close(grads[0][b], lo.grad.numpy(), 'grad_flow b%d' % b)


@pytest.mark.parametrize('L', [24, 36])
def test_deferral(dev, L):
    mov, fix, trf = synth.cfg2_batch(2, 32, L, device=dev, seed0=11)
    st = ne.layers.SpatialTransformer()
    w = st([mov, trf])
    assert isinstance(w, ne.deferred.DeferredWarp) and w.pending
    D = ne.metrics.Dice(check_input_limits=False)
    d = D.dice(fix, w)
    d_e = eager(lambda: D.dice(fix, st([mov, trf])))
    np.testing.assert_allclose(N(d), N(d_e), rtol=1e-6)
    w_e = eager(lambda: st([mov, trf]))
    assert bits_equal(N(ne.deferred.materialize(st([mov, trf]))), N(w_e))
    # three labels still warp eagerly
    assert type(st([mov[..., :3].contiguous(), trf])) is torch.Tensor


def test_graph_capture_recomputes(dev):
    mov, fix, trf = synth.cfg2_batch(2, 48, 24, device=dev, seed0=31)
    fix_a, fix_b = fix.clone(), torch.roll(fix, 5, dims=-1).contiguous()
    trf_a, trf_b = trf.clone(), (trf * 0.5).contiguous()

    def fn():
        return ne.fused.warp_dice(mov, trf, fix)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    try:
        seen = []
        for fsrc, tsrc in ((fix_a, trf_a), (fix_b, trf_a), (fix_b, trf_b), (fix_a, trf_a)):
            fix.copy_(fsrc)
            trf.copy_(tsrc)
            g.replay()
            torch.cuda.synchronize()
            got = out.clone()
            assert torch.equal(got, fn())
            seen.append(got)
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and torch.equal(seen[0], seen[3])
    finally:
        fix.copy_(fix_a)


def test_full_size_24_labels(dev):
    mov, fix, trf = synth.cfg2_batch(2, 160, 24, device=dev, seed0=1)
    d, w = ne.fused.warp_dice(mov, trf, fix, return_warped=True)
    w2 = eager(lambda: ne.layers.SpatialTransformer()([mov, trf]))
    assert torch.equal(w, w2)
    d2 = ne.metrics.Dice(check_input_limits=False).dice(fix, w2)
    np.testing.assert_allclose(N(d), N(d2), rtol=1e-6)
    sums, _ = co.dice_sums(N(fix), N(w2))
    np.testing.assert_allclose(N(d), co.dice_from_sums(sums), rtol=RTOL)
    assert bits_equal(N(ne.fused.warp_dice(mov, trf, fix)), N(d))
