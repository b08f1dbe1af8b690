"""
GPU tests of the segmentation losses on an integer label map as y_true (csrc/segloss_labels.hip; fused.seg_loss_labels, and the same
integer y_true given to losses.Dice, losses.CategoricalCrossentropy and their pair behind losses.multiple_losses_decorator).

Reference: the unchanged oracle (oracle.np_oracle.dice / cce_per_voxel, oracle.grad_oracle) applied to the one-hot map built on the host
from the ids, with an all-zero row for an id outside [0, L).  Tolerances are those of tests/test_gpu_segloss.py: the label counts
exact, Dice rtol 1e-5 / atol 1e-7 and the CCE sum rtol 1e-5 against float64, 1e-6 against the one-hot kernels of this package,
gradients 1e-5 of their largest magnitude against float64 and 2e-6 against the one-hot path.

One label (L = 1): p / sum p is 1 at every voxel and is clipped to 1 - 1e-7, so the whole CCE is w * -log(1 - 1e-7) -- and float32 has no
1 - 1e-7: the reference framework's float32 graph, the one-hot kernels of this package (cce.hip) and these kernels all clip to
float32(1) - float32(1e-7) = 1 - 2^-23, whose logarithm is -1.19209e-7, while the float64 oracle clips to 1 - 1e-7 exactly, whose
logarithm is -1.00000e-7: 19 % apart, for any float32 arithmetic.  For that one case the float64 sum is therefore scaled by
log(1 - 2^-23) / log(1 - 1e-7) (the oracle with the clip bound float32 holds); the tolerance stays 1e-5.
"""

import contextlib
import io
import warnings

import numpy as np
import pytest
import torch

import neurite_amd as ne
from neurite_amd import _lib
from neurite_amd import metrics as MT
from neurite_amd import models as M
from oracle import grad_oracle as go
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu
F = np.float32
BOTH = _lib.SEG_WANT_DICE | _lib.SEG_WANT_CCE
L1_CLIP = float(np.log(np.float64(F(1) - F(1e-7))) / np.log(1 - 1e-7))

SHAPES = [(4, (2, 9, 7, 5)), (8, (1, 33, 5, 4)), (32, (3, 12, 11, 10)), (64, (2, 6, 5, 7)), (256, (1, 5, 3, 4)),      # lane groups
          (12, (2, 7, 6, 5)), (24, (2, 7, 6, 5)),                                                                    # padded groups
          (1, (2, 9, 7, 5)), (5, (2, 9, 7, 5)), (33, (2, 9, 7, 5)),                                                  # generic arm
          (4, (2, 37, 29, 23)), (32, (2, 37, 29, 23))]                                 # several blocks per entry, ragged last pass


def G(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def N(t):
    return t.detach().cpu().numpy()


def close(got, want, what, tol=1e-5):
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got.astype(np.float64) - want).max()) / scale
    print('%s: max error %.3g of the largest magnitude (tolerance %.1g)' % (what, err, tol))
    assert err <= tol, '%s: max error %.3g of the largest magnitude (tolerance %.1g)' % (what, err, tol)


def one_hot(ids, L):
    """float32 one-hot map on the host, an all-zero row for an id outside [0, L) (tf.one_hot)"""
    return (np.asarray(ids)[..., None] == np.arange(L)).astype(F)


_inputs = {}


def inputs(dev, L, shape):
    """ids in [-2, L + 2] (int32), their host one-hot map, logits, the device soft-max of the logits and random label weights; made once
    per (L, shape) and shared, never modified"""
    key = (L, shape)
    if key not in _inputs:
        rng = np.random.default_rng(100 * L + len(shape) + shape[1])
        ids = rng.integers(-2, L + 3, shape).astype(np.int32)
        z = rng.standard_normal(shape + (L,)).astype(F) * 2
        p = torch.softmax(G(z, dev), -1)
        _inputs[key] = (ids, one_hot(ids, L), z, p, rng.uniform(0.5, 2, L).astype(F))
    return _inputs[key]


def raw(ids, p, w, want, ls, eps):
    """the C ABI itself: sums, dice, minmax, cce_sum (None where `want` leaves a loss out)"""
    lib = _lib.lib()
    dev = p.device
    B, L = p.shape[0], p.shape[-1]
    V = p.numel() // (B * L)
    wd, wc = bool(want & _lib.SEG_WANT_DICE), bool(want & _lib.SEG_WANT_CCE)
    sums = torch.full((B, 3, L), -7.0, device=dev) if wd else None
    dice = torch.full((B, L), -7.0, device=dev) if wd else None
    mm = torch.full((4,), -7.0, device=dev) if wd else None
    cce = torch.full((1,), -7.0, device=dev) if wc else None
    nws = lib.nrt_seg_loss_labels_workspace_bytes(V, L, B)
    ws = _lib.workspace(dev, nws)
    rc = lib.nrt_seg_loss_labels_f32(_lib.ptr(ids), _lib.ptr(p), _lib.ptr(w), V, L, B, want, ls, eps, _lib.ptr(sums), _lib.ptr(dice),
                                     _lib.ptr(mm), _lib.ptr(cce), _lib.ptr(ws), nws, _lib.stream_ptr(dev))
    assert rc == 0
    return sums, dice, mm, cce


@pytest.mark.parametrize('L,shape', SHAPES)
@pytest.mark.parametrize('eps,ls', [(0., 0.), (0.1, 0.2)])
def test_forward(dev, L, shape, eps, ls):
    ids, t, z, p, w = inputs(dev, L, shape)
    idt, tt = G(ids, dev), G(t, dev)
    B = shape[0]
    counts = t.reshape(B, -1, L).sum(1)
    want_dice = npo.dice(t, N(p), laplace_smoothing=eps)
    for weights in (w, None):
        wt = None if weights is None else G(weights, dev)
        cce_sum, dice = ne.fused.seg_loss_labels(idt, p, weights, label_smoothing=ls, laplace_smoothing=eps)
        sums, dice_r, mm, cce_r = raw(idt, p, wt, BOTH, ls, eps)
        # two runs on the same inputs (one through the Python wrapper, one through the C ABI): bit-identical
        assert torch.equal(dice, dice_r) and torch.equal(cce_sum, cce_r)
        assert np.array_equal(N(sums[:, 1, :]), counts)                             # the label counts, exactly
        pn = N(p)
        assert N(mm).tolist() == [0.0, 1.0, float(pn.min()), float(pn.max())]
        # the oracle (float64 accumulation)
        np.testing.assert_allclose(N(dice), want_dice, rtol=1e-5, atol=1e-7)
        want = npo.cce_per_voxel(t, pn, weights, label_smoothing=ls).astype(np.float64).sum() * (L1_CLIP if L == 1 else 1.0)
        print('L %d %s eps %g ls %g weights %s: cce %.9g oracle %.9g rel %.3g; dice max abs diff %.3g'
              % (L, shape, eps, ls, weights is not None, float(cce_sum), want, abs(float(cce_sum) - want) / abs(want),
                 float(np.abs(N(dice) - want_dice).max())))
        np.testing.assert_allclose(float(cce_sum), want, rtol=1e-5)
        # the one-hot kernels of this package on the device map
        if _lib.lib().nrt_seg_loss_supported(L):
            cce_o, dice_o = MT._SegLossFn.apply(tt, p, wt, (eps, ls, True), None)
        else:
            _, dice_o, _ = MT.dice_partial_sums(tt, p, False, eps)
            cce_o = MT._WcceFn.apply(tt, p, wt, False, ls, False)
        np.testing.assert_allclose(N(dice), N(dice_o), rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(N(cce_sum), N(cce_o), rtol=1e-6)
        # a single loss: the same numbers from the kernel that leaves the other one out
        _, dice_d, _, none = raw(idt, p, wt, _lib.SEG_WANT_DICE, ls, eps)
        assert none is None and torch.equal(dice_d, dice)
        _, _, _, cce_c = raw(idt, p, wt, _lib.SEG_WANT_CCE, ls, eps)
        assert torch.equal(cce_c, cce_sum)


def test_label_absent_from_both_maps_has_dice_zero(dev):
    ids, t, z, p, w = inputs(dev, 8, (1, 33, 5, 4))
    ids = np.where(ids == 3, 5, ids)
    pz = p.clone()
    pz[..., 3] = 0.0
    for L, idv, pv in ((8, ids, pz), (5, np.where(ids == 3, 1, ids), pz[..., :5].contiguous())):
        cce_sum, dice = ne.fused.seg_loss_labels(G(idv, dev), pv)
        d = N(dice)
        assert d[0, 3] == 0.0 and (np.delete(d[0], 3) > 0).all() and np.isfinite(float(cce_sum))
        np.testing.assert_allclose(d, npo.dice(one_hot(idv, L), N(pv)), rtol=1e-5, atol=1e-7)
    # every id out of range: all-zero rows, Dice 0 everywhere, no cross-entropy
    cce_sum, dice = ne.fused.seg_loss_labels(torch.full((1, 33, 5, 4), 8, dtype=torch.int32, device=dev), p)
    assert float(cce_sum) == 0.0 and not N(dice).any()


def test_rows_off_16_byte_alignment_take_the_generic_arm(dev):
    """a multiple-of-4 label count whose rows do not start on 16 bytes (a view at an odd float offset) cannot be read as float4: the
    scalar-load arm gives the numbers of the lane-group arm to float32 rounding, forward and backward"""
    L, shape = 8, (1, 33, 5, 4)
    ids, t, z, p, w = inputs(dev, L, shape)
    idt = G(ids, dev)
    buf = torch.zeros(p.numel() + 1, device=dev)
    pu = buf[1:].view(p.shape)
    pu.copy_(p)
    assert pu.data_ptr() % 16 == 4 and pu.is_contiguous()
    pa, pu = p.detach().clone().requires_grad_(), pu.requires_grad_()
    gd = G(np.random.default_rng(1).standard_normal((1, L)).astype(F), dev)
    for y in (pa, pu):
        cce_sum, dice = ne.fused.seg_loss_labels(idt, y, w, label_smoothing=0.2, laplace_smoothing=0.1)
        (cce_sum[0] / 660 + (gd * dice).sum()).backward()
    np.testing.assert_allclose(N(dice), npo.dice(t, N(p), laplace_smoothing=0.1), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(float(cce_sum.detach()), npo.cce_per_voxel(t, N(p), w, label_smoothing=0.2).astype(np.float64).sum(), rtol=1e-5)
    close(N(pu.grad), N(pa.grad).astype(np.float64), 'unaligned rows vs aligned rows, d / d y_pred', 2e-6)


def test_range_check_looks_at_y_pred(dev):
    ids, t, z, p, w = inputs(dev, 8, (1, 33, 5, 4))
    bad = p.clone()
    bad[0, 1, 2, 3, 4] = 1.5
    for idt, pp in ((G(ids, dev), bad), (G(ids, dev), bad[..., :5].contiguous())):                  # L = 8: lane groups, L = 5: generic
        with pytest.raises(ne.errors.InvalidArgumentError):
            ne.fused.seg_loss_labels(idt, pp)
        ne.fused.seg_loss_labels(idt, pp, check_input_limits=False)
        with pytest.raises(ne.errors.InvalidArgumentError):
            ne.losses.Dice().loss(idt, pp)
        ne.losses.Dice(check_input_limits=False).loss(idt, pp)


def _float64_loss(z64, t64, w64, eps, ls, a, gd, softmax):
    p = torch.softmax(z64, -1) if softmax else z64
    n = p.numel() // p.shape[-1]
    total = 0.0
    if a is not None:
        total = total + a * go.cce_per_voxel(t64, p, w64, label_smoothing=ls).sum() / n
    if gd is not None:
        total = total + (gd * go.soft_dice(t64, p, eps)).sum()
    return total


def _one_hot_path(tt, y, wt, eps, ls, L):
    """(cce_sum, dice) of the device one-hot map on this package's one-hot kernels"""
    if _lib.lib().nrt_seg_loss_supported(L):
        src = getattr(y, '_nrt_softmax_src', None)
        if src is not None:
            return MT._SegLossFn.apply(tt, y.detach(), wt, (eps, ls, False), src, *src.inputs)
        return MT._SegLossFn.apply(tt, y, wt, (eps, ls, False), None)
    return MT._WcceFn.apply(tt, y, wt, False, ls, False), MT._SoftDiceFn.apply(tt, y, eps, False, False)


@pytest.mark.parametrize('L,shape', [(4, (2, 7, 6, 5)), (32, (2, 9, 8, 7)), (128, (1, 4, 3, 5)), (24, (2, 7, 6, 5)), (5, (2, 9, 7, 5))])
@pytest.mark.parametrize('eps,ls', [(0., 0.), (0.1, 0.2)])
def test_backward(dev, L, shape, eps, ls):
    ids, t, z, p, w = inputs(dev, L, shape)
    rng = np.random.default_rng(7 + L)
    gd = rng.standard_normal((shape[0], L)).astype(F)
    a = 1.7
    n = int(np.prod(shape))
    idt, tt, wt, gdt = G(ids, dev), G(t, dev), G(w, dev), G(gd, dev)
    t64, w64, gd64 = torch.from_numpy(t).double(), torch.from_numpy(w).double(), torch.from_numpy(gd).double()

    # (1) y_pred is a leaf: the gradient wrt the probabilities
    p0 = p.detach().clone().requires_grad_()
    before = MT._SegLossLabelsFn.through_softmax
    cce_sum, dice = ne.fused.seg_loss_labels(idt, p0, w, label_smoothing=ls, laplace_smoothing=eps)
    assert MT._SegLossLabelsFn.through_softmax == before
    (a * cce_sum[0] / n + (gdt * dice).sum()).backward()
    cce_leaf, dice_leaf = cce_sum.detach(), dice.detach()
    p64 = torch.from_numpy(N(p0)).double().requires_grad_()
    _float64_loss(p64, t64, w64, eps, ls, a, gd64, False).backward()
    close(N(p0.grad), p64.grad.numpy(), 'd / d y_pred vs float64')
    p1 = p.detach().clone().requires_grad_()
    cce_o, dice_o = _one_hot_path(tt, p1, wt, eps, ls, L)
    (a * cce_o[0] / n + (gdt * dice_o).sum()).backward()
    close(N(p0.grad), N(p1.grad).astype(np.float64), 'd / d y_pred vs the one-hot path', 2e-6)

    # (2) through the soft-max: the stamp of models._softmax_with_grad is taken and its input receives the gradient
    zt = G(z, dev, grad=True)
    y = M._softmax_with_grad(zt)
    src = y._nrt_softmax_src
    assert src.valid_for(y) and src.inputs[0] is zt
    cce_sum, dice = ne.fused.seg_loss_labels(idt, y, w, label_smoothing=ls, laplace_smoothing=eps)
    assert MT._SegLossLabelsFn.through_softmax == before + 1
    (a * cce_sum[0] / n + (gdt * dice).sum()).backward()
    z64 = torch.from_numpy(z).double().requires_grad_()
    _float64_loss(z64, t64, w64, eps, ls, a, gd64, True).backward()
    close(N(zt.grad), z64.grad.numpy(), 'd / d logits vs float64')
    zs = G(z, dev, grad=True)
    ys = M._softmax_with_grad(zs) if _lib.lib().nrt_seg_loss_supported(L) else M._SoftmaxFn.apply(zs)
    cce_o, dice_o = _one_hot_path(tt, ys, wt, eps, ls, L)
    (a * cce_o[0] / n + (gdt * dice_o).sum()).backward()
    close(N(zt.grad), N(zs.grad).astype(np.float64), 'd / d logits vs the one-hot path', 2e-6)

    # (3) one loss at a time (the kernels that get a null grad_cce / grad_dice), through the loss objects
    p2 = p.detach().clone().requires_grad_()
    d = ne.losses.Dice(laplace_smoothing=eps).dice(idt, p2)
    assert torch.equal(d, dice_leaf)
    (gdt * d).sum().backward()
    p64 = torch.from_numpy(N(p2)).double().requires_grad_()
    _float64_loss(p64, t64, w64, eps, ls, None, gd64, False).backward()
    close(N(p2.grad), p64.grad.numpy(), 'Dice only, d / d y_pred vs float64')
    p3 = p.detach().clone().requires_grad_()
    c = ne.losses.CategoricalCrossentropy(w, label_smoothing=ls).loss(idt, p3)
    np.testing.assert_allclose(float(c.detach()), float(cce_leaf) / n, rtol=1e-6)
    (a * c).backward()
    p64 = torch.from_numpy(N(p3)).double().requires_grad_()
    _float64_loss(p64, t64, w64, eps, ls, a, None, False).backward()
    close(N(p3.grad), p64.grad.numpy(), 'CCE only, d / d y_pred vs float64')


def _small_unet(dev, rng, L=4):
    with contextlib.redirect_stdout(io.StringIO()):
        net = ne.models.unet(8, (16, 8, 16, 1), 2, 3, L, feat_mult=2).to(dev)
    for m in net.layers_by_name.values():
        with torch.no_grad():
            m.kernel.copy_(G((rng.standard_normal(tuple(m.kernel.shape)) * 0.2).astype(F), dev))
            m.bias.copy_(G((rng.standard_normal(tuple(m.bias.shape)) * 0.1).astype(F), dev))
    net.train()
    return net


@pytest.mark.parametrize('L', [4, 5])
def test_decorator_takes_ids_through_the_unet_head(dev, L):
    """losses.multiple_losses_decorator([cce.loss, dice.mean_loss]) on a unet with an ids target: the loss value and the gradient of
    every parameter that the one-hot target gives, from the labels kernels (no one-hot map), through the head's soft-max"""
    rng = np.random.default_rng(5)
    B = 2
    net = _small_unet(dev, rng, L)
    x = G(rng.standard_normal((B, 16, 8, 16, 1)).astype(F), dev)
    ids = rng.integers(-1, L + 1, (B, 16, 8, 16)).astype(np.int32)
    idt, t = G(ids, dev), G(one_hot(ids, L), dev)
    cce = ne.losses.CategoricalCrossentropy(rng.uniform(0.5, 2, L).astype(F))
    dice = ne.losses.Dice(weights=np.ones((1, L), F) * 0.5, laplace_smoothing=0.01)
    joint = ne.losses.multiple_losses_decorator([cce.loss, dice.mean_loss], [1.0, 2.0])

    want_loss = joint(t, net(x))
    want_loss.backward()
    want = {k: (m.kernel.grad.clone(), m.bias.grad.clone()) for k, m in net.layers_by_name.items()}
    net.zero_grad()

    before = (MT.JointSegLoss.applications, MT.JointSegLoss.through_softmax, MT._SegLossLabelsFn.applications,
              MT._SegLossLabelsFn.through_softmax)
    y = net(x)
    assert isinstance(getattr(y, '_nrt_softmax_src', None), M.SoftmaxSource)
    total = joint(idt, y)
    after = (MT.JointSegLoss.applications, MT.JointSegLoss.through_softmax, MT._SegLossLabelsFn.applications,
             MT._SegLossLabelsFn.through_softmax)
    assert after == tuple(v + 1 for v in before)                  # one evaluation, by the labels kernels, attached to the head
    np.testing.assert_allclose(float(total), float(want_loss), rtol=2e-6)
    total.backward()
    for k, m in net.layers_by_name.items():
        close(N(m.kernel.grad), N(want[k][0]).astype(np.float64), 'L %d %s kernel' % (L, k), 2e-6)
        close(N(m.bias.grad), N(want[k][1]).astype(np.float64), 'L %d %s bias' % (L, k), 2e-6)

    # every id dtype and the trailing-1 shape: the results of int32 (ids in [0, L]: what uint8 can hold)
    with torch.no_grad():
        y = net(x)
        idp = idt.clamp(0, L)
        ref = joint(idp, y)
        for dtype in (torch.uint8, torch.int8, torch.int16, torch.int64):
            assert torch.equal(joint(idp.to(dtype), y), ref), dtype
            assert torch.equal(joint(idp.to(dtype).unsqueeze(-1), y), ref), dtype
        assert torch.equal(cce.loss(idp.long().unsqueeze(-1), y), cce.loss(idp, y))
        assert torch.equal(dice.mean_loss(idp.to(torch.int16).unsqueeze(-1), y), dice.mean_loss(idp, y))
        # an int64 id beyond int32 stays out of range instead of wrapping into [0, L)
        big, out = idp.long().clone(), idp.clone()
        big[0, 0, 0, :4] = (1 << 40) + 1
        out[0, 0, 0, :4] = L
        assert torch.equal(joint(big, y), joint(out, y))


def test_fallback_configurations_equal_their_one_hot_call(dev):
    """what has no labels kernel builds the float32 one-hot map on the device and takes the path it always took: the same numbers"""
    L, shape = 8, (1, 33, 5, 4)
    ids, t, z, p, w = inputs(dev, L, shape)
    idt, tt, zt = G(ids, dev), G(t, dev), G(z, dev)
    sw = G(np.random.default_rng(2).uniform(0.5, 2, shape).astype(F), dev)
    before = MT._SegLossLabelsFn.applications
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name, fn in (('normalize', lambda a: ne.losses.SoftDice(normalize=True).loss(a, p)),
                         ('logits', lambda a: ne.losses.CategoricalCrossentropy(w, from_logits=True).loss(a, zt)),
                         ('none', lambda a: ne.losses.CategoricalCrossentropy(w, reduction='none').loss(a, p)),
                         ('sample_weight', lambda a: ne.losses.CategoricalCrossentropy(w)(a, p, sample_weight=sw)),
                         ('hard', lambda a: ne.losses.HardDice(L, input_type='prob').loss(a, p)),
                         ('bfloat16 cce', lambda a: ne.losses.CategoricalCrossentropy(w).loss(a, p.bfloat16())),
                         ('bfloat16 dice', lambda a: ne.losses.Dice().loss(a, p.bfloat16()))):
            got, want = fn(idt), fn(tt)
            assert got.shape == want.shape and torch.equal(got, want), name
            assert torch.equal(fn(idt.long().unsqueeze(-1)), want), name
    assert MT._SegLossLabelsFn.applications == before              # no labels kernel ran: these are the one-hot kernels' own numbers
    # a pair that does not qualify as a pair: each half on its own, the half with a labels kernel on that kernel
    for c, d in ((ne.losses.CategoricalCrossentropy(w), ne.losses.SoftDice(normalize=True)),
                 (ne.losses.CategoricalCrossentropy(from_logits=True), ne.losses.Dice())):
        f = ne.losses.multiple_losses_decorator([c.loss, d.mean_loss])
        np.testing.assert_allclose(float(f(idt, p)), float(f(tt, p)), rtol=2e-6)
    assert MT._SegLossLabelsFn.applications == before + 2
    # a pending warp as y_pred: the fused warp + Dice kernel still takes it, on the device one-hot map
    mov, fix, trf = ne.synth.cfg2_batch(2, 16, 8, device=dev, seed0=11)
    fid = fix.argmax(-1).to(torch.int32)
    d = ne.metrics.Dice(check_input_limits=False)
    warped = ne.layers.SpatialTransformer()([mov, trf])
    assert isinstance(warped, ne.deferred.DeferredWarp) and warped.pending
    got = d.dice(fid, warped)
    assert warped.pending
    assert torch.equal(got, d.dice(fix, ne.layers.SpatialTransformer()([mov, trf])))
    c = ne.losses.CategoricalCrossentropy()
    assert torch.equal(c.loss(fid, ne.layers.SpatialTransformer()([mov, trf])), c.loss(fix, ne.layers.SpatialTransformer()([mov, trf])))
    # the fused configurations on the same inputs do run the labels kernels, and agree with the one-hot call to float32 rounding
    before = MT._SegLossLabelsFn.applications
    for fn in (lambda a: ne.losses.Dice(laplace_smoothing=0.1).mean_loss(a, p), lambda a: ne.losses.CategoricalCrossentropy(w).loss(a, p),
               lambda a: ne.losses.CategoricalCrossentropy(w, reduction='sum', label_smoothing=0.1).loss(a, p),
               lambda a: ne.losses.CategoricalCrossentropy(reduction='sum_over_batch_size')(a, p)):
        np.testing.assert_allclose(float(fn(idt)), float(fn(tt)), rtol=2e-6)
    assert MT._SegLossLabelsFn.applications == before + 4


def test_training_step_with_an_ids_target_captures_into_one_hipgraph(dev):
    """the training step of test_gpu_segloss.py::test_training_step_captures_into_one_hipgraph with an ids target: forward + joint loss
    + backward + SGD as ONE hipGraph launch; replays walk the same parameter trajectory as eager steps"""
    rng = np.random.default_rng(11)
    L, B = 4, 2
    x = G(rng.standard_normal((B, 16, 8, 16, 1)).astype(F), dev)
    t = G(rng.integers(0, L, (B, 16, 8, 16)).astype(np.int32), dev)
    cce, dice = ne.losses.CategoricalCrossentropy(), ne.losses.Dice(check_input_limits=False)
    seg = ne.losses.multiple_losses_decorator([cce.loss, dice.loss])
    lr = 5e-3

    def make():
        net = _small_unet(dev, np.random.default_rng(12), L)
        return net, list(net.parameters())

    def step(net, params):
        for p in params:
            p.grad = None
        loss = seg(t, net(x)).mean()
        loss.backward()
        with torch.no_grad():
            torch._foreach_add_(params, [p.grad for p in params], alpha=-lr)
        return loss

    net_e, par_e = make()
    eager = [float(step(net_e, par_e)) for _ in range(4)]
    assert eager[-1] < eager[0]

    net_g, par_g = make()
    start = [p.detach().clone() for p in par_g]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(net_g, par_g)                                   # warm-up outside the capture: one-time uploads, workspace growth
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():
        for p, s in zip(par_g, start):
            p.copy_(s)
    for p in par_g:
        p.grad = None
    before = MT._SegLossLabelsFn.through_softmax
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step(net_g, par_g)
    assert MT._SegLossLabelsFn.through_softmax == before + 1
    replayed = []
    for _ in range(4):
        graph.replay()
        replayed.append(float(loss))
    np.testing.assert_allclose(replayed, eager, rtol=1e-4)
    for a, b in zip(par_e, par_g):
        close(N(b), N(a).astype(np.float64), 'parameters after 4 steps', 1e-4)
