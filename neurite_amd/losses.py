"""
neurite_amd.losses -- neurite/tf/losses.py:46-205 for the hot path: the metrics classes with
`loss` (negative Dice [B, L] / the CCE scalar) and `mean_loss` (negative mean Dice); and the two losses of an unsupervised
VoxelMorph registration run, `NCC` and `Grad` (vxm.losses; restated), on csrc/vxmloss.hip; and `NegJacobian`, the
folding penalty on the Jacobian determinant of a field (an extension), on csrc/jacobian.hip; and `SignedDistanceMSE`,
the regression of a signed distance map drawn from a label map (an extension), on csrc/edt.hip.
"""

import numpy as np
import torch

from . import _lib, metrics, utils
from .deferred import materialize

__all__ = ['Dice', 'SoftDice', 'HardDice', 'CategoricalCrossentropy', 'WeightedCategoricalCrossentropy',
           'MeanSquaredErrorProb', 'multiple_losses_decorator', 'NCC', 'Grad', 'NegJacobian', 'SignedDistanceMSE']


class _DiceLossMixin:
    def loss(self, y_true, y_pred):
        """dice loss (negative Dice score), [batch_size, nb_labels] (neurite/tf/losses.py:68-80)."""
        return - self.dice(y_true, y_pred)

    def mean_loss(self, y_true, y_pred):
        """negative mean dice, scalar (neurite/tf/losses.py:82-95)."""
        return - self.mean_dice(y_true, y_pred)


class Dice(_DiceLossMixin, metrics.Dice):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)


class SoftDice(_DiceLossMixin, metrics.SoftDice):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)


class HardDice(_DiceLossMixin, metrics.HardDice):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)


class CategoricalCrossentropy(metrics.CategoricalCrossentropy):
    """neurite/tf/losses.py:193-205."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)

    def loss(self, *args, **kwargs):
        return self.cce(*args, **kwargs)


WeightedCategoricalCrossentropy = CategoricalCrossentropy


class MeanSquaredErrorProb(metrics.MeanSquaredErrorProb):
    """neurite/tf/losses.py:208-220."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)

    def loss(self, *args, **kwargs):
        return self.mse(*args, **kwargs)


def _owner(fn, cls, names):
    """the `cls` instance a loss callable belongs to (a bound method named in `names`, or the callable object itself)"""
    if isinstance(fn, cls):
        return fn
    obj = getattr(fn, '__self__', None)
    return obj if isinstance(obj, cls) and getattr(fn, '__name__', '') in names else None


def multiple_losses_decorator(losses, weights=None):
    """
    Weighted sum of several losses of one output (neurite/tf/losses.py:225-246): returns loss(y_true, y_pred).
    When the list holds exactly one soft-Dice method and one CategoricalCrossentropy method of this package -- the segmentation
    pair -- both take their numbers from one pass over the maps, and one pass back that also runs through the soft-max that made
    y_pred (metrics.JointSegLoss, csrc/segloss.hip); every value is what the two losses return on their own.  With an integer label
    map as y_true the pair runs on csrc/segloss_labels.hip, for any label count up to 256, and no one-hot target exists.
    """
    scale = np.ones(len(losses)) if weights is None else weights
    dice_objs = [o for o in (_owner(f, metrics.Dice, ('loss', 'mean_loss', 'dice', 'mean_dice')) for f in losses) if o is not None]
    cce_objs = [o for o in (_owner(f, metrics.CategoricalCrossentropy, ('loss', 'cce', '__call__')) for f in losses) if o is not None]
    pair = (dice_objs[0], cce_objs[0]) if len(dice_objs) == 1 and len(cce_objs) == 1 else None

    def weighted_sum(y_true, y_pred):
        return sum(scale[k] * fn(y_true, y_pred) for k, fn in enumerate(losses))

    def loss(y_true, y_pred):
        joint = metrics.JointSegLoss.open(*pair, y_true, y_pred) if pair is not None else None
        if joint is None:
            return weighted_sum(y_true, y_pred)
        with joint:
            return weighted_sum(y_true, y_pred)

    return loss


# --------------------------------------------------------------------------------------
# VoxelMorph's registration losses (csrc/vxmloss.hip)
# --------------------------------------------------------------------------------------

_MAX_WIN, _MAX_NCC_CHANNELS = 15, 16


def _spatial3(t):
    """[B, *S, C] with 1 .. 3 spatial axes -> (batch, [1, .., *S] of length 3, ndims, channels)"""
    nd = t.dim() - 2
    return int(t.shape[0]), [1] * (3 - nd) + [int(v) for v in t.shape[1:-1]], nd, int(t.shape[-1])


def _checked(t, what):
    """the host-side checks every tensor argument passes, before its device is looked at; returns the real tensor"""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(t).__name__))
    t = materialize(t)
    if t.dim() < 3 or t.dim() > 5:
        raise ValueError('%s: expected [batch, *spatial, channels] with 1 to 3 spatial axes, got shape %s' % (what, tuple(t.shape)))
    if t.numel() == 0:
        raise ValueError('%s: empty tensor of shape %s' % (what, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise NotImplementedError('%s: float32 only, got %s' % (what, t.dtype))
    return t


class _NCCFn(torch.autograd.Function):
    """I, J [B, *S, C] float32 contiguous -> the map cc [B, *S, 1] (as_loss False) or -mean(cc) [B] (as_loss True).  The backward keeps
    I and J only: two launches of the forward's box-sum kernel rebuild what it needs."""

    @staticmethod
    def forward(ctx, I, J, win, eps, as_loss):
        lib = _lib.lib()
        dev = I.device
        batch, shape, nd, channels = _spatial3(I)
        cshape, cwin = _lib.ints(shape), _lib.ints(win)
        nws = int(lib.nrt_ncc_workspace_bytes(batch, cshape, channels, cwin))
        if as_loss:
            out = torch.empty((batch,), dtype=torch.float32, device=dev)
            ws = _lib.workspace(dev, max(nws, 16))
            args = (None, None, _lib.ptr(out), _lib.ptr(ws), nws)
        else:
            out = torch.empty(tuple(I.shape[:-1]) + (1,), dtype=torch.float32, device=dev)
            args = (None, _lib.ptr(out), None, None, 0)
        _lib.call(dev, 'nrt_ncc_f32', _lib.ptr(I), _lib.ptr(J), batch, cshape, channels, cwin, eps, *args)
        ctx.save_for_backward(I, J)
        ctx.cfg = (batch, shape, channels, tuple(win), eps, as_loss)
        return out

    @staticmethod
    def backward(ctx, g):
        I, J = ctx.saved_tensors
        batch, shape, channels, win, eps, as_loss = ctx.cfg
        lib = _lib.lib()
        dev = I.device
        g = g.to(torch.float32).contiguous()
        need_i, need_j = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_i or need_j):
            return None, None, None, None, None
        gI = torch.empty_like(I) if need_i else None
        gJ = torch.empty_like(J) if need_j else None
        cshape, cwin = _lib.ints(shape), _lib.ints(win)
        nws = int(lib.nrt_ncc_workspace_bytes(batch, cshape, channels, cwin))
        ws = _lib.workspace(dev, max(nws, 16))
        _lib.call(dev, 'nrt_ncc_bwd_f32', _lib.ptr(I), _lib.ptr(J), None if as_loss else _lib.ptr(g), _lib.ptr(g) if as_loss else None,
                  batch, cshape, channels, cwin, eps, _lib.ptr(gI), _lib.ptr(gJ), _lib.ptr(ws), nws)
        return gI, gJ, None, None, None


class NCC:
    """
    Local (over a window) normalised cross-correlation loss, vxm.losses.NCC restated (voxelmorph is not in the reference tree; DESIGN 8
    gives the exact operation order).  Tensors are channels-last, [B, *S, C], 1 to 3 spatial axes, float32.

    win:  the window, an int or one int per spatial axis, each 1 .. 15; None means 9 per axis.  The five sums run over the window and
          over all channels (1 .. 16), zero padded as TensorFlow's 'SAME' pads, so even windows are allowed.
    eps:  the floor of the cross term and of both variances.

    Differentiable in both images.  Nothing travels to the host: forward and backward capture into a graph.
    """

    def __init__(self, win=None, eps=1e-5):
        if win is not None:
            try:
                seq = [win] if isinstance(win, (int, np.integer)) else list(win)
            except TypeError:
                raise ValueError('NCC: win is an int or a sequence of ints, got %r' % (win,))
            if not seq or not all(isinstance(w, (int, np.integer)) and not isinstance(w, bool) for w in seq):
                raise ValueError('NCC: win is an int or a sequence of ints, got %r' % (win,))
            if any(w < 1 for w in seq):
                raise ValueError('NCC: a window is at least 1, got %r' % (win,))
            if any(w > _MAX_WIN for w in seq):
                raise NotImplementedError('NCC: windows up to %d, got %r' % (_MAX_WIN, win))
        eps = float(eps)
        if not eps >= 0.0:
            raise ValueError('NCC: eps must be non-negative, got %r' % (eps,))
        self.win = win
        self.eps = eps

    def _window(self, nd):
        if self.win is None:
            return [9] * nd
        if isinstance(self.win, (int, np.integer)):
            return [int(self.win)] * nd
        win = [int(w) for w in self.win]
        if len(win) != nd:
            raise ValueError('NCC: win has %d entries, the images have %d spatial axes' % (len(win), nd))
        return win

    def _run(self, I, J, as_loss):
        I, J = _checked(I, 'NCC'), _checked(J, 'NCC')
        if I.shape != J.shape:
            raise ValueError('NCC: the images differ in shape: %s and %s' % (tuple(I.shape), tuple(J.shape)))
        nd = I.dim() - 2
        win = [1] * (3 - nd) + self._window(nd)
        if I.shape[-1] > _MAX_NCC_CHANNELS:
            raise NotImplementedError('NCC: up to %d channels, got %d' % (_MAX_NCC_CHANNELS, I.shape[-1]))
        _lib.require_device(I, J)
        return _NCCFn.apply(I.contiguous(), J.contiguous(), win, self.eps, as_loss)

    def ncc(self, I, J):
        """the map of local squared correlation coefficients, [B, *S, 1]"""
        return self._run(I, J, False)

    def loss(self, y_true, y_pred, reduce='mean'):
        """-mean(cc) over each batch entry, [B] (reduce='mean'); -cc, [B, *S, 1] (reduce=None)"""
        if reduce == 'mean':
            return self._run(y_true, y_pred, True)
        if reduce is None:
            return -self._run(y_true, y_pred, False)
        raise ValueError('NCC: unknown NCC reduction type: %r' % (reduce,))


class _GradLossFn(torch.autograd.Function):
    """y [B, *S, C] float32 contiguous -> loss [B]"""

    @staticmethod
    def forward(ctx, y, penalty, mult):
        dev = y.device
        batch, shape, nd, channels = _spatial3(y)
        loss = torch.empty((batch,), dtype=torch.float32, device=dev)
        nws = batch * 6144
        ws = _lib.workspace(dev, nws)
        _lib.call(dev, 'nrt_grad_loss_f32', _lib.ptr(y), batch, _lib.ints(shape), nd, channels, penalty, mult, _lib.ptr(loss), _lib.ptr(ws),
                  nws)
        ctx.save_for_backward(y)
        ctx.cfg = (batch, shape, nd, channels, penalty, mult)
        return loss

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        batch, shape, nd, channels, penalty, mult = ctx.cfg
        dev = y.device
        g = g.to(torch.float32).contiguous()
        gy = torch.empty_like(y)
        _lib.call(dev, 'nrt_grad_loss_bwd_f32', _lib.ptr(y), _lib.ptr(g), batch, _lib.ints(shape), nd, channels, penalty, mult,
                  _lib.ptr(gy))
        return gy, None, None


class Grad:
    """
    N-D gradient loss of a displacement field, vxm.losses.Grad restated: for each spatial axis the mean over everything but
    the batch of |d| ('l1') or d^2 ('l2') of the forward differences d, averaged over the axes, times loss_mult if given.  [B, *S, C]
    float32, 1 to 3 spatial axes -> [B].  An axis of extent 1 has no differences and gives NaN, as the mean of an empty tensor does.
    Differentiable in y_pred; captures into a graph.  vox_weight is not implemented.
    """

    def __init__(self, penalty='l1', loss_mult=None, vox_weight=None):
        if penalty not in ('l1', 'l2'):
            raise ValueError('Grad: penalty can only be l1 or l2. Got: %s' % (penalty,))
        if vox_weight is not None:
            raise NotImplementedError('Grad: vox_weight is not implemented')
        self.penalty = penalty
        self.loss_mult = loss_mult
        self.vox_weight = None

    def loss(self, _, y_pred):
        y = _checked(y_pred, 'Grad')
        _lib.require_device(y)
        mult = 1.0 if self.loss_mult is None else float(self.loss_mult)        # (times 1 changes no bit)
        return _GradLossFn.apply(y.contiguous(), 1 if self.penalty == 'l1' else 2, mult)


class NegJacobian:
    """
    Folding penalty on a displacement field: mean over each batch entry of max(0, -det), det the Jacobian determinant of
    utils.jacobian_determinant (csrc/jacobian.hip), times loss_mult if given.  [B, *S, D] (or [*S, D], a batch of one) float32,
    D = len(S) in {2, 3} -> [B].  An extension: VoxelMorph has the determinant (restated), not this penalty.
    Differentiable in y_pred (the sub-gradient at det == 0 is 0); one pass each way that writes no map; captures into a graph.
    """

    def __init__(self, loss_mult=None):
        self.loss_mult = loss_mult

    def loss(self, _, y_pred):
        disp, _ = utils._jacdet_checked(y_pred, 'NegJacobian')
        out = utils._JacDetFn.apply(disp, True)
        return out if self.loss_mult is None else out * float(self.loss_mult)


class SignedDistanceMSE:
    """
    Mean squared error between a predicted signed distance map and the signed distance transform of a foreground mask drawn from a
    label map (utils.signed_dist_trf on csrc/edt.hip, positive outside the foreground): what a SynthStrip-style network with a linear
    one-channel head regresses.  An extension, like NegJacobian: the definition is this project's, not SynthStrip's
    published loss.

        loss(ids, y_pred)        ids [B, *S] or [B, *S, 1] integer label ids, y_pred [B, *S, 1]
        loss(None, y_pred)       y_pred [B, *S, 2], SynthStrip's stacked output: channel 0 the prediction, channel 1 the ids as float

    target = signed distance (in units of voxel_size) to the set {ids in foreground}, clipped to +-max_dist when given; the result [B] is
    the mean over voxels of (pred - target)^2.  The target is formed on the device from the id map (no mask tensor, nothing on the host)
    and is a constant: the loss is differentiable in the prediction only.  With an empty or a full foreground the target is +-inf; give
    max_dist to keep such samples finite.
    """

    def __init__(self, foreground, max_dist=None, voxel_size=None):
        self.foreground = utils._edt_labels([foreground] if np.isscalar(foreground) else foreground, 'SignedDistanceMSE')
        if not 1 <= len(self.foreground) <= utils._EDT_MAX_LABELS:
            raise NotImplementedError('SignedDistanceMSE: 1 to %d foreground ids, got %d' % (utils._EDT_MAX_LABELS, len(self.foreground)))
        if max_dist is not None and not float(max_dist) > 0:
            raise ValueError('SignedDistanceMSE: max_dist must be positive, got %r' % (max_dist,))
        self.max_dist = None if max_dist is None else float(max_dist)
        self.voxel_size = voxel_size

    def target(self, ids):
        """the regression target [B, *S] of a label map [B, *S]"""
        with torch.no_grad():
            sdt = utils._label_dist_trf(ids, self.foreground, self.voxel_size, _lib.EDT_SIGNED, 'SignedDistanceMSE', any_of=True)[..., 0]
            return sdt if self.max_dist is None else sdt.clamp(-self.max_dist, self.max_dist)

    def loss(self, y_true, y_pred):
        what = 'SignedDistanceMSE'
        if not isinstance(y_pred, torch.Tensor):
            raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(y_pred).__name__))
        y_pred = materialize(y_pred)
        if not y_pred.dtype.is_floating_point:
            raise NotImplementedError('%s: a floating-point prediction, got %s' % (what, y_pred.dtype))
        if y_true is None:
            if y_pred.dim() < 3 or y_pred.shape[-1] != 2:
                raise ValueError('%s: without y_true, y_pred must be [batch, *spatial, 2] (prediction, ids), got shape %s'
                                 % (what, tuple(y_pred.shape)))
            pred, ids = y_pred[..., 0], y_pred[..., 1].detach().round().to(torch.int32)
        else:
            if not isinstance(y_true, torch.Tensor):
                raise TypeError('%s: expected a torch.Tensor, got %s' % (what, type(y_true).__name__))
            if y_pred.dim() < 3 or y_pred.shape[-1] != 1:
                raise ValueError('%s: y_pred must be [batch, *spatial, 1], got shape %s' % (what, tuple(y_pred.shape)))
            pred, ids = y_pred[..., 0], materialize(y_true)
            if ids.dim() == y_pred.dim():
                if ids.shape[-1] != 1:
                    raise ValueError('%s: y_true must be [batch, *spatial] or [batch, *spatial, 1], got shape %s' % (what, tuple(ids.shape)))
                ids = ids[..., 0]
            if ids.shape != pred.shape:
                raise ValueError('%s: y_true %s does not match y_pred %s' % (what, tuple(y_true.shape), tuple(y_pred.shape)))
        utils._edt_check_geometry(utils._edt_ids_checked(ids, what).shape, 1, what)
        _lib.require_device(pred, ids)
        target = self.target(ids)
        return ((pred.to(torch.float32) - target) ** 2).flatten(1).mean(1)
