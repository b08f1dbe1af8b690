"""
Restatement of voxelmorph's NCC and Grad losses (TEST INFRASTRUCTURE, no test of its own name: tests/test_vxm_losses_abi.py checks it
against itself, tests/test_gpu_vxm_losses.py checks the kernels of csrc/vxmloss.hip against it).

voxelmorph is not part of the reference tree, so these semantics are restated from the formulas of DESIGN 8, not recorded.  Tensors are
channels-last, [B, *S, C] with 1 to 3 spatial axes.

NCC(win, eps).  n = prod(win) C.  S_I, S_J, S_II, S_JJ, S_IJ are the sums of I, J, I I, J J, I J over the window and over all channels
(a ones filter [*win, C, 1], stride 1), zero padded as TensorFlow's 'SAME' pads: (w - 1) // 2 zeros in front, the rest behind.  Then
    uI = S_I / n, uJ = S_J / n
    cross = max(((S_IJ - uJ S_I) - uI S_J) + (uI uJ) n, eps)
    Ivar  = max((S_II - (2 uI) S_I) + (uI uI) n, eps)        (Jvar likewise)
    cc    = (cross / Ivar) (cross / Jvar)
and loss = -mean(cc) over each batch entry.  max passes its gradient where its first argument >= eps (torch.clamp does).
Grad(penalty, loss_mult).  d_i = y[.., 1:, ..] - y[.., :-1, ..]; m_i = the mean over everything but the batch of |d_i| ('l1') or d_i^2
('l2'); loss = ((m_0 + m_1) + m_2) / ndims (* loss_mult).

Box sums come from zero-padded slicing, one axis after the other, in torch (float64 unless said otherwise: differentiable).
"""

import numpy as np
import torch


def window_of(win, nd):
    if win is None:
        return [9] * nd
    if isinstance(win, int):
        return [win] * nd
    assert len(win) == nd
    return [int(w) for w in win]


def box_sum(x, win, mirrored=False):
    """x [B, *S] -> the zero-padded window sums, same shape.  mirrored: w - 1 - (w - 1) // 2 zeros in front (the transpose)"""
    for ax, w in enumerate(win, start=1):
        front = (w - 1) // 2
        if mirrored:
            front = w - 1 - front
        size = x.shape[ax]
        pad = [0, 0] * (x.dim() - 1 - ax) + [front, w - 1 - front]
        xp = torch.nn.functional.pad(x, pad)
        x = sum(xp.narrow(ax, k, size) for k in range(w))
    return x


def ncc_sums(I, J, win=None, absolute=False):
    """[B, *S, 5]: S_I, S_J, S_II, S_JJ, S_IJ; absolute: the sums of the magnitudes of the same terms (the scale of a rounding bound)"""
    win = window_of(win, I.dim() - 2)
    fields = (I, J, I * I, J * J, I * J)
    if absolute:
        fields = tuple(f.abs() for f in fields)
    return torch.stack([box_sum(f.sum(-1), win) for f in fields], -1)


def ncc_from_sums(S, n, eps):
    """the epilogue on torch tensors of any float type; returns cc and the unclamped (c0, vI0, vJ0) and clamped (cross, Ivar, Jvar)"""
    SI, SJ, SII, SJJ, SIJ = S.unbind(-1)
    uI, uJ = SI / n, SJ / n
    c0 = ((SIJ - uJ * SI) - uI * SJ) + (uI * uJ) * n
    vI0 = (SII - (2 * uI) * SI) + (uI * uI) * n
    vJ0 = (SJJ - (2 * uJ) * SJ) + (uJ * uJ) * n
    cross, Ivar, Jvar = c0.clamp(min=eps), vI0.clamp(min=eps), vJ0.clamp(min=eps)
    return (cross / Ivar) * (cross / Jvar), (c0, vI0, vJ0), (cross, Ivar, Jvar), (uI, uJ)


def ncc_map(I, J, win=None, eps=1e-5):
    """cc [B, *S, 1] in the dtype of I (float64 for the reference)"""
    win = window_of(win, I.dim() - 2)
    n = float(np.prod(win) * I.shape[-1])
    return ncc_from_sums(ncc_sums(I, J, win), n, eps)[0].unsqueeze(-1)


def ncc_loss(I, J, win=None, eps=1e-5):
    cc = ncc_map(I, J, win, eps)
    return -cc.reshape(cc.shape[0], -1).mean(1)


def ncc_epilogue32(sums, n, eps):
    """the float32 evaluation of the epilogue from given sums [.., 5], in the stated operation order, one rounding per operation"""
    S = np.asarray(sums, np.float32)
    n, eps, two = np.float32(n), np.float32(eps), np.float32(2)
    SI, SJ, SII, SJJ, SIJ = (S[..., k] for k in range(5))
    uI, uJ = SI / n, SJ / n
    cross = np.maximum(((SIJ - uJ * SI) - uI * SJ) + (uI * uJ) * n, eps)
    Ivar = np.maximum((SII - (two * uI) * SI) + (uI * uI) * n, eps)
    Jvar = np.maximum((SJJ - (two * uJ) * SJ) + (uJ * uJ) * n, eps)
    cc = (cross / Ivar) * (cross / Jvar)
    assert cc.dtype == np.float32
    return cc


def ncc_grad_analytic(I, J, g, win=None, eps=1e-5):
    """the backward's formula: g [B, *S] is the upstream gradient of cc.  Returns gI, gJ in the dtype of I."""
    win = window_of(win, I.dim() - 2)
    n = float(np.prod(win) * I.shape[-1])
    _, (c0, vI0, vJ0), (cross, Ivar, Jvar), (uI, uJ) = ncc_from_sums(ncc_sums(I, J, win), n, eps)
    zero = torch.zeros_like(g)
    A = torch.where(c0 >= eps, 2 * cross / (Ivar * Jvar) * g, zero)
    BJ = torch.where(vJ0 >= eps, -2 * cross ** 2 / (Ivar * Jvar ** 2) * g, zero)
    BI = torch.where(vI0 >= eps, -2 * cross ** 2 / (Ivar ** 2 * Jvar) * g, zero)

    def W(x):
        return box_sum(x, win, mirrored=True).unsqueeze(-1)

    gJ = I * W(A) - W(A * uI) + J * W(BJ) - W(BJ * uJ)
    gI = J * W(A) - W(A * uJ) + I * W(BI) - W(BI * uI)
    return gI, gJ


def grad_diffs(y):
    """the forward differences along each spatial axis of y [B, *S, C]"""
    return [y.narrow(ax, 1, y.shape[ax] - 1) - y.narrow(ax, 0, y.shape[ax] - 1) for ax in range(1, y.dim() - 1)]


def grad_loss(y, penalty='l1', loss_mult=None):
    """[B], in the dtype of y (float64 for the reference), differentiable"""
    means = []
    for d in grad_diffs(y):
        d = d.abs() if penalty == 'l1' else d * d
        means.append(d.reshape(d.shape[0], -1).mean(1))
    total = means[0]
    for m in means[1:]:
        total = total + m
    total = total / len(means)
    return total if loss_mult is None else total * loss_mult


def grad_loss32(y, penalty='l1', loss_mult=None):
    """the float32 evaluation: exact sums of the terms (float64, exact on small-integer fields), then float32(sum) / float32(count) per
    axis and the stated operation order, one float32 rounding per operation"""
    y = torch.as_tensor(y, dtype=torch.float64)
    nd = y.dim() - 2
    total = None
    for d in grad_diffs(y):
        d = d.abs() if penalty == 'l1' else d * d
        flat = d.reshape(d.shape[0], -1)
        m = flat.sum(1).numpy().astype(np.float32) / np.float32(flat.shape[1])
        total = m if total is None else total + m
    total = total / np.float32(nd)
    total = total * np.float32(1.0 if loss_mult is None else loss_mult)
    assert total.dtype == np.float32
    return total
