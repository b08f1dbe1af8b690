"""
The Jacobian determinant of a displacement field as the tests know it (csrc/jacobian.hip is compared against this file).  voxelmorph is
not in the reference tree, so `det_numpy` restates vxm.py.utils.jacobian_determinant: its expression copied as written, on
np.gradient, which IS runnable here -- the oracle is NumPy's own stencil.  float32 + an integer grid promotes to float64 there, so the
oracle is float64.

    det_numpy(disp)                 [*S, D] -> [*S] float64, the VoxelMorph expression on np.gradient(disp + grid)
    stencil(disp)                   torch, any dtype: G[a][c] = the np.gradient difference of disp[..., c] along spatial axis a
    det_torch(disp)                 torch restatement of the same stencil on [B, *S, D] (J = G + identity), for autograd
    neg_loss(disp)                  mean(max(0, -det)) per batch entry
    error_scale(disp)               sum over permutations pi of prod_a (|G[a][pi(a)]| + delta): the float32 error of det is at most
                                    12 * 2^-24 times this (2u per entry x 3 entries, + 2u for the multiplications, + 3u for the
                                    additions, rounded up).  |G| + delta, not |J|: an entry 1 + G cancels.
    grad_analytic(disp, w)          the gather formula of the backward: gdisp[q][c] = sum_a sum_p coef_a(p, q) w[p] cof[p][a][c]
    even_integer_field(shape, rng)  entries even integers in -6 .. 6: every G is an integer (or an even one at a border), det exact in float32
"""

import itertools

import numpy as np
import torch


def det_numpy(disp):
    """vxm.py.utils.jacobian_determinant: disp [*S, D], D = len(S) in {2, 3}; np.gradient raises ValueError for an extent below 2"""
    volshape = disp.shape[:-1]
    nb_dims = len(volshape)
    assert nb_dims in (2, 3) and disp.shape[-1] == nb_dims
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in volshape], indexing='ij'), len(volshape))
    J = np.gradient(disp + grid)
    if nb_dims == 3:
        dx, dy, dz = J[0], J[1], J[2]
        Jdet0 = dx[..., 0] * (dy[..., 1] * dz[..., 2] - dy[..., 2] * dz[..., 1])
        Jdet1 = dx[..., 1] * (dy[..., 0] * dz[..., 2] - dy[..., 2] * dz[..., 0])
        Jdet2 = dx[..., 2] * (dy[..., 0] * dz[..., 1] - dy[..., 1] * dz[..., 0])
        return Jdet0 - Jdet1 + Jdet2
    dfdx, dfdy = J[0], J[1]
    return dfdx[..., 0] * dfdy[..., 1] - dfdy[..., 0] * dfdx[..., 1]


def _diff_axis(f, ax):
    """np.gradient along axis `ax` of a torch tensor: central differences inside, one-sided first-order ones at both ends"""
    n = f.shape[ax]
    if n < 2:
        raise ValueError('an extent of at least 2 is required')
    first = f.narrow(ax, 1, 1) - f.narrow(ax, 0, 1)
    last = f.narrow(ax, n - 1, 1) - f.narrow(ax, n - 2, 1)
    if n == 2:
        return torch.cat([first, last], ax)
    mid = (f.narrow(ax, 2, n - 2) - f.narrow(ax, 0, n - 2)) * 0.5
    return torch.cat([first, mid, last], ax)


def stencil(disp):
    """disp [B, *S, D] -> G as a list over spatial axes a of [B, *S, D] tensors"""
    nd = disp.dim() - 2
    return [_diff_axis(disp, 1 + a) for a in range(nd)]


def _det_of(J):
    """J: list over a of [..., D]; the expansion in the VoxelMorph order"""
    if len(J) == 3:
        return (J[0][..., 0] * (J[1][..., 1] * J[2][..., 2] - J[1][..., 2] * J[2][..., 1])
                - J[0][..., 1] * (J[1][..., 0] * J[2][..., 2] - J[1][..., 2] * J[2][..., 0])
                + J[0][..., 2] * (J[1][..., 0] * J[2][..., 1] - J[1][..., 1] * J[2][..., 0]))
    return J[0][..., 0] * J[1][..., 1] - J[1][..., 0] * J[0][..., 1]


def jacobian(disp):
    nd = disp.dim() - 2
    assert nd in (2, 3) and disp.shape[-1] == nd
    eye = torch.eye(nd, dtype=disp.dtype)
    return [g + eye[a] for a, g in enumerate(stencil(disp))]


def det_torch(disp):
    """[B, *S, D] -> [B, *S], the dtype of disp"""
    return _det_of(jacobian(disp))


def neg_loss(disp):
    """mean(max(0, -det)) per batch entry; relu passes no gradient at det == 0 (clamp would)"""
    d = det_torch(disp)
    return torch.relu(-d).reshape(d.shape[0], -1).mean(1)


def error_scale(disp):
    """[B, *S, D] float64 -> [B, *S]"""
    nd = disp.dim() - 2
    eye = torch.eye(nd, dtype=disp.dtype)
    A = [g.abs() + eye[a] for a, g in enumerate(stencil(disp))]
    total = 0
    for pi in itertools.permutations(range(nd)):
        term = 1
        for a in range(nd):
            term = term * A[a][..., pi[a]]
        total = total + term
    return total


def cofactors(J):
    """cof[a][..., c] = d det / d J[a][c]"""
    if len(J) == 3:
        return [torch.linalg.cross(J[(a + 1) % 3], J[(a + 2) % 3], dim=-1) for a in range(3)]
    return [torch.stack([J[1][..., 1], -J[1][..., 0]], -1), torch.stack([-J[0][..., 1], J[0][..., 0]], -1)]


def grad_analytic(disp, w):
    """the backward kernel's formula, as a scatter from p (the transpose of the gather): disp [B, *S, D], w [B, *S] -> gdisp"""
    nd = disp.dim() - 2
    cof = cofactors(jacobian(disp))
    out = torch.zeros_like(disp)
    for a in range(nd):
        ax = 1 + a
        n = disp.shape[ax]
        t = w.unsqueeze(-1) * cof[a]                                     # what p sends along axis a, before the stencil weight
        for p in range(n):
            lo, hi = max(p - 1, 0), min(p + 1, n - 1)
            s = 0.5 if hi - lo == 2 else 1.0
            out.narrow(ax, hi, 1).add_(s * t.narrow(ax, p, 1))
            out.narrow(ax, lo, 1).sub_(s * t.narrow(ax, p, 1))
    return out


def even_integer_field(shape, rng):
    """[B, *S, D] float32 with entries in {-6, -4, .., 6}"""
    return (2 * rng.integers(-3, 4, shape)).astype(np.float32)
