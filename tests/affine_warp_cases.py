"""
TEST INFRASTRUCTURE ONLY -- the shapes and matrices of the affine-warp tests (tests/test_affine_warp_abi.py, tests/test_gpu_affine_warp.py)
and the float64 reference of the matrix gradient.  NumPy and CPU torch only; nothing here touches a device.
"""

import numpy as np
import torch

from oracle import grad_oracle as go
from oracle import np_oracle as no

F = np.float32

# (vol spatial, output spatial, batch, channel counts)
SHAPES = {
    # channels: 1, 3, 4 and 32 everywhere; 2 (the 8-byte rows) and 5 (one thread per channel, several per voxel) on one shape per rank
    '3d': ((12, 10, 9), (12, 10, 9), 2, (1, 2, 3, 4, 5, 32)),
    '3d_shape': ((12, 10, 9), (10, 11, 8), 2, (1, 3, 4, 32)),
    '2d': ((13, 11), (13, 11), 2, (1, 3, 4, 32)),
    '2d_shape': ((13, 11), (16, 9), 2, (1, 2, 3, 4, 5, 32)),
    '3d_blocks': ((33, 20, 17), (33, 20, 17), 1, (1,)),          # several blocks and a grid-stride tail
}
SHAPE_CHANNELS = [(name, C) for name, case in SHAPES.items() for C in case[3]]


def recipe_c(D, k):
    """eye + 0.05 N(0, 1), the translation column + 0.75 N(0, 1); float32"""
    rng = np.random.default_rng(100 + k)
    A = rng.standard_normal((D, D + 1)).astype(F)
    t = rng.standard_normal(D).astype(F)
    M = (np.eye(D, D + 1, dtype=F) + F(0.05) * A).astype(F)
    M[:, D] += F(0.75) * t
    return M


def matrices(D, B):
    """name -> [B, D, D + 1] (or [B, D + 1, D + 1]) float32"""
    eye = np.eye(D, D + 1, dtype=F)
    shift = eye.copy()
    shift[:, D] = np.array([2, -1, 3], F)[:D]
    c = np.stack([recipe_c(D, k) for k in range(B)], 0)
    square = np.concatenate([c, np.broadcast_to(np.eye(D + 1, dtype=F)[D:], (B, 1, D + 1))], 1)
    return {
        'identity': np.broadcast_to(eye, (B, D, D + 1)).copy(),
        'translation': np.broadcast_to(shift, (B, D, D + 1)).copy(),
        'c': c,
        'c_half': (c * F(0.5)).astype(F),
        'c_double': (c * F(2)).astype(F),
        'c_square': square.astype(F),
    }


def oob_fraction(M, S, O, shift_center=True):
    """share of the output voxels whose sampling location leaves the source volume (oracle.np_oracle, CPU)"""
    shift = no.affine_to_dense_shift(M, O, shift_center=shift_center)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=F) for n in O], indexing='ij'), -1)
    loc = grid + shift
    oob = np.zeros(loc.shape[:-1], bool)
    for d in range(len(S)):
        oob |= (loc[..., d] < 0) | (loc[..., d] > S[d] - 1)
    return float(oob.mean())


def assert_recipe_c_crosses_the_border(S, O, B):
    """between 5 % and 50 % of the output voxels of recipe (c) lie out of bounds: the clamp and the fill arm both run"""
    for k in range(B):
        f = oob_fraction(recipe_c(len(S), k), S, O)
        assert 0.05 <= f <= 0.50, 'recipe (c), seed %d, %s -> %s: %.3f of the voxels out of bounds' % (100 + k, S, O, f)


def volume(S, B, C, seed=7):
    return np.random.default_rng(seed).standard_normal((B,) + tuple(S) + (C,)).astype(F)


def matrix_gradient_f64(vol, shift32, w, fill_value, shift_center, single_transform):
    """
    d (sum out w) / d matrix in float64 at the float32 sampling locations the kernels use: shift32 [Bm, *O, D] is the device's own
    dense field, loc32 = float32(q) + shift32 (one float32 add), gloc comes from the gradient oracle at loc32, and
    grad[b][i][j] = sum_q gloc_i(q) p_j(q) with p = q - c, p_D = 1.  vol [B, *S, C], w [B, *O, C].  Returns [Bm, D, D + 1] float64.
    """
    B = vol.shape[0]
    O = shift32.shape[1:-1]
    D = len(O)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=F) for n in O], indexing='ij'), -1)
    c = np.array([(n - 1) / 2 if shift_center else 0.0 for n in O], np.float64)
    p = np.concatenate([grid.astype(np.float64) - c, np.ones(tuple(O) + (1,))], -1).reshape(-1, D + 1)
    grads = []
    for b in range(B):
        loc32 = (grid + shift32[0 if single_transform else b]).astype(F)
        loc = torch.tensor(loc32.astype(np.float64), requires_grad=True)
        out = go.interpn(torch.tensor(vol[b].astype(np.float64)), loc, fill_value)
        gloc, = torch.autograd.grad((out * torch.tensor(w[b].astype(np.float64))).sum(), loc)
        grads.append(gloc.reshape(-1, D).numpy().T @ p)
    g = np.stack(grads, 0)
    return g.sum(0, keepdims=True) if single_transform else g
