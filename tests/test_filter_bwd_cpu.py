"""
CPU tests of the backward of the separable filter family (no kernel is launched): the NumPy restatements of
tests/filter_bwd_restatement.py against torch float64 autograd, and the C ABI of the new entry points (declared, typed, exported,
refusing bad arguments before any launch).

The autograd target of a pass is F.conv1d on a row padded explicitly by the TF rules (SAME puts total // 2 of the padding in front),
so the padding convention is checked too, not restated.
"""

import numpy as np
import torch
import torch.nn.functional as TF

import filter_bwd_restatement as R
from neurite_amd import _lib

F = np.float32

ENTRY_POINTS = ['nrt_conv1d_axis_bwd_f32', 'nrt_conv1d_axis_bwd_kernel_workspace_bytes', 'nrt_conv1d_axis_bwd_kernel_f32',
                'nrt_minmax_norm_bwd_workspace_bytes', 'nrt_minmax_norm_bwd_f32', 'nrt_synth_axis_gather_bwd_f32']


def conv_autograd(x, k, g, n, W, stride, dil, padding):
    """(dx, dk) of sum(g * conv(x, k)) by torch float64 autograd; x [outer, n, inner]"""
    outer, _, inner = x.shape
    ke = (W - 1) * dil + 1
    if padding == 'SAME':
        o = -(-n // stride)
        total = max((o - 1) * stride + ke - n, 0)
        front, back = total // 2, total - total // 2
    else:
        front = back = 0
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    kt = torch.tensor(k, dtype=torch.float64, requires_grad=True)
    rows = xt.permute(0, 2, 1).reshape(outer * inner, 1, n)
    rows = TF.pad(rows, (front, back))
    y = TF.conv1d(rows, kt.reshape(1, 1, W), stride=stride, dilation=dil)       # cross-correlation, as tf.nn.convolution
    y = y.reshape(outer, inner, -1).permute(0, 2, 1)
    (y * torch.tensor(g, dtype=torch.float64)).sum().backward()
    return xt.grad.numpy(), kt.grad.numpy(), y.shape[1]


def test_conv_restatements_against_autograd():
    rng = np.random.default_rng(11)
    outer, inner = 2, 3
    worst = 0.0
    cases = 0
    for n in (5, 8, 13):
        for W in (1, 2, 3, 4, 7):                               # even widths: asymmetric padding; W = 7 > n = 5
            for stride in (1, 2, 3):
                for dil in (1, 2):
                    for padding in ('SAME', 'VALID'):
                        geo = R.geometry(n, W, stride, dil, padding)
                        if geo is None:
                            continue
                        Aout, pad = geo
                        x = rng.standard_normal((outer, n, inner))
                        k = rng.standard_normal(W)
                        g = rng.standard_normal((outer, Aout, inner))
                        dx_want, dk_want, o = conv_autograd(x, k, g, n, W, stride, dil, padding)
                        assert o == Aout
                        dx, S = R.conv_dx_ref64(g, k, outer, n, inner, Aout, stride, dil, pad)
                        dk, Sk = R.conv_dk_ref64(x, g, W, outer, n, inner, Aout, stride, dil, pad)
                        what = (n, W, stride, dil, padding)
                        assert np.abs(dx - dx_want).max() <= 1e-12, what
                        assert np.abs(dk - dk_want).max() <= 1e-12, what
                        worst = max(worst, float(np.abs(dx - dx_want).max()), float(np.abs(dk - dk_want).max()))
                        # the float32 restatement within the bound the kernels are held to
                        g32, k32 = g.astype(F), k.astype(F)
                        r64, S32 = R.conv_dx_ref64(g32, k32, outer, n, inner, Aout, stride, dil, pad)
                        r32 = R.conv_dx_ref32(g32, k32, outer, n, inner, Aout, stride, dil, pad)
                        assert r32.dtype == F
                        assert (np.abs(r32.astype(np.float64) - r64) <= R.gamma(W + 1) * S32 + R.ulp32(r64) / 2).all(), what
                        cases += 1
    print('%d cases, largest difference from autograd %.3g' % (cases, worst))
    assert cases > 150


def test_conv_width_larger_than_axis_is_covered():
    assert R.geometry(5, 7, 1, 2, 'SAME') == (5, 6) and R.geometry(5, 7, 1, 1, 'VALID') is None


def test_stride1_dx_is_the_forward_with_reversed_taps():
    """the identity nrt_conv1d_axis_bwd_f32 relies on for stride 1, bit for bit in float32: forward contract over g with the taps
    reversed, pad' = (W - 1) dil - pad, out_len = axis_len"""
    rng = np.random.default_rng(3)
    for n, W, dil, padding in ((13, 4, 1, 'SAME'), (13, 7, 2, 'SAME'), (9, 3, 2, 'VALID'), (5, 7, 1, 'SAME')):
        Aout, pad = R.geometry(n, W, 1, dil, padding)
        g = rng.standard_normal((2, Aout, 3)).astype(F)
        k = rng.standard_normal(W).astype(F)
        want = R.conv_dx_ref32(g, k, 2, n, 3, Aout, 1, dil, pad)
        kr, padr = k[::-1], (W - 1) * dil - pad
        fwd = np.zeros((2, n, 3), F)
        for t in range(W):                                      # ascending reversed taps = descending taps
            for a in range(n):
                ai = a + t * dil - padr
                if 0 <= ai < Aout:
                    fwd[:, a] = fwd[:, a] + kr[t] * g[:, ai]
        assert (fwd.view(np.uint32) == want.view(np.uint32)).all(), (n, W, dil, padding)


def test_minmax_formula_against_autograd():
    rng = np.random.default_rng(5)
    outer, Rn, inner = 3, 17, 2
    x = rng.standard_normal((outer, Rn, inner)).astype(F)
    x[0, 3, 0] = x[0, 9, 0] = x[0, :, 0].min() - 1               # a tie of the minimum
    x[0, 5, 1] = x[0, 6, 1] = x[0, 7, 1] = x[0, :, 1].max() + 1 # a three-way tie of the maximum
    x[1, :, 0] = 2.5                                            # a constant group
    x[2, :, 1] = np.abs(x[2, :, 1])
    x[2, 4, 1], x[2, 11, 1] = -0.0, 0.0                         # -0 ties with +0 at the minimum
    g = rng.standard_normal((outer, Rn, inner))
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    mn, mx = xt.amin(1, keepdim=True), xt.amax(1, keepdim=True)
    den = mx - mn
    y = torch.where(den != 0, (xt - mn) / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(xt))
    (y * torch.tensor(g)).sum().backward()
    dx, info = R.minmax_bwd_ref64(x, g, outer, Rn, inner)
    assert np.abs(dx - xt.grad.numpy()).max() <= 1e-12
    assert (dx[1, :, 0] == 0).all() and int(info['nmin'][2, 0, 1]) == 2 and int(info['nmax'][0, 0, 1]) == 3 and int(info['nmin'][0, 0, 0]) == 2


def test_segmented_sum_against_autograd():
    rng = np.random.default_rng(7)
    outer, A, inner = 2, 9, 3
    for index in ([0, 0, 0, 2, 2, 5, 8, 8], [1, 4, 7], list(range(9))):
        g = rng.standard_normal((outer, len(index), inner)).astype(F)
        xt = torch.zeros((outer, A, inner), dtype=torch.float64, requires_grad=True)
        (xt.index_select(1, torch.tensor(index)) * torch.tensor(g.astype(np.float64))).sum().backward()
        got = R.gather_bwd_ref32(g, index, outer, A, inner)
        assert got.dtype == F
        # a run holds at most 3 terms: two rounded additions
        assert np.abs(got.astype(np.float64) - xt.grad.numpy()).max() <= 3 * R.U * np.abs(g).sum(1).max()
        rs = R.run_starts(index, A)
        assert rs[0] == 0 and rs[-1] == len(index) and all((np.asarray(index)[rs[a]:rs[a + 1]] == a).all() for a in range(A))
        assert sum(rs[a + 1] - rs[a] for a in range(A)) == len(index)


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------------

def test_entry_points_declared_typed_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in _lib._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_entry_points_refuse_before_any_launch():
    lib = _lib.lib()
    d = 64                                          # a non-NULL, 8-byte aligned "pointer"; nothing is launched on an argument error
    inv, wsp, unsup = _lib.NRT_ERR_INVALID_ARG, _lib.NRT_ERR_WORKSPACE, _lib.NRT_ERR_UNSUPPORTED
    big = 1 << 30
    # (grad_y, kernel, grad_x, outer, axis_len, inner, out_len, width, stride, dilation, pad_before, stream)
    for ptrs in ((None, d, d), (d, None, d), (d, d, None)):
        assert lib.nrt_conv1d_axis_bwd_f32(*ptrs, 2, 8, 3, 4, 3, 2, 1, 0, None) == inv
    for stride, dil, width in ((0, 1, 3), (-1, 1, 3), (2, 0, 3), (2, 1, 0)):
        assert lib.nrt_conv1d_axis_bwd_f32(d, d, d, 2, 8, 3, 4, width, stride, dil, 0, None) == inv
        assert lib.nrt_conv1d_axis_bwd_kernel_f32(d, d, d, 2, 8, 3, 4, width, stride, dil, 0, d, big, None) == inv
    assert lib.nrt_conv1d_axis_bwd_f32(d, d, d, 0, 8, 3, 4, 3, 2, 1, 0, None) == _lib.NRT_OK            # nothing to do
    # (x, grad_y, grad_kernel, ...geometry..., workspace, workspace_bytes, stream)
    for ptrs in ((None, d, d), (d, None, d), (d, d, None)):
        assert lib.nrt_conv1d_axis_bwd_kernel_f32(*ptrs, 2, 8, 3, 4, 3, 2, 1, 0, d, big, None) == inv
    need = lib.nrt_conv1d_axis_bwd_kernel_workspace_bytes(2, 4, 3, 19)
    assert need == 24 * 8                           # one block, 19 taps padded to 24, float64
    # 4 x 160^3 outputs = 4000 runs of 256 x 16: above the cap of 1024 blocks, so 4 runs per block, 1000 blocks
    assert lib.nrt_conv1d_axis_bwd_kernel_workspace_bytes(4, 160, 160 * 160, 19) == 1000 * 24 * 8
    assert lib.nrt_conv1d_axis_bwd_kernel_f32(d, d, d, 2, 8, 3, 4, 19, 2, 1, 0, None, 0, None) == wsp
    assert lib.nrt_conv1d_axis_bwd_kernel_f32(d, d, d, 2, 8, 3, 4, 19, 2, 1, 0, d, need - 1, None) == wsp
    # (x, grad_y, grad_x, outer, reduce_len, inner, workspace, workspace_bytes, stream)
    for ptrs in ((None, d, d), (d, None, d), (d, d, None)):
        assert lib.nrt_minmax_norm_bwd_f32(*ptrs, 2, 100, 3, d, big, None) == inv
    assert lib.nrt_minmax_norm_bwd_f32(d, d, d, 2, 100, 0, d, big, None) == inv
    assert lib.nrt_minmax_norm_bwd_f32(d, d, d, 2, 100, 1025, d, big, None) == unsup                   # the forward's limits
    assert lib.nrt_minmax_norm_bwd_f32(d, d, d, 65536, 100, 1, d, big, None) == unsup
    for inner in (1, 3):
        need = lib.nrt_minmax_norm_bwd_workspace_bytes(2, 100, inner)
        assert need >= lib.nrt_minmax_workspace_bytes(2, inner) + 2 * inner * 24
        assert lib.nrt_minmax_norm_bwd_f32(d, d, d, 2, 100, inner, None, 0, None) == wsp
        assert lib.nrt_minmax_norm_bwd_f32(d, d, d, 2, 100, inner, d, need - 1, None) == wsp
    assert lib.nrt_minmax_norm_bwd_f32(d, d, d, 0, 100, 1, None, 0, None) == _lib.NRT_OK
    # (grad_y, run_start, grad_x, outer, axis_len, out_len, inner, stream)
    for ptrs in ((None, d, d), (d, None, d), (d, d, None)):
        assert lib.nrt_synth_axis_gather_bwd_f32(*ptrs, 2, 8, 5, 3, None) == inv
    assert lib.nrt_synth_axis_gather_bwd_f32(d, d, d, 2, 0, 5, 3, None) == inv
    assert lib.nrt_synth_axis_gather_bwd_f32(d, d, d, 2, 8, 5, 0, None) == inv
