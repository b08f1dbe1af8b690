"""
CPU tests of utils.barycenter (no kernel is launched): the three entry points of csrc/barycenter.hip are declared, typed and exported and
refuse bad arguments before any launch; nrt_barycenter_workspace_bytes is 0 for a shape the calls refuse; utils.barycenter has the
reference's signature (by AST; the reference's side is recorded in tests/golden/barycenter_small.npz by
tests/golden/make_barycenter_golden.py), validates `axes` and refuses CPU tensors.
"""

import json
import os
import sys

import numpy as np
import pytest
import torch

import neurite_amd as ne
from neurite_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import ast_signatures as sigs          # noqa: E402

ENTRY_POINTS = ['nrt_barycenter', 'nrt_barycenter_bwd', 'nrt_barycenter_workspace_bytes']
F32, BF16, F16, F64, I32 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F16, _lib.DT_F64, _lib.DT_I32
D = 16                                             # a non-NULL "pointer"; nothing is launched on an argument error
BIG = 1 << 30


def _fwd(x=D, dtype=F32, outer=2, red=(5, 6), k=None, inner=3, y=D, sums=D, ws=D, nws=BIG, shape_null=False):
    k = len(red) if k is None else k
    shape = None if shape_null else _lib.ints(red)
    return _lib.lib().nrt_barycenter(x, dtype, outer, shape, k, inner, 1, 1, y, sums, ws, nws, None)


def _bwd(gy=D, y=D, sums=D, dtype=F32, outer=2, red=(5, 6), k=None, inner=3, gx=D, ws=D, nws=BIG, shape_null=False):
    k = len(red) if k is None else k
    shape = None if shape_null else _lib.ints(red)
    return _lib.lib().nrt_barycenter_bwd(gy, y, sums, dtype, outer, shape, k, inner, 1, 1, gx, ws, nws, None)


def _bytes(dtype=F32, outer=2, red=(5, 6), k=None, inner=3):
    k = len(red) if k is None else k
    return _lib.lib().nrt_barycenter_workspace_bytes(dtype, outer, _lib.ints(red), k, inner)


def test_entry_points_declared_typed_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in _lib._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_null_pointers_are_invalid_arguments():
    inv = _lib.NRT_ERR_INVALID_ARG
    for kw in ({'x': None}, {'y': None}, {'sums': None}, {'shape_null': True}):
        assert _fwd(**kw) == inv, kw
    for kw in ({'gy': None}, {'y': None}, {'sums': None}, {'gx': None}, {'shape_null': True}):
        assert _bwd(**kw) == inv, kw


def test_non_positive_sizes_and_k_out_of_range_are_invalid_arguments():
    inv = _lib.NRT_ERR_INVALID_ARG
    for kw in ({'outer': 0}, {'outer': -2}, {'inner': 0}, {'inner': -1}, {'red': (5, 0)}, {'red': (-5, 6)}, {'red': (5, 6), 'k': 0},
               {'red': (5, 6), 'k': -1}, {'red': (2,) * 9}, {'red': (2,) * 9, 'k': 100}):
        assert _fwd(**kw) == inv, kw
        assert _bwd(**kw) == inv, kw
        assert _bytes(**kw) == 0, kw
    assert _bytes(red=(2,) * 8) > 0                                 # k = 8 itself is in range


def test_other_dtypes_and_size_limits_are_unsupported():
    unsup = _lib.NRT_ERR_UNSUPPORTED
    for kw in ({'dtype': F64}, {'dtype': I32}, {'dtype': 7}, {'dtype': -1},
               {'red': (1 << 24,), 'outer': 1, 'inner': 1},                      # coordinates stop being exact in float32
               {'red': (2, 1 << 24), 'outer': 1, 'inner': 1},
               {'red': (1 << 15, 1 << 15), 'outer': 2, 'inner': 1},              # outer * R * inner = 2^31
               {'red': (1 << 10, 1 << 10), 'outer': 1 << 10, 'inner': 2},
               {'red': (46341, 46341), 'outer': 1, 'inner': 1},
               {'red': (3,), 'outer': 1 << 31, 'inner': 1},
               {'red': (3,), 'outer': 1, 'inner': 1 << 40}):
        assert _fwd(**kw) == unsup, kw
        assert _bwd(**kw) == unsup, kw
        assert _bytes(**kw) == 0, kw
    # just inside the limits: the workspace size is reported (nothing is launched by asking)
    assert _bytes(red=((1 << 24) - 1,), outer=1, inner=1) > 0
    assert _bytes(red=(1 << 15, 1 << 15), outer=1, inner=1) > 0


def test_missing_or_short_workspace_is_refused():
    ws = _lib.NRT_ERR_WORKSPACE
    for dtype in (F32, BF16, F16):
        need = _bytes(dtype=dtype)
        assert need > 0
        assert _fwd(dtype=dtype, ws=None, nws=0) == ws
        assert _fwd(dtype=dtype, ws=None, nws=BIG) == ws
        assert _fwd(dtype=dtype, ws=256, nws=4) == ws
        assert _bwd(dtype=dtype, ws=None, nws=0) == ws
        assert _bwd(dtype=dtype, ws=256, nws=4) == ws


def test_workspace_covers_partials_and_gradient_coefficients():
    # at least one [k + 1] row of float32 per output (the backward's coefficients; one slab of partials)
    for red, outer, inner in (((5, 6), 2, 3), ((160, 160, 160), 4, 32), ((70001,), 4, 1), ((2,) * 8, 3, 5)):
        assert _bytes(red=red, outer=outer, inner=inner) >= outer * inner * (len(red) + 1) * 4
    # a long reduction is cut into slabs: more than one partial per output
    assert _bytes(red=(160, 160, 160), outer=1, inner=32) >= 2 * 32 * 4 * 4


def test_signature_equals_the_reference():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'barycenter_small.npz'), allow_pickle=False) as z:
        want = json.loads(str(z['__signature__']))
    here = sigs.signature(os.path.join(ROOT, 'neurite_amd', 'utils.py'), 'barycenter')
    assert want['defaults'][-1] == 'tf.float32' and here['defaults'][-1] == 'torch.float32'
    here['defaults'][-1] = here['defaults'][-1].replace('torch.', 'tf.')
    assert here == want
    assert 'barycenter' in ne.utils.__all__


def test_axes_validation_raises_value_error():
    x = torch.zeros(2, 3, 4, 5)
    for axes in ((1, 1), (1, -3), (4,), (-5,), (0, 1, 2, 3, 0), 4, -5, (1.0,), ()):
        with pytest.raises(ValueError):
            ne.utils.barycenter(x, axes=axes)
    with pytest.raises(ValueError):
        ne.utils.barycenter(torch.zeros(()))


def test_cpu_tensors_are_refused():
    x = torch.ones(2, 3, 4, 5)
    for axes in (None, (1, 2), -1, (3, 1)):
        with pytest.raises(_lib.NeuriteAmdError, match='no CPU fallback'):
            ne.utils.barycenter(x, axes=axes)
    with pytest.raises(_lib.NeuriteAmdError, match='no CPU fallback'):
        ne.utils.barycenter(x.to(torch.int32), axes=(1, 2), normalize=True, shift_center=True, dtype=torch.float64)
