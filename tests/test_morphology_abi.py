"""
CPU tests of the binary morphology, the box minimum / maximum filters and the box rank filters (no kernel is launched): the entry
points of csrc/morph.hip are declared, typed and exported; every invalid argument is refused with NRT_ERR_INVALID_ARG and every limit
with NRT_ERR_UNSUPPORTED before any launch, the workspace check coming last; the Python functions (neurite_amd.utils) validate on the
host -- ValueError for a malformed argument (an even size, a bad structure shape), NotImplementedError for a stated limit, naming it
(more than 27 samples, iterations < 1, a last axis beyond 1024, 'wrap') -- before they refuse a CPU tensor.
"""

import ctypes as C

import numpy as np
import pytest
import torch

ENTRY_POINTS = ['nrt_binary_morph_workspace_bytes', 'nrt_binary_morph', 'nrt_minmax_filter_workspace_bytes', 'nrt_minmax_filter',
                'nrt_rank_filter']
FUNCTIONS = ['binary_erosion', 'binary_dilation', 'binary_opening', 'binary_closing', 'minimum_filter', 'maximum_filter', 'grey_erosion',
             'grey_dilation', 'grey_opening', 'grey_closing', 'median_filter', 'rank_filter', 'percentile_filter']
D = 16                                             # a non-NULL, 16-byte aligned "pointer"; nothing is launched on an argument error
BIG = 1 << 40
CONN1 = sum(1 << i for i in (4, 10, 12, 13, 14, 16, 22))


def _L():
    from neurite_amd import _lib
    return _lib


def _u():
    import neurite_amd as ne
    return ne.utils


def _binary(x=D, dtype=5, batch=2, shape=(5, 6, 7), nd=None, structure=CONN1, iterations=1, border=0, dilate=0, out=D, ws=D, nws=BIG,
            shape_null=False):
    L = _L()
    return L.lib().nrt_binary_morph(x, dtype, batch, None if shape_null else L.ints(shape), len(shape) if nd is None else nd, structure,
                                    iterations, border, dilate, out, ws, nws, None)


def _minmax(x=D, dtype=0, batch=2, shape=(5, 6, 7), nd=None, size=(3, 3, 3), mode=0, cval=0.0, want_max=0, out=D, ws=D, nws=BIG,
            size_null=False):
    L = _L()
    return L.lib().nrt_minmax_filter(x, dtype, batch, L.ints(shape), len(shape) if nd is None else nd, None if size_null else L.ints(size),
                                     mode, cval, want_max, out, ws, nws, None)


def _rank(x=D, dtype=0, batch=2, shape=(5, 6, 7), nd=None, size=(3, 3, 3), rank=13, mode=0, cval=0.0, out=D):
    L = _L()
    return L.lib().nrt_rank_filter(x, dtype, batch, L.ints(shape), len(shape) if nd is None else nd, L.ints(size), rank, mode, cval, out,
                                   None)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name
    sigs = L.signatures()
    ip, vp, i = C.POINTER(C.c_int), C.c_void_p, C.c_int
    assert sigs['nrt_binary_morph'] == (i, [vp, i, i, ip, i, i, i, i, i, vp, vp, C.c_size_t, vp],
                                        ['x', 'dtype', 'batch', 'shape', 'nd', 'structure', 'iterations', 'border_value', 'dilate', 'out',
                                         'workspace', 'workspace_bytes', 'stream'])
    assert sigs['nrt_minmax_filter'] == (i, [vp, i, i, ip, i, ip, i, C.c_double, i, vp, vp, C.c_size_t, vp],
                                         ['x', 'dtype', 'batch', 'shape', 'nd', 'size', 'mode', 'cval', 'want_max', 'out', 'workspace',
                                          'workspace_bytes', 'stream'])
    assert sigs['nrt_rank_filter'] == (i, [vp, i, i, ip, i, ip, i, i, C.c_double, vp, vp],
                                       ['x', 'dtype', 'batch', 'shape', 'nd', 'size', 'rank', 'mode', 'cval', 'out', 'stream'])
    assert sigs['nrt_binary_morph_workspace_bytes'] == (C.c_size_t, [i, ip, i, i], ['batch', 'shape', 'nd', 'iterations'])
    assert sigs['nrt_minmax_filter_workspace_bytes'] == (C.c_size_t, [i, ip, i, ip], ['batch', 'shape', 'nd', 'size'])
    assert (L.DT_F32, L.DT_I32, L.DT_U8) == (0, 4, 5)
    u = _u()
    assert all(name in u.__all__ and callable(getattr(u, name)) for name in FUNCTIONS)


def test_workspace_sizes():
    L = _L()
    lib = L.lib()
    shape = L.ints((5, 6, 7))
    assert [lib.nrt_binary_morph_workspace_bytes(2, shape, 3, n) for n in (1, 4, 5, 9)] == [0, 0, 420, 420]
    assert lib.nrt_minmax_filter_workspace_bytes(2, shape, 3, L.ints((3, 1, 1))) == 0
    assert lib.nrt_minmax_filter_workspace_bytes(2, shape, 3, L.ints((3, 1, 5))) == 4 * 420
    assert lib.nrt_binary_morph_workspace_bytes(2, shape, 4, 9) == 0 and lib.nrt_binary_morph_workspace_bytes(0, shape, 3, 9) == 0


def test_invalid_arguments_are_refused_before_any_launch():
    L = _L()
    inv = L.NRT_ERR_INVALID_ARG
    for kw in ({'x': None}, {'out': None}, {'shape_null': True}, {'dtype': 1}, {'dtype': 3}, {'dtype': -1}, {'dtype': 6}, {'batch': 0},
               {'shape': (5, 0, 7)}, {'shape': (5, 6, 7, 8)}, {'nd': 1}, {'nd': 4}, {'structure': -1}, {'structure': 1 << 27},
               {'shape': (6, 7), 'structure': CONN1}, {'iterations': 0}, {'iterations': -2}, {'border': 2}, {'border': -1}, {'dilate': 2}):
        assert _binary(**kw) == inv, kw
        if 'iterations' not in kw:
            assert _binary(iterations=9, ws=None, nws=0, **kw) == inv, kw                # an argument error wins over the workspace
    assert _binary(shape=(6, 7), structure=0x1FF << 9, iterations=9, ws=None, nws=0) == L.NRT_ERR_WORKSPACE       # a 2-D structure is fine
    assert _binary(batch=65536, iterations=0) == inv                                    # an argument error wins over a limit
    for call, extra in ((_minmax, ({'want_max': 2}, {'size_null': True}, {'size': (3, 3, 33), 'mode': 9})),
                        (_rank, ({'rank': -1}, {'rank': 27}, {'size': (1, 3, 3), 'rank': 9}))):
        for kw in ({'x': None}, {'out': None}, {'dtype': 5}, {'dtype': 1}, {'batch': 0}, {'shape': (5, 6, -7)}, {'nd': 4}, {'size': (3, 2, 3)},
                   {'size': (3, 0, 3)}, {'size': (3, -1, 3)}, {'mode': 4}, {'mode': -1}, {'cval': float('nan')},
                   {'dtype': 4, 'cval': 3e9}) + extra:
            assert call(**kw) == inv, (call.__name__, kw)


def test_limits_are_unsupported_and_the_workspace_comes_last():
    L = _L()
    uns, wsp = L.NRT_ERR_UNSUPPORTED, L.NRT_ERR_WORKSPACE
    assert _binary(shape=(2, 2, 1025)) == uns and _binary(shape=(2, 1025), structure=0x1FF << 9) == uns and _binary(shape=(2, 1025), iterations=0) != uns
    assert _binary(batch=65536) == uns and _binary(shape=(2048, 1024, 1024)) == uns and _binary(batch=1024, shape=(2, 1024, 1024)) == uns
    assert _binary(shape=(524281, 2, 2)) == uns and _binary(shape=(524280, 2, 2), iterations=5, ws=None, nws=0) == wsp
    assert _binary(iterations=5, ws=None, nws=0) == wsp and _binary(iterations=5, nws=419) == wsp
    assert _binary(iterations=5, shape=(2, 2, 1025), ws=None, nws=0) == uns              # a limit wins over the workspace
    assert _minmax(size=(3, 3, 33)) == uns and _minmax(batch=65536) == uns and _minmax(shape=(1 << 11, 1 << 10, 1 << 10)) == uns
    assert _minmax(ws=None, nws=0) == wsp and _minmax(nws=4 * 420 - 1) == wsp and _minmax(ws=18) == wsp
    assert _minmax(size=(3, 3, 33), ws=None, nws=0) == uns
    assert _rank(size=(3, 3, 5), rank=0) == uns and _rank(size=(1, 1, 29), rank=0) == uns and _rank(batch=65536) == uns


def _x(shape=(5, 6, 7), dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def test_python_argument_errors():
    u = _u()
    L = _L()
    for fn in (u.minimum_filter, u.maximum_filter, u.grey_erosion, u.grey_dilation, u.grey_opening, u.grey_closing, u.median_filter):
        for size in (2, (3, 4, 3), 0, (3, 3), 3.0, True, (3, -1, 3)):
            with pytest.raises(ValueError, match='size'):
                fn(_x(), size=size)
        with pytest.raises(NotImplementedError, match='wrap'):
            fn(_x(), mode='wrap')
        with pytest.raises(ValueError, match='mode'):
            fn(_x(), mode='grid-wrap')
        with pytest.raises(ValueError, match='cval'):
            fn(_x(), mode='constant', cval=float('nan'))
        with pytest.raises(NotImplementedError, match='float32 / int32'):
            fn(_x(dtype=torch.float64))
        with pytest.raises(NotImplementedError, match='2 or 3 spatial axes'):
            fn(_x((7,)))
        with pytest.raises(NotImplementedError, match='2 or 3 spatial axes'):
            fn(_x((2, 3, 4, 5, 6)), batched=True)
        with pytest.raises(ValueError, match='empty'):
            fn(_x((5, 0, 7)))
        with pytest.raises(L.NeuriteAmdError, match='CPU fallback'):                     # every check passed: only the device is missing
            fn(_x())
    with pytest.raises(NotImplementedError, match='31'):
        u.minimum_filter(_x(), size=33)
    for size in (5, (3, 3, 5), (1, 1, 29)):
        with pytest.raises(NotImplementedError, match='27 samples'):
            u.median_filter(_x(), size=size)
        with pytest.raises(NotImplementedError, match='27 samples'):
            u.rank_filter(_x(), 0, size=size)
        with pytest.raises(NotImplementedError, match='27 samples'):
            u.percentile_filter(_x(), 50, size=size)
    for rank in (27, -28, 1.0, True):
        with pytest.raises(ValueError, match='rank'):
            u.rank_filter(_x(), rank)
    for p in (101, -100.5, 'x'):
        with pytest.raises(ValueError, match='percentile'):
            u.percentile_filter(_x(), p)
    with pytest.raises(L.NeuriteAmdError, match='CPU fallback'):
        u.rank_filter(_x(), -27, size=3)
    with pytest.raises(L.NeuriteAmdError, match='CPU fallback'):
        u.percentile_filter(_x(dtype=torch.int32), -100, size=(1, 5, 5))


def test_python_argument_errors_binary():
    u = _u()
    L = _L()
    for fn in (u.binary_erosion, u.binary_dilation, u.binary_opening, u.binary_closing):
        for n in (0, -1):
            with pytest.raises(NotImplementedError, match='iterations'):
                fn(_x(), iterations=n)
        with pytest.raises(ValueError, match='iterations'):
            fn(_x(), iterations=1.5)
        for structure in (np.ones((3, 3)), np.ones((3, 3, 5)), np.ones(27), 0, 4, True, 'cross'):
            with pytest.raises(ValueError, match='structure|connectivity'):
                fn(_x(), structure)
        with pytest.raises(ValueError, match='connectivity'):
            fn(_x((6, 7)), 3)
        for border in (2, -1, 0.5, None):
            with pytest.raises(ValueError, match='border_value'):
                fn(_x(), border_value=border)
        with pytest.raises(NotImplementedError, match='1024'):
            fn(_x((2, 2, 1025), torch.bool))
        with pytest.raises(NotImplementedError, match='1024'):
            fn(_x((2, 2, 1025), torch.uint8), batched=True)
        with pytest.raises(NotImplementedError, match='524280'):
            fn(_x((524281, 2, 2), torch.bool))
        with pytest.raises(NotImplementedError, match='bool / uint8 / int32 / float32'):
            fn(_x(dtype=torch.int64))
        with pytest.raises(NotImplementedError, match='2 or 3 spatial axes'):
            fn(_x((7,)))
        with pytest.raises(ValueError, match='radius'):
            fn(_x(), 'ball')
        with pytest.raises(ValueError, match='radius'):
            fn(_x(), 2, radius=1.0)
        with pytest.raises(NotImplementedError, match='ball'):
            fn(_x(), 'ball', radius=2, iterations=2)
        with pytest.raises(NotImplementedError, match='ball'):
            fn(_x(), 'ball', radius=2, border_value=1)
        for ok in (dict(), dict(structure=3, iterations=9, border_value=1), dict(structure=np.eye(3)[None].repeat(3, 0)),
                   dict(structure='ball', radius=1.5)):
            with pytest.raises(L.NeuriteAmdError, match='CPU fallback'):
                fn(_x(dtype=torch.bool), **ok)
        with pytest.raises(L.NeuriteAmdError, match='CPU fallback'):
            fn(_x((1, 1024), torch.int32), np.ones((3, 3)))
