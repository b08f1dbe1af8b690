"""
CPU tests of what design_dnn / EncoderNet add below the builders (no kernel is launched): the entry points of csrc/globalmax.hip and
the pad-before convolution are declared, typed and exported and refuse bad arguments before any launch; the global-max workspace is
monotone in V; bf16 networks with the new layers are refused on CPU tensors; layers.RescaleValues / layers.Negate have the
reference's constructor and get_config() (neurite/tf/layers.py:49-88).
"""

import contextlib
import ctypes as C
import io

import pytest
import torch

import neurite_amd as ne
from neurite_amd import _lib
from neurite_amd import layers as L
from neurite_amd import models

_vp, _i, _ll, _f, _sz = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_size_t
_ip = C.POINTER(C.c_int)
ENTRY_POINTS = {
    'nrt_global_max_workspace_bytes': (_sz, [_i, _ll, _i]),
    'nrt_global_max_f32': (_i, [_vp, _i, _ll, _i, _vp, _vp, _vp, _sz, _vp]),
    'nrt_global_max_bwd_f32': (_i, [_vp, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _sz, _vp]),
    'nrt_maxnorm_f32': (_i, [_vp, _i, _ll, _f, _f, _vp]),
    'nrt_conv3d_pad_f32': (_i, [_vp, _i, _vp, _i, _ip, _vp, _vp, _vp, _vp, _i, _ip, _ip, _i, _i, _ip, _i, _i, _vp]),
    'nrt_hyperconv3d_pad_f32': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _ip, _ip, _i, _i, _ip, _i, _i, _vp]),
}
INV, UNSUP, WS = _lib.NRT_ERR_INVALID_ARG, _lib.NRT_ERR_UNSUPPORTED, _lib.NRT_ERR_WORKSPACE


def _quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*args, **kwargs)


def test_entry_points_declared_typed_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name, (res, args) in ENTRY_POINTS.items():
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name
        assert _lib._SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_global_max_refuses_before_any_launch():
    lib = _lib.lib()
    d, big = 16, 1 << 30                            # a non-NULL "pointer"; nothing is launched on an argument error
    # forward: (x, batch, v, channels, y, count, workspace, workspace_bytes, stream)
    assert lib.nrt_global_max_f32(None, 2, 8, 4, d, d, d, big, None) == INV
    assert lib.nrt_global_max_f32(d, 2, 8, 4, None, d, d, big, None) == INV
    assert lib.nrt_global_max_f32(d, 2, 8, 4, d, None, d, big, None) == INV
    # backward: (x, y, count, g, batch, v, channels, gx, workspace, workspace_bytes, stream)
    for k in range(4):
        a = [d, d, d, d]
        a[k] = None
        assert lib.nrt_global_max_bwd_f32(*a, 2, 8, 4, d, d, big, None) == INV
    assert lib.nrt_global_max_bwd_f32(d, d, d, d, 2, 8, 4, None, d, big, None) == INV
    for batch, v, c in ((0, 8, 4), (2, 0, 4), (2, 8, 0), (-1, 8, 4), (2, -8, 4), (2, 8, -4)):
        assert lib.nrt_global_max_f32(d, batch, v, c, d, d, d, big, None) == INV
        assert lib.nrt_global_max_bwd_f32(d, d, d, d, batch, v, c, d, d, big, None) == INV
        assert lib.nrt_global_max_workspace_bytes(batch, v, c) == 0
    # batch * v * channels >= 2^31
    for batch, v, c in ((2, 1 << 30, 1), (1, 1 << 31, 1), (4, 1 << 24, 32), (1, 1 << 40, 1), (2, 1 << 20, 1 << 10)):
        assert lib.nrt_global_max_f32(d, batch, v, c, d, d, d, big, None) == UNSUP
        assert lib.nrt_global_max_bwd_f32(d, d, d, d, batch, v, c, d, d, big, None) == UNSUP
        assert lib.nrt_global_max_workspace_bytes(batch, v, c) == 0
    assert lib.nrt_global_max_workspace_bytes(2, (1 << 30) - 1, 1) > 0             # the largest tensor that runs
    # a missing or short workspace
    need = lib.nrt_global_max_workspace_bytes(2, 100000, 4)
    assert need > 0
    assert lib.nrt_global_max_f32(d, 2, 100000, 4, d, d, None, big, None) == WS
    assert lib.nrt_global_max_f32(d, 2, 100000, 4, d, d, d, need - 1, None) == WS
    assert lib.nrt_global_max_bwd_f32(d, d, d, d, 2, 100000, 4, d, None, big, None) == WS
    assert lib.nrt_global_max_bwd_f32(d, d, d, d, 2, 100000, 4, d, d, need - 1, None) == WS


def test_global_max_workspace_is_monotone_in_v():
    lib = _lib.lib()
    for batch, c in ((1, 1), (2, 1), (2, 3), (4, 16), (2, 100), (64, 4)):
        last = 0
        for v in (1, 2, 7, 100, 4096, 4097, 16384, 16385, 40000, 100000, 1 << 20, 4096000, 1 << 24):
            if batch * v * c >= 1 << 31:
                break
            n = lib.nrt_global_max_workspace_bytes(batch, v, c)
            assert n >= max(last, batch * max(c, 4) * 8), (batch, v, c)
            last = n


def test_maxnorm_refuses_before_any_launch():
    lib = _lib.lib()
    d = 16
    # (w, k0, rest, max_value, eps, stream)
    assert lib.nrt_maxnorm_f32(None, 3, 64, 2.0, 1e-7, None) == INV
    for k0, rest in ((0, 64), (3, 0), (-3, 64), (3, -64)):
        assert lib.nrt_maxnorm_f32(d, k0, rest, 2.0, 1e-7, None) == INV
    for mv, eps in ((0.0, 1e-7), (-1.0, 1e-7), (float('nan'), 1e-7), (2.0, -1e-7), (2.0, float('nan'))):
        assert lib.nrt_maxnorm_f32(d, 3, 64, mv, eps, None) == INV
    assert lib.nrt_maxnorm_f32(d, 1 << 11, 1 << 20, 2.0, 1e-7, None) == UNSUP


def test_pad_before_convolution_refuses_before_any_launch():
    lib = _lib.lib()
    d = 16
    S, k2 = _lib.ints([5, 6, 7]), _lib.ints([2, 2, 2])

    def call(pad, variant=0, weights=d, ksize=k2, dil=1):
        return lib.nrt_conv3d_pad_f32(d, 4, None, 0, None, weights, None, None, d, 2, S, ksize, 4, dil, pad, 0, variant, None)
    assert call(None) == INV
    assert call(_lib.ints([2, 0, 0])) == INV and call(_lib.ints([0, -1, 0])) == INV      # outside 0 .. (k - 1) * dilation
    assert call(_lib.ints([3, 0, 0]), dil=2) == INV
    assert call(_lib.ints([1, 1, 1]), variant=2) == UNSUP                                  # not what 'same' pads: direct kernel only
    assert call(_lib.ints([1, 1, 1]), weights=None) == INV
    assert lib.nrt_hyperconv3d_pad_f32(d, 4, d, None, None, d, 2, S, k2, 4, 1, None, 0, 0, None) == INV
    assert lib.nrt_hyperconv3d_pad_f32(d, 4, d, None, None, d, 2, S, k2, 4, 1, _lib.ints([1, 1, 1]), 0, 2, None) == UNSUP
    assert lib.nrt_hyperconv3d_pad_f32(d, 4, d, None, None, d, 2, S, k2, 4, 1, _lib.ints([1, 2, 1]), 0, 0, None) == INV


def test_bf16_networks_with_the_new_layers_are_refused_on_cpu_tensors():
    net = _quiet(models.design_dnn, 4, (8, 8, 8), 1, 3, 2, final_layer='globalmaxpooling').bfloat16()
    with pytest.raises(NotImplementedError, match='model_1_global_max_pool:'):
        net(torch.zeros(1, 8, 8, 8, 1))
    net = _quiet(models.design_dnn, 4, (8, 8, 8), 1, 3, 2, final_layer='myglobalmaxpooling', batch_norm=-1).bfloat16()
    with pytest.raises(NotImplementedError, match='model_1_global_max_pool:'):
        net(torch.zeros(1, 8, 8, 8, 1))
    net = _quiet(models.design_dnn, 4, (8, 8, 8), 1, 3, 2, conv_dropout=0.5, final_layer='none').bfloat16()
    with pytest.raises(NotImplementedError, match='model_1_dropout_0_0:'):               # the first such layer in graph order
        net(torch.zeros(1, 8, 8, 8, 1))
    net = _quiet(models.EncoderNet, 4, (8, 8, 8, 1), 1, 3, rescale=2.0).bfloat16()
    with pytest.raises(NotImplementedError, match='flatten:'):
        net(torch.zeros(1, 8, 8, 8, 1))


def test_rescale_values_and_negate_have_the_reference_interface():
    assert {'RescaleValues', 'Negate'} <= set(L.__all__) and hasattr(ne.layers, 'RescaleValues') and hasattr(ne.layers, 'Negate')
    lay = L.RescaleValues(0.25, name='r')
    cfg = lay.get_config()
    assert cfg == {'name': 'r', 'resize': 0.25}
    again = L.RescaleValues(**cfg)
    assert again.get_config() == cfg and again.resize == 0.25
    assert L.RescaleValues(3).name == 'rescalevalues'
    assert lay.compute_output_shape((None, 5, 3)) == (None, 5, 3)
    with pytest.raises(TypeError):
        L.RescaleValues()
    with pytest.raises(TypeError):
        L.RescaleValues(2.0, scale=1.0)
    neg = L.Negate(name='n')
    assert neg.get_config() == {'name': 'n'} and L.Negate(**neg.get_config()).get_config() == {'name': 'n'}
    assert L.Negate().name == 'negate' and neg.compute_output_shape((None, 4)) == (None, 4)
    with pytest.raises(TypeError):
        L.Negate(resize=2.0)
    for layer in (lay, neg):
        with pytest.raises(NotImplementedError, match='float32'):
            layer(torch.zeros(2, 5, dtype=torch.float64))
        with pytest.raises(_lib.NeuriteAmdError, match='no CPU fallback'):
            layer(torch.zeros(2, 5))


def test_apply_constraints_is_a_no_op_without_constraints():
    net = _quiet(models.design_dnn, 4, (8, 8, 8), 1, 3, 2)
    assert not any(getattr(m, 'max_norm', None) for m in net.layers_by_name.values())
    net.apply_constraints()                                                              # CPU parameters: nothing is launched
    net = _quiet(models.design_dnn, 4, (8, 8, 8), 1, 3, 2, conv_maxnorm=2)
    assert [n for n, m in net.layers_by_name.items() if getattr(m, 'max_norm', None)] == \
        ['model_1_conv_0_0', 'model_1_conv_0_1', 'model_1_strided_conv_0']
    with pytest.raises(_lib.NeuriteAmdError, match='no CPU fallback'):
        net.apply_constraints()
