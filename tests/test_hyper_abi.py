"""
CPU tests of the hyper-convolution / hyper-dense layers (no kernel is launched): the C entry points are declared, typed and exported and
validate their arguments; the eight layer classes have the reference's constructor defaults, get_config() keys, output-shape rule and
error behaviour (neurite/tf/layers.py:2515-3033); every refusal is raised on CPU tensors, before the device check; the FromDense
layers build parameters with the reference's names and shapes.
"""

import inspect

import pytest
import torch

import neurite_amd as ne
from neurite_amd import _lib
from neurite_amd import layers as L

HYPER_ENTRY_POINTS = ['nrt_hyperconv3d_pack_weights_f32', 'nrt_hyperconv3d_uses_packed', 'nrt_hyperconv3d_f32',
                      'nrt_hyperconv3d_wgrad_f32']
HYPER_LAYERS = ['HyperConv', 'HyperConv2D', 'HyperConv3D', 'HyperConvFromDense', 'HyperConv2DFromDense', 'HyperConv3DFromDense',
                'HyperDense', 'HyperDenseFromDense']


def test_hyper_entry_points_declared_typed_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in HYPER_ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in _lib._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_hyper_entry_points_validate_arguments():
    lib = _lib.lib()
    k3, k5, s = _lib.ints([3, 3, 3]), _lib.ints([5, 5, 5]), _lib.ints([8, 8, 16])
    dummy = 16
    inv, unsup = _lib.NRT_ERR_INVALID_ARG, _lib.NRT_ERR_UNSUPPORTED
    # pack: NULL pointers, empty batch
    assert lib.nrt_hyperconv3d_pack_weights_f32(None, 2, k3, 16, 16, 0, dummy, None) == inv
    assert lib.nrt_hyperconv3d_pack_weights_f32(dummy, 2, k3, 16, 16, 0, None, None) == inv
    assert lib.nrt_hyperconv3d_pack_weights_f32(dummy, 2, None, 16, 16, 1, dummy, None) == inv
    assert lib.nrt_hyperconv3d_pack_weights_f32(dummy, 0, k3, 16, 16, 0, dummy, None) == inv
    # forward: NULL tensors, no weights in either form, activations beyond none / elu / relu are not fused (never a linear result)
    assert lib.nrt_hyperconv3d_f32(None, 16, dummy, dummy, None, dummy, 2, s, k3, 16, 1, 1, 0, 0, None) == inv
    assert lib.nrt_hyperconv3d_f32(dummy, 16, dummy, dummy, None, None, 2, s, k3, 16, 1, 1, 0, 0, None) == inv
    assert lib.nrt_hyperconv3d_f32(dummy, 16, None, None, None, dummy, 2, s, k3, 16, 1, 1, 0, 0, None) == inv
    assert lib.nrt_hyperconv3d_f32(dummy, 16, dummy, dummy, None, dummy, 2, None, k3, 16, 1, 1, 0, 0, None) == inv
    for act in (3, 4, 10, -1):
        assert lib.nrt_hyperconv3d_f32(dummy, 16, dummy, dummy, None, dummy, 2, s, k3, 16, 1, 1, act, 0, None) == inv
    assert lib.nrt_hyperconv3d_f32(dummy, 16, dummy, dummy, None, dummy, 0, s, k3, 16, 1, 1, 0, 0, None) == inv
    assert lib.nrt_hyperconv3d_f32(dummy, 16, dummy, dummy, None, dummy, 2, s, k3, 16, 1, 1, 0, 7, None) == inv      # unknown variant
    # weight gradient: NULL tensors, the limits of nrt_conv3d_wgrad_f32
    assert lib.nrt_hyperconv3d_wgrad_f32(None, dummy, dummy, None, 2, s, 16, 16, k3, 1, None) == inv
    assert lib.nrt_hyperconv3d_wgrad_f32(dummy, None, dummy, None, 2, s, 16, 16, k3, 1, None) == inv
    assert lib.nrt_hyperconv3d_wgrad_f32(dummy, dummy, None, None, 2, s, 16, 16, k3, 1, None) == inv
    assert lib.nrt_hyperconv3d_wgrad_f32(dummy, dummy, dummy, None, 2, s, 16, 16, k5, 1, None) == unsup
    assert lib.nrt_hyperconv3d_wgrad_f32(dummy, dummy, dummy, None, 2, s, 16, 16, k3, 3, None) == unsup
    # the rule of nrt_conv3d_f32 for the matrix-core kernels (k in {1, 3}, SAME, dilation <= 2, cout <= 64, cin >= 8)
    assert lib.nrt_hyperconv3d_uses_packed(s, k3, 16, 16, 1, 1) == 1
    assert lib.nrt_hyperconv3d_uses_packed(s, k3, 16, 16, 1, 0) == 0
    assert lib.nrt_hyperconv3d_uses_packed(s, k3, 1, 16, 1, 1) == 0
    assert lib.nrt_hyperconv3d_uses_packed(s, k3, 16, 128, 1, 1) == 0
    assert lib.nrt_hyperconv3d_uses_packed(s, k5, 16, 16, 1, 1) == 0
    assert lib.nrt_hyperconv3d_uses_packed(None, k3, 16, 16, 1, 1) == 0


def test_batched_packed_size_is_batch_times_the_shared_size():
    """the packed sets of the batch lie nrt_conv3d_packed_weight_floats apart (the header's contract for `packed`); with
    transpose_flip the set is that of the convolution from cout to cin channels"""
    lib = _lib.lib()
    k3 = _lib.ints([3, 3, 3])
    assert lib.nrt_conv3d_packed_weight_floats(k3, 20, 24) == 2 * 27 * 2 * 256
    assert lib.nrt_conv3d_packed_weight_floats(k3, 48, 16) == 3 * 27 * 1 * 256
    assert lib.nrt_conv3d_packed_weight_floats(k3, 16, 48) == 1 * 27 * 3 * 256


def test_hyper_layers_are_exported():
    for name in HYPER_LAYERS:
        assert name in L.__all__
        assert hasattr(ne.layers, name)


def _defaults(cls):
    sig = inspect.signature(cls.__init__)
    return [(n, p.default) for n, p in sig.parameters.items()
            if n != 'self' and p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)]


def test_constructor_signatures_equal_the_reference():
    E = inspect.Parameter.empty
    # neurite/tf/layers.py:2536-2546
    assert _defaults(L.HyperConv) == [('rank', E), ('filters', E), ('kernel_size', E), ('strides', 1), ('padding', 'valid'),
                                      ('dilation_rate', 1), ('activation', None), ('use_bias', True), ('name', None)]
    # :2689-2698
    assert _defaults(L.HyperConvFromDense) == [('rank', E), ('filters', E), ('kernel_size', E), ('hyperkernel_use_bias', True),
                                               ('hyperbias_use_bias', True), ('hyperkernel_activation', None),
                                               ('hyperbias_activation', None), ('name', None)]
    # :2840-2844, :2923-2929
    assert _defaults(L.HyperDense) == [('units', E), ('activation', None), ('use_bias', True)]
    assert _defaults(L.HyperDenseFromDense) == [('units', E), ('hyperkernel_use_bias', True), ('hyperbias_use_bias', True),
                                                ('hyperkernel_activation', None), ('hyperbias_activation', None)]
    # the rank-fixing subclasses forward everything (:2655-2656, 2664-2665, 2812-2813, 2821-2822)
    assert L.HyperConv2D(4, 3).rank == 2 and L.HyperConv3D(4, 3).rank == 3
    assert L.HyperConv2DFromDense(4, 3).rank == 2 and L.HyperConv3DFromDense(4, 3).rank == 3
    c = L.HyperConv3D(4, 3)
    assert (c.filters, c.kernel_size, c.strides, c.padding, c.dilation_rate, c.activation, c.use_bias) == \
        (4, (3, 3, 3), (1, 1, 1), 'valid', (1, 1, 1), None, True)
    f = L.HyperConv3DFromDense(4, 3, padding='SAME', activation='elu')
    assert (f.padding, f.activation, f.hyperkernel_use_bias, f.hyperbias_use_bias, f.hyperkernel_activation,
            f.hyperbias_activation) == ('same', 'elu', True, True, None, None)


CONV_KEYS = ['rank', 'filters', 'kernel_size', 'strides', 'padding', 'dilation_rate', 'activation', 'use_bias']    # :2636-2645
FROM_DENSE_KEYS = ['hyperkernel_use_bias', 'hyperbias_use_bias', 'hyperkernel_activation', 'hyperbias_activation']  # :2797-2802, 3026-3031
DENSE_KEYS = ['units', 'activation', 'use_bias']                                                                    # :2898-2902


def test_get_config_keys_equal_the_reference():
    for cls in (L.HyperConv2D, L.HyperConv3D):
        cfg = cls(4, 3, name='hc').get_config()
        assert list(cfg) == ['name'] + CONV_KEYS
        assert cfg['name'] == 'hc' and cfg['activation'] == 'linear' and cfg['kernel_size'] == (3,) * cfg['rank']
    assert list(L.HyperConv(1, 4, 3).get_config()) == ['name'] + CONV_KEYS
    for cls in (L.HyperConv2DFromDense, L.HyperConv3DFromDense):
        cfg = cls(4, 3, hyperkernel_activation='tanh').get_config()
        assert list(cfg) == ['name'] + CONV_KEYS + FROM_DENSE_KEYS
        assert cfg['hyperkernel_activation'] == 'tanh' and cfg['hyperbias_activation'] == 'linear'
    assert list(L.HyperConvFromDense(2, 4, 3).get_config()) == ['name'] + CONV_KEYS + FROM_DENSE_KEYS
    assert list(L.HyperDense(7, activation='relu').get_config()) == ['name'] + DENSE_KEYS
    assert L.HyperDense(7, activation='relu').get_config()['activation'] == 'relu'
    assert list(L.HyperDenseFromDense(7).get_config()) == ['name'] + DENSE_KEYS + FROM_DENSE_KEYS
    # a config rebuilds the layer
    cfg = L.HyperConv3D(4, 3, padding='same', dilation_rate=2, activation='elu', use_bias=False).get_config()
    cfg['activation'] = None if cfg['activation'] == 'linear' else cfg['activation']
    again = L.HyperConv(**cfg)
    assert again.get_config()['dilation_rate'] == (2, 2, 2) and again.use_bias is False and again.activation == 'elu'


def test_compute_output_shape():
    shapes = [(2, 20, 21, 22, 5), (2, 3, 3, 3, 5, 4), (2, 4)]
    assert L.HyperConv3D(4, 3, padding='same').compute_output_shape(shapes) == (2, 20, 21, 22, 4)
    assert L.HyperConv3D(4, 3, padding='valid').compute_output_shape(shapes) == (2, 18, 19, 20, 4)
    assert L.HyperConv3D(4, 3, padding='valid', dilation_rate=2).compute_output_shape(shapes) == (2, 16, 17, 18, 4)
    assert L.HyperConv3D(4, 3, padding='same', dilation_rate=2).compute_output_shape(shapes) == (2, 20, 21, 22, 4)
    assert L.HyperConv3D(4, (1, 3, 3), padding='valid', strides=2).compute_output_shape(shapes) == (2, 10, 10, 10, 4)
    assert L.HyperConv2D(6, 3).compute_output_shape([(None, 9, 12, 5)]) == (None, 7, 10, 6)
    assert L.HyperDense(7).compute_output_shape([(2, 5, 6, 3), (2, 3, 7)]) == (2, 5, 6, 7)
    with pytest.raises(ValueError):
        L.HyperDense(7).compute_output_shape([(2,)])


def test_causal_padding_raises_value_error():
    for make in (lambda: L.HyperConv(1, 4, 3, padding='causal'), lambda: L.HyperConv3D(4, 3, padding='Causal'),
                 lambda: L.HyperConv2DFromDense(4, 3, padding='causal')):
        with pytest.raises(ValueError, match='Causal padding is not supported for HyperConv'):
            make()
    with pytest.raises(ValueError):
        L.HyperConv3D(4, 3, padding='full')
    with pytest.raises(ValueError):
        L.HyperConv3D(4, (3, 3))                              # normalize_tuple


def _inputs(B=2, S=(4, 4, 4), cin=3, cout=4, k=3, dtype=torch.float32):
    x = torch.zeros((B,) + tuple(S) + (cin,), dtype=dtype)
    kern = torch.zeros((B,) + (k,) * len(S) + (cin, cout), dtype=dtype)
    bias = torch.zeros(B, cout, dtype=dtype)
    return x, kern, bias


def test_refusals_come_before_any_device_use():
    """CPU tensors: reaching the device check would raise NeuriteAmdError"""
    x, k, b = _inputs()
    with pytest.raises(NotImplementedError, match='strides'):
        L.HyperConv3D(4, 3, strides=2)([x, k, b])
    with pytest.raises(NotImplementedError, match='stride'):
        L.HyperConv3D(4, 3, strides=(1, 2, 1))([x, k, b])
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match='float32'):
            L.HyperConv3D(4, 3)([x.to(dt), k.to(dt), b.to(dt)])
    with pytest.raises(NotImplementedError, match='float32'):
        L.HyperConv3D(4, 3)([x, k.double(), b])
    x4 = torch.zeros(2, 4, 4, 4, 4, 3)
    k4 = torch.zeros(2, 3, 3, 3, 3, 3, 4)
    with pytest.raises(NotImplementedError, match='rank'):
        L.HyperConv(4, 4, 3)([x4, k4, b])
    with pytest.raises(NotImplementedError, match='dilation'):
        L.HyperConv3D(4, 3, dilation_rate=(1, 2, 1))([x, k, b])
    # shape errors
    with pytest.raises(ValueError, match='batch'):
        L.HyperConv3D(4, 3)([x, k[:1], b])
    with pytest.raises(ValueError, match='channel mismatch'):
        L.HyperConv3D(4, 3)([x, torch.zeros(2, 3, 3, 3, 5, 4), b])
    with pytest.raises(ValueError, match='channel mismatch'):
        L.HyperConv3D(5, 3)([x, k, b])
    with pytest.raises(ValueError, match='bias'):
        L.HyperConv3D(4, 3)([x, k])                           # use_bias=True without a bias input
    with pytest.raises(ValueError, match='bias'):
        L.HyperConv3D(4, 3)([x, k, b[:, :3]])
    with pytest.raises(ValueError, match='kernel_size'):
        L.HyperConv3D(4, 1)([x, k, b])
    # the dense forms
    xd, kd, bd = torch.zeros(2, 5, 3), torch.zeros(2, 3, 7), torch.zeros(2, 7)
    with pytest.raises(NotImplementedError, match='float32'):
        L.HyperDense(7)([xd.double(), kd.double(), bd.double()])
    with pytest.raises(ValueError, match='batch'):
        L.HyperDense(7)([xd, kd[:1], bd])
    with pytest.raises(ValueError, match='channel mismatch'):
        L.HyperDense(7)([xd, torch.zeros(2, 4, 7), bd])
    with pytest.raises(ValueError, match='bias'):
        L.HyperDense(7)([xd, kd])
    with pytest.raises(NotImplementedError, match='strides'):
        L.HyperConv3DFromDense(4, 3, strides=2)([x, torch.zeros(2, 6)])
    with pytest.raises(NotImplementedError, match='float32'):
        L.HyperDenseFromDense(7)([xd.double(), torch.zeros(2, 6)])
    # well-formed float32 calls still reach the device check
    for layer, inputs in ((L.HyperConv3D(4, 3), [x, k, b]), (L.HyperConv3D(4, 3, use_bias=False, padding='same'), [x, k]),
                          (L.HyperConv2D(4, 3), list(_inputs(S=(4, 4)))), (L.HyperDense(7), [xd, kd, bd]),
                          (L.HyperConv3DFromDense(4, 3), [x, torch.zeros(2, 6)]), (L.HyperDenseFromDense(7), [xd, torch.zeros(2, 6)])):
        with pytest.raises(ne.errors.NeuriteAmdError):
            layer(inputs)


def test_from_dense_builds_the_reference_parameters():
    x, _, _ = _inputs(cin=3)
    hyp = torch.zeros(2, 6)
    layer = L.HyperConv3DFromDense(4, 3)
    assert not layer.built and list(layer.parameters()) == []
    with pytest.raises(ne.errors.NeuriteAmdError):            # built on the first call; the call itself stops at the device check
        layer([x, hyp])
    assert layer.built
    shapes = {n: tuple(p.shape) for n, p in layer.named_parameters()}
    assert shapes == {'hyperkernel_kernel': (6, 27 * 3 * 4), 'hyperkernel_bias': (27 * 3 * 4,), 'hyperbias_kernel': (6, 4),
                      'hyperbias_bias': (4,)}
    assert all(p.requires_grad and p.dtype == torch.float32 for p in layer.parameters())
    lim = (6.0 / (6 + 27 * 3 * 4)) ** 0.5                      # glorot uniform, the add_weight default
    assert float(layer.hyperkernel_kernel.detach().abs().max()) <= lim and float(layer.hyperkernel_kernel.detach().abs().max()) > 0.5 * lim
    # the pseudo-dense mapping: hyp @ kernel + bias -> activation -> reshape(-1, *target_shape)   (:2776-2794)
    h = torch.randn(2, 6)
    kern = layer._call_dense_pseudo_layer(h, layer.hyperkernel)
    assert tuple(kern.shape) == (2, 3, 3, 3, 3, 4)
    want = (h.double() @ layer.hyperkernel_kernel.double() + layer.hyperkernel_bias.double()).reshape(2, 3, 3, 3, 3, 4)
    assert torch.allclose(kern.double(), want, rtol=1e-5, atol=1e-6)
    assert tuple(layer._call_dense_pseudo_layer(h, layer.hyperbias).shape) == (2, 4)

    nobias = L.HyperConv2DFromDense(5, (1, 3), use_bias=False, hyperkernel_use_bias=False, hyperkernel_activation='tanh')
    nobias.build([(2, 8, 8, 3), (2, 9)])
    assert {n: tuple(p.shape) for n, p in nobias.named_parameters()} == {'hyperkernel_kernel': (9, 3 * 3 * 5)}
    out = nobias._call_dense_pseudo_layer(torch.ones(2, 9), nobias.hyperkernel)
    assert tuple(out.shape) == (2, 1, 3, 3, 5)
    assert torch.allclose(out.reshape(2, -1), torch.tanh(torch.ones(2, 9) @ nobias.hyperkernel_kernel))

    dense = L.HyperDenseFromDense(7, hyperbias_use_bias=False)
    dense.build([(2, 5, 3), (2, 6)])
    assert {n: tuple(p.shape) for n, p in dense.named_parameters()} == {'hyperkernel_kernel': (6, 21), 'hyperkernel_bias': (21,),
                                                                        'hyperbias_kernel': (6, 7)}
    assert tuple(dense._call_dense_pseudo_layer(torch.zeros(2, 6), dense.hyperkernel).shape) == (2, 3, 7)
    with pytest.raises(ValueError, match='hypernetwork output'):
        L.HyperConv3DFromDense(4, 3)([x, torch.zeros(3, 6)])
