"""
CPU tests of the per-voxel parameter layers and the stream layers (no kernel is launched): the seven C entry points are declared,
typed and exported and validate their arguments; the seven layer classes have the reference's constructor defaults, get_config()
keys and output-shape rules (neurite/tf/layers.py:746-808, 1535-1607, 1711-1844, 1915-2073); every refusal is raised on CPU tensors,
before the device check.
"""

import inspect
import warnings

import pytest
import torch

import neurite_amd as ne
from neurite_amd import _lib
from neurite_amd import layers as L

ENTRY_POINTS = ['nrt_local_affine_f32', 'nrt_local_affine_bwd_f32', 'nrt_local_cross_linear_f32', 'nrt_local_cross_linear_bwd_f32',
                'nrt_stream_mean_f32', 'nrt_stream_mean_bwd_f32', 'nrt_stream_cov_f32']
LAYERS = ['LocalBias', 'LocalLinear', 'LocalCrossLinear', 'LocalParamLayer', 'LocalParamWithInput', 'MeanStream', 'CovStream']


def _pwi(*args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return L.LocalParamWithInput(*args, **kwargs)


def test_entry_points_declared_typed_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in _lib._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_entry_points_validate_arguments():
    lib = _lib.lib()
    d = 16                                         # a non-NULL "pointer"; nothing is launched on an argument error
    inv, unsup = _lib.NRT_ERR_INVALID_ARG, _lib.NRT_ERR_UNSUPPORTED
    # affine forward: (x, probe, probe_stride, mult, bias, bias_scale, y, batch, n, stream)
    assert lib.nrt_local_affine_f32(d, None, 0, d, None, 1.0, d, 2, 8, None) == inv          # no bias
    assert lib.nrt_local_affine_f32(d, None, 0, d, d, 1.0, None, 2, 8, None) == inv          # no output
    assert lib.nrt_local_affine_f32(d, None, 0, d, d, 1.0, d, 0, 8, None) == inv             # zero batch
    assert lib.nrt_local_affine_f32(d, None, 0, d, d, 1.0, d, 2, 0, None) == inv             # n <= 0
    assert lib.nrt_local_affine_f32(d, None, 0, d, d, 1.0, d, 2, -4, None) == inv
    assert lib.nrt_local_affine_f32(d, d, 8, d, d, 1.0, d, 2, 8, None) == inv                # x and probe together
    assert lib.nrt_local_affine_f32(None, d, 8, d, d, 1.0, d, 2, 8, None) == inv             # mult without x
    # affine backward: (g, x, probe, probe_stride, mult, bias_scale, gx, gmult, gbias, batch, n, stream)
    assert lib.nrt_local_affine_bwd_f32(None, d, None, 0, d, 1.0, d, d, d, 2, 8, None) == inv
    assert lib.nrt_local_affine_bwd_f32(d, d, None, 0, None, 1.0, d, None, None, 2, 8, None) == inv      # gx needs mult
    assert lib.nrt_local_affine_bwd_f32(d, None, None, 0, d, 1.0, None, d, None, 2, 8, None) == inv      # gmult needs x
    assert lib.nrt_local_affine_bwd_f32(d, d, None, 0, d, 1.0, d, d, d, 0, 8, None) == inv
    assert lib.nrt_local_affine_bwd_f32(d, d, None, 0, d, 1.0, d, d, d, 2, 0, None) == inv
    # cross linear: (x, w, bias, y, batch, nvox, cin, cout, stream)
    assert lib.nrt_local_cross_linear_f32(None, d, d, d, 2, 8, 4, 4, None) == inv
    assert lib.nrt_local_cross_linear_f32(d, None, d, d, 2, 8, 4, 4, None) == inv
    assert lib.nrt_local_cross_linear_f32(d, d, d, None, 2, 8, 4, 4, None) == inv
    assert lib.nrt_local_cross_linear_f32(d, d, d, d, 0, 8, 4, 4, None) == inv
    assert lib.nrt_local_cross_linear_f32(d, d, d, d, 2, 0, 4, 4, None) == inv
    for cin, cout in ((0, 4), (65, 4), (4, 0), (4, 65)):
        assert lib.nrt_local_cross_linear_f32(d, d, d, d, 2, 8, cin, cout, None) == unsup
        assert lib.nrt_local_cross_linear_bwd_f32(d, d, d, d, d, d, 2, 8, cin, cout, None) == unsup
    # (g, x, w, gx, gw, gbias, batch, nvox, cin, cout, stream)
    assert lib.nrt_local_cross_linear_bwd_f32(None, d, d, d, d, d, 2, 8, 4, 4, None) == inv
    assert lib.nrt_local_cross_linear_bwd_f32(d, d, None, d, None, None, 2, 8, 4, 4, None) == inv        # gx needs w
    assert lib.nrt_local_cross_linear_bwd_f32(d, None, d, None, d, None, 2, 8, 4, 4, None) == inv        # gw needs x
    assert lib.nrt_local_cross_linear_bwd_f32(d, d, d, d, d, d, 0, 8, 4, 4, None) == inv
    assert lib.nrt_local_cross_linear_bwd_f32(d, d, d, d, d, d, 2, 0, 4, 4, None) == inv
    # stream mean: (x, mean, count, cap, y, coef, batch, n, training, stream)
    assert lib.nrt_stream_mean_f32(None, d, d, 3.0, d, d, 2, 8, 1, None) == inv              # training needs x
    assert lib.nrt_stream_mean_f32(d, None, d, 3.0, d, d, 2, 8, 1, None) == inv
    assert lib.nrt_stream_mean_f32(d, d, None, 3.0, d, d, 2, 8, 1, None) == inv
    assert lib.nrt_stream_mean_f32(d, d, d, 3.0, None, d, 2, 8, 1, None) == inv
    assert lib.nrt_stream_mean_f32(d, d, d, 3.0, d, d, 0, 8, 1, None) == inv
    assert lib.nrt_stream_mean_f32(d, d, d, 3.0, d, d, 2, 0, 0, None) == inv
    # (g, coef, gx, batch, n, stream)
    assert lib.nrt_stream_mean_bwd_f32(None, d, d, 2, 8, None) == inv
    assert lib.nrt_stream_mean_bwd_f32(d, None, d, 2, 8, None) == inv
    assert lib.nrt_stream_mean_bwd_f32(d, d, None, 2, 8, None) == inv
    assert lib.nrt_stream_mean_bwd_f32(d, d, d, 0, 8, None) == inv
    assert lib.nrt_stream_mean_bwd_f32(d, d, d, 2, 0, None) == inv
    # stream cov: (x, mean, cov, count, cap, y, batch, v, training, stream)
    assert lib.nrt_stream_cov_f32(None, d, d, d, 3.0, d, 2, 8, 1, None) == inv
    assert lib.nrt_stream_cov_f32(d, None, d, d, 3.0, d, 2, 8, 1, None) == inv
    assert lib.nrt_stream_cov_f32(d, d, None, d, 3.0, d, 2, 8, 0, None) == inv
    assert lib.nrt_stream_cov_f32(d, d, d, None, 3.0, d, 2, 8, 0, None) == inv
    assert lib.nrt_stream_cov_f32(d, d, d, d, 3.0, None, 2, 8, 0, None) == inv
    assert lib.nrt_stream_cov_f32(d, d, d, d, 3.0, d, 0, 8, 1, None) == inv
    assert lib.nrt_stream_cov_f32(d, d, d, d, 3.0, d, 2, 0, 1, None) == inv


def test_layers_are_exported():
    for name in LAYERS:
        assert name in L.__all__
        assert hasattr(ne.layers, name)


def _defaults(cls):
    sig = inspect.signature(cls.__init__)
    return [(n, p.default) for n, p in sig.parameters.items()
            if n != 'self' and p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)]


def test_constructor_signatures_equal_the_reference():
    E = inspect.Parameter.empty
    assert _defaults(L.LocalBias) == [('my_initializer', 'RandomNormal'), ('biasmult', 1.0)]                      # :757
    assert _defaults(L.LocalLinear) == [('initializer', 'RandomNormal')]                                           # :788
    assert _defaults(L.LocalCrossLinear) == [('output_features', E), ('mult_initializer', None), ('bias_initializer', None),
                                             ('mult_regularizer', None), ('bias_regularizer', None), ('use_bias', True)]   # :1545-1551
    assert _defaults(L.LocalParamLayer) == [('shape', E), ('my_initializer', 'RandomNormal'), ('dtype', None), ('name', None),
                                            ('mult', 1.0)]                                                         # :1727-1733
    assert _defaults(L.LocalParamWithInput) == [('shape', E), ('initializer', 'RandomNormal'), ('mult', 1.0)]     # :1814
    assert _defaults(L.MeanStream) == [('cap', 100)]                                                               # :1928
    assert _defaults(L.CovStream) == [('cap', 100)]                                                                # :1991
    # the attribute names of the reference
    b = L.LocalBias('zeros', biasmult=0.5)
    assert (b.initializer, b.biasmult) == ('zeros', 0.5)
    c = L.LocalCrossLinear(5, use_bias=False)
    assert (c.output_features, c.mult_initializer, c.bias_initializer, c.mult_regularizer, c.bias_regularizer, c.use_bias) == \
        (5, None, None, None, None, False)
    p = L.LocalParamLayer((3, 4), mult=2.0)
    assert p.shape == [1, 3, 4] and p.mult == 2.0 and p.my_initializer == 'RandomNormal' and p.name.startswith('local_param_')
    assert tuple(p.kernel.shape) == (3, 4) and p.kernel.requires_grad and p.built          # created at construction (:1752-1758)
    with pytest.warns(UserWarning, match='LocalParamWithInput'):                            # the reference prints (:1818)
        w = L.LocalParamWithInput((3, 4), mult=2.5)
    assert (w.shape, w.initializer, w.biasmult) == ((3, 4), 'RandomNormal', 2.5)
    assert L.MeanStream(cap=7).cap == 7.0 and isinstance(L.CovStream(cap=7).cap, float)
    assert L.MeanStream().trainable is True and L.MeanStream(trainable=False).trainable is False
    assert L.CovStream(trainable=False).trainable is False


def test_get_config_keys_and_output_shapes():
    assert list(L.LocalBias(name='lb').get_config()) == ['name'] and L.LocalBias(name='lb').get_config()['name'] == 'lb'
    assert list(L.LocalLinear().get_config()) == ['name']
    assert list(L.LocalCrossLinear(4).get_config()) == ['name']
    assert list(L.LocalParamLayer((3, 4)).get_config()) == ['dtype', 'sparse', 'name']                             # :1783-1789
    assert L.LocalParamLayer((3, 4), name='atlas').get_config() == {'dtype': 'float32', 'sparse': False, 'name': 'atlas'}
    assert list(_pwi((3, 4)).get_config()) == ['name', 'shape'] and _pwi((3, 4)).get_config()['shape'] == (3, 4)   # :1821-1826
    assert list(L.MeanStream().get_config()) == ['name'] and list(L.CovStream().get_config()) == ['name']
    shape = (2, 5, 6, 7, 3)
    assert L.LocalBias().compute_output_shape(shape) == shape
    assert L.LocalLinear().compute_output_shape(shape) == shape
    assert L.LocalCrossLinear(4).compute_output_shape(shape) == (2, 5, 6, 7, 4)
    assert L.LocalParamLayer((3, 4)).compute_output_shape() == (1, 3, 4)
    assert _pwi((8, 9, 1)).compute_output_shape(shape) == (2, 8, 9, 1)
    assert L.MeanStream().compute_output_shape(shape) == shape
    assert L.CovStream().compute_output_shape((3, 5, 7)) == (3, 35, 35)
    assert L.CovStream().compute_output_shape((3, 6, 11, 2)) == (3, 132, 132)


def test_weights_and_buffers_are_built_as_the_reference_builds_them():
    b = L.LocalBias()
    b.build((2, 5, 6, 3))
    assert {n: tuple(p.shape) for n, p in b.named_parameters()} == {'kernel': (5, 6, 3)}
    assert 0.03 < float(b.kernel.detach().std()) < 0.07 and abs(float(b.kernel.detach().mean())) < 0.03    # Keras' RandomNormal: 0 +- 0.05
    ll = L.LocalLinear('zeros')
    ll.build((2, 5, 6, 3))
    assert {n: tuple(p.shape) for n, p in ll.named_parameters()} == {'mult': (5, 6, 3), 'bias': (5, 6, 3)}
    assert float(ll.mult.detach().abs().max()) == 0.0
    g = L.LocalBias('glorot_uniform')
    g.build((2, 5, 6, 3))
    lim = (6.0 / (5 * 6 + 5 * 3)) ** 0.5                        # fans of (5, 6, 3): receptive field 5, fan_in 30, fan_out 15
    assert 0.5 * lim < float(g.kernel.detach().abs().max()) <= lim
    c = L.LocalCrossLinear(4)
    c.build((2, 5, 6, 8))
    assert {n: tuple(p.shape) for n, p in c.named_parameters()} == {'mult': (1, 5, 6, 8, 4), 'bias': (1, 5, 6, 4)}
    assert abs(float(c.mult.detach().mean()) - 1 / 8) < 0.005 and 0.005 < float(c.mult.detach().std()) < 0.02   # N(1 / Cin, 0.01)
    assert abs(float(c.bias.detach().mean()) - 1 / 8) < 0.01
    nb = L.LocalCrossLinear(4, use_bias=False)
    nb.build((2, 5, 8))
    assert [n for n, _ in nb.named_parameters()] == ['mult'] and nb.bias is None
    m = L.MeanStream(cap=3)
    assert m.state_dict() == {} and m.mean is None
    m.build((2, 5, 6, 3))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {'mean': (5, 6, 3), 'count': (1,)}
    assert list(m.parameters()) == [] and float(m.count) == 0.0 and float(m.mean.abs().max()) == 0.0
    cv = L.CovStream()
    cv.build((2, 5, 7))
    assert {k: tuple(v.shape) for k, v in cv.state_dict().items()} == {'mean': (5, 7), 'count': (1,), 'cov': (35, 35)}
    assert list(cv.parameters()) == []
    fresh = L.CovStream()
    fresh.build((2, 5, 7))
    fresh.load_state_dict(cv.state_dict())


def test_refusals_come_before_any_device_use():
    """CPU tensors: reaching the device check would raise NeuriteAmdError"""
    x = torch.zeros(2, 4, 5, 3)
    makers = [lambda: L.LocalBias(), lambda: L.LocalLinear(), lambda: L.LocalCrossLinear(4), lambda: _pwi((4, 5, 1)),
              lambda: L.MeanStream(), lambda: L.CovStream()]
    for make in makers:
        for dt in (torch.float64, torch.float16, torch.bfloat16):
            layer = make()
            with pytest.raises(NotImplementedError, match='float32'):
                layer(x.to(dt))
            assert list(layer.parameters()) == []               # refused before anything was built
    with pytest.raises(NotImplementedError, match='float32'):
        L.LocalParamLayer((4, 5), dtype='float64')
    with pytest.raises(NotImplementedError, match='float32'):
        L.LocalParamLayer((4, 5), dtype=torch.bfloat16)
    # regularizers: no Keras loss collection
    with pytest.raises(NotImplementedError, match='regularizer'):
        L.LocalCrossLinear(4, mult_regularizer='l2')
    with pytest.raises(NotImplementedError, match='regularizer'):
        L.LocalCrossLinear(4, bias_regularizer=lambda w: w.sum())
    # initializers beyond 'RandomNormal', 'glorot_uniform', 'zeros'
    for layer in (L.LocalBias('he_normal'), L.LocalLinear('ones'), L.LocalCrossLinear(4, mult_initializer='orthogonal'),
                  L.LocalCrossLinear(4, bias_initializer='ones'), _pwi((4, 5, 1), initializer='he_normal')):
        with pytest.raises(NotImplementedError, match='initializer'):
            layer(x)
    with pytest.raises(NotImplementedError, match='initializer'):
        L.LocalParamLayer((4, 5), my_initializer='ones')
    # more than 64 features
    with pytest.raises(NotImplementedError, match='64'):
        L.LocalCrossLinear(65)(x)
    with pytest.raises(NotImplementedError, match='64'):
        L.LocalCrossLinear(4)(torch.zeros(2, 3, 65))
    # CovStream has no gradient (training mode, grad mode, an input that requires grad): refused before the device check
    with pytest.raises(NotImplementedError, match='gradient'):
        L.CovStream()(torch.zeros(2, 5, 7, requires_grad=True), training=True)
    # well-formed float32 calls reach the device check
    for make in makers:
        with pytest.raises(ne.errors.NeuriteAmdError):
            make()(x)
    with pytest.raises(ne.errors.NeuriteAmdError):
        L.LocalParamLayer((4, 5))()
    with pytest.raises(ne.errors.NeuriteAmdError):
        L.MeanStream()(x, training=False)
