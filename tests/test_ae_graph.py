"""
The layer graphs `models.single_ae` / `models.ae` build against the graphs the REFERENCE's own builders construct
(neurite/tf/models.py:249-375, 438-646), recorded in tests/golden/ae_graph.json by tests/golden/make_ae_golden.py: per layer its name,
Keras class, constructor arguments, the producers of its inputs and its output shape, in Keras' layer order.  Then the weight API on
the new layers: `get_weights()` order and shapes, `save_weights` / `load_weights` through .npz and .h5, `save` / `models.load`.
CPU only; no kernel runs.
"""

import contextlib
import io
import json
import os
import warnings

import numpy as np
import pytest

from neurite_amd import models

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, 'golden', 'ae_graph.json')) as f:
    GRAPHS = {k: v for k, v in json.load(f).items() if not k.startswith('__')}


def _build(case, **override):
    kwargs = dict(case['kwargs'])
    kwargs.update(override)
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        warnings.simplefilter('ignore')
        return getattr(models, case['builder'])(*case['args'], **kwargs)


def _pairs(tag):
    """[(network, recorded graph)] of a case: one, or three for `ae` in tuple form"""
    case = GRAPHS[tag]
    built = _build(case)
    if 'graphs' in case:
        assert isinstance(built, tuple) and len(built) == len(case['graphs']) == 3
        return list(zip(built, case['graphs']))
    assert isinstance(built, models.ConvNet)
    return [(built, case['graph'])]


# variables a Keras layer owns, in `layer.weights` order
def _keras_variables(layer):
    if layer['class'] in ('Conv1D', 'Conv2D', 'Conv3D', 'Dense'):
        return ['kernel'] + (['bias'] if layer['config'].get('use_bias', True) else [])
    if layer['class'] == 'BatchNormalization':
        return ['gamma', 'beta', 'moving_mean', 'moving_variance']
    if layer['class'] == 'LocalBias':
        return ['kernel']
    return []


def _keras_variable_shape(layer, var, by_name):
    cfg, out = layer['config'], layer['output_shape']
    cin = by_name[layer['inputs'][0]]['output_shape'][-1]
    if layer['class'].startswith('Conv'):
        return tuple(cfg['kernel_size']) + (cin, cfg['filters']) if var == 'kernel' else (cfg['filters'],)
    if layer['class'] == 'Dense':
        return (cin, cfg['units']) if var == 'kernel' else (cfg['units'],)
    if layer['class'] == 'LocalBias':
        return tuple(out[1:])
    return (out[-1],)


def test_the_recording_covers_the_cases_the_builders_have():
    kinds = set()
    for case in GRAPHS.values():
        for g in case.get('graphs', [case.get('graph')]):
            kinds.update(l['class'] for l in g['layers'])
    assert {'Flatten', 'Dense', 'Reshape', 'Resize', 'LocalBias', 'SampleNormalLogVar', 'Lambda', 'BatchNormalization'} <= kinds
    assert any('graphs' in c for c in GRAPHS.values()) and any(c['kwargs'].get('single_model') for c in GRAPHS.values())
    assert any(c['kwargs'].get('add_prior_layer') for c in GRAPHS.values())


@pytest.mark.parametrize('tag', sorted(GRAPHS))
def test_graph_matches_reference_builder(tag):
    for net, ref in _pairs(tag):
        got = net.keras_graph()
        assert got['inputs'] == ref['inputs']
        assert got['outputs'] == ref['outputs']
        assert [l['name'] for l in got['layers']] == [l['name'] for l in ref['layers']]          # names AND order
        for g, r in zip(got['layers'], ref['layers']):
            assert g['class'] == r['class'], r['name']
            assert g['inputs'] == r['inputs'], r['name']
            assert g['output_shape'] == r['output_shape'], r['name']
            assert g['config'] == r['config'], (r['name'], g['config'], r['config'])


@pytest.mark.parametrize('tag', sorted(GRAPHS))
def test_get_weights_has_keras_order_and_shapes(tag):
    for net, ref in _pairs(tag):
        by_name = {l['name']: l for l in ref['layers']}
        expected = [('%s/%s' % (l['name'], v), _keras_variable_shape(l, v, by_name)) for l in ref['layers'] for v in _keras_variables(l)]
        assert [n for n, _, _ in net._weight_tensors()] == [n for n, _ in expected]
        assert [tuple(w.shape) for w in net.get_weights()] == [s for _, s in expected]


def _randomise(net, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.standard_normal(w.shape).astype(np.float32) for w in net.get_weights()]
    net.set_weights(ws)
    return ws


@pytest.mark.parametrize('ext', ['npz', 'h5'])
@pytest.mark.parametrize('tag', ['sae_dense_vae_shift', 'sae_conv_resize_vae', 'sae_dense_flat_bn_default_vae', 'ae_2d_dense_single',
                                 'ae_3d_conv_vae_prior_single'])
def test_save_weights_load_weights_round_trip_bit_for_bit(tag, ext, tmp_path):
    (net, _), = _pairs(tag)
    ws = _randomise(net, 5)
    assert any(w.ndim == 2 for w in ws) or 'conv' in tag
    path = str(tmp_path / ('w.' + ext))
    net.save_weights(path)
    (other, _), = _pairs(tag)
    _randomise(other, 6)
    other.load_weights(path)
    got = other.get_weights()
    assert len(got) == len(ws)
    for a, b in zip(got, ws):
        assert a.dtype == np.float32 and a.shape == b.shape
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_set_weights_refuses_a_transposed_dense_kernel():
    (net, _), = _pairs('sae_dense')
    ws = net.get_weights()
    assert ws[0].shape == (192, 6)                       # Keras' [in, out], as a .h5 file stores it
    ws[0] = ws[0].T.copy()
    with pytest.raises(ValueError, match='not compatible'):
        net.set_weights(ws)


@pytest.mark.parametrize('ext', ['npz', 'h5'])
def test_models_load_rebuilds_an_ae_from_its_saved_config(ext, tmp_path):
    case = GRAPHS['ae_2d_dense_vae_prior_single']
    net = _build(case)
    ws = _randomise(net, 7)
    net.metadata['note'] = 'bottleneck 5'
    path = str(tmp_path / ('ae.' + ext))
    net.save(path)
    builder, config = models.load_config(path)
    assert builder == 'ae' and config['enc_size'] == [5] and config['do_vae'] is True and config['single_model'] is True
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        back = models.load(path)
    assert back.layer_names == net.layer_names
    assert back.keras_graph() == net.keras_graph()
    assert back.metadata['note'] == 'bottleneck 5'
    for a, b in zip(back.get_weights(), ws):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a single_ae on its own is loadable too
    sae = _build(GRAPHS['sae_dense_vae_shift'])
    path = str(tmp_path / ('sae.' + ext))
    sae.save(path)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        back = models.load(path)
    assert back.config['builder'] == 'single_ae' and back.keras_graph() == sae.keras_graph()
