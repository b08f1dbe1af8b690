"""
CPU tests of the auto-encoder bottleneck (no kernel is launched): the three dense entry points of csrc/dense.hip are declared, typed and
exported and refuse bad arguments before any launch; layers.SampleNormalLogVar has the reference's constructor, get_config() keys and
output shape (neurite/tf/layers.py:2261-2302); models.ae / models.single_ae have the reference's signatures (by AST, as
tests/test_reference_switch.py compares the others; the reference's side is recorded in tests/golden/ae_graph.json by
tests/golden/make_ae_golden.py); and every refusal of the builders and of the bf16 path is raised on CPU tensors.
"""

import contextlib
import io
import json
import os
import sys

import pytest
import torch

import neurite_amd as ne
from neurite_amd import _lib
from neurite_amd import layers as L
from neurite_amd import models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import ast_signatures as sigs          # noqa: E402

with open(os.path.join(ROOT, 'tests', 'golden', 'ae_graph.json')) as f:
    REFERENCE_SIGNATURES = json.load(f)['__signatures__']

ENTRY_POINTS = ['nrt_dense_f32', 'nrt_dense_bwd_f32', 'nrt_dense_workspace_bytes']


def _quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*args, **kwargs)


def test_entry_points_declared_typed_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in _lib._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_entry_points_refuse_before_any_launch():
    lib = _lib.lib()
    d = 16                                         # a non-NULL "pointer"; nothing is launched on an argument error
    inv, unsup = _lib.NRT_ERR_INVALID_ARG, _lib.NRT_ERR_UNSUPPORTED
    big = 1 << 20
    # forward: (x, w, bias, y, batch, in, out, act, variant, workspace, workspace_bytes, stream)
    assert lib.nrt_dense_f32(None, d, d, d, 2, 8, 4, 0, 0, d, big, None) == inv
    assert lib.nrt_dense_f32(d, None, d, d, 2, 8, 4, 0, 0, d, big, None) == inv
    assert lib.nrt_dense_f32(d, d, d, None, 2, 8, 4, 0, 0, d, big, None) == inv
    for batch, cin, cout in ((0, 8, 4), (2, 0, 4), (2, 8, 0), (-1, 8, 4), (2, -8, 4), (2, 8, -4)):
        assert lib.nrt_dense_f32(d, d, d, d, batch, cin, cout, 0, 0, d, big, None) == inv
        assert lib.nrt_dense_bwd_f32(d, d, d, d, d, d, batch, cin, cout, 0, d, big, None) == inv
        assert lib.nrt_dense_workspace_bytes(batch, cin, cout, 0) == 0
    for act in (-1, 11, 0x100):
        assert lib.nrt_dense_f32(d, d, d, d, 2, 8, 4, act, 0, d, big, None) == inv
    for variant in (-1, 3):
        assert lib.nrt_dense_f32(d, d, d, d, 2, 8, 4, 0, variant, d, big, None) == inv
        assert lib.nrt_dense_bwd_f32(d, d, d, d, d, d, 2, 8, 4, variant, d, big, None) == inv
    # in * out >= 2^31
    for cin, cout in ((1 << 16, 1 << 15), (1 << 15, 1 << 16), (1 << 30, 2), (46341, 46341)):
        assert lib.nrt_dense_f32(d, d, d, d, 2, cin, cout, 0, 0, d, big, None) == unsup
        assert lib.nrt_dense_bwd_f32(d, d, d, d, d, d, 2, cin, cout, 0, d, big, None) == unsup
    # backward: (g, x, w, gx, gw, gbias, batch, in, out, variant, workspace, workspace_bytes, stream)
    assert lib.nrt_dense_bwd_f32(None, d, d, d, d, d, 2, 8, 4, 0, d, big, None) == inv
    assert lib.nrt_dense_bwd_f32(d, d, None, d, None, None, 2, 8, 4, 0, d, big, None) == inv          # gx needs w
    assert lib.nrt_dense_bwd_f32(d, None, d, None, d, None, 2, 8, 4, 0, d, big, None) == inv          # gw needs x
    # a missing or short workspace is refused before the launch that would write it
    need = lib.nrt_dense_workspace_bytes(2, 4096, 64, 1)
    assert need > 0
    assert lib.nrt_dense_f32(d, d, d, d, 2, 4096, 64, 0, 1, None, 0, None) == _lib.NRT_ERR_WORKSPACE
    assert lib.nrt_dense_f32(d, d, d, d, 2, 4096, 64, 0, 1, 256, 4, None) == _lib.NRT_ERR_WORKSPACE
    assert lib.nrt_dense_bwd_f32(d, d, d, d, None, None, 2, 4096, 64, 1, None, 0, None) == _lib.NRT_ERR_WORKSPACE


def test_workspace_is_zero_where_no_partials_are_written():
    lib = _lib.lib()
    assert lib.nrt_dense_workspace_bytes(4, 7, 12, 2) == 0               # expand arm forced, one block spans a row in the backward
    assert lib.nrt_dense_workspace_bytes(4, 64, 1 << 20, 2) > 0          # gx of a wide row goes through partials
    # the reduce arm: slabs x chunk x out floats; a batch beyond 16 runs in chunks of 16 and needs no more than one chunk does
    assert lib.nrt_dense_workspace_bytes(16, 70001, 12, 1) == lib.nrt_dense_workspace_bytes(33, 70001, 12, 1)


def test_sample_layer_has_the_reference_interface():
    assert 'SampleNormalLogVar' in L.__all__ and hasattr(ne.layers, 'SampleNormalLogVar')
    here = sigs.signature(os.path.join(ROOT, 'neurite_amd', 'layers.py'), 'SampleNormalLogVar')
    assert here == REFERENCE_SIGNATURES[sigs.key('tf/layers.py', 'SampleNormalLogVar')]
    lay = L.SampleNormalLogVar(name='z')
    assert lay.name == 'z' and sorted(lay.get_config()) == ['name']
    assert L.SampleNormalLogVar().name == 'samplenormallogvar'
    assert lay.compute_output_shape([(None, 5), (None, 5)]) == (None, 5)
    with pytest.raises(TypeError):
        L.SampleNormalLogVar(sigma=1.0)
    # float32 only, refused before the device is looked at
    with pytest.raises(NotImplementedError, match='float32'):
        lay([torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 5, dtype=torch.float64)])
    with pytest.raises(_lib.NeuriteAmdError, match='no CPU fallback'):
        lay([torch.zeros(2, 5), torch.zeros(2, 5)])


@pytest.mark.parametrize('name', ['ae', 'single_ae'])
def test_builder_signatures_equal_the_reference(name):
    here = sigs.signature(os.path.join(ROOT, 'neurite_amd', 'models.py'), name)
    assert here == REFERENCE_SIGNATURES[sigs.key('tf/models.py', name)]
    assert name in models.__all__


def test_graph_valued_arguments_raise_as_in_conv_enc():
    for kw in ({'src': object()}, {'src_input': object()}):
        with pytest.raises(NotImplementedError, match='Keras-graph arguments'):
            _quiet(models.ae, 4, (8, 8, 1), 2, 3, 3, [5], ae_type='dense', **kw)
    with pytest.raises(TypeError, match='input_model'):
        _quiet(models.single_ae, [5], None, input_model=object())


def test_batch_norm_axis_must_be_the_last_one():
    # the default batch_norm=True is Keras' axis 1: the last axis of a [B, E] tensor, not of a [B, 4, 4, 4, 3] one
    net = _quiet(models.single_ae, [5], (12,))
    assert [op['name'] for op in net.ops if op['kind'] == 'bn'] == ['single_ae_ae_mu_bn', 'single_ae_bn_ae_dense_dec']
    with pytest.raises(NotImplementedError, match='single_ae_bn_ae_dense_dec'):
        _quiet(models.single_ae, [6], (4, 4, 4, 3))
    with pytest.raises(NotImplementedError, match='single_ae_ae_mu_bn'):
        _quiet(models.single_ae, (4, 4, 4, 5), (4, 4, 4, 3), ae_type='conv', conv_size=3, batch_norm=2)
    _quiet(models.single_ae, (4, 4, 4, 5), (4, 4, 4, 3), ae_type='conv', conv_size=3, batch_norm=4)
    _quiet(models.single_ae, [6], (4, 4, 4, 3), batch_norm=-1)


def test_a_bottleneck_without_a_feature_count_needs_equal_spatial_sizes():
    """enc_size[-1] = None is the pass-through branch only where the spatial sizes agree (neurite/tf/models.py:506-524); with other
    sizes the reference reaches Conv3D(filters=None) and fails, and so does this builder"""
    with pytest.raises(TypeError):
        _quiet(models.single_ae, (2, 2, 2, None), (4, 4, 4, 3), ae_type='conv', conv_size=3, batch_norm=None)
    net = _quiet(models.single_ae, (4, 4, 4, None), (4, 4, 4, 3), ae_type='conv', conv_size=3, batch_norm=None)
    assert net.get_layer('single_ae_ae_mu_enc')['kind'] == 'identity'


def test_bf16_networks_with_these_layers_are_refused_on_cpu_tensors():
    net = _quiet(models.single_ae, [6], (4, 4, 4, 3), batch_norm=None).bfloat16()
    with pytest.raises(NotImplementedError, match='single_ae_ae_dense_down_flat'):
        net(torch.zeros(1, 4, 4, 4, 3))
    net = _quiet(models.ae, 4, (8, 8, 1), 2, 3, 3, (4, 4, 2), single_model=True, do_vae=True).bfloat16()
    with pytest.raises(NotImplementedError, match='ae_ae_mu:'):                   # the first such layer in graph order
        net(torch.zeros(1, 8, 8, 1))


def test_enc_lambda_layers_are_named_by_their_function():
    def softsign(x):
        return x / (1 + x.abs())
    net = _quiet(models.single_ae, [6], (4, 4, 4, 3), batch_norm=None, do_vae=True, enc_lambda_layers=[softsign])
    names = net.layer_names
    assert names.index('single_ae_ae_mu_softsign') == names.index('single_ae_ae_mu_enc_dense_6') + 1
    assert names.index('single_ae_ae_sigma_softsign') == names.index('single_ae_ae_sigma_enc_dense_6') + 1
    assert net.get_layer('single_ae_ae_mu_softsign')['fn'] is softsign
    assert not net.config['loadable'] and net.config['params']['enc_lambda_layers'] is None


def test_ae_returns_three_models_or_one():
    dec, mid, enc = _quiet(models.ae, 4, (8, 8, 1), 2, 3, 3, [5], ae_type='dense')
    assert [m.config['builder'] for m in (dec, mid, enc)] == ['conv_dec', 'single_ae', 'conv_enc']
    assert tuple(mid.input_shapes[0]) == (4, 4, 4) and tuple(dec.input_shapes[0]) == (4, 4, 4)
    one = _quiet(models.ae, 4, (8, 8, 1), 2, 3, 3, [5], ae_type='dense', single_model=True)
    assert one.config['builder'] == 'ae' and one.config['loadable']
    assert one.layer_names == enc.layer_names + mid.layer_names[1:] + dec.layer_names[1:]
