"""
Record the layer graphs the REFERENCE's own `models.single_ae` (neurite/tf/models.py:438-646) and `models.ae` (:249-375) build, into
tests/golden/ae_graph.json (the format of unet_graph.json; `ae` in tuple form stores its three graphs as `graphs` = [decoder, middle,
encoder]), and the AST signatures of `ae`, `single_ae` and `layers.SampleNormalLogVar` into the same file under `__signatures__`.

    python tests/golden/make_ae_golden.py PATH/TO/REFERENCE        # the directory that holds the reference's `neurite` package

TEST INFRASTRUCTURE, run once where a checkout of the reference exists; tests/test_ae_graph.py and tests/test_ae_abi.py read only the
JSON.  The builders run on tests/golden/tf_shim.py + keras_record.py as make_golden.py runs the U-Net builders.  Two things are added
here, without touching those files:
  * recorders for the three Keras layers keras_record lacks (Dense, Flatten, Reshape), set on the shim's tensorflow.keras.layers;
  * recording stand-ins for the reference's own Resize, LocalBias and SampleNormalLogVar, swapped into its `layers` module while a
    builder runs: they are Keras Layer subclasses whose call() needs real tensors, the builders only need name, arguments and shape.
"""

import contextlib
import io
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tf_shim  # noqa: E402

tf_shim.install()
import keras_record  # noqa: E402
import ast_signatures  # noqa: E402


class Flatten(keras_record._KLayer):
    keras_class = 'Flatten'
    auto_base = 'flatten'

    def out_shape(self, shapes):
        n = 1
        for v in shapes[0][1:]:
            n *= int(v)
        return (shapes[0][0], n)


class Dense(keras_record._KLayer):
    keras_class = 'Dense'
    auto_base = 'dense'

    def __init__(self, units, activation=None, use_bias=True, name=None, **kw):
        super().__init__(name=name)
        self.units, self.activation, self.use_bias = int(units), keras_record._act_name(activation), bool(use_bias)

    def config(self):
        return {'units': self.units, 'activation': self.activation, 'use_bias': self.use_bias}

    def out_shape(self, shapes):
        assert len(shapes[0]) == 2, (self.name, shapes[0])
        return (shapes[0][0], self.units)


class Reshape(keras_record._KLayer):
    keras_class = 'Reshape'
    auto_base = 'reshape'

    def __init__(self, target_shape, name=None, **kw):
        super().__init__(name=name)
        self.target_shape = [int(v) for v in target_shape]

    def config(self):
        return {'target_shape': list(self.target_shape)}

    def out_shape(self, shapes):
        n = 1
        for v in shapes[0][1:]:
            n *= int(v)
        m = 1
        for v in self.target_shape:
            m *= v
        assert n == m, (self.name, shapes[0], self.target_shape)
        return (shapes[0][0],) + tuple(self.target_shape)


class Resize(keras_record._KLayer):
    """neurite/tf/layers.py:91-181: constructor arguments and compute_output_shape"""
    keras_class = 'Resize'
    auto_base = 'resize'

    def __init__(self, zoom_factor, interp_method='linear', name=None, **kw):
        super().__init__(name=name)
        self.zoom_factor, self.interp_method = zoom_factor, interp_method

    def config(self):
        return {'zoom_factor': [float(z) for z in self.zoom_factor], 'interp_method': self.interp_method}

    def out_shape(self, shapes):
        s = shapes[0]
        nd = len(s) - 2
        zf = list(self.zoom_factor) if isinstance(self.zoom_factor, (list, tuple)) else [self.zoom_factor] * nd
        assert len(zf) == nd
        self.zoom_factor = zf
        return (s[0],) + tuple(int(s[1 + f] * zf[f]) for f in range(nd)) + (s[-1],)


class LocalBias(keras_record._KLayer):
    """neurite/tf/layers.py:746-774"""
    keras_class = 'LocalBias'
    auto_base = 'local_bias'

    def __init__(self, my_initializer='RandomNormal', biasmult=1.0, name=None, **kw):
        super().__init__(name=name)
        self.my_initializer, self.biasmult = my_initializer, float(biasmult)

    def config(self):
        return {'my_initializer': self.my_initializer, 'biasmult': self.biasmult}


class SampleNormalLogVar(keras_record._KLayer):
    """neurite/tf/layers.py:2261-2302: two inputs, the shape of the first"""
    keras_class = 'SampleNormalLogVar'
    auto_base = 'sample_normal_log_var'

    def out_shape(self, shapes):
        assert len(shapes) == 2 and tuple(shapes[0]) == tuple(shapes[1]), (self.name, shapes)
        return shapes[0]


# (tag, builder, args, kwargs)
CASES = [
    ('sae_dense', 'single_ae', [[6], [4, 4, 4, 3]], {'batch_norm': None}),
    ('sae_dense_vae', 'single_ae', [[6], [4, 4, 4, 3]], {'batch_norm': None, 'do_vae': True}),
    ('sae_dense_vae_shift', 'single_ae', [[6], [4, 4, 4, 3]], {'batch_norm': None, 'do_vae': True, 'include_mu_shift_layer': True}),
    ('sae_dense_shift', 'single_ae', [[6], [4, 4, 4, 3]], {'batch_norm': None, 'include_mu_shift_layer': True}),
    ('sae_dense_flat_bn_default', 'single_ae', [[5], [12]], {}),
    ('sae_dense_flat_bn_default_vae', 'single_ae', [[5], [12]], {'do_vae': True}),
    ('sae_dense_bn_last', 'single_ae', [[6], [4, 4, 3]], {'batch_norm': -1, 'do_vae': True, 'activation': None}),
    ('sae_conv_resize', 'single_ae', [[2, 2, 2, 4], [4, 4, 4, 3]], {'ae_type': 'conv', 'conv_size': 3, 'batch_norm': None}),
    ('sae_conv_resize_vae', 'single_ae', [[2, 2, 2, 4], [4, 4, 4, 3]],
     {'ae_type': 'conv', 'conv_size': 3, 'batch_norm': None, 'do_vae': True, 'include_mu_shift_layer': True}),
    ('sae_conv_passthrough', 'single_ae', [[4, 4, 4, None], [4, 4, 4, 3]], {'ae_type': 'conv', 'conv_size': 3, 'batch_norm': None}),
    ('sae_conv_passthrough_vae', 'single_ae', [[4, 4, 4, None], [4, 4, 4, 3]],
     {'ae_type': 'conv', 'conv_size': 3, 'batch_norm': None, 'do_vae': True}),
    ('sae_conv_plain', 'single_ae', [[4, 4, 4, 5], [4, 4, 4, 3]], {'ae_type': 'conv', 'conv_size': 3, 'batch_norm': -1, 'activation': 'elu'}),
    ('sae_conv_plain_vae_2d', 'single_ae', [[6, 5, 2], [6, 5, 3]], {'ae_type': 'conv', 'conv_size': [3, 1], 'batch_norm': None, 'do_vae': True,
                                                                      'padding': 'same'}),
    ('ae_2d_dense_tuple', 'ae', [4, [8, 8, 1], 2, 3, 3, [5]], {'ae_type': 'dense'}),
    ('ae_2d_dense_single', 'ae', [4, [8, 8, 1], 2, 3, 3, [5]], {'ae_type': 'dense', 'single_model': True}),
    ('ae_2d_dense_vae_prior_single', 'ae', [4, [8, 8, 1], 2, 3, 3, [5]],
     {'ae_type': 'dense', 'single_model': True, 'do_vae': True, 'add_prior_layer': True, 'enc_batch_norm': -1}),
    ('ae_3d_conv_tuple', 'ae', [2, [4, 4, 4, 1], 2, 3, 2, [2, 2, 2, 3]], {}),
    ('ae_3d_conv_vae_prior_single', 'ae', [2, [4, 4, 4, 1], 2, 3, 2, [2, 2, 2, 3]],
     {'do_vae': True, 'add_prior_layer': True, 'single_model': True}),
    ('ae_3d_conv_vae_prior_tuple', 'ae', [2, [4, 4, 4, 1], 2, 3, 2, [2, 2, 2, 3]], {'do_vae': True, 'add_prior_layer': True}),
    ('ae_3d_dense_resid_bn_single', 'ae', [3, [4, 4, 4, 2], 2, 3, 2, [4]],
     {'ae_type': 'dense', 'single_model': True, 'use_residuals': True, 'nb_conv_per_level': 2, 'batch_norm': -1, 'feat_mult': 2,
      'include_mu_shift_layer': True, 'final_pred_activation': 'linear'}),
]

SIGNATURES = [('tf/models.py', 'ae'), ('tf/models.py', 'single_ae'), ('tf/layers.py', 'SampleNormalLogVar')]


def graph_of(model):
    """model.graph(), with the input layers of OTHER models dropped: `ae` in tuple form builds three models whose inputs share one
    name (`<name>_input`), and keras_record keeps its records by name -- a model's own input is the one with its input tensor's shape"""
    g = model.graph()
    own = {t._layer.name: [None if v is None else int(v) for v in t.shape] for t in model.inputs}
    layers, seen = [], set()
    for r in g['layers']:
        if r['class'] == 'InputLayer' and r['name'] in own and (r['output_shape'] != own[r['name']] or r['name'] in seen):
            continue
        seen.add(r['name'])
        layers.append(r)
    g['layers'] = layers
    return g


def main(ref_root):
    sys.path.insert(0, ref_root)
    import tensorflow.keras.layers as KL
    for cls in (Dense, Flatten, Reshape):
        setattr(KL, cls.__name__, cls)
    import neurite as ne
    ref_layers = sys.modules[ne.models.__name__].layers
    out = {}
    for tag, builder, args, kwargs in CASES:
        keras_record.reset()
        saved = {k: getattr(ref_layers, k) for k in ('Resize', 'LocalBias', 'SampleNormalLogVar')}
        try:
            for cls in (Resize, LocalBias, SampleNormalLogVar):
                setattr(ref_layers, cls.__name__, cls)
            with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                warnings.simplefilter('ignore')
                res = getattr(ne.models, builder)(*args, **kwargs)
        finally:
            for k, v in saved.items():
                setattr(ref_layers, k, v)
        entry = {'builder': builder, 'args': args, 'kwargs': kwargs}
        if isinstance(res, tuple):
            entry['graphs'] = [graph_of(m) for m in res]
        else:
            entry['graph'] = graph_of(res)
        out[tag] = entry
    pkg = os.path.join(ref_root, 'neurite')
    out['__signatures__'] = {ast_signatures.key(f, n): ast_signatures.signature(os.path.join(pkg, f), n) for f, n in SIGNATURES}
    path = os.path.join(HERE, 'ae_graph.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%-28s %7.1f KB  (%d cases)' % ('ae_graph.json', os.path.getsize(path) / 1024, len(CASES)))


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], 'neurite', '__init__.py')):
        raise SystemExit('usage: python tests/golden/make_ae_golden.py PATH/TO/REFERENCE   (the directory holding the `neurite` package)')
    main(sys.argv[1])
