"""
Record the layer graphs the REFERENCE's own `models.design_dnn` (neurite/tf/models.py:1620-1775) and `models.EncoderNet` (:1782-1848)
build, into tests/golden/classifier_graph.json (the format of unet_graph.json / ae_graph.json; a case whose builder raises is stored
as `error` = {type, message}), and the AST signatures of the two builders and of `layers.RescaleValues` / `layers.Negate` into the
same file under `__signatures__`.

    python tests/golden/make_classifier_golden.py PATH/TO/REFERENCE        # the directory that holds the reference's `neurite` package

TEST INFRASTRUCTURE, run once where a checkout of the reference exists; tests/test_classifier_graph.py reads only the JSON.  The
builders run on tests/golden/tf_shim.py + keras_record.py as make_golden.py runs the U-Net builders.  Added here, without touching
those files:
  * the Dense / Flatten / Reshape recorders of make_ae_golden.py, and one for GlobalMaxPooling3D;
  * Conv{1,2,3}D recorders that also keep a `kernel_constraint`, and a recording `maxnorm` set on the reference's models module (the
    shim has none);
  * a Lambda recorder that follows `K.batch_flatten` and `K.max` (design_dnn's _global_max_nd) besides the pass-through softmax;
  * a recording stand-in for the reference's own RescaleValues, swapped into its `layers` module while a builder runs.
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
from make_ae_golden import Dense, Flatten, Reshape  # noqa: E402


class GlobalMaxPooling3D(keras_record._KLayer):
    keras_class = 'GlobalMaxPooling3D'
    auto_base = 'global_max_pooling3d'

    def out_shape(self, shapes):
        assert len(shapes[0]) == 5, (self.name, shapes[0])
        return (shapes[0][0], shapes[0][-1])


class MaxNorm:
    """tensorflow.python.keras.constraints.maxnorm: MaxNorm(max_value=2, axis=0)"""

    def __init__(self, max_value=2, axis=0):
        self.max_value, self.axis = max_value, axis


def _with_constraint(base):
    class Conv(base):
        def __init__(self, *args, kernel_constraint=None, **kw):
            super().__init__(*args, **kw)
            self.kernel_constraint = kernel_constraint

        def config(self):
            cfg = super().config()
            if self.kernel_constraint is not None:
                assert isinstance(self.kernel_constraint, MaxNorm), self.kernel_constraint
                cfg['kernel_constraint'] = {'class': 'MaxNorm', 'max_value': self.kernel_constraint.max_value,
                                            'axis': self.kernel_constraint.axis}
            return cfg
    Conv.__name__ = base.__name__
    return Conv


Conv1D, Conv2D, Conv3D = (_with_constraint(c) for c in (keras_record.Conv1D, keras_record.Conv2D, keras_record.Conv3D))


def k_batch_flatten(x):
    n = 1
    for v in x.shape[1:]:
        n *= int(v)
    keras_record._LAMBDA_TRACE.append(('batch_flatten',))
    return keras_record._Probe((x.shape[0], n), x._layer)


def k_max(x, axis=None, keepdims=False):
    assert isinstance(axis, int) and axis > 0, axis
    keras_record._LAMBDA_TRACE.append(('max', int(axis), bool(keepdims)))
    shape = list(x.shape)
    if keepdims:
        shape[axis] = 1
    else:
        del shape[axis]
    return keras_record._Probe(tuple(shape), x._layer)


class Lambda(keras_record.Lambda):
    """a Lambda whose function may change the shape through the two backend calls above"""

    def out_shape(self, shapes):
        del keras_record._LAMBDA_TRACE[:]
        r = self.function(keras_record._Probe(shapes[0], self))
        assert isinstance(r, keras_record._Probe), 'Lambda %s: only K.batch_flatten / K.max / activations are modelled' % self.name
        self.trace = [list(t) for t in keras_record._LAMBDA_TRACE]
        return tuple(r.shape)


class RescaleValues(keras_record._KLayer):
    """neurite/tf/layers.py:67-88"""
    keras_class = 'RescaleValues'
    auto_base = 'rescale_values'

    def __init__(self, resize, name=None, **kw):
        super().__init__(name=name)
        self.resize = resize

    def config(self):
        return {'resize': self.resize}


# (tag, builder, args, kwargs)
CASES = [
    ('dnn_dense_sigmoid', 'design_dnn', [4, [8, 8, 8], 2, 3, 2], {}),
    ('dnn_dense_softmax', 'design_dnn', [4, [8, 8, 8], 2, 3, 3], {'final_layer': 'dense-softmax', 'nb_input_features': 2}),
    ('dnn_globalmaxpooling', 'design_dnn', [4, [8, 9, 10], 2, 3, 2], {'final_layer': 'globalmaxpooling'}),
    ('dnn_myglobalmaxpooling_bn_last', 'design_dnn', [4, [8, 8, 8], 2, 3, 2], {'final_layer': 'myglobalmaxpooling', 'batch_norm': -1}),
    ('dnn_2d_dense_sigmoid', 'design_dnn', [4, [10, 12], 2, 3, 2], {'name': 'dnn2d'}),
    ('dnn_maxpool', 'design_dnn', [4, [8, 8, 12], 2, 3, 2], {'use_strided_convolution_maxpool': False}),
    ('dnn_dropout', 'design_dnn', [4, [8, 8, 8], 2, 3, 2], {'conv_dropout': 0.2}),
    ('dnn_maxnorm', 'design_dnn', [4, [8, 8, 8], 2, 3, 2], {'conv_maxnorm': 2}),
    ('dnn_feat_mult', 'design_dnn', [4, [8, 8, 8], 2, 3, 2], {'feat_mult': 2, 'nb_conv_per_level': 1}),
    ('dnn_pool_221', 'design_dnn', [4, [8, 8, 8], 2, 3, 2], {'pool_size': [2, 2, 1]}),
    ('dnn_unknown_final', 'design_dnn', [4, [8, 8, 8], 2, 3, 2], {'final_layer': 'no-such-layer'}),
    ('dnn_dense_tanh', 'design_dnn', [4, [8, 8, 8], 2, 3, 2], {'final_layer': 'dense-tanh'}),
    ('enc_default', 'EncoderNet', [4, [8, 8, 8, 1], 2, 3], {}),
    ('enc_dropout', 'EncoderNet', [4, [8, 8, 8, 1], 2, 3], {'dropout': 0.3, 'dense_size': 16}),
    ('enc_rescale', 'EncoderNet', [4, [8, 8, 8, 1], 2, 3], {'rescale': 0.5, 'dense_size': 16}),
    ('enc_regression', 'EncoderNet', [4, [8, 8, 8, 1], 2, 3], {'nb_labels': 0, 'dense_size': 16}),
    ('enc_sigmoid', 'EncoderNet', [4, [8, 8, 8, 1], 2, 3], {'final_activation': 'sigmoid', 'dense_size': 16, 'nb_labels': 3}),
    ('enc_batch_norm', 'EncoderNet', [4, [8, 8, 8, 1], 2, 3], {'batch_norm': -1, 'dense_size': 16}),
    ('enc_residuals', 'EncoderNet', [4, [8, 8, 8, 2], 2, 3], {'use_residuals': True, 'dense_size': 16, 'name': 'encnet'}),
]

SIGNATURES = [('tf/models.py', 'design_dnn'), ('tf/models.py', 'EncoderNet'), ('tf/layers.py', 'RescaleValues'), ('tf/layers.py', 'Negate')]


def main(ref_root):
    sys.path.insert(0, ref_root)
    import tensorflow.keras.layers as KL
    import tensorflow.keras.backend as K
    for cls in (Dense, Flatten, Reshape, GlobalMaxPooling3D, Conv1D, Conv2D, Conv3D, Lambda):
        setattr(KL, cls.__name__, cls)
    K.batch_flatten, K.max = k_batch_flatten, k_max
    import neurite as ne
    ref_models = sys.modules[ne.models.__name__]
    ref_layers = ref_models.layers
    ref_models.maxnorm = MaxNorm
    out = {}
    for tag, builder, args, kwargs in CASES:
        keras_record.reset()
        saved = ref_layers.RescaleValues
        entry = {'builder': builder, 'args': args, 'kwargs': kwargs}
        try:
            ref_layers.RescaleValues = RescaleValues
            with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                warnings.simplefilter('ignore')
                res = getattr(ne.models, builder)(*args, **kwargs)
            entry['graph'] = res.graph()
        except Exception as e:   # noqa: the reference's own error is the record
            entry['error'] = {'type': type(e).__name__, 'message': str(e)}
        finally:
            ref_layers.RescaleValues = saved
        out[tag] = entry
    pkg = os.path.join(ref_root, 'neurite')
    out['__signatures__'] = {ast_signatures.key(f, n): ast_signatures.signature(os.path.join(pkg, f), n) for f, n in SIGNATURES}
    path = os.path.join(HERE, 'classifier_graph.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%-28s %7.1f KB  (%d cases, %d errors)' % ('classifier_graph.json', os.path.getsize(path) / 1024, len(CASES),
                                                     sum('error' in v for v in out.values() if isinstance(v, dict))))


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], 'neurite', '__init__.py')):
        raise SystemExit('usage: python tests/golden/make_classifier_golden.py PATH/TO/REFERENCE   (the directory holding the `neurite` package)')
    main(sys.argv[1])
