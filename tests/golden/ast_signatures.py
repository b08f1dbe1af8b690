"""
Public signatures by AST: argument names, order, defaults, *args / **kwargs of a function or class (its __init__) in a
source file, without importing it.  tests/test_reference_switch.py compares neurite_amd's signatures with the reference's, which
this script records once into reference_signatures.json from a checkout of the reference (TEST INFRASTRUCTURE):

    python tests/golden/ast_signatures.py PATH/TO/neurite        # the reference's package directory (neurite/__init__.py, tf/, py/)

The same run records two facts of the reference's backend switch (neurite/__init__.py:33-42) that the switch tests rely on.
"""

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'reference_signatures.json')

SIGNATURES = [        # (reference file, reference name, neurite_amd file, neurite_amd name)
    ('tf/utils/utils.py', 'interpn', 'utils.py', 'interpn'),
    ('tf/utils/utils.py', 'resize', 'utils.py', 'resize'),
    ('tf/utils/utils.py', 'zoom', 'utils.py', 'zoom'),
    ('tf/utils/utils.py', 'volshape_to_ndgrid', 'utils.py', 'volshape_to_ndgrid'),
    ('tf/utils/utils.py', 'volshape_to_meshgrid', 'utils.py', 'volshape_to_meshgrid'),
    ('tf/layers.py', 'Resize', 'layers.py', 'Resize'),
    ('tf/layers.py', 'Zoom', 'layers.py', 'Zoom'),
    ('tf/layers.py', 'LocallyConnected3D', 'layers.py', 'LocallyConnected3D'),
    ('tf/models.py', 'unet', 'models.py', 'unet'),
    ('tf/models.py', 'conv_enc', 'models.py', 'conv_enc'),
    ('tf/models.py', 'conv_dec', 'models.py', 'conv_dec'),
    ('tf/metrics.py', 'Dice', 'metrics.py', 'Dice'),
    ('tf/metrics.py', 'Dice.dice', 'metrics.py', 'Dice.dice'),
    ('tf/metrics.py', 'Dice.mean_dice', 'metrics.py', 'Dice.mean_dice'),
    ('tf/metrics.py', 'Dice.loss', 'metrics.py', 'Dice.loss'),
    ('tf/metrics.py', 'SoftDice', 'metrics.py', 'SoftDice'),
    ('tf/metrics.py', 'HardDice', 'metrics.py', 'HardDice'),
    ('tf/metrics.py', 'CategoricalCrossentropy', 'metrics.py', 'CategoricalCrossentropy'),
    ('tf/metrics.py', 'CategoricalCrossentropy.cce', 'metrics.py', 'CategoricalCrossentropy.cce'),
    ('tf/metrics.py', 'CategoricalCrossentropy.__call__', 'metrics.py', 'CategoricalCrossentropy.__call__'),
    ('tf/losses.py', 'Dice.loss', 'losses.py', 'Dice.loss'),
    ('tf/losses.py', 'Dice.mean_loss', 'losses.py', 'Dice.mean_loss'),
    ('tf/losses.py', 'CategoricalCrossentropy.loss', 'losses.py', 'CategoricalCrossentropy.loss'),
]

# The availability check of the reference's switch as it ships (neurite/__init__.py:33-39) and the check INTEGRATION.md section 1
# replaces it with; the switch imports its sub-package right after it
SWITCH_AS_SHIPPED = """    try:
        import torch
    except ImportError:
        raise ImportError('Please install pytorch to use this neurite backend')
"""
SWITCH_PATCHED = """    import importlib.util
    if importlib.util.find_spec('torch') is None:
        raise ImportError('Please install pytorch to use this neurite backend')
"""
SWITCH_SUBPACKAGE_IMPORT = '    from . import torch\n'


def key(ref_file, ref_name):
    return ref_file + '::' + ref_name


def _find(tree, qual):
    node = tree
    for part in qual.split('.'):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.FunctionDef, ast.ClassDef)) and child.name == part:
                node = child
                break
            if isinstance(child, ast.Assign) and any(isinstance(t, ast.Name) and t.id == part for t in child.targets):
                node = child                      # an alias: `zoom = resize`
                break
        else:
            raise KeyError(qual)
    return node


def _value(node):
    try:
        return repr(ast.literal_eval(node))
    except Exception:       # noqa
        return ast.unparse(node)


def _signature(fn):
    a = fn.args
    pos = [x.arg for x in a.posonlyargs + a.args]
    defaults = [_value(d) for d in a.defaults]
    kwonly = [[x.arg, None if d is None else _value(d)] for x, d in zip(a.kwonlyargs, a.kw_defaults)]
    return {'args': pos, 'defaults': defaults, 'vararg': a.vararg.arg if a.vararg else None, 'kwonly': kwonly,
            'kwarg': bool(a.kwarg)}


_trees = {}


def _tree(path):
    if path not in _trees:
        _trees[path] = ast.parse(open(path).read())
    return _trees[path]


def _resolve(path, qual):
    try:
        node = _find(_tree(path), qual)
    except KeyError:
        # a method inherited from a base class defined in the same file (neurite_amd.losses keeps loss / mean_loss in one mixin)
        cls, _, meth = qual.rpartition('.')
        if not cls:
            raise
        for base in _find(_tree(path), cls).bases:
            try:
                return _resolve(path, ast.unparse(base) + '.' + meth)
            except KeyError:
                continue
        raise
    if isinstance(node, ast.Assign):                                     # alias -> what it names
        return _resolve(path, ast.unparse(node.value))
    if isinstance(node, ast.ClassDef):
        return _find(node, '__init__')
    return node


def signature(path, qual):
    """{'args', 'defaults', 'vararg', 'kwonly', 'kwarg'} of `qual` in the source file `path` (JSON-shaped: lists, no tuples)"""
    return _signature(_resolve(path, qual))


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def main(ref):
    init = open(os.path.join(ref, '__init__.py')).read()
    out = {'signatures': {key(rf, rn): signature(os.path.join(ref, rf), rn) for rf, rn, _, _ in SIGNATURES},
           'switch': {'as_shipped_check_present': SWITCH_AS_SHIPPED in init,
                      'imports_torch_subpackage_after_the_check': SWITCH_AS_SHIPPED + '\n' + SWITCH_SUBPACKAGE_IMPORT in init}}
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', FIXTURE)


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], '__init__.py')):
        raise SystemExit('usage: python tests/golden/ast_signatures.py PATH/TO/neurite   (the reference package directory)')
    main(sys.argv[1])
