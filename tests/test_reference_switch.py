"""
The drop-in boundary checked against the reference, self-contained: what is taken from the reference tree is recorded
in tests/golden/reference_signatures.json by tests/golden/ast_signatures.py; nothing here touches a device.

1. The reference's own backend switch (neurite/__init__.py:33-42, neurite/py/utils.py:15-20): with NEURITE_BACKEND=pytorch it does
   `from . import torch`, a sub-package it does not ship.  INTEGRATION.md section 1 gives the 8-line neurite/torch/__init__.py a
   maintainer adds; the test builds that overlay (a stand-in `neurite` package whose switch is the reference's availability check --
   as shipped or as INTEGRATION.md repairs it -- followed by `from . import torch`, plus the binding copied OUT OF INTEGRATION.md) in a
   temp directory, imports `neurite` through it and checks that ne.torch.* are the neurite_amd objects.  The fixture records that the
   reference's switch is exactly that check followed by that import.
2. Every public signature SURVEY 8(b) lists is compared by AST with the reference's, as the fixture records them: argument names,
   order, defaults, *args / **kwargs.
"""

import os
import re
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import ast_signatures as sigs          # noqa: E402

REFERENCE = sigs.load()


def _binding_from_integration_md():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    m = re.search(r'```python\n(# neurite/torch/__init__\.py.*?)```', text, re.S)
    assert m, 'INTEGRATION.md no longer shows the neurite/torch/__init__.py binding'
    return m.group(1)


# The switch as the reference ships it cannot reach ANY neurite/torch sub-package: `import torch` (the availability check) binds the
# name `torch` in the package namespace, and the `from . import torch` two lines later finds that attribute and never imports the
# sub-package -- `neurite.torch` is then PyTorch itself.  INTEGRATION.md section 1 therefore lists a two-line change of the check
# next to the new file; the test applies exactly that change to the stand-in's switch.
SWITCH_AS_SHIPPED = sigs.SWITCH_AS_SHIPPED
SWITCH_PATCHED = sigs.SWITCH_PATCHED

# the stand-in for the reference's neurite/__init__.py: its backend switch, nothing else (the TensorFlow branch is never taken here)
STANDIN_INIT = """import os
backend = os.environ.get('NEURITE_BACKEND', 'tensorflow')
if backend == 'pytorch':
%s
%s"""


def _overlay(tmp_path, patched):
    sw = REFERENCE['switch']
    assert sw['as_shipped_check_present'] and sw['imports_torch_subpackage_after_the_check'], \
        'neurite/__init__.py:33-42 changed upstream: update INTEGRATION.md section 1'
    assert SWITCH_PATCHED in open(os.path.join(ROOT, 'INTEGRATION.md')).read(), 'INTEGRATION.md must show the patched check'
    pkg = tmp_path / 'neurite'
    (pkg / 'torch').mkdir(parents=True)
    (pkg / '__init__.py').write_text(STANDIN_INIT % (SWITCH_PATCHED if patched else SWITCH_AS_SHIPPED, sigs.SWITCH_SUBPACKAGE_IMPORT))
    (pkg / 'torch' / '__init__.py').write_text(_binding_from_integration_md())


def _run(script, tmp_path):
    head = textwrap.dedent('''
        import os, sys
        sys.path.insert(0, %r)
        sys.path.insert(0, %r)
        import neurite as ne
        import neurite_amd
    ''') % (ROOT, str(tmp_path))
    env = dict(os.environ, NEURITE_BACKEND='pytorch', MPLBACKEND='Agg')
    return subprocess.run([sys.executable, '-c', head + textwrap.dedent(script)], env=env, capture_output=True, text=True, timeout=300)


def test_reference_switch_as_shipped_shadows_its_own_subpackage(tmp_path):
    """the upstream defect the integration note has to work around (neurite/__init__.py:33-42)"""
    _overlay(tmp_path, patched=False)
    p = _run('''
        import torch
        assert ne.torch is torch, 'upstream changed: the shipped switch now reaches its sub-package'
        print('SHADOWED')
    ''', tmp_path)
    assert p.returncode == 0 and 'SHADOWED' in p.stdout, p.stderr[-3000:]


def test_reference_backend_switch_resolves_to_neurite_amd(tmp_path):
    _overlay(tmp_path, patched=True)
    p = _run('''
        assert ne.backend == 'pytorch'
        assert not hasattr(ne, 'tf'), 'the TensorFlow backend must not have been imported'
        assert ne.torch.backend == 'pytorch'
        for mod in ('utils', 'layers', 'metrics', 'losses', 'models', 'augment'):
            assert getattr(ne.torch, mod) is getattr(neurite_amd, mod), mod
        assert ne.torch.utils.interpn is neurite_amd.utils.interpn and ne.torch.interpn is neurite_amd.utils.interpn
        assert ne.torch.layers.Resize is neurite_amd.layers.Resize and ne.torch.layers.Zoom is neurite_amd.layers.Resize
        assert ne.torch.layers.SpatialTransformer is neurite_amd.layers.SpatialTransformer
        assert ne.torch.layers.LocallyConnected3D is neurite_amd.layers.LocallyConnected3D
        assert ne.torch.metrics.Dice is neurite_amd.metrics.Dice and ne.torch.losses.Dice is neurite_amd.losses.Dice
        assert ne.torch.metrics.CategoricalCrossentropy is neurite_amd.metrics.CategoricalCrossentropy
        assert ne.torch.models.unet is neurite_amd.models.unet and ne.torch.models.conv_enc is neurite_amd.models.conv_enc
        # host-side behaviour through the switch: shapes / errors need no device
        import torch
        assert ne.torch.layers.Resize(2, name='up').get_config()['zoom_factor'] == 2
        try:
            ne.torch.utils.interpn(torch.zeros(4, 4, 4, 2), torch.zeros(2, 2, 2, 3))
        except neurite_amd.errors.NeuriteAmdError as e:
            assert 'no CPU fallback' in str(e)
        else:
            raise AssertionError('a CPU tensor must be refused')
        print('SWITCH_OK')
    ''', tmp_path)
    assert p.returncode == 0 and 'SWITCH_OK' in p.stdout, p.stderr[-3000:]


# ---- signatures by AST ------------------------------------------------------------------------------------------------------

SIGNATURES = sigs.SIGNATURES


@pytest.mark.parametrize('ref_file,ref_name,our_file,our_name', SIGNATURES, ids=[s[0].split('/')[-1][:-3] + '.' + s[1] for s in SIGNATURES])
def test_public_signatures_equal_the_reference_by_ast(ref_file, ref_name, our_file, our_name):
    ref = REFERENCE['signatures'][sigs.key(ref_file, ref_name)]
    ours = sigs.signature(os.path.join(ROOT, 'neurite_amd', our_file), our_name)
    # keyword-only arguments whose names start with an underscore are this package's private tuning knobs (_variant, _tune): they
    # cannot collide with a reference call
    ours['kwonly'] = [kv for kv in ours['kwonly'] if not kv[0].startswith('_')]
    assert ours == ref, '%s: reference %s, neurite_amd %s' % (ref_name, ref, ours)
