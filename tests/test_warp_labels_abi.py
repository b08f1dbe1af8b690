"""
CPU tests of ne.fused.warp_labels / fuse_labels, ne.utils.resize_labels and the two label layers (no kernel is launched): the three entry
points of csrc/warp_argmax.hip are declared, typed and exported and refuse bad arguments and over-limit sizes before any launch; the
Python wrappers validate their arguments on the host and refuse CPU tensors.
"""

import pytest
import torch

ENTRY_POINTS = ['nrt_warp_labels_argmax_i32', 'nrt_affine_warp_labels_argmax_i32', 'nrt_fuse_labels_i32']
D = 16                                             # a non-NULL "pointer"; nothing is launched on an argument error
ABSOLUTE, SHIFT, LINSPACE = 0, 1, 2


def _L():
    from neurite_amd import _lib
    return _lib


def _warp(moving=D, loc=D, ids=D, prob=None, vol=(5, 6, 7), out=(4, 5, 6), L=5, batch=2, loc_bs=360, mode=SHIFT, has_fill=0, fill=0,
          vol_null=False, out_null=False):
    lib = _L()
    return lib.lib().nrt_warp_labels_argmax_i32(moving, loc, ids, prob, None if vol_null else lib.ints(vol), None if out_null else lib.ints(out),
                                                L, batch, loc_bs, mode, has_fill, fill, None)


def _affine(moving=D, matrix=D, ids=D, prob=None, vol=(5, 6, 7), out=(4, 5, 6), L=5, batch=2, mb=2, center=1, has_fill=0, fill=0,
            vol_null=False, out_null=False):
    lib = _L()
    return lib.lib().nrt_affine_warp_labels_argmax_i32(moving, matrix, ids, prob, None if vol_null else lib.ints(vol),
                                                       None if out_null else lib.ints(out), L, batch, mb, center, has_fill, fill, None)


def _fuse(atlases=D, loc=D, weights=None, ids=D, votes=None, vol=(5, 6, 7), out=(4, 5, 6), L=5, n=3, loc_as=360, has_fill=0, fill=0,
          vol_null=False, out_null=False):
    lib = _L()
    return lib.lib().nrt_fuse_labels_i32(atlases, loc, weights, ids, votes, None if vol_null else lib.ints(vol),
                                         None if out_null else lib.ints(out), L, n, loc_as, has_fill, fill, None)


def test_entry_points_declared_typed_exported():
    L = _L()
    lib = L.lib()
    declared = L.declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in L._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name
        assert L.signatures()[name][2][-1] == 'stream'


def test_bad_arguments_are_refused_before_any_launch():
    inv = _L().NRT_ERR_INVALID_ARG
    for kw in ({'moving': None}, {'loc': None}, {'ids': None}, {'vol_null': True}, {'out_null': True}, {'L': -1}, {'L': -(1 << 31)},
               {'batch': 0}, {'batch': -1}, {'vol': (5, 0, 7)}, {'vol': (-5, 6, 7)}, {'out': (4, -5, 6)}, {'out': (4, 0, 6)},
               {'mode': 3}, {'mode': -1}, {'mode': LINSPACE}, {'mode': LINSPACE, 'loc': D, 'loc_bs': 0}, {'loc_bs': -1},
               {'mode': ABSOLUTE, 'loc': None}):
        assert _warp(**kw) == inv, kw
    for kw in ({'moving': None}, {'matrix': None}, {'ids': None}, {'vol_null': True}, {'out_null': True}, {'L': -1}, {'batch': 0},
               {'vol': (5, 6, 0)}, {'out': (0, 5, 6)}, {'mb': 0}, {'mb': 3}, {'mb': -1}, {'batch': 5, 'mb': 2}):
        assert _affine(**kw) == inv, kw
    for kw in ({'atlases': None}, {'loc': None}, {'ids': None}, {'vol_null': True}, {'out_null': True}, {'L': -1}, {'n': 0}, {'n': -2},
               {'vol': (5, 6, 0)}, {'out': (4, 5, -6)}, {'loc_as': -1}):
        assert _fuse(**kw) == inv, kw


def test_limits_are_unsupported():
    unsup = _L().NRT_ERR_UNSUPPORTED
    big = ((1 << 10, 1 << 10, 1 << 11), (1 << 20, 1 << 20, 1 << 20))            # 2^31 voxels and far beyond
    for shape in big:
        for kw in ({'vol': shape}, {'out': shape}):
            assert _warp(**kw) == unsup and _warp(mode=LINSPACE, loc=None, **kw) == unsup, kw
            assert _affine(**kw) == unsup, kw
            assert _fuse(**kw) == unsup, kw
    assert _warp(batch=65536) == unsup and _affine(batch=65536, mb=65536) == unsup and _affine(batch=65536, mb=1) == unsup
    assert _fuse(n=17) == unsup and _fuse(n=65536) == unsup
    # an argument error is reported before a limit
    inv = _L().NRT_ERR_INVALID_ARG
    assert _warp(vol=big[0], L=-1) == inv and _fuse(n=17, loc=None) == inv and _affine(batch=65536, mb=2) == inv


def test_functions_and_layers_are_public():
    import neurite_amd as ne
    for name in ('warp_labels', 'fuse_labels'):
        assert name in ne.fused.__all__ and callable(getattr(ne.fused, name))
    for name in ('resize_labels', 'zoom_labels'):
        assert name in ne.utils.__all__ and callable(getattr(ne.utils, name))
    assert ne.utils.zoom_labels is ne.utils.resize_labels
    for name in ('LabelTransformer', 'LabelResize'):
        assert name in ne.layers.__all__ and issubclass(getattr(ne.layers, name), torch.nn.Module)
    cfg = ne.layers.LabelTransformer(nb_labels=4, indexing='xy', single_transform=True, fill_label=2, shift_center=False).get_config()
    assert (cfg['nb_labels'], cfg['indexing'], cfg['single_transform'], cfg['fill_label'], cfg['shift_center']) == (4, 'xy', True, 2, False)
    cfg = ne.layers.LabelResize(2, nb_labels=7).get_config()
    assert (cfg['zoom_factor'], cfg['nb_labels']) == (2, 7)
    # no new interpolation method on the float layers
    with pytest.raises(AssertionError):
        ne.utils.resize(torch.zeros(4, 4, 4, 1), 2, interp_method='labels')


def test_cpu_tensors_are_refused():
    import neurite_amd as ne
    L = _L()
    ids, t = torch.zeros(2, 5, 6, 7, dtype=torch.int32), torch.zeros(2, 5, 6, 7, 3)
    for fn in (lambda: ne.fused.warp_labels(ids, t),
               lambda: ne.fused.warp_labels(ids.long().unsqueeze(-1), t, nb_labels=4, fill_label=0, return_prob=True),
               lambda: ne.fused.warp_labels(ids, torch.eye(3, 4)[None].repeat(2, 1, 1), shape=(4, 5, 6)),
               lambda: ne.fused.warp_labels(ids[:, 0], t[:, 0, ..., :2]),
               lambda: ne.fused.fuse_labels(ids, t, weights=[1.0, 0.5]),
               lambda: ne.fused.fuse_labels(ids, t[0], nb_labels=4, return_votes=True),
               lambda: ne.utils.resize_labels(ids[0], 2),
               lambda: ne.utils.zoom_labels(ids[0, 0], (2, 0.5), nb_labels=3),
               lambda: ne.layers.LabelTransformer()([ids, t]),
               lambda: ne.layers.LabelResize(2)(ids),
               lambda: ne.layers.LabelResize((2, 1, 0.5), nb_labels=3)(ids.unsqueeze(-1))):
        with pytest.raises(L.NeuriteAmdError, match='no CPU fallback'):
            fn()


def test_host_side_argument_errors():
    import neurite_amd as ne
    t = torch.zeros(2, 5, 6, 7, 3)
    ids = torch.zeros(2, 5, 6, 7, dtype=torch.int32)
    eye = torch.eye(3, 4)[None].repeat(2, 1, 1)
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.bool):
        with pytest.raises(TypeError):
            ne.fused.warp_labels(ids.to(dtype), t)
        with pytest.raises(TypeError):
            ne.fused.fuse_labels(ids.to(dtype), t)
        with pytest.raises(TypeError):
            ne.utils.resize_labels(ids[0].to(dtype), 2)
        with pytest.raises(TypeError):
            ne.layers.LabelTransformer()([ids.to(dtype), t])
        with pytest.raises(TypeError):
            ne.layers.LabelResize(2)(ids.to(dtype))
    for fn in (lambda: ne.fused.warp_labels(ids.numpy(), t), lambda: ne.fused.warp_labels(ids, t.numpy()),
               lambda: ne.fused.warp_labels(ids, t.long()), lambda: ne.fused.fuse_labels(ids, t.int()),
               lambda: ne.utils.resize_labels(ids[0].numpy(), 2)):
        with pytest.raises(TypeError):
            fn()
    for kw in ({'nb_labels': 0}, {'nb_labels': -3}, {'nb_labels': 1 << 31}, {'nb_labels': 2.5}, {'fill_label': 1 << 31},
               {'fill_label': -(1 << 31) - 1}, {'fill_label': 0.5}, {'indexing': 'yx'}, {'shape': (5, 6, 7)}):
        with pytest.raises(ValueError):
            ne.fused.warp_labels(ids, t, **kw)
    for fn in (lambda: ne.fused.warp_labels(ids, t[:1]),                                 # batch mismatch without single_transform
               lambda: ne.fused.warp_labels(ids, t[..., :2]),                            # a 2-component field of rank 5
               lambda: ne.fused.warp_labels(ids[:, 0], t),                               # a 2-D map under a 3-D field
               lambda: ne.fused.warp_labels(ids, torch.zeros(2, 3, 3)),                  # a 2-D affine
               lambda: ne.fused.warp_labels(ids, eye, indexing='xy'),                    # 'xy' is for dense fields only
               lambda: ne.fused.warp_labels(ids, eye, shape=(4, 5)),
               lambda: ne.fused.warp_labels(ids, eye[:1]),
               lambda: ne.fused.warp_labels(ids[:, :0], t),                              # an empty map
               lambda: ne.fused.warp_labels(ids.long() + (1 << 31), t),                  # every value a label: beyond int32
               lambda: ne.fused.warp_labels(ids.long() - (1 << 31) - 1, t),
               lambda: ne.fused.fuse_labels(ids.long() + (1 << 40), t),
               lambda: ne.fused.fuse_labels(ids, t, nb_labels=0),
               lambda: ne.fused.fuse_labels(ids, t, fill_label=1 << 31),
               lambda: ne.fused.fuse_labels(ids, t, weights=[1.0]),
               lambda: ne.fused.fuse_labels(ids, t, weights=[1.0, -0.5]),
               lambda: ne.fused.fuse_labels(ids, t, weights=[1.0, float('nan')]),
               lambda: ne.fused.fuse_labels(ids, t, weights=torch.tensor([1.0, float('inf')])),
               lambda: ne.fused.fuse_labels(ids, torch.zeros(3, 5, 6, 7, 3)),            # three fields for two atlases
               lambda: ne.fused.fuse_labels(ids, torch.zeros(2, 5, 6, 2)),
               lambda: ne.fused.fuse_labels(ids[:, 0], t),
               lambda: ne.utils.resize_labels(ids[0], (2, 2)),
               lambda: ne.utils.resize_labels(ids[0], 2, nb_labels=0)):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: ne.fused.fuse_labels(torch.zeros(17, 2, 2, 2, dtype=torch.int32), torch.zeros(2, 2, 2, 3)),
               lambda: ne.utils.resize_labels(torch.zeros(2, 2, 2, 2, dtype=torch.int32), 2),      # a 4-D map
               lambda: ne.utils.resize_labels(torch.zeros(4, dtype=torch.int32), 2)):
        with pytest.raises(NotImplementedError):
            fn()
    # restricted labels: an int64 id beyond int32 is background, not an error (the CPU tensor is what is refused)
    with pytest.raises(_L().NeuriteAmdError, match='no CPU fallback'):
        ne.fused.warp_labels(ids.long() + (1 << 40), t, nb_labels=4)
    # unit zoom factors return the map as it is, as resize does
    assert ne.utils.resize_labels(ids[0], 1) is not None and torch.equal(ne.utils.resize_labels(ids[0], (1, 1, 1)), ids[0])
