"""
NumPy restatement of the patch grid of neurite_amd.seg (TEST INFRASTRUCTURE, no test of its own name: tests/test_seg_abi.py checks it).

The reference quilts with pystrum's patchlib.quilt (neurite/tf/utils/seg.py:370), which is not part of the reference tree, so these
semantics are restated, not recorded: patch n of a grid sits at unravel_index(n, grid_size) * patch_stride; the quilted volume has
(grid_size - 1) * patch_stride + patch_size voxels per axis; every patch is laid into its own NaN-filled layer of that volume and
`nan_func` (np.nanmean / np.nanmedian) reduces the layers, so an element no patch covers, or that holds only NaN, is NaN.
"""

import warnings

import numpy as np


def grid_of(vol_shape, patch, stride):
    return tuple((v - p) // s + 1 for v, p, s in zip(vol_shape, patch, stride))


def quilt_shape(patch, grid, stride):
    return tuple((g - 1) * s + p for g, s, p in zip(grid, stride, patch))


def _window(n, patch, grid, stride):
    idx = np.unravel_index(n, grid)
    return tuple(slice(int(i) * s, int(i) * s + p) for i, s, p in zip(idx, stride, patch))


def extract(vol, patch, stride, grid=None):
    """vol [*vol_shape, C] -> [prod(grid), *patch, C]"""
    grid = grid_of(vol.shape[:-1], patch, stride) if grid is None else tuple(grid)
    return np.stack([vol[_window(n, patch, grid, stride)] for n in range(int(np.prod(grid)))])


def layers(patches, patch, grid, stride):
    """patches [N, *patch, C] -> the stack [N, *quilt_shape, C] (float32 for float32 / integer patches), NaN outside each patch"""
    patches = np.asarray(patches)
    dtype = np.float64 if patches.dtype == np.float64 else np.float32
    out = np.full((patches.shape[0],) + quilt_shape(patch, grid, stride) + (patches.shape[-1],), np.nan, dtype)
    for n in range(patches.shape[0]):
        out[n][_window(n, patch, grid, stride)] = patches[n]
    return out


def quilt(patches, patch, grid, stride, nan_func=np.nanmean):
    """patches [N, *patch, C] -> [*quilt_shape, C] in the dtype of the stack"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                 # all-NaN slices, means of empty slices
        return nan_func(layers(patches, patch, grid, stride), axis=0)
