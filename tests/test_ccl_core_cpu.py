"""
CPU test of the union-find core of the connected-component kernels (neurite_amd/csrc/ccl_core.h: run heads, the enumeration of the
unions a voxel has to make, find, union, the representative test), the very functions the kernels of csrc/ccl.hip call.
tests/ccl_core_main.cpp, a stand-alone program, is built with the host compiler and -fsanitize=address,undefined and run as a child
process (nothing is loaded into Python, nothing is preloaded).  It applies the functions serially: the forest starts from the run
heads, the unions of ccl_for_each_union (those that the runs imply are left out, as in the kernels) are applied in raster order and in
two shuffled orders, one of them with the arguments of every union swapped, at the kernels' chunk of 1024 voxels and at a chunk of 7
that cuts runs everywhere.  The component maps it writes, for the shapes and patterns of the GPU tests, must equal the flood fill of
tests/ccl_restatement.py.  An out-of-bounds neighbour or a loop that does not end is found here, not on the GPU.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import ccl_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'neurite_amd', 'csrc')


def _cases():
    """(keys int32 [*S] with 0 = background, connectivity, chunk: where the runs are cut)"""
    out = []
    for shape in R.SHAPES + R.CHUNK_SHAPES[:4]:
        nd = len(shape)
        maps = [R.pattern(name, shape, seed=3).astype(np.int32) for name in ('empty', 'full', 'corners', 'checker', 'comb',
                                                                            'random0.3', 'random0.5', 'random0.7')]
        maps.append(R.two_combs(shape))
        maps.append(R.random_ids(shape, 4, seed=5))
        for keys in maps:
            for connectivity in range(1, nd + 1):
                for chunk in ((1024, 7) if keys.size <= 2100 else (1024,)):
                    out.append((keys, connectivity, chunk))
    return out


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('ccl_core') / 'ccl_core_main')
    # (the sanitizer runtimes are linked statically: the program then needs nothing from its environment)
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-Wall', '-Werror', '-I', CSRC, os.path.join(HERE, 'ccl_core_main.cpp'), '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_core_functions_equal_the_flood_fill_under_sanitizers(program, tmp_path):
    cases = _cases()
    src, dst = str(tmp_path / 'cases.bin'), str(tmp_path / 'maps.bin')
    with open(src, 'wb') as f:
        f.write(np.int32(len(cases)).tobytes())
        for keys, connectivity, chunk in cases:
            n = (1,) * (3 - keys.ndim) + keys.shape
            f.write(np.asarray(n + (connectivity, chunk), dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(keys, dtype=np.int32).tobytes())
    res = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, 'exit %d\n%s' % (res.returncode, res.stderr[-4000:])
    assert res.stderr == '', res.stderr[-4000:]
    got = np.fromfile(dst, dtype=np.int32)
    assert got.size == 3 * sum(keys.size for keys, _, _ in cases)
    pos = 0
    for keys, connectivity, chunk in cases:
        want, _ = R.label(keys, connectivity, labels=[int(v) for v in np.unique(keys) if v != 0] or [1])
        for order in range(3):
            comp = got[pos:pos + keys.size].reshape(keys.shape)
            pos += keys.size
            assert np.array_equal(comp, want), (keys.shape, connectivity, chunk, order)
