"""
CPU test of the word core of the binary morphology (neurite_amd/csrc/morph_core.h: the shift with carry, the tail mask, the border
fill, the step of one word from its neighbour-row triples, the reflection of the structure, and the index fold of the filters' boundary
modes), the very functions the kernels of csrc/morph.hip call.  tests/morph_core_main.cpp, a stand-alone program, is built with the
host compiler and -fsanitize=address,undefined and run as a child process (nothing is loaded into Python, nothing is preloaded).  It
runs the GPU tests' binary cases serially and must reproduce tests/morphology_restatement.py bit for bit: rows of 1, 63, 64, 65, 128,
130 and 1024 voxels among them, where a shift by 64 or a wrong tail mask shows.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import morphology_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'neurite_amd', 'csrc')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('morph_core') / 'morph_core_main')
    # (the sanitizer runtimes are linked statically: the program then needs nothing from its environment)
    version = subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout
    static = ['-static-libsan'] if 'clang' in version else ['-static-libasan', '-static-libubsan']     # (clang's spelling, GCC's)
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static + [
        '-Wall', '-Werror', '-I', CSRC, os.path.join(HERE, 'morph_core_main.cpp'), '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_binary_cases_equal_the_restatement_under_sanitizers(program, tmp_path):
    cases = R.binary_cases()
    src, dst = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        f.write(np.int32(len(cases)).tobytes())
        for (shape, _, structure, iterations, border, op), m, _ in cases:
            nd = len(shape) - 1
            stages = R.STAGES[op]
            head = [R.structure_bits(R.structure_arg(structure, nd), nd), iterations, border, len(stages), stages[0], stages[-1],
                    shape[0], nd] + list(shape[1:])
            f.write(np.asarray(head, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(m, dtype=np.int32).tobytes())
    res = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, 'exit %d\n%s' % (res.returncode, res.stderr[-4000:])
    assert res.stderr == '', res.stderr[-4000:]
    got = np.fromfile(dst, dtype=np.uint8)
    pos = 0
    for key, _, want in cases:
        assert np.array_equal(got[pos:pos + want.size], want.reshape(-1).astype(np.uint8)), key
        pos += want.size
    assert pos == got.size
    assert {1, 63, 64, 65, 128, 130, 1024} <= {key[0][-1] for key, _, _ in cases}
