"""
CPU test of the core of the percentile kernels (neurite_amd/csrc/select_core.h: the monotone key of a float and its inverse, the
digits of the three passes, the walk from a rank to a bin), the very functions the kernels of csrc/select.hip call.
tests/select_core_main.cpp, a stand-alone program, is built with the host compiler and -fsanitize=address,undefined and run as a child
process (nothing is loaded into Python, nothing is preloaded).  It runs the three-pass select serially on the cases of the GPU tests
(two passes on values that bfloat16 holds) and must return the bit patterns of np.sort(x)[k] for the ranks 0, n - 1 and the floor and
ceiling ranks of the tests' percentiles; and it writes the key of sampled bit patterns (both zeros, denormals, +-inf, NaNs of both
signs among them), which must be monotone in the float order and turn back into the float.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import percentile_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'neurite_amd', 'csrc')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('select_core') / 'select_core_main')
    # (the sanitizer runtimes are linked statically: the program then needs nothing from its environment)
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-Wall', '-Werror', '-I', CSRC, os.path.join(HERE, 'select_core_main.cpp'), '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _run(program, mode, src, dst):
    res = subprocess.run([program, mode, src, dst], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, 'exit %d\n%s' % (res.returncode, res.stderr[-4000:])
    assert res.stderr == '', res.stderr[-4000:]
    return np.fromfile(dst, dtype=np.uint32)


def _cases():
    """(values float32, ranks, passes)"""
    out = []
    for n in R.SIZES + (4551,):
        for name in R.DISTRIBUTIONS + ('nan',):
            v = R.draw(name, n, seed=1)
            ranks = {0, n - 1}
            for q in R.QS:
                lo, hi, _ = R.ranks(n, np.float64(q) / 100.0)
                ranks.update((lo, hi))
            out.append((v, sorted(ranks), 3))
            if name in ('normal', 'ties', 'zeros70', 'nan', 'inf'):
                out.append((R.store(v, 'bfloat16')[1], sorted(ranks), 2))
    return out


def test_three_pass_select_equals_the_sort_under_sanitizers(program, tmp_path):
    cases = _cases()
    src, dst = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        f.write(np.uint32(len(cases)).tobytes())
        for v, ranks, passes in cases:
            f.write(np.asarray([v.size, len(ranks), passes], dtype=np.uint32).tobytes())
            f.write(np.asarray(ranks, dtype=np.uint32).tobytes())
            f.write(np.ascontiguousarray(v, dtype=np.float32).tobytes())
    got = _run(program, 'select', src, dst)
    assert got.size == sum(len(ranks) for _, ranks, _ in cases)
    pos = 0
    for v, ranks, passes in cases:
        want = np.sort(v)[np.asarray(ranks)] + np.float32(0)                                 # (-0.0 + 0.0 = +0.0: one zero)
        have = got[pos:pos + len(ranks)].view(np.float32)
        pos += len(ranks)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(have), nan), (v.size, passes)
        assert np.array_equal(have[~nan].view(np.uint32), want[~nan].view(np.uint32)), (v.size, passes)


def test_key_is_monotone_and_round_trips(program, tmp_path):
    rng = np.random.default_rng(7)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF,
                        0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7F800001, 0xFF800001, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF,
                        0x3F800000, 0xBF800000], dtype=np.uint32)
    bits = np.concatenate([special, rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32),
                           rng.integers(0, 1 << 24, 2000, dtype=np.uint64).astype(np.uint32),                       # denormals, small
                           (0x80000000 + rng.integers(0, 1 << 24, 2000, dtype=np.uint64)).astype(np.uint32)])
    src, dst = str(tmp_path / 'bits.bin'), str(tmp_path / 'keys.bin')
    bits.tofile(src)
    got = _run(program, 'keys', src, dst).reshape(-1, 2)
    assert got.shape[0] == bits.size
    key, back = got[:, 0], got[:, 1]
    val = bits.view(np.float32)
    nan = np.isnan(val)
    assert nan.sum() >= 8 and np.all(key[nan] == 0xFFFFFFFF) and np.all(np.isnan(back[nan].view(np.float32)))
    # the inverse gives the float back, bit for bit but for -0.0, which reads as +0.0
    want = np.where(bits == 0x80000000, np.uint32(0), bits)
    assert np.array_equal(back[~nan], want[~nan])
    # monotone: the order of the keys is the order of the floats, equal keys exactly for equal floats, every NaN above +inf
    order = np.argsort(key[~nan], kind='stable')
    v, k = val[~nan][order].astype(np.float64), key[~nan][order]
    assert np.all(np.diff(v) >= 0)
    assert np.array_equal(np.diff(v) == 0, np.diff(k.astype(np.int64)) == 0)
    assert key[~nan].max() < 0xFFFFFFFF and int(key[bits == 0x7F800000][0]) == 0xFF800000 == int(key[~nan].max())
    assert int(key[bits == 0xFF800000][0]) == int(key[~nan].min())
