"""
CPU test of the integer core of the label statistics (neurite_amd/csrc/labelstats_core.h: the sort of the label list, the id -> slot
lookup, the voxel -> coordinates split, the per-wave peeling of distinct slots and the butterfly merge of their summaries), the very
functions the kernels of csrc/labelstats.hip call.  tests/label_stats_core_main.cpp, a stand-alone program, is built with the host
compiler and -fsanitize=address,undefined and run as a child process (nothing is loaded into Python, nothing is preloaded).  It runs
the GPU tests' cases serially and must reproduce the counts, coordinate sums, boxes and confusion matrices of
tests/label_stats_restatement.py exactly: label lists of 1, 2, 255 and 256 entries among them, unsorted lists, and ids in no slot.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import label_stats_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'neurite_amd', 'csrc')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('label_stats_core') / 'label_stats_core_main')
    # (the sanitizer runtimes are linked statically: the program then needs nothing from its environment)
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
           '-static-libubsan', '-Wall', '-Werror', '-I', CSRC, os.path.join(HERE, 'label_stats_core_main.cpp'), '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _run(program, cases, tmp_path):
    """cases: (kind, n, listed, slots, a, b or None) -> the program's int64 output"""
    src, dst = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        f.write(np.int32(len(cases)).tobytes())
        for kind, n, listed, slots, a, b in cases:
            f.write(np.asarray([kind, n, int(listed), a.shape[0], a.ndim - 1] + list(a.shape[1:]), dtype=np.int32).tobytes())
            if listed:
                f.write(np.asarray(slots, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
            if kind == 1:
                f.write(np.ascontiguousarray(b, dtype=np.int32).tobytes())
    res = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, 'exit %d\n%s' % (res.returncode, res.stderr[-4000:])
    assert res.stderr == '', res.stderr[-4000:]
    return np.fromfile(dst, dtype=np.int64)


COUNTS = (1, 2, 3, 33, 255, 256)


def _stat_cases():
    out = []
    for shape in R.SHAPES[:4]:
        for n in COUNTS:
            for listed in (False, True):
                for kind in ('blobs', 'outside') + (('iid', 'constant', 'absent') if shape == R.SHAPES[0] else ()):
                    out.append((kind, shape, n, listed))
    out.append(('blobs', R.SHAPES[4], 33, True))
    out.append(('outside', R.SHAPES[4], 256, True))
    return out


def test_statistics_equal_the_restatement_under_sanitizers(program, tmp_path):
    keys = _stat_cases()
    cases = []
    for kind, shape, n, listed in keys:
        slots, ids, _ = R.case(kind, shape, n, listed)
        cases.append((0, n, listed, slots, ids, None))
    got = _run(program, cases, tmp_path)
    pos = 0
    for kind, shape, n, listed in keys:
        want = R.case(kind, shape, n, listed)[2]
        batch, nd = shape[0], len(shape) - 1
        for name, size, ref in (('count', batch * n, want['count']), ('coord_sums', batch * n * nd, want['coord_sums']),
                                ('bbox', batch * n * 2 * nd, np.stack([want['bbox_min'], want['bbox_max']], 2))):
            assert np.array_equal(got[pos:pos + size], ref.reshape(-1).astype(np.int64)), (name, kind, shape, n, listed)
            pos += size
        assert (want['count'].sum() == np.prod(shape)) == (kind != 'outside' and not (kind == 'absent' and n == 1)), (kind, shape, n)
    assert pos == got.size


def test_confusion_equals_the_restatement_under_sanitizers(program, tmp_path):
    keys = [(shape, n, listed) for shape in (R.SHAPES[0], R.SHAPES[2]) for n in COUNTS for listed in (False, True)]
    cases, wants = [], []
    for shape, n, listed in keys:
        slots, a, _ = R.case('outside', shape, n, listed)
        _, b, _ = R.case('blobs', shape, n, listed)
        cases.append((1, n, listed, slots, a, b))
        wants.append(R.confusion(a, b, slots))
    got = _run(program, cases, tmp_path)
    pos = 0
    for (shape, n, listed), want in zip(keys, wants):
        assert np.array_equal(got[pos:pos + want.size], want.reshape(-1)), (shape, n, listed)
        assert all(int(want[e].sum()) == int(np.prod(shape[1:])) for e in range(shape[0]))
        pos += want.size
    assert pos == got.size
