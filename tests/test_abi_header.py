"""
CPU tests of the binding's one source of signatures (no kernel is launched): neurite_amd/_lib.py reads the argument types of every
entry point from the declarations of include/neurite_amd.h -- `T name[]` is a host array (POINTER(T)), `T *name` device memory or a
handle (c_void_p) -- and refuses a declaration its rules do not cover; _lib.call counts its arguments before it touches a device; the
constants that Python keeps as literals equal the header's enums and #defines, in both directions; the header is C99.
"""

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from neurite_amd import _lib, models, seg

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')


def test_every_declared_symbol_has_a_derived_signature():
    sigs = _lib.signatures()
    declared = _lib.declared_symbols()
    assert len(declared) >= 163 and sorted(sigs) == declared
    assert _lib._SIGNATURES == {name: (res, args) for name, (res, args, _) in sigs.items()}
    assert _lib._SIGNATURES is _lib._SIGNATURES and _lib.signatures() is sigs          # parsed once
    for name, (res, args, names) in sigs.items():
        assert res in (C.c_int, C.c_size_t, C.c_char_p), name
        assert len(args) == len(names) == len(set(names)), name
        assert all(re.fullmatch(r'[A-Za-z_]\w*', n) for n in names), name
    # the launching entry points end in `void *stream`
    assert sigs['nrt_softmax_lastdim_f32'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p],
                                               ['x', 'y', 'n', 'channels', 'stream'])
    assert sigs['nrt_abi_version'] == (C.c_int, [], []) and sigs['nrt_status_string'] == (C.c_char_p, [C.c_int], ['status'])


def test_the_loaded_handle_carries_the_derived_signatures():
    handle = _lib.lib()
    for name, (res, args, _) in _lib.signatures().items():
        fn = getattr(handle, name)
        assert fn.restype is res, name
        assert len(fn.argtypes) == len(args) and all(a is b for a, b in zip(fn.argtypes, args)), name


def test_brackets_are_host_arrays_and_stars_are_device_memory():
    ip, fp, dp, vp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p
    sigs = _lib.parse_declarations('int nrt_a(const int shape[], const int *labels, const float sampling[], const float *x,\n'
                                   '          const double positions[], const double *d, long long counts[], long long *c,\n'
                                   '          int32_t fill, size_t n, double f, void *stream);')
    assert sigs == {'nrt_a': (C.c_int, [ip, vp, fp, vp, dp, vp, C.POINTER(C.c_longlong), vp, C.c_int32, C.c_size_t, C.c_double, vp],
                              ['shape', 'labels', 'sampling', 'x', 'positions', 'd', 'counts', 'c', 'fill', 'n', 'f', 'stream'])}
    assert all(a is b for a, b in zip(sigs['nrt_a'][1][:6], [ip, vp, fp, vp, dp, vp]))
    # the header itself: the `const int *` that are device buffers next to the ones that are host arrays
    real = {name: dict(zip(names, args)) for name, (_, args, names) in _lib.signatures().items()}
    edt = real['nrt_edt_f32']
    assert (edt['ids'], edt['labels'], edt['shape'], edt['sampling']) == (vp, vp, ip, fp)
    assert real['nrt_percentile']['positions'] is dp and real['nrt_percentile']['out_count'] is vp
    assert real['nrt_global_max_bwd_f32']['count'] is vp and real['nrt_synth_axis_gather_f32']['index'] is vp
    assert real['nrt_ccl_select']['shape'] is ip and real['nrt_ccl_select']['table'] is vp
    assert real['nrt_conv3d_f32']['ksize'] is ip and real['nrt_conv3d_f32']['up'] is ip
    # every host array of the header is const: the call reads it, never writes it
    text = re.sub(r'/\*.*?\*/', ' ', open(_lib.HEADER_PATH).read(), flags=re.S)
    arrays = re.findall(r'([^,()]*)\[\s*\]', text)
    assert len(arrays) >= 125 and all(a.strip().startswith('const ') for a in arrays)


def test_comments_between_parameters_do_not_split_them():
    sigs = _lib.parse_declarations('/* a, b */ int nrt_a(const float *w /* Keras [kx,ky,kz,cin,cout] */, const int ksize[],\n'
                                   '   float *packed /* [16 * n], aligned */, void *stream); size_t nrt_b(void);\n'
                                   '#define NRT_X 1\ntypedef enum { NRT_P = 0, NRT_Q = 1 } nrt_e;\nconst char *nrt_c(int s);')
    assert {n: len(a) for n, (_, a, _) in sigs.items()} == {'nrt_a': 4, 'nrt_b': 0, 'nrt_c': 1}
    assert sigs['nrt_b'][0] is C.c_size_t and sigs['nrt_c'][0] is C.c_char_p
    real = _lib.signatures()
    assert real['nrt_conv3d_pack_weights_f32'][2] == ['weights', 'ksize', 'cin', 'cout', 'packed', 'stream']
    assert len(real['nrt_conv3d_pool_f32'][1]) == 11 and len(real['nrt_conv3d_up2_f32'][1]) == 12
    assert len(real['nrt_conv3d_up2_head_f32'][1]) == 15


@pytest.mark.parametrize('text, named', [
    ('int nrt_a(unsigned n, void *stream);', 'unsigned n'),                     # an unknown scalar type
    ('int nrt_a(long n, void *stream);', 'long n'),
    ('int nrt_a(const int n, void *stream);', 'const int n'),
    ('int nrt_a(unsigned shape[], void *stream);', 'unsigned shape'),
    ('int nrt_a(int, void *stream);', 'int'),                                   # an unnamed parameter
    ('int nrt_a(const float *, void *stream);', 'const float *'),
    ('int nrt_a(long long, void *stream);', 'long long'),
    ('int nrt_a(float **rows, void *stream);', 'float * * rows'),               # a pointer to pointers
    ('int nrt_a(const int *shape[], void *stream);', 'const int * shape'),
    ('int nrt_a(const int shape[3], void *stream);', 'const int shape'),
    ('int nrt_a(const *x, void *stream);', 'const * x'),
    ('int nrt_a(int n, void *stream)\nint nrt_b(int n);', 'nrt_a'),             # declarations it cannot split
    ('int nrt_a(int (*fn)(int), void *stream);', 'nrt_a'),
    ('int nrt_a(int n, void *stream', 'nrt_a'),
    ('int nrt_a();', 'nrt_a'),
    ('float nrt_a(int n);', 'float nrt_a'),                                     # a return type outside int / size_t / const char *
    ('void *nrt_a(int n);', 'void * nrt_a'),
    ('int nrt_a(int n);\nint nrt_a(int n);', 'nrt_a'),                          # declared twice
    ('struct nrt_s { int a; };', 'struct nrt_s'),
])
def test_the_parser_refuses_what_its_rules_do_not_cover(text, named):
    with pytest.raises(_lib.NeuriteAmdError) as err:
        _lib.parse_declarations(text)
    assert named in str(err.value)


def test_call_counts_its_arguments_before_any_device_is_touched(monkeypatch):
    def touched(*a, **k):
        raise AssertionError('reached the device')
    monkeypatch.setattr(_lib, 'stream_ptr', touched)
    monkeypatch.setattr(_lib, 'lib', touched)
    monkeypatch.setattr(_lib.torch.cuda, 'device', touched)
    p = C.c_void_p(16)
    for args in ((p, p, 10, 4, 0), (p, p, 10), (), (p, p, 10, 4, None, None)):
        with pytest.raises(TypeError) as err:
            _lib.call(None, 'nrt_softmax_lastdim_f32', *args)
        assert 'nrt_softmax_lastdim_f32(x, y, n, channels, stream)' in str(err.value) and 'got %d' % len(args) in str(err.value)
    with pytest.raises(AssertionError, match='reached the device'):                        # the right number goes on
        _lib.call(None, 'nrt_softmax_lastdim_f32', p, p, 10, 4)


def _header_constants():
    """name -> value of every enumerator and every NRT_* #define of the header, and enum name -> its enumerators"""
    text = re.sub(r'/\*.*?\*/', ' ', open(_lib.HEADER_PATH).read(), flags=re.S)
    values, enums = {}, {}
    for body, enum in re.findall(r'typedef\s+enum\s*\{([^{}]*)\}\s*(\w+)\s*;', text):
        for item in body.split(','):
            m = re.fullmatch(r'\s*(NRT_\w+)\s*=\s*(-?\w+)\s*', item)
            assert m, 'enumerator without an explicit value in %s: %r' % (enum, item)
            values[m.group(1)] = int(m.group(2), 0)
            enums.setdefault(enum, []).append(m.group(1))
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(NRT_\w+)[ \t]+(\S+)[ \t]*$', text, flags=re.M):
        assert name not in values, name
        values[name] = int(value, 0)
    return values, enums


def _python_constants():
    """the same names as Python spells them: header name -> value"""
    consts = {}
    for attr, value in vars(_lib).items():
        if re.fullmatch(r'(NRT_OK|NRT_ERR_\w+)', attr):
            consts[attr] = value
        elif re.fullmatch(r'(LOC|INTERP|DT|SEG_WANT|EDT|CCL|PCT)_[A-Z0-9_]+', attr):
            consts['NRT_' + attr] = value
    for attr, value in vars(seg).items():
        if re.fullmatch(r'QUILT_[A-Z]+', attr):
            consts['NRT_' + attr] = value
    for key, value in models._ACTS.items():
        if key is not None:                                         # None and 'linear' are both NRT_ACT_NONE
            consts['NRT_ACT_' + ('NONE' if key == 'linear' else key.upper())] = value
    consts['NRT_ACT_MUL_B'] = models._ACT_MUL_B
    return consts


def test_python_constants_equal_the_header():
    header, enums = _header_constants()
    python = _python_constants()
    assert len(header) >= 45                                        # 5 status, 3 + 2 + 5 + 11 + 2 enumerators, 17 #defines
    assert {k: python.get(k) for k in header} == header             # every value of the header is there, and equal
    assert set(python) == set(header)                               # and Python names nothing the header does not have
    assert models._ACTS[None] == header['NRT_ACT_NONE'] == 0
    assert sorted(set(models._ACTS.values())) == sorted(header[n] for n in enums['nrt_activation'])
    assert models._ACT_LAST_FUSED == header['NRT_ACT_RELU']
    assert models._ACT_MUL_B > max(models._ACTS.values()) and models._ACT_MUL_B & max(models._ACTS.values()) == 0
    # the families the issue names are all there
    for family in ('NRT_ERR_', 'NRT_LOC_', 'NRT_INTERP_', 'NRT_DT_', 'NRT_SEG_WANT_', 'NRT_EDT_', 'NRT_CCL_', 'NRT_PCT_', 'NRT_ACT_'):
        assert sum(k.startswith(family) for k in header) >= 2, family
    assert header['NRT_OK'] == _lib.NRT_OK == 0


@pytest.mark.skipif(shutil.which('gcc') is None, reason='no gcc')
def test_the_header_is_c99():
    done = subprocess.run(['gcc', '-std=c99', '-Wall', '-fsyntax-only', '-Iinclude', 'examples/c_abi_example.c'], cwd=ROOT,
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
