"""
ctypes binding of libneurite_amd.so (C ABI: include/neurite_amd.h).

PyTorch is only plumbing here: it owns device memory (caching allocator) and streams.  Every
compute call goes through the C ABI with raw device pointers; there is NO CPU or eager-PyTorch
fallback -- if the HIP library is missing or a tensor is not on a ROCm device the call raises.

The argument types of every entry point are read from the header's declarations (parse_declarations):
there is no second list of signatures to keep in step with it.
"""

import ctypes as C
import functools
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NEURITE_AMD_LIB') or os.path.join(_HERE, 'lib', 'libneurite_amd.so')      # NEURITE_AMD_LIB: another build of the same ABI
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'neurite_amd.h')

# the header's enums and flag #defines, literal so that a search finds them; tests/test_abi_header.py pins each to the header's value
NRT_OK = 0
NRT_ERR_INVALID_ARG, NRT_ERR_UNSUPPORTED, NRT_ERR_LAUNCH, NRT_ERR_WORKSPACE = -1, -2, -3, -4
LOC_ABSOLUTE, LOC_SHIFT, LOC_LINSPACE = 0, 1, 2
INTERP_LINEAR, INTERP_NEAREST = 0, 1
DT_F32, DT_BF16, DT_F16, DT_F64, DT_I32, DT_U8 = 0, 1, 2, 3, 4, 5
SEG_WANT_DICE, SEG_WANT_CCE = 1, 2
EDT_SURFACE, EDT_INVERT, EDT_SIGNED, EDT_SQUARED, EDT_ANY_OF = 1, 2, 4, 8, 16
CCL_LARGEST, CCL_MIN_SIZE, CCL_BORDER_FREE, CCL_INVERT = 1, 2, 4, 8
PCT_LINEAR, PCT_LOWER, PCT_HIGHER, PCT_MIDPOINT = 0, 1, 2, 3
PCT_IGNORE_NAN = 1

_lib = None


class NeuriteAmdError(RuntimeError):
    pass


def _header_text():
    with open(HEADER_PATH) as f:
        return f.read()


def declared_symbols():
    """Every function name declared in include/neurite_amd.h."""
    text = re.sub(r'/\*.*?\*/', '', _header_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(nrt_[a-z0-9_]+)\s*\(', text)))


_SCALARS = {'int': C.c_int, 'long long': C.c_longlong, 'float': C.c_float, 'double': C.c_double, 'size_t': C.c_size_t,
            'int32_t': C.c_int32}
_RESTYPES = {'int': C.c_int, 'size_t': C.c_size_t, 'const char *': C.c_char_p}


def parse_declarations(text):
    """name -> (restype, argtypes, parameter names) of every `RET nrt_name(PARAMS);` in the header text `text`.  The header's own
    convention decides the types: a scalar is its ctypes scalar, `T name[]` (a host array) is POINTER(T), `T *name` (device memory
    or a handle) is c_void_p.  Anything else raises: a type guessed wrong here truncates an argument or shifts the ones behind it."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)            # first: some comments sit between parameters and hold commas
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    text = re.sub(r'typedef\s+enum\s*\{[^{}]*\}\s*\w+\s*;', '', text)
    text = re.sub(r'extern\s+"C"\s*\{|\}', '', text)              # what is left of the __cplusplus guards
    sigs = {}
    for decl in text.split(';'):
        decl = ' '.join(decl.replace('*', ' * ').replace('[', ' [').split())
        if not decl:
            continue
        head, _, params = decl[:-1].partition('(')
        ret, _, name = head.strip().rpartition(' ')
        if (decl[-1] != ')' or '(' in params or ')' in params or ret not in _RESTYPES or not re.fullmatch(r'nrt_[a-z0-9_]+', name)
                or name in sigs):
            raise NeuriteAmdError('include/neurite_amd.h: cannot bind the declaration `%s`' % decl)
        argtypes, names = [], []
        for param in [] if params.strip() == 'void' else params.split(','):
            words = param.split()                                  # int n | const float * x | const int shape []
            array = words[-1:] == ['[]']
            star = not array and words[-2:-1] == ['*']
            if array or star:                                      # leaves `[const] T name`; the const of a pointee does not matter here
                del words[-1 if array else -2]
                if words[:1] == ['const']:
                    del words[0]
            ctype, pname = ' '.join(words[:-1]), words[-1] if words else ''
            if not pname.isidentifier() or not (ctype.replace(' ', '').isidentifier() if star else ctype in _SCALARS):
                raise NeuriteAmdError('include/neurite_amd.h: cannot bind the parameter `%s` of `%s`' % (param.strip(), decl))
            argtypes.append(C.c_void_p if star else C.POINTER(_SCALARS[ctype]) if array else _SCALARS[ctype])
            names.append(pname)
        sigs[name] = (_RESTYPES[ret], argtypes, names)
    return sigs


@functools.lru_cache(maxsize=None)
def signatures():
    """name -> (restype, argtypes, parameter names) of every entry point the header declares; parsed once."""
    sigs = parse_declarations(_header_text())
    unbound = set(declared_symbols()) ^ set(sigs)
    if unbound:
        raise NeuriteAmdError('include/neurite_amd.h: named but not bound as a declaration: %s' % ', '.join(sorted(unbound)))
    return sigs


def __getattr__(attr):
    if attr == '_SIGNATURES':                       # name -> (restype, argtypes); made on first use, then a plain module global
        table = globals()[attr] = {name: (res, args) for name, (res, args, _) in signatures().items()}
        return table
    raise AttributeError('module %r has no attribute %r' % (__name__, attr))


def lib():
    """Load the HIP library (once).  Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NeuriteAmdError(
                'libneurite_amd.so not found at %s: build it with `python -m neurite_amd.build` '
                '(hipcc, --offload-arch=gfx950). neurite_amd has no CPU fallback.' % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for name, (res, args, _) in signatures().items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=''):
    if rc != NRT_OK:
        msg = lib().nrt_status_string(rc).decode()
        raise NeuriteAmdError('%s failed: %s (status %d)' % (what or 'neurite_amd call', msg, rc))


def require_device(*tensors):
    """All tensors must live on one ROCm device; returns it."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError('expected a torch.Tensor, got %s' % type(t).__name__)
        if t.device.type != 'cuda':
            raise NeuriteAmdError(
                'neurite_amd runs on MI355X (ROCm) tensors only; got a tensor on %s. '
                'There is deliberately no CPU fallback.' % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise NeuriteAmdError('tensors live on different devices: %s vs %s' % (dev, t.device))
    if dev is not None and dev.index not in _initialised:
        init_device(dev)
    return dev


_initialised = set()


def init_device(dev):
    """nrt_init() on `dev`, once: the library resolves the address of its counter pool now -- outside any stream capture, where nothing
    but launches should happen (include/neurite_amd.h)."""
    with torch.cuda.device(dev):
        check(lib().nrt_init(), 'nrt_init')
    _initialised.add(dev.index)


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(dev, name, *args, what=None):
    """Launch entry point `name` (one that returns an NRT_* status and takes `void *stream` last) on `dev`: under the device guard,
    on torch's current stream of `dev`, and checked.  `what` replaces the name in the error text.  The arguments go through as
    they are; the entry point is looked up on the handle now, so one replaced there is honoured.  Their number is checked here:
    ctypes accepts more arguments than `argtypes` lists, and the stream appended below would then land one slot too late."""
    names = signatures()[name][2]
    if len(args) + 1 != len(names):
        raise TypeError('%s(%s) takes %d arguments before the stream, got %d' % (name, ', '.join(names), len(names) - 1, len(args)))
    with torch.cuda.device(dev):
        rc = getattr(lib(), name)(*args, stream_ptr(dev))
    check(rc, what or name)


def ptr(t):
    # a DeferredWarp (neurite_amd/deferred.py) evaluates itself when its address is asked for
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ints(values):
    return (C.c_int * len(values))(*[int(v) for v in values])


_workspaces = {}


def workspace(device, nbytes):
    """A per-device scratch buffer owned by the torch caching allocator, grown on demand.
    Kernels on one stream are ordered, so one buffer per (device, stream) is enough."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf
