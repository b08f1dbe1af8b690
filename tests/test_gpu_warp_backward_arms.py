"""
Every dispatch arm of the warp backward (csrc/backward.hip: nrt_interpn_bwd_f32, nrt_interpn_nearest_bwd_f32 -- the gradient of
interpn, SpatialTransformer, Resize, VecInt and compose), each under an id that names the kernel instance the dispatcher takes
(profiles/dispatch_arms/README.md says how a kernel trace of this file and tools/arm_coverage.py confirm that).  The dispatcher
chooses among about forty template instances from the channel count, the rank, the alignment of `vol` and `grad_out`, the location
mode and the grid size; a wrong lane permutation or a wrong second grid-stride pass lives in one instance only.

The C ABI is called directly on guarded buffers (tests/arm_buffers.py): alignment is exact and a write outside grad_vol / grad_loc
is caught; grad_vol is zero-filled by the caller, as utils._launch_interpn_bwd does.

Every comparison is ELEMENT-WISE against the float64 reference of oracle/warp_bwd_oracle.py with the bound derived there,
    |got - ref| <= (T + 16) u A' + (A' - A) + T 2^-126,   u = 2^-24,
and exactly 0 where nothing contributes; each id prints its worst err / bound (profiles/dispatch_arms/warp_bwd_bounds.txt is the
record of one run).  Before a GPU result is looked at, the inputs are checked on the reference alone: with a fill value between
25 % and 75 % of the voxels are masked; a smooth field without fill gives >= 60 % of the grad_loc components and >= 40 % of the
grad_vol rows a non-zero bound; a rough field >= 30 % of the rows (the second-pass volumes are too large for a field of amplitude
1.5 to leave them often: there 5 % masked voxels are asked for).

Base shape: source (9, 8, 7) -- distinct extents, an axis swap shows -- output (7, 6, 7) = 294 voxels, no multiple of 256 / G for
any G; two batch entries with a location tensor each, plus one case with a shared location tensor (loc_batch_stride = 0) and one
with a single entry.  The second-pass cases hold just over the voxel count at which a kernel's grid is capped (8.65 M output
floats at most).

Not covered: the block cap of interpn_bwd_vol_elems (65536 x 4 blocks) needs more than 67 M output elements.
interpn_bwd_generic<3, LINSPACE> is reachable only with NRT_BWD_VOL_SORT_ANY=0 at one channel (grad_loc does not exist in LINSPACE
mode, and every other grad_vol request in 3-D goes to vol_sort_any, vol_elems or the row kernels); it has an id of its own.
"""

import zlib

import numpy as np
import pytest
import torch

import neurite_amd as ne
from arm_buffers import Buf, call
from neurite_amd import _lib
from oracle import warp_bwd_oracle as wbo

pytestmark = pytest.mark.gpu
F = np.float32
MODES = {'ABSOLUTE': wbo.ABSOLUTE, 'SHIFT': wbo.SHIFT, 'LINSPACE': wbo.LINSPACE}
S3, O3 = (9, 8, 7), (7, 6, 7)
FIELDS = (('smooth', False), ('smooth', True), ('rough', False))
REQUESTS = ((True, True), (True, False), (False, True))                # (grad_vol, grad_loc)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs + reference, the launch, the comparison
# ------------------------------------------------------------------------------------------------------------------------------

class Case:
    """B batch entries of one field with their float64 references (computed once, shared by every request and alignment)"""

    def __init__(self, arm, S, O, C, kind, mode, fill, B=2, shared_loc=False, conditions=True):
        rng = np.random.default_rng(zlib.crc32(('%s %s %s %d %s %d %d' % (arm, S, O, C, kind, fill, B)).encode()))
        self.S, self.O, self.C, self.mode, self.fill, self.B, self.kind = tuple(S), tuple(O), C, mode, fill, B, kind
        fields = [wbo.make_field(rng, S, O, C, kind, mode) for _ in range(B)]
        self.vol = np.stack([f[0] for f in fields])
        self.gout = np.stack([f[2] for f in fields])
        self.loc = None if mode == wbo.LINSPACE else np.stack([f[1] for f in fields[:1 if shared_loc else B]])
        self.shared_loc = shared_loc
        self.refs = [wbo.warp_bwd(self.vol[b], wbo.locations(mode, S, O, None if self.loc is None else self.loc[0 if shared_loc else b]),
                                  self.gout[b], fill) for b in range(B)]
        self.bvol = [wbo.bound_vol(r) for r in self.refs]
        self.bloc = [wbo.bound_loc(r) for r in self.refs]
        if conditions and mode != wbo.LINSPACE:
            self.check_inputs(0.25 if conditions is True else conditions)

    def check_inputs(self, least_masked):
        """on the reference alone.  least_masked: 25 % at the base shape; the second-pass volumes are so large that a smooth field
        leaves the volume on a thin shell only, there 5 % masked voxels (tens of thousands) are asked for"""
        masked = float(np.mean([r['oob_share'] for r in self.refs]))
        rows = float(np.mean([(b[..., 0] > 0).mean() for b in self.bvol]))
        comps = float(np.mean([(b > 0).mean() for b in self.bloc]))
        what = '%s fill %d: masked %.2f, rows with a bound %.2f, grad_loc components with a bound %.2f' % (self.kind, self.fill, masked, rows, comps)
        if self.fill:
            assert least_masked <= masked <= 0.75, what
        elif self.kind == 'smooth':
            assert comps >= 0.60 and rows >= 0.40, what
        else:
            assert rows >= 0.30, what


def launch(dev, c, want_vol, want_loc, vol_off=0, gout_off=0, expect=_lib.NRT_OK):
    """nrt_interpn_bwd_f32 on guarded buffers; vol_off / gout_off = 1 start `vol` / `grad_out` one float off a 16-byte boundary.
    Returns (grad_vol [B, *S, C] or None, grad_loc [B, *O, D] or None)."""
    D, nout, rows = len(c.S), int(np.prod(c.O)), int(np.prod(c.S))
    vb, gb = Buf(dev, c.vol.size, vol_off, c.vol), Buf(dev, c.gout.size, gout_off, c.gout)
    lb = None if c.loc is None else Buf(dev, c.loc.size, 0, c.loc)
    gv = gl = None
    if want_vol:
        gv = Buf(dev, c.vol.size, vol_off)
        gv.t.zero_()
    if want_loc:
        gl = Buf(dev, c.B * nout * D)
    args = (vb.p, None if lb is None else lb.p, gb.p, None if gv is None else gv.p, None if gl is None else gl.p, D,
            _lib.ints(c.S), _lib.ints(c.O), c.C, c.B, rows * c.C, 0 if (c.shared_loc or lb is None) else nout * D, c.mode, int(c.fill))
    if expect != _lib.NRT_OK:
        with torch.cuda.device(dev):
            assert _lib.lib().nrt_interpn_bwd_f32(*args, _lib.stream_ptr(dev)) == expect
        return None, None
    call(dev, 'nrt_interpn_bwd_f32', *args)
    return (None if gv is None else gv.get((c.B,) + c.S + (c.C,)), None if gl is None else gl.get((c.B,) + c.O + (D,)))


class Worst:
    """the worst err / bound of an id, printed once per id"""

    def __init__(self, arm):
        self.arm, self.vol, self.loc = arm, 0.0, 0.0

    def compare(self, c, gv, gl, what):
        for b in range(c.B):
            if gv is not None:
                self.vol = max(self.vol, wbo.check(gv[b], c.refs[b]['grad_vol'], c.bvol[b], '%s %s grad_vol b%d' % (self.arm, what, b)))
            if gl is not None:
                self.loc = max(self.loc, wbo.check(gl[b], c.refs[b]['grad_loc'], c.bloc[b], '%s %s grad_loc b%d' % (self.arm, what, b)))

    def report(self):
        print('BOUND %-64s worst err / bound: grad_vol %.3f grad_loc %.3f' % (self.arm, self.vol, self.loc))


def run_family(dev, arm, C, mode, vol_off=0, gout_off=0, fields=FIELDS, requests=REQUESTS, S=S3, O=O3, extras=True, worst=None):
    """the cases of one id: every field x every request, then (extras) a shared location tensor and a single batch entry"""
    w = worst or Worst(arm)
    out = {}
    for kind, fill in fields:
        c = Case(arm, S, O, C, kind, mode, fill)
        for rv, rl in requests:
            gv, gl = launch(dev, c, rv, rl, vol_off, gout_off)
            w.compare(c, gv, gl, '%s fill %d req %d%d' % (kind, fill, rv, rl))
            out[(kind, fill, rv, rl)] = (c, gv, gl)
    if extras:
        rv, rl = requests[0]
        for B, shared in ((2, True), (1, False)):
            c = Case(arm, S, O, C, 'smooth', mode, False, B=B, shared_loc=shared)
            gv, gl = launch(dev, c, rv, rl, vol_off, gout_off)
            w.compare(c, gv, gl, 'B %d shared loc %d' % (B, shared))
    if worst is None:
        w.report()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# interpn_bwd_rows<G, MODE>: C = 4 G, aligned, 3-D
# ------------------------------------------------------------------------------------------------------------------------------

GS = (1, 2, 4, 8, 16, 32, 64)


def ids(fmt, *lists):
    """[(id, *values)] over the product of the lists, and the ids alone"""
    import itertools
    cases = [(fmt % v,) + v for v in itertools.product(*lists)]
    return dict(argvalues=cases, ids=[c[0] for c in cases])


@pytest.mark.parametrize('arm,G,mode', **ids('interpn_bwd_rows<%d,%s>', GS, ('ABSOLUTE', 'SHIFT')))
def test_rows(dev, arm, G, mode):
    """ids interpn_bwd_rows<G,MODE>.  O[0] = 7 < 16 keeps G = 8 off the x-march schedule.  The G-dependent code: the __shfl channel
    permutation from the row-load layout (channel 4 lg + e) to the scatter layout (channel G e + lg), the xor-shuffle sum of d loc
    over G lanes (the whole wave at G = 64), the LDS scatter of G = 8."""
    run_family(dev, arm, 4 * G, MODES[mode])


@pytest.mark.parametrize('arm,G', **ids('interpn_bwd_rows<%d,LINSPACE>', GS))
def test_rows_linspace(dev, arm, G):
    """ids interpn_bwd_rows<G,LINSPACE> (Resize): loc = NULL, (9, 8, 7) -> (13, 11, 9), grad_vol only; a grad_loc request is
    refused"""
    w = Worst(arm)
    for fill in (False, True):
        c = Case(arm, S3, (13, 11, 9), 4 * G, 'linspace', wbo.LINSPACE, fill)
        gv, _ = launch(dev, c, True, False)
        w.compare(c, gv, None, 'fill %d' % fill)
    launch(dev, c, True, True, expect=_lib.NRT_ERR_INVALID_ARG)
    launch(dev, c, False, True, expect=_lib.NRT_ERR_INVALID_ARG)
    w.report()


# nout just above 2^21 / G: the 4096-block cap binds, the second voxel of a lane group (u = 1) and the second iteration (it = 1) run
ROWS_SECOND_PASS = ((4, (33, 128, 128)), (8, (15, 136, 136)), (64, (33, 32, 32)))


@pytest.mark.parametrize('G,O', ROWS_SECOND_PASS, ids=['interpn_bwd_rows<%d,SHIFT>-second-pass' % g for g, _ in ROWS_SECOND_PASS])
def test_rows_second_pass(dev, G, O):
    """O[0] = 15 < 16 at G = 8: the row kernel with its LDS scatter, not the x-march kernels.  Source extents half the output's."""
    assert int(np.prod(O)) > 2 ** 21 // G and int(np.prod(O)) > 4096 * 256 // G
    arm = 'interpn_bwd_rows<%d,SHIFT>-second-pass' % G
    S = tuple((o + 1) // 2 for o in O)
    w = Worst(arm)
    for fill in (False, True):
        c = Case(arm, S, O, 4 * G, 'smooth', wbo.SHIFT, fill, B=1, conditions=0.05)
        gv, gl = launch(dev, c, True, True)
        w.compare(c, gv, gl, 'fill %d' % fill)
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------
# interpn_bwd_generic<3> + interpn_bwd_vol_elems<3>
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('arm,mode,C', **ids('interpn_bwd_generic<3,%s>-quads+interpn_bwd_vol_elems<3> C=%d', ('ABSOLUTE', 'SHIFT'), (12, 20, 36)))
def test_generic3_quads(dev, arm, mode, C):
    """multiples of four that are no power of two, aligned: the float4 arm of interpn_bwd_generic<3> (d loc) and
    interpn_bwd_vol_elems<3> (d vol)"""
    run_family(dev, arm, C, MODES[mode])


SCALAR_ARMS = (('C=16 vol+4B', 16, 1, 0), ('C=32 vol+4B', 32, 1, 0), ('C=64 vol+4B', 64, 1, 0), ('C=16 grad_out+4B', 16, 0, 1),
               ('C=12 vol+4B', 12, 1, 0), ('C=9', 9, 0, 0), ('C=10', 10, 0, 0))


@pytest.mark.parametrize('name,C,vol_off,gout_off', SCALAR_ARMS, ids=['interpn_bwd_generic<3>-scalar+interpn_bwd_vol_elems<3> ' + a[0] for a in SCALAR_ARMS])
def test_generic3_scalar(dev, name, C, vol_off, gout_off):
    """the alignment fallbacks of the row kernels and of the float4 arm (`vol` or `grad_out` 4 bytes off a 16-byte boundary), and
    channel counts that are no multiple of four: the scalar arm of interpn_bwd_generic<3> and interpn_bwd_vol_elems<3>"""
    arm = 'interpn_bwd_generic<3>-scalar+interpn_bwd_vol_elems<3> ' + name
    w = Worst(arm)
    for mode in ('ABSOLUTE', 'SHIFT'):
        run_family(dev, arm + ' ' + mode, C, MODES[mode], vol_off, gout_off, requests=((True, True), (False, True)), worst=w)
    w.report()


SORT_ANY_ARMS = (('C=6', 6, 0), ('C=7', 7, 0), ('C=4 vol+4B', 4, 1), ('C=8 vol+4B', 8, 1))


@pytest.mark.parametrize('name,C,vol_off', SORT_ANY_ARMS, ids=['interpn_bwd_vol_sort_any+interpn_bwd_generic<3> ' + a[0] for a in SORT_ANY_ARMS])
def test_vol_sort_any(dev, name, C, vol_off):
    """the counting-sort merge up to its limit BG_CMAX = 8 (an ALIGNED 4- or 8-channel volume takes interpn_bwd_rows<1|2>; one that
    is 4 bytes off comes here) with d loc by interpn_bwd_generic<3>; at C = 4 and 8 the aligned arm's result agrees within the sum
    of both bounds"""
    arm = 'interpn_bwd_vol_sort_any+interpn_bwd_generic<3> ' + name
    w = Worst(arm)
    for mode in ('ABSOLUTE', 'SHIFT'):
        got = run_family(dev, arm + ' ' + mode, C, MODES[mode], vol_off, requests=((True, True), (True, False)), worst=w)
        if vol_off:
            for (kind, fill, rv, rl), (c, gv, gl) in got.items():
                av, al = launch(dev, c, rv, rl)
                w.compare(c, av, al, 'aligned %s fill %d' % (kind, fill))
                for b in range(c.B):
                    assert (np.abs(av[b].astype(np.float64) - gv[b]) <= 2 * c.bvol[b]).all()
                    assert al is None or (np.abs(al[b].astype(np.float64) - gl[b]) <= 2 * c.bloc[b]).all()
    for fill in (False, True):                          # Resize of a few-channel volume: interpn_bwd_vol_sort_any<LINSPACE>
        c = Case(arm, S3, (13, 11, 9), C, 'linspace', wbo.LINSPACE, fill)
        gv, _ = launch(dev, c, True, False, vol_off)
        w.compare(c, gv, None, 'LINSPACE fill %d' % fill)
    w.report()


def test_generic3_second_pass(dev):
    """id interpn_bwd_generic<3,SHIFT>-second-pass: C = 1, (33, 180, 180) = 1 069 200 voxels > 4096 x 256, so the grid-stride loop
    of interpn_bwd_generic runs twice in the first blocks; d vol comes from interpn_bwd_vol_sort_any (9315 tiles > 2048 blocks)"""
    O = (33, 180, 180)
    assert int(np.prod(O)) > 4096 * 256
    arm = 'interpn_bwd_generic<3,SHIFT>-second-pass'
    w = Worst(arm)
    for fill in (False, True):
        c = Case(arm, (17, 90, 90), O, 1, 'smooth', wbo.SHIFT, fill, B=1, conditions=0.05)
        gv, gl = launch(dev, c, True, True)
        w.compare(c, gv, gl, 'fill %d' % fill)
    w.report()


def test_vol_sort_any_second_pass(dev):
    """id interpn_bwd_vol_sort_any<SHIFT>-second-pass: C = 3, (33, 64, 128) = 9 x 16 x 16 = 2304 tiles of 4 x 4 x 8 > 2048 blocks"""
    O = (33, 64, 128)
    assert ((O[0] + 3) // 4) * ((O[1] + 3) // 4) * ((O[2] + 7) // 8) > 2048
    arm = 'interpn_bwd_vol_sort_any<SHIFT>-second-pass'
    w = Worst(arm)
    for kind, fill in FIELDS:
        c = Case(arm, (17, 32, 64), O, 3, kind, wbo.SHIFT, fill, B=1, conditions=0.05)
        gv, _ = launch(dev, c, True, False)
        w.compare(c, gv, None, '%s fill %d' % (kind, fill))
    w.report()


def test_generic3_linspace(dev, monkeypatch):
    """id interpn_bwd_generic<3,LINSPACE>: one channel with the counting-sort merge switched off (the only way to this instance);
    the same switch sends 3 and 8 unaligned channels to interpn_bwd_vol_elems<3,LINSPACE>"""
    monkeypatch.setenv('NRT_BWD_VOL_SORT_ANY', '0')
    arm = 'interpn_bwd_generic<3,LINSPACE>'
    w = Worst(arm)
    for C, off in ((1, 0), (3, 0), (8, 1)):
        c = Case(arm, S3, (13, 11, 9), C, 'linspace', wbo.LINSPACE, False)
        gv, _ = launch(dev, c, True, False, off)
        w.compare(c, gv, None, 'C %d' % C)
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------
# 1-D and 2-D: interpn_bwd_generic<1|2> + interpn_bwd_vol_elems<1|2>
# ------------------------------------------------------------------------------------------------------------------------------

LOW = {1: ((13,), (29,)), 2: ((11, 9), (17, 13))}


@pytest.mark.parametrize('arm,D,mode', **ids('interpn_bwd_generic<%d,%s>+interpn_bwd_vol_elems', (1, 2), ('ABSOLUTE', 'SHIFT', 'LINSPACE')))
def test_lower_ranks(dev, arm, D, mode):
    """ids interpn_bwd_generic<D,MODE>+interpn_bwd_vol_elems (the same D and MODE).  C = 3 and 4: d vol by vol_elems, d loc by generic; C = 1:
    both by generic (the only way to generic<D,LINSPACE>, which has no d loc)"""
    S, O = LOW[D]
    w = Worst(arm)
    for C in (1, 3, 4):
        if mode == 'LINSPACE':
            for fill in (False, True):
                c = Case(arm, S, O, C, 'linspace', wbo.LINSPACE, fill)
                gv, _ = launch(dev, c, True, False)
                w.compare(c, gv, None, 'C %d fill %d' % (C, fill))
            launch(dev, c, True, True, expect=_lib.NRT_ERR_INVALID_ARG)
        else:
            for kind, fill in FIELDS:
                c = Case(arm, S, O, C, kind, MODES[mode], fill, conditions=False)
                for rv, rl in REQUESTS:
                    gv, gl = launch(dev, c, rv, rl)
                    w.compare(c, gv, gl, 'C %d %s fill %d req %d%d' % (C, kind, fill, rv, rl))
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------
# interpn_nearest_bwd<D, MODE>
# ------------------------------------------------------------------------------------------------------------------------------

def launch_nearest(dev, S, O, C, B, mode, fill, loc, gout):
    D, nout, rows = len(S), int(np.prod(O)), int(np.prod(S))
    gb, lb, gv = Buf(dev, gout.size, 0, gout), None if loc is None else Buf(dev, loc.size, 0, loc), Buf(dev, B * rows * C)
    gv.t.zero_()
    call(dev, 'nrt_interpn_nearest_bwd_f32', None if lb is None else lb.p, gb.p, gv.p, D, _lib.ints(S), _lib.ints(O), C, B, rows * C,
         0 if lb is None else nout * D, mode, int(fill))
    return gv.get((B,) + tuple(S) + (C,))


def nearest(dev, arm, S, O, C, mode, fill, B, w):
    rng = np.random.default_rng(zlib.crc32(('%s %s %d %d' % (arm, O, C, fill)).encode()))
    fields = [wbo.make_field(rng, S, O, C, 'smooth', mode) for _ in range(B)]
    gout = np.stack([f[2] for f in fields])
    loc = None if mode == wbo.LINSPACE else np.stack([f[1] for f in fields])
    refs = [wbo.nearest_bwd(S, C, wbo.locations(mode, S, O, None if loc is None else loc[b]), gout[b], fill) for b in range(B)]
    assert all((r['T_vol'] > 0).mean() >= 0.3 for r in refs)
    got = launch_nearest(dev, S, O, C, B, mode, fill, loc, gout)
    for b in range(B):
        w.vol = max(w.vol, wbo.check(got[b], refs[b]['grad_vol'], wbo.bound_nearest(refs[b]), '%s C %d fill %d b%d' % (arm, C, fill, b)))


@pytest.mark.parametrize('arm,D,mode', **ids('interpn_nearest_bwd<%d,%s>', (1, 2, 3), ('ABSOLUTE', 'SHIFT', 'LINSPACE')))
def test_nearest(dev, arm, D, mode):
    """ids interpn_nearest_bwd<D,MODE>: grad_vol is the scatter of grad_out into the rounded location's row, a sum of exact float32
    terms: within (T + 1) u A of the float64 scatter"""
    S, O = LOW[D] if D < 3 else (S3, (13, 11, 9))
    w = Worst(arm)
    for C in (1, 3, 8):
        for fill in (False, True):
            nearest(dev, arm, S, O, C, MODES[mode], fill, 2, w)
    w.report()


def test_nearest_second_pass(dev):
    """id interpn_nearest_bwd<3,SHIFT>-second-pass: (33, 128, 128) x 8 channels = 16896 blocks of 256 elements > the 16384-block cap"""
    O, C = (33, 128, 128), 8
    assert int(np.prod(O)) * C > 16384 * 256
    w = Worst('interpn_nearest_bwd<3,SHIFT>-second-pass')
    for fill in (False, True):
        nearest(dev, w.arm, (17, 64, 64), O, C, wbo.SHIFT, fill, 1, w)
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python wrappers reach the same arms with the same numbers
# ------------------------------------------------------------------------------------------------------------------------------

def G_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_()


@pytest.mark.parametrize('C,single', [(16, False), (64, False), (12, True)], ids=['SpatialTransformer C=16', 'SpatialTransformer C=64',
                                                                                   'SpatialTransformer C=12 single_transform'])
def test_spatial_transformer_autograd(dev, C, single):
    """SpatialTransformer's autograd function on interpn_bwd_rows<4|16,SHIFT> and on the float4 arm of interpn_bwd_generic.  With
    single_transform the wrapper sums grad_loc over the batch in float32: B - 1 more roundings of at most sum_b (|ref_b| + bound_b)"""
    arm = 'SpatialTransformer C=%d%s' % (C, ' single_transform' if single else '')
    c = Case(arm, S3, S3, C, 'smooth', wbo.SHIFT, False, B=2, shared_loc=single)
    v, s = G_(c.vol, dev), G_(c.loc, dev)
    out = ne.layers.SpatialTransformer(single_transform=single)([v, s])
    (out * torch.from_numpy(c.gout).to(dev)).sum().backward()
    w = Worst(arm)
    w.compare(c, v.grad.cpu().numpy(), None if single else s.grad.cpu().numpy(), 'autograd')
    if single:
        ref = sum(r['grad_loc'] for r in c.refs)
        each = sum(np.abs(r['grad_loc']) + b for r, b in zip(c.refs, c.bloc))
        bound = sum(c.bloc) + (c.B - 1) * wbo.U * each
        assert tuple(s.grad.shape) == (1,) + S3 + (3,)
        w.loc = wbo.check(s.grad[0].cpu().numpy(), ref, bound, arm + ' grad_shift summed over the batch')
    w.report()


def test_resize_autograd(dev):
    """id Resize(2) C=64: the layer's backward on interpn_bwd_rows<16,LINSPACE>, and on interpn_nearest_bwd<3,LINSPACE>"""
    arm = 'Resize(2) C=64'
    S = (6, 5, 4)
    O = tuple(2 * s for s in S)
    c = Case(arm, S, O, 64, 'linspace', wbo.LINSPACE, False)
    x = G_(c.vol, dev)
    out = ne.layers.Resize(2)(x)
    assert tuple(out.shape) == (2,) + O + (64,)
    (out * torch.from_numpy(c.gout).to(dev)).sum().backward()
    w = Worst(arm)
    w.compare(c, x.grad.cpu().numpy(), None, 'autograd')
    # Resize(nearest): element by element (tests/test_gpu_backward.py::test_nearest_backward checks the sum of this gradient only)
    x = G_(c.vol, dev)
    (ne.layers.Resize(2, interp_method='nearest')(x) * torch.from_numpy(c.gout).to(dev)).sum().backward()
    for b in range(c.B):
        r = wbo.nearest_bwd(S, 64, wbo.locations(wbo.LINSPACE, S, O), c.gout[b])
        wbo.check(x.grad[b].cpu().numpy(), r['grad_vol'], wbo.bound_nearest(r), arm + ' nearest b%d' % b)
    w.report()
