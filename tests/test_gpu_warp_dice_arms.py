"""
Every dispatch arm of the fused warp + soft Dice forward (csrc/fused.hip, csrc/fused_wc.h: warp_dice_tile, warp_dice_tile_pad and the
wave-cache kernel warp_dice_wc, with and without its Dice half), each under an id that names the kernel instance its call takes and the
geometry of the launch.  Both are derived by oracle/warp_dice_oracle.py, a restatement of the host dispatch; every test asserts, with the
compute-unit count of the device it runs on, that the instance in its id is the one `plan` gives for each of its launches and, for
float32, the one nrt_warp_dice_kernel_name returns -- so the benchmark's key and the restatement check each other; a kernel trace of
this file and tools/arm_coverage.py --families warp_dice confirm the names on the device (profiles/dispatch_arms/README.md).  The table
of cases, their inputs and references are in tests/warp_dice_cases.py (which says how each shape follows from its condition);
tests/test_warp_dice_oracle.py checks the table and the premises below without a device.

The C ABI is called directly -- nrt_warp_dice_soft_f32, nrt_warp_dice_soft_bf16, nrt_warp_dice_workspace_bytes,
nrt_warp_dice_kernel_name and, for the twelve DICE = false instances, nrt_interpn_f32_ex variant 10 -- on guarded buffers
(tests/arm_buffers.py): a workspace of exactly the size the library asks for, outputs pre-filled with a byte pattern, guards checked
after every call; a refused call must leave every output byte untouched.

Two runs per id on the same shapes, both against references that do not come from the code under test:

  exact    maps of small integers, locations on a lattice with dyadic weights (one axis of a voxel on a quarter step, the others on
           half steps or integers; LINSPACE: O = 2 S - 1): every sum of absolute terms stays below 2^24 units of 2^-8 (asserted on the
           reference), so `sums` must equal the float64 reference BIT FOR BIT -- also from the STORE = false and wave-cache instances,
           whose only output it is.  With and without a fill value; laplace_smoothing 0 (with a label whose denominator is 0) and 0.5.
           Each map's extrema sit in one voxel and label of the whole launch and are compared as values.
  random   uniform [0, 1) maps rounded to the storage type on smooth, incoherent and lattice fields (LINSPACE: a step that is not
           dyadic): |sums - ref| <= (n + 1) 2^-24 A element-wise, ref the float64 sums of `fixed` and the reference's float32 `warped`
           (derived in the oracle's docstring).  Each id prints its worst err / bound in a BOUND line
           (profiles/dispatch_arms/warp_dice_bounds.txt is the record of one run).

In both, `warped` (where stored) is compared bit for bit with oracle.warp_fwd_oracle's reference and `dice` bit for bit with the float32
op sequence of the second stage on the sums the device returned.
"""

import numpy as np
import pytest
import torch

import warp_dice_cases as cs
from arm_buffers import Bytes, Raw
from neurite_amd import _lib
from oracle import dice_cce_oracle as dco
from oracle import warp_dice_oracle as wdo

pytestmark = pytest.mark.gpu
F = np.float32
OK = _lib.NRT_OK


def norm(name):
    """the profiler's spelling without blanks (tools/arm_coverage.norm)"""
    return name.replace(' ', '')


def status(dev, name, *args):
    with torch.cuda.device(dev):
        return getattr(_lib.lib(), name)(*args, _lib.stream_ptr(dev))


def num_cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def guards_ok(ws):
    g = ws.GUARD
    return bool((ws.whole[:g] == ws.MARK).all().item() and (ws.whole[g + ws.n:] == ws.MARK).all().item())


class Ws(Bytes):
    """a workspace pre-filled with 0x4b bytes: a partial row that no block wrote reads as 1.3e7 in every sum and extremum (the 0xa5 of the
    other buffers would be -2.9e-16, which no float32 sum shows)"""
    MARK = 0x4B


class Launch:
    """one call on fresh, pre-filled outputs; the results are read later (`results`), so that launches can be queued back to back"""

    def __init__(self, dev, c, inp, fill, fv, eps, ws=None):
        self.c, self.dev = c, dev
        B, L, n = c.B, c.L, c.nout
        lib = _lib.lib()
        self.nws = lib.nrt_warp_dice_workspace_bytes(_lib.ints(c.O), L, B, c.tune) if c.entry == 'dice' else 0
        self.ws = ws or Ws(dev, max(self.nws - c.ws_short, 0))
        mov, fix = cs.storage(inp.mov, c.dtype), cs.storage(inp.fix, c.dtype)
        self.mov = Raw(dev, mov.nbytes, c.mov_off, mov)
        self.fix = Raw(dev, fix.nbytes, c.fix_off, fix)
        self.loc = Raw(dev, inp.loc.nbytes, 0, inp.loc) if inp.loc is not None else None
        self.warped = Raw(dev, B * n * L * 4, c.warped_off) if c.store else None
        self.sums, self.dice = Raw(dev, B * 3 * L * 4), Raw(dev, B * L * 4)
        self.mm = Raw(dev, 16) if c.minmax else None

        def p(buf, name):
            return None if buf is None or name in c.null else buf.p
        loc_bs = 0 if c.shared_loc else n * 3
        S, O = _lib.ints(c.S), _lib.ints(c.O)
        if c.entry == 'interpn':
            self.rc = status(dev, 'nrt_interpn_f32_ex', p(self.mov, 'moving'), p(self.loc, 'loc'), p(self.warped, 'warped'), 3, S, O, L, B,
                             c.rows * L, loc_bs, c.mode, 0, int(fill), fv, 10, c.tune)
        elif c.dtype == 'f32':
            self.rc = status(dev, 'nrt_warp_dice_soft_f32', p(self.mov, 'moving'), p(self.loc, 'loc'), p(self.fix, 'fixed'), p(self.warped, 'warped'),
                             S, O, L, B, loc_bs, c.mode, int(fill), fv, eps, p(self.sums, 'sums'), p(self.dice, 'dice'), p(self.mm, 'minmax'),
                             c.tune, self.ws.p, self.nws - c.ws_short)
        else:
            assert not c.store
            self.rc = status(dev, 'nrt_warp_dice_soft_bf16', p(self.mov, 'moving'), p(self.loc, 'loc'), p(self.fix, 'fixed'), S, O, L, B, loc_bs,
                             c.mode, int(fill), fv, eps, p(self.sums, 'sums'), p(self.dice, 'dice'), p(self.mm, 'minmax'), c.tune, self.ws.p,
                             self.nws - c.ws_short)

    def untouched(self):
        outs = [self.sums, self.dice] + [b for b in (self.mm, self.warped) if b is not None]
        return all(b.untouched() for b in outs) and bool((self.ws.whole == self.ws.MARK).all().item())

    def results(self):
        """(sums [B, 3, L], dice [B, L], minmax [4] or None, warped [B, *O, L] or None), the guards of every buffer checked"""
        c = self.c
        assert guards_ok(self.ws), 'a write outside the workspace'
        warped = self.warped.get(F, (c.B,) + tuple(c.O) + (c.L,)) if self.warped else None
        if c.entry == 'interpn':
            return None, None, None, warped
        return self.sums.get(F, (c.B, 3, c.L)), self.dice.get(F, (c.B, c.L)), self.mm.get(F) if self.mm else None, warped


def check_run(c, kind, eps, inp, res, what):
    """the checks of the module docstring on one launch's results; the worst err / bound of a random run"""
    sums, dice, mm, warped = res
    if warped is not None:
        same = warped.view(np.uint32) == inp.warped.view(np.uint32)
        assert same.all(), '%s: %d of %d warped values differ, first at %s' % (what, (~same).sum(), same.size, np.argwhere(~same)[0].tolist())
    if c.entry == 'interpn':
        return 0.0
    r = inp.ref
    worst = 0.0
    if kind == 'exact':
        wdo.assert_exact(r)
        dco.check_exact(sums, r['sums'], what + ' sums')
    else:
        worst = dco.check_bounded(sums, r['sums'], (r['n'] + r['k']) * wdo.U * r['A'], what + ' sums')
    dco.check_exact(dice, dco.dice_f32(sums, eps), what + ' dice, laplace_smoothing %g' % eps)
    if kind == 'exact' and eps == 0 and inp.zero_label is not None:
        assert (dice[:, inp.zero_label] == 0).all() and (sums[:, :, inp.zero_label] == 0).all()
    if mm is not None:
        assert mm.tolist() == r['minmax'].astype(F).tolist(), (what, mm, r['minmax'])
    return worst


def agree(dev, rc, cid, fill):
    """the id, the restatement with the device's compute units, and the library's own name and workspace size agree"""
    p = wdo.plan(rc, num_cus(dev))
    assert p.get('instance') == cs.inst_of(cid), (cid, p)
    if rc.entry == 'dice':
        lib = _lib.lib()
        assert lib.nrt_warp_dice_workspace_bytes(_lib.ints(rc.O), rc.L, rc.B, rc.tune) == p['ws'], cid
        if rc.dtype == 'f32':
            with torch.cuda.device(dev):
                name = lib.nrt_warp_dice_kernel_name(_lib.ints(rc.O), _lib.ints(rc.S), rc.L, rc.B, rc.mode, int(fill), int(rc.store), int(rc.minmax), rc.tune)
            assert norm(name.decode()) == p['instance'], (cid, name)
    return p


@pytest.mark.parametrize('c', cs.CASES, ids=cs.IDS)
def test_arm(dev, c):
    worst = None
    for kind, fill, eps in cs.runs(c):
        rc = cs.run_call(c.call, kind)
        agree(dev, rc, c.id, fill)
        inp = cs.inputs(c.call, kind, fill)
        run = Launch(dev, rc, inp, fill, cs.fill_value(kind), eps)
        what = '%s %s fill %d' % (c.id, kind, fill)
        assert run.rc == OK, '%s: status %d' % (what, run.rc)
        w = check_run(rc, kind, eps, inp, run.results(), what)
        if kind != 'exact' and rc.entry == 'dice':
            worst = max(worst or 0.0, w)
    if worst is not None:
        print('BOUND %-150s worst err / bound: sums %.3g' % (c.id, worst))


def test_back_to_back(dev):
    """ids warp_dice_wc<1,false,true,false,true,true> and <...,false>: five launches on one stream and one workspace -- persistent, one
    block per item, persistent (on a random field), persistent, one block per item -- every output pre-filled, no result read before
    the last launch is queued (each launch uploads its own inputs first, with copies that block the host).  All five come out right only
    if each persistent launch leaves the work counters of its ring slot clean for the next."""
    big = next(c for c in cs.CASES if c.id.startswith('warp_dice_wc<1,false,true,false,true,true>') and ' O7x51x63 ' in c.id)
    small = next(c for c in cs.CASES if c.id.startswith('warp_dice_wc<1,false,true,false,true,false>') and 'default' not in c.id)
    cus = num_cus(dev)
    assert wdo.plan(big.call, cus)['persist'] and not wdo.plan(small.call, cus)['persist']
    order = (big, small, big, big, small)
    nws = max(wdo.plan(c.call, cus)['ws'] for c in order)
    ws = Ws(dev, nws)
    queued = []
    for i, c in enumerate(order):
        kind = 'exact' if i != 2 else c.kinds[1]
        inp = cs.inputs(c.call, kind, False)
        queued.append((c, kind, inp, Launch(dev, c.call, inp, False, cs.fill_value(kind), 0.5, ws=ws)))
    for c, kind, inp, run in queued:
        assert run.rc == OK
        check_run(c.call, kind, 0.5, inp, run.results(), c.id + ' back to back ' + kind)


@pytest.mark.parametrize('c,want', [r[1:] for r in cs.REFUSED], ids=[r[0] for r in cs.REFUSED])
def test_refused_calls(dev, c, want):
    """5, 2 and 260 labels; `moving`, `fixed` or `warped` 4 bytes off 16-byte alignment; `sums`, `dice` or `fixed` NULL; a workspace one byte
    short; an empty output: the status the restatement derives from warp_dice_soft_impl, and not one byte of any output or of the
    workspace written"""
    assert wdo.plan(c, num_cus(dev)).get('status', OK) == want
    rng = np.random.default_rng(5)
    inp = cs.Inputs(rng.random((c.B,) + tuple(c.S) + (c.L,)).astype(F), rng.random((c.B,) + tuple(c.O) + (c.L,)).astype(F),
                    rng.random((c.B,) + tuple(c.O) + (3,)).astype(F), None, None, None, None)
    run = Launch(dev, c, inp, False, 0.0, 0.5)
    assert run.rc == want, (c, run.rc)
    if want == OK:                                   # the control: the same call without a fault is accepted and writes its outputs
        assert not run.sums.untouched() and not run.dice.untouched()
    else:
        assert run.untouched(), 'a refused call wrote an output'
