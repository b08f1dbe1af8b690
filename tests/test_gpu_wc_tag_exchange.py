"""
The wave-cache gather (csrc/fused_wc.h: wc_item) claims its cache slots with ONE LDS exchange per pass: every lane swaps the id of its
row into tags[slot] and reads the word back.  What the exchange returned says whether the row was there (hit / miss), what the read
returns says whether the row keeps the slot (served / orphan); loader = miss and served.  Which lane of a slot comes first is up to the
hardware, so the number and the order of the fetch-list entries are too -- the results must not be: the cache decides where a row is
read from, never which row.

Before anything is launched a NumPy restatement of the rule, serial over the lanes, ascending and descending, asserts on the chosen
inputs that the fetch list never exceeds its 64 entries and that each of these events occurs in at least one wave and pass:
  (a) a row that was resident before the pass ends the pass as an orphan (a hit that is evicted behind its back);
  (b) two loaders of one row in one pass (r1, r2, r1 in one slot);
  (c) two corners of one voxel name the same row (clipped border);
  (d) more than 16 orphans: the fallback;
  (e) an empty fetch list.

Fused forward (two pass states), per input, whole columns and columns cut in x, fill None and 0.25: warped volume bit-equal to the oracle
and to the register kernel, Dice within 1e-5 relative of the oracle, sums within rtol 2e-5 / atol 1e-4 of the register kernel's (the
figures of test_gpu_dice_cce.py::test_fused_wave_cache_kernel), three calls bit-equal to each other.  Three pass states (stand-alone
warp, variant 10, and both backward forms) at (X, 8, 8), X in {18, 19, 20}, 256 entries cycling through the fields: the warp bit-equal
to the oracle, d loc bit-equal to warp_dice_bwd_xm (NRT_BWD_WC=0).  One captured graph of the fused forward, inputs changed between
replays, bit-equal to eager.
"""

import functools

import numpy as np
import pytest
import torch

import neurite_amd as ne
import test_gpu_wc_fetch_groups as fg
from conftest import bits_equal
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu
F = np.float32
RTOL = 1e-5
NO_WC, WC = fg.NO_WC, fg.WC
TUNES = fg.TUNES                                                # whole columns; columns cut into three x segments
SHAPES = fg.SHAPES                                              # batch 2 (21, 18, 29) -> same; batch 1 (40, 33, 47) -> (37, 30, 41)
FIELDS = ('zero', 'smooth4', 'iid0.7', 'iid3', 'incoherent', 'edge')
EDGE_SHIFT = (-3.0, 2.5, -2.0)                                  # locations leave the volume on three faces
XS = (18, 19, 20)
B3 = 256
G, N = fg.G, fg.N


def field(name, rng, B, S, So):
    if name == 'edge':
        return (fg.field('iid0.7', rng, B, S, So) + np.array(EDGE_SHIFT, F)).astype(F)
    return fg.field(name, rng, B, S, So)


# ----------------------------------------------------------------------------------------------------------------------------------
# the restatement of the exchange rule
# ----------------------------------------------------------------------------------------------------------------------------------

def exchange_events(trf, S, ascending=True):
    """A whole-column march over the SHIFT field trf [B, *So, 3] into a source of shape S with the lanes of every exchange served in
    ascending or descending order.  Returns n per (wave, pass) and the number of wave-passes in which each event (a) - (e) occurs.
    A wave owns a 2 x 4 (y, z) sub-patch; lane = 8 g + p: voxel g (z offsets 0, 2, 3, 1 for g & 3), corner p."""
    B, So = trf.shape[0], trf.shape[1:4]
    g, p = np.arange(64) >> 3, np.arange(64) & 7
    dz = np.array([0, 2, 3, 1])[g & 3]
    ys, zs = np.arange(0, So[1], 2), np.arange(0, So[2], 4)
    b_, y_, z_ = [a.ravel() for a in np.meshgrid(np.arange(B), ys, zs, indexing='ij')]
    W = b_.size
    yc = np.minimum(y_[:, None] + (g >> 2)[None], So[1] - 1)
    zc = np.minimum(z_[:, None] + dz[None], So[2] - 1)
    tags = np.full((W, 128), -1, np.int64)                     # the id of the slot's row
    w = np.arange(W)
    lanes = range(64) if ascending else range(63, -1, -1)
    ns, ev = [], dict.fromkeys('abcde', 0)
    for x in range(So[0]):
        d = trf[b_[:, None], x, yc, zc]                        # [W, 64, 3]
        idx = []
        for ax, (q, hi) in enumerate(((F(x), p & 4), (yc.astype(F), p & 2), (zc.astype(F), p & 1))):
            mx = F(S[ax] - 1)
            l0 = np.floor(np.clip((q + d[..., ax]).astype(F), F(0), mx))
            idx.append(np.where(hi != 0, np.minimum(l0 + 1, mx), l0).astype(np.int64))
        ix, iy, iz = idx
        rid = (ix * S[1] + iy) * S[2] + iz
        slot = ((ix & 3) << 5) | ((iy & 3) << 3) | (iz & 7)
        before = tags[w[:, None], slot]                        # what the pass found
        old = np.empty_like(rid)
        for ln in lanes:                                       # one exchange, its lanes one after the other
            old[:, ln] = tags[w, slot[:, ln]]
            tags[w, slot[:, ln]] = rid[:, ln]
        fin = tags[w[:, None], slot]                           # the read behind the exchange
        miss, orphan = old != rid, fin != rid
        loader = miss & ~orphan
        fb = orphan.sum(1) > 16
        n = np.where(fb, 64, (miss | orphan).sum(1))
        assert ((loader | orphan).sum(1) == (miss | orphan).sum(1)).all() and (n <= 64).all()
        # (b): the loaders of a wave name fewer distinct rows than there are loaders
        dup = np.array([np.unique(r[m]).size < m.sum() for r, m in zip(rid, loader)])
        r8 = np.sort(rid.reshape(W, 8, 8), -1)
        ev['a'] += int(((before == rid) & orphan).any(1).sum())
        ev['b'] += int(dup.sum())
        ev['c'] += int((r8[..., 1:] == r8[..., :-1]).any((1, 2)).sum())
        ev['d'] += int(fb.sum())
        ev['e'] += int((n == 0).sum())
        tags[fb] = -1
        ns.append(n)
    return np.stack(ns, 1), ev


@functools.lru_cache(maxsize=None)
def forward_case(si, name):
    """inputs and oracle results of one forward case, computed once and shared (never modified)"""
    B, S, So = SHAPES[si]
    rng = np.random.default_rng(5150 + 17 * si + FIELDS.index(name))
    mov = rng.random((B,) + S + (32,)).astype(F)               # (positive maps: no cancellation in the Dice sums)
    fix = rng.random((B,) + So + (32,)).astype(F)
    trf = field(name, rng, B, S, So)
    ref = {}
    for fill in (None, 0.25):
        wp = npo.spatial_transformer(mov, trf, fill_value=fill)
        ref[fill] = (wp, npo.dice(fix, wp, check_input_limits=False))
    return mov, fix, trf, ref


@functools.lru_cache(maxsize=None)
def three_state_case(X):
    """256 entries of (X, 8, 8) cycling through the six fields"""
    S = (X, 8, 8)
    rng = np.random.default_rng(6160 + X)
    mov = rng.random((B3,) + S + (32,)).astype(F)
    fix = rng.random((B3,) + S + (32,)).astype(F)
    per = -(-B3 // len(FIELDS))
    trf = np.stack([field(name, rng, per, S, S) for name in FIELDS], 1)                    # [per, 6, X, 8, 8, 3]
    trf = np.ascontiguousarray(trf.reshape((-1,) + trf.shape[2:])[:B3])
    return mov, fix, trf


@pytest.fixture(scope='module')
def cap():
    """the coverage cap, on the restatement alone, before anything is launched"""
    for ascending in (True, False):
        tot = dict.fromkeys('abcde', 0)
        for si, (B, S, So) in enumerate(SHAPES):
            for name in FIELDS:
                n, ev = exchange_events(forward_case(si, name)[2], S, ascending)
                assert n.max() <= 64
                print('CAP %s lanes first, %s %s: max n %d, wave-passes with (a) .. (e): %s'
                      % ('low' if ascending else 'high', So, name, n.max(), [ev[k] for k in 'abcde']))
                for k in tot:
                    tot[k] += ev[k]
        assert all(v > 0 for v in tot.values()), (ascending, tot)
        for X in XS:
            n, ev = exchange_events(three_state_case(X)[2], (X, 8, 8), ascending)
            print('CAP three states X = %d: max n %d, (a) .. (e): %s' % (X, n.max(), [ev[k] for k in 'abcde']))
            assert n.max() <= 64 and all(v > 0 for v in ev.values()), (ascending, X, ev)
    return True


# ----------------------------------------------------------------------------------------------------------------------------------
# the fused forward: two pass states
# ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', FIELDS)
@pytest.mark.parametrize('si', range(len(SHAPES)), ids=['21x18x29', '40x33x47-37x30x41'])
def test_fused_forward_exchange(dev, cap, si, name):
    mov, fix, trf, ref = forward_case(si, name)
    m, t, f = G(mov, dev), G(trf, dev), G(fix, dev)
    for fill in (None, 0.25):
        w_ref, d_ref = ref[fill]
        for tune in TUNES:
            what = str((SHAPES[si][1], name, fill, tune))
            fg.assert_kernels(*SHAPES[si], fill, tune)
            d, wp, s = [N(v) for v in ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, _tune=tune)]
            assert bits_equal(wp, w_ref), what
            np.testing.assert_allclose(d, d_ref, rtol=RTOL, err_msg=what)
            for _ in range(2):                                  # three calls, bit for bit: the order of the lanes must not show
                d2, w2, s2 = ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, _tune=tune)
                assert bits_equal(N(w2), wp) and bits_equal(N(d2), d) and bits_equal(N(s2), s), what
            # the register kernel on the same schedule: same warped bits, same sums up to the order of the additions
            d0, w0, s0 = ne.fused.warp_dice(m, t, f, fill_value=fill, return_warped=True, return_sums=True, _tune=(tune & ~WC) | NO_WC)
            assert bits_equal(N(w0), wp), what
            np.testing.assert_allclose(N(s0), s, rtol=2e-5, atol=1e-4, err_msg=what)


# ----------------------------------------------------------------------------------------------------------------------------------
# three pass states: the stand-alone warp and the backward forms
# ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('X', XS)
def test_standalone_warp_exchange(dev, cap, X):
    mov, _, trf = three_state_case(X)
    m, t = G(mov, dev), G(trf, dev)
    for fill in (None, 0.25):
        st = ne.layers.SpatialTransformer(fill_value=fill)
        st._variant = 10
        got = N(st([m, t]))
        assert bits_equal(got, npo.spatial_transformer(mov, trf, fill_value=fill)), (X, fill)
        assert bits_equal(N(st([m, t])), got), (X, fill)


@pytest.mark.parametrize('X', XS)
def test_backward_forms_exchange(dev, cap, X, monkeypatch):
    mov, fix, trf = three_state_case(X)
    rng = np.random.default_rng(8180 + X)
    wgt = rng.standard_normal(mov.shape).astype(F)
    m, f, wt = G(mov, dev), G(fix, dev), G(wgt, dev)
    for fill in (None, 0.25):
        got = {}
        for wc in ('1', '0'):
            monkeypatch.setenv('NRT_BWD_WC', wc)
            t1 = G(trf, dev, True)
            (-ne.fused.warp_dice(m, t1, f, fill_value=fill, laplace_smoothing=0.05).mean()).backward()
            t2 = G(trf, dev, True)
            (ne.layers.SpatialTransformer(fill_value=fill)([m, t2]) * wt).sum().backward()
            got[wc] = (N(t1.grad), N(t2.grad))
        assert np.isfinite(got['1'][0]).all() and np.abs(got['1'][0]).max() > 0 and np.abs(got['1'][1]).max() > 0
        assert bits_equal(got['1'][0], got['0'][0]), 'fused, X %d fill %r: %g' % (X, fill, np.abs(got['1'][0] - got['0'][0]).max())
        assert bits_equal(got['1'][1], got['0'][1]), 'plain, X %d fill %r: %g' % (X, fill, np.abs(got['1'][1] - got['0'][1]).max())


# ----------------------------------------------------------------------------------------------------------------------------------
# graph replay
# ----------------------------------------------------------------------------------------------------------------------------------

def test_fused_forward_exchange_under_graph_replay(dev, cap):
    """one capture of the fused forward; the field and the fixed map change between replays; every replay bit-equal to the eager call"""
    si = 1
    mov, fix, _, _ = forward_case(si, 'iid0.7')
    fields = [G(forward_case(si, name)[2], dev) for name in ('iid0.7', 'smooth4', 'edge', 'incoherent')]
    m, f, t = G(mov, dev), G(fix, dev), fields[0].clone()
    f_a, f_b = f.clone(), torch.roll(f, 3, dims=-1).contiguous()
    keep = ne.deferred.enabled
    ne.deferred.enabled = False
    try:
        def fn():
            return ne.fused.warp_dice(m, t, f, return_warped=True, return_sums=True, _tune=TUNES[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn()
        for k, tsrc in enumerate(fields + fields[:1]):
            t.copy_(tsrc)
            f.copy_(f_b if k & 1 else f_a)
            g.replay()
            torch.cuda.synchronize()
            got = [N(v) for v in out]
            for a, b in zip(got, fn()):
                assert bits_equal(a, N(b)), k
    finally:
        ne.deferred.enabled = keep
