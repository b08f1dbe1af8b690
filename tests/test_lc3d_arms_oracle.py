"""
CPU tests of oracle/lc3d_arms_oracle.py (the float64 references and the restated dispatch behind tests/test_gpu_lc3d_arms.py): the
backward reference against float64 autograd of oracle/grad_oracle.lc3d, the premise of the exact check (integer sums below 2^24,
bfloat16 outputs within 256) on the reference of every case, and the case table of the GPU file against the kernel instances the
compiler emitted (profiles/dispatch_arms/lc3d_kernels.txt) -- the part of "every arm has an id" that needs no GPU.
"""

import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import grad_oracle as go
from oracle import lc3d_arms_oracle as lco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import arm_coverage                                                                       # noqa: E402
import test_gpu_lc3d_arms as arms                                                         # noqa: E402  (the case table; nothing is launched)


@pytest.mark.parametrize('act', [None, 'elu', 'relu'])
@pytest.mark.parametrize('ksize,strides', [((3, 3, 3), (1, 1, 1)), ((2, 3, 2), (2, 1, 1)), ((1, 2, 2), (1, 2, 3))])
def test_backward_reference_against_autograd(act, ksize, strides):
    rng = np.random.default_rng(len(str(act)) + ksize[0])
    B, S, cin, cout = 3, (5, 6, 7), 3, 4
    osh = lco.out_shape(S, ksize, strides)
    O, Fd = int(np.prod(osh)), int(np.prod(ksize)) * cin
    x, K, bias, g = rng.standard_normal((B,) + S + (cin,)), rng.standard_normal((O, Fd, cout)), rng.standard_normal(osh + (cout,)), rng.standard_normal((B, O, cout))
    xt, kt, bt = (torch.from_numpy(v).requires_grad_() for v in (x, K, bias))
    yt = go.lc3d(xt, kt, bt, ksize, strides, act)
    (yt * torch.from_numpy(g).reshape(yt.shape)).sum().backward()
    pre, A, n = lco.forward(x, K, bias, ksize, strides)
    y = lco.activate(pre, act)
    assert n == Fd + 1 and np.abs(y - yt.detach().numpy().reshape(B, O, cout)).max() < 1e-12
    assert np.all(A >= np.abs(pre) - 1e-12)
    assert np.abs(np.einsum('bof,ofc->boc', lco.patches(x, ksize, strides), K) + bias.reshape(1, O, cout) - pre).max() < 1e-12
    r = lco.backward(x, K, y, g, ksize, strides, act)
    for got, want, A_, n_ in ((r.dK, kt.grad, r.A_dK, B), (r.dbias, bt.grad.reshape(O, cout), r.A_dbias, B), (r.dx, xt.grad, r.A_dx, r.n_dx)):
        want = want.numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert np.all(A_ >= np.abs(got) - 1e-12)
    # a voxel is read by n_dx / cout (position, patch element) pairs: all of them, counted
    assert r.n_dx.sum() == B * O * Fd * cout and r.n_b == B
    assert r.dx[r.n_dx == 0].size == 0 or not r.dx[r.n_dx == 0].any()


def test_bf16_bits():
    v = np.array([1.0, -3.0, 256.0, 257.0, 258.0, 259.0, 1.00390625, 1.01171875, 3.0e-5], np.float32)
    back = lco.bf16_value(lco.bf16_bits(v))
    assert np.array_equal(back[:3], v[:3]) and back[3] == 256.0 and back[4] == 258.0 and back[5] == 260.0          # ties to even
    assert back[6] == 1.0 and back[7] == 1.015625 and abs(back[8] - v[8]) <= 2.0 ** -9 * v[8]
    t = torch.from_numpy(v).bfloat16().float().numpy()
    assert np.array_equal(back, t)


def test_plans_outside_the_table():
    K3 = (3, 3, 3)
    # the bfloat16 matrix-core form never needs two patch pieces per lane: F <= 16 NCMAX gives at most 56 pieces
    for cout, ncmax in ((16, 27), (32, 28)):
        assert lco.stage_chunks('bfloat16', 16, K3) == 54 and ncmax * 16 * 2 // 16 <= 56
    assert lco.plan_fwd('bfloat16', 8, (6, 6, 6), 16, K3, (1, 1, 1), 16)[0].name == 'lc3d_fwd_mfma_blk<unsignedshort,4,2,27,4>'
    assert lco.plan_fwd('bfloat16', 8, (6, 6, 6), 16, K3, (1, 1, 2), 16)[0].name == 'lc3d_fwd_mfma<unsignedshort,4,2,27,1>'
    assert lco.plan_fwd('float32', 8, (6, 6, 6), 16, K3, (1, 1, 2), 16)[0].name == 'lc3d_fwd_mfma<float,4,2,28,2>'
    assert lco.plan_fwd('float32', 2, (6, 6, 6), 16, K3, (1, 1, 1), 16)[0].name == 'lc3d_fwd<float,2,16,true,2>'           # batch < 3
    assert lco.plan_fwd('float32', 8, (6, 6, 6), 16, K3, (1, 1, 1), 16, y_aligned=False)[0].name == 'lc3d_fwd<float,4,16,true,2>'
    assert lco.plan_fwd('float32', 2, (6, 6, 6), 16, K3, (1, 1, 1), 64)[0].name == 'lc3d_generic<float>'                   # nit 108
    assert lco.plan_fwd('float32', 2, (6, 6, 6), 16, K3, (1, 1, 1), 64, variant=2) == 'unsupported'
    assert lco.plan_bwd('float32', 2, (6, 6, 6), 16, K3, (1, 1, 1), 64) == 'unsupported'
    assert lco.plan_bwd('float32', 2, (6, 6, 6), 3, K3, (1, 1, 1), 12) == 'unsupported' and lco.plan_bwd('float32', 2, (6, 6, 6), 3, K3, (1, 1, 1), 5) == 'unsupported'
    assert lco.plan_bwd('float32', 2, (6, 6, 6), 3, K3, (1, 1, 1), 8, aligned=False) == 'unsupported'
    # the grid caps: 5 x 4 x 256 blocks forward, 16 x 256 backward; SPLIT waves share a position
    assert lco.plan_fwd('float32', 1, (1, 1, 30000), 1, (1, 1, 1), (1, 1, 1), 4)[0].blocks == 5120
    assert lco.plan_bwd('float32', 1, (1, 1, 30000), 1, (1, 1, 1), (1, 1, 1), 4)[0].blocks == 4096
    assert lco.plan_bwd('float32', 1, (1, 1, 100), 129, (1, 1, 1), (1, 1, 1), 32)[0].blocks == 50
    assert lco.plan_fwd('float32', 1, (1, 1, 100), 257, (1, 1, 1), (1, 1, 1), 32)[0].blocks == 100
    assert lco.plan_pad(4, 16, 32) == 'pad3d_rows<unsignedint>' and lco.plan_pad(4, 18, 32) == lco.plan_pad(6, 16, 32) == 'pad3d_rows<unsignedshort>'


def family_instances():
    fam = re.compile('^(?:%s)$' % '|'.join(arm_coverage.FAMILY_SETS['lc3d']))
    found = set()
    for ln in open(os.path.join(ROOT, 'profiles', 'dispatch_arms', 'lc3d_kernels.txt')):
        m = re.match(r'(.*?)\s+v\d+\s+s\d+\s+spill\d+', ln)
        if m and fam.match(arm_coverage.norm(m.group(1))):
            found.add(arm_coverage.norm(m.group(1)))
    return found


def test_case_table_names_every_emitted_instance():
    """every instance of lc3d_kernels.txt is named by a case of tests/test_gpu_lc3d_arms.py or matched by the unreachable list, every
    id is what the plans derive for each of the case's geometries, and the ids are distinct"""
    inst = family_instances()
    assert len(inst) == 148, len(inst)
    count = lambda pre: sum(k.startswith(pre) for k in inst)                              # noqa: E731
    assert [count(p) for p in ('lc3d_fwd<', 'lc3d_bwd<', 'lc3d_fwd_mfma<', 'lc3d_fwd_mfma_blk<', 'lc3d_generic<', 'pad3d_rows<')] == [60, 60, 16, 8, 2, 2]
    unreachable = re.compile('^(?:%s)$' % '|'.join(arm_coverage.UNREACHABLE['lc3d']))
    dead = {k for k in inst if unreachable.match(k)}
    assert len(dead) == 4
    ids = arms.FWD_IDS + arms.BWD_IDS + arms.STRIDE_IDS + arms.REFUSAL_IDS + arms.PAD_IDS
    assert len(set(ids)) == len(ids)
    named = set()
    for cid, c in zip(arms.FWD_IDS, arms.FWD_CASES):
        for geom in c.geoms:
            p = arms.fwd_plan(c, geom)
            assert lco.plan_id(p) + ' ' + arms.label(c) == cid, (cid, geom, p)
            named |= {l.name for l in p}
    for cid, c in zip(arms.BWD_IDS, arms.BWD_CASES):
        for geom in c.geoms:
            assert lco.plan_id(arms.bwd_plan(c, geom)) + ' ' + arms.label(c) == cid, (cid, geom)
            named |= {l.name for has_dx in (True, False) for l in arms.bwd_plan(c, geom, has_dx)}
    for cid, c in zip(arms.STRIDE_IDS, arms.STRIDE):
        assert arms.stride_id(c) == cid and cid.count(' walks 2 ') == 2
    assert sorted(int(cid.split('|')[0].split(',')[-1][0]) for cid in arms.STRIDE_IDS) == [1, 2, 4]            # one per SPLIT
    named |= {pid.split(' ')[0] for pid in arms.PAD_IDS}
    assert named <= inst and not (named & dead), sorted(named - inst)
    assert named | dead == inst, sorted(inst - named - dead)
    # what the batches are there for: a dead entry in NB 4, a second chunk, a third chunk of one entry, per (type, MAXIT, SPLIT)
    for t in ('float', 'unsignedshort'):
        for m, s in ((8, 1), (14, 1), (16, 1), (16, 2), (16, 4)):
            for pat in ('lc3d_bwd<%s,%d,4,true,%d> nb3 ' % (t, m, s), '> nb4 + lc3d_bwd<%s,%d,2,true,%d> nb2 ' % (t, m, s),
                        '> nb4 + lc3d_bwd<%s,%d,1,true,%d> nb1 ' % (t, m, s)):
                assert any(pat in cid for cid in arms.BWD_IDS), pat
            for staged in ('true', 'false'):
                for pat in ('lc3d_fwd<%s,4,%d,%s,%d> nb3 ' % (t, m, staged, s), '> nb4 + lc3d_fwd<%s,1,%d,%s,%d> nb1 ' % (t, m, staged, s)):
                    assert any(pat in cid for cid in arms.FWD_IDS), pat
    # CH = 8, the two-pass chunking of lc3d_bwd<T, 16, 4, true, SPLIT>: ids at MAXIT 16 with a full NB 4 chunk and dx
    assert any(cid.startswith('lc3d_bwd<float,16,4,true,1> nb4 + ') for cid in arms.BWD_IDS)


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_exact_premise_holds_on_the_reference(dtype):
    """with the integer inputs of every case, the sums of absolute terms are below 2^24 and, for bfloat16, y, dK and dbias are
    integers of magnitude <= 256: checked here on the reference alone (the GPU tests assert it again before they compare)"""
    bf = dtype == 'bfloat16'
    seen = set()
    for c in arms.FWD_CASES + arms.BWD_CASES:
        if c.dtype != dtype:
            continue
        for geom in c.geoms:
            key = (arms.label(c), geom)
            if key in seen:
                continue
            seen.add(key)
            S, osh, O, Fd, x, K, bias, g = arms.inputs('', c, geom, 'exact')
            assert set(np.unique(x)) <= set(range(-3, 4))
            pre, A, n = lco.forward(x.astype(np.float64), K.astype(np.float64), bias.astype(np.float64), c.k, geom[1])
            assert A.max() < 2 ** 24
            for act in (None, 'relu'):
                y = lco.activate(pre, act)
                lco.exact_range(y, bf, '%s %s y' % key)
                r = lco.backward(x, K, y, g, c.k, geom[1], act)
                assert max(r.A_dK.max(), r.A_dbias.max(), r.A_dx.max()) < 2 ** 24
                lco.exact_range(r.dK, bf, '%s %s dK' % key)
                lco.exact_range(r.dbias, bf, '%s %s dbias' % key)
                lco.exact_range(r.dx, False, '%s %s dx' % key)
            pre0, _, _ = lco.forward(x.astype(np.float64), K.astype(np.float64), None, c.k, geom[1])
            lco.exact_range(pre0, bf, '%s %s y without bias' % key)
