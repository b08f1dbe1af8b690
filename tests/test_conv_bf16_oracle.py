"""
CPU tests of oracle/conv_bf16_oracle.py (the rounding, the references and the restated dispatch behind
tests/test_gpu_conv_bf16_arms.py): `rne_bf16` against torch's conversion and on hand-written ties, the glue references against torch in
float64, and the case table of the GPU file against `plan` at 256 compute units and against the kernel instances the compiler emitted
(profiles/dispatch_arms/conv_bf16_kernels.txt) -- the part of "every arm has an id" that needs no GPU.
"""

import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import conv_bf16_oracle as cbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import arm_coverage                                                                       # noqa: E402
import test_gpu_conv_bf16_arms as arms                                                    # noqa: E402  (the case table; nothing is launched)

F, F64 = np.float32, np.float64


def torch_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(torch.bfloat16).float().numpy()


def test_rne_bf16_against_torch():
    ints = np.arange(-70000, 70001).astype(F)
    assert np.array_equal(cbo.rne_bf16(ints).view(np.uint32), torch_bf16(ints).view(np.uint32))
    rng = np.random.default_rng(0)
    g = (rng.standard_normal(200000) * np.exp(rng.uniform(-20, 20, 200000))).astype(F)
    assert np.array_equal(cbo.rne_bf16(g).view(np.uint32), torch_bf16(g).view(np.uint32))
    assert cbo.rne_bf16(g.reshape(4, -1)).shape == (4, 50000)


def test_rne_bf16_on_ties():
    """bf16 keeps 8 significant bits: between 256 and 512 the values are the even integers, between 512 and 1024 the multiples of 4"""
    tie = [(257, 256), (259, 260), (261, 260), (263, 264), (514, 512), (518, 520), (522, 520), (1 + 2.0 ** -8, 1.0), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6),
           (2.0 ** -20 * 257, 2.0 ** -20 * 256), (2.0 ** 20 * 259, 2.0 ** 20 * 260), (511, 512), (1022, 1024), (1018, 1016)]
    near = [(1023, 1024), (513, 512), (515, 516), (517, 516), (519, 520), (1 + 3 * 2.0 ** -9, 1 + 2.0 ** -7), (1 + 2.0 ** -9, 1.0), (257.5, 258), (256.99, 256)]
    for v, want in tie + near:
        for s in (1.0, -1.0):
            assert cbo.rne_bf16(np.array([s * v], F))[0] == F(s * want), (s * v, want)
    assert cbo.rne_bf16(np.array([0.0, -0.0], F)).view(np.uint32).tolist() == [0, 0x80000000]
    up, down = [v for v, w in tie if w > v], [v for v, w in tie if w < v]
    s = cbo.rounding_shares(np.array(up + up + down + [v for v, _ in near] + [256, 512, 3], F64))
    n = 2 * len(up) + len(down) + len(near) + 3
    assert s == cbo.Shares((n - 3) / n, 2 * len(up) / n, len(down) / n, len(near) / n)
    # bits and back
    v = cbo.gaussian_bf16(np.random.default_rng(1), (5, 7))
    assert np.array_equal(cbo.from_bits(cbo.to_bits(v)), v) and cbo.to_bits(v).dtype == np.uint16
    with pytest.raises(AssertionError):
        cbo.to_bits(np.array([257], F))
    assert cbo.expected_bits(np.array([257.0, 259.0, -3.0, -0.0, 0.0])).tolist() == [0x4380, 0x4382, 0xC040, 0x8000, 0]
    with pytest.raises(AssertionError):
        cbo.expected_bits(np.array([2.0 ** 24 + 1]))


def test_rounding_bias_and_premise():
    rng = np.random.default_rng(2)
    for n in (4, 5, 7, 16, 50, 160):
        b = cbo.rounding_bias(rng, n)
        assert b.dtype == F and np.array_equal(b, np.round(b)) and np.abs(b).min() >= 257 and np.abs(b).max() <= 1000
        assert np.array_equal(np.sign(b), np.where(np.arange(n) % 2, -1, 1))
        # with a spread of 16 products of integers -3 .. 3 on top (the narrowest case of the table), none and relu
        ref = b.astype(F64) + (rng.integers(-3, 4, (4000, n, 16)) * rng.integers(-3, 4, (4000, n, 16))).sum(-1)
        cbo.check_shares([ref])
        cbo.check_shares([np.maximum(ref, 0)], 'relu')
    with pytest.raises(AssertionError):
        cbo.check_shares([np.arange(-200, 200.0)])


def test_glue_references_against_torch():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 9, 8, 7, 5))
    xt = torch.from_numpy(x).permute(0, 4, 1, 2, 3)
    for pool in ((2, 2, 2), (3, 1, 2), (1, 2, 4)):
        want = Fn.max_pool3d(xt, pool).permute(0, 2, 3, 4, 1).numpy()
        assert np.array_equal(cbo.maxpool(x, pool, False), want) and want.shape[1:4] == cbo.pooled_shape((9, 8, 7), pool, False)
        want = Fn.max_pool3d(xt, pool, ceil_mode=True).permute(0, 2, 3, 4, 1).numpy()
        assert np.array_equal(cbo.maxpool(x, pool, True), want) and want.shape[1:4] == cbo.pooled_shape((9, 8, 7), pool, True)
    lo, skip = rng.standard_normal((2, 3, 4, 2, 5)), rng.standard_normal((2, 3, 8, 6, 3))
    up = torch.from_numpy(lo).repeat_interleave(1, 1).repeat_interleave(2, 2).repeat_interleave(3, 3)
    assert np.array_equal(cbo.upsample_concat(skip, lo, (1, 2, 3)), torch.cat([torch.from_numpy(skip), up], -1).numpy())
    assert np.array_equal(cbo.upsample_concat(None, lo, (1, 2, 3)), up.numpy())
    z = rng.standard_normal((50, 33)) * 4
    assert np.abs(cbo.softmax_lastdim(z) - torch.softmax(torch.from_numpy(z), -1).numpy()).max() < 1e-15
    xv, w, b = rng.standard_normal((50, 7)), rng.standard_normal((7, 11)), rng.standard_normal(11)
    pre, S = cbo.conv1x1(xv, w, b)
    assert np.abs(pre - (torch.from_numpy(xv) @ torch.from_numpy(w) + torch.from_numpy(b)).numpy()).max() < 1e-13
    assert np.abs(S - (np.abs(xv) @ np.abs(w) + np.abs(b))).max() < 1e-13 and np.array_equal(cbo.conv1x1(xv, w)[0], xv @ w)
    a, c = torch.from_numpy(xv), torch.from_numpy(rng.standard_normal((50, 7)))
    sc, sh = torch.from_numpy(rng.standard_normal(7)), torch.from_numpy(rng.standard_normal(7))
    for act, fn in ((None, lambda v: v), ('elu', Fn.elu), ('relu', torch.relu), ('sigmoid', torch.sigmoid)):
        for got, want in ((cbo.add_act_affine(a, c, act=act), fn(a + c)), (cbo.add_act_affine(a, None, sc, sh, act), fn(a) * sc + sh),
                          (cbo.add_act_affine(a, c, sc, sh, act), fn(a + c) * sc + sh), (cbo.add_act_affine(a, c, act=act, mul=True), fn(a) * c),
                          (cbo.add_act_affine(a, c, sc, sh, act, True), fn(a) * c * sc + sh)):
            assert np.abs(got - want.numpy()).max() < 1e-14
    # the bounds are the suite's own
    assert np.array_equal(cbo.bound_conv(pre, S, 'elu'), 2.0 ** -8 * np.abs(pre) + 9 * 2.0 ** -24 * S + 3e-6)
    assert np.array_equal(cbo.bound_conv(pre, S), 2.0 ** -8 * np.abs(pre) + 9 * 2.0 ** -24 * S)
    assert np.array_equal(cbo.bound_prob(S), 2.0 ** -8 * S + 1e-6)
    assert np.array_equal(cbo.bound_elementwise(pre), 2.0 ** -8 * np.abs(pre) + 4e-7 * (1 + np.abs(pre)))


def test_plan_by_hand():
    """the arithmetic the issue's holes rest on, at 256 CUs"""
    P = cbo.plan
    big = cbo.batch_for('unsplit', 256, 12)
    assert big == 43
    assert [P(256, (5, 9, 17), 2, 16, co).name for co in (16, 32, 40, 64)] == ['conv3d_bf16<1>'] * 4
    assert [P(256, (5, 9, 17), 2, 16, co).nsplit for co in (16, 32, 40, 64)] == [1, 2, 3, 4]
    assert [P(256, (5, 9, 17), big, 16, co).name for co in (16, 32, 33, 40, 48, 64)] == ['conv3d_bf16<%d>' % n for n in (1, 2, 3, 3, 3, 4)]
    assert P(256, (5, 9, 17), big - 1, 16, 40).name == 'conv3d_bf16<1>'
    p = P(256, (5, 9, 17), 2, 16, 80)
    assert (p.name, p.nsplit, p.live_last) == ('conv3d_bf16<4>', 2, 1)
    # halo rows x bytes per row: CG 4 at dilation 1 and 2 (above 64 KB), 2 at 3, 1 at 4, none at 6; dense rows are 16 bytes
    assert [(P(256, (4, 4, 16), 1, 16, 16, dilation=d).CG, P(256, (4, 4, 16), 1, 16, 16, dilation=d).lds) for d in (1, 2, 3, 4)] == [
        (4, 648 * 80 + 112), (4, 1280 * 80 + 112), (2, 2200 * 48 + 112), (1, 3456 * 32 + 112)]
    assert P(256, (4, 4, 16), 1, 16, 16, dilation=6).name.startswith('unsupported') and P(256, (4, 4, 16), 1, 4, 16, dilation=6).lds == 7168 * 16 + 4 * 128
    assert P(256, (4, 4, 16), 1, 16, 16, out_off=2).name.startswith('invalid') and P(256, (4, 4, 16), 1, 16, 16, out_off=8).store == 'pack'
    p = P(256, (4, 4, 16), 1, 40, 16, dilation=3)
    assert (p.CG, p.nchunk, p.last, p.nks) == (2, 3, 1, 35)
    assert [P(256, (4, 4, 16), 1, c0, 16, c1=c1, src0_off=o).loader for c0, c1, o in ((16, 0, 0), (16, 0, 2), (12, 0, 0), (7, 0, 0), (2, 4, 0), (16, 32, 0), (4, 12, 0))
            ] == ['vec', 'scalar', 'scalar', 'dense', 'dense', 'vec', 'scalar']
    assert P(256, (4, 4, 16), 1, 7, 16).nks == 6 and P(256, (4, 4, 16), 1, 1, 16).nks == 1
    assert cbo.packed_weight_bytes((3, 3, 3), 256, 160) == 2 * 1146880 and cbo.plan_pack((3, 3, 3), 256, 160).passes == 2
    assert cbo.plan_conv1x1(4096 * 256, 16, 16).passes == 1 and cbo.plan_conv1x1(4096 * 256 + 1, 16, 16).passes == 2
    assert cbo.plan_add(8 * 8192 * 256, 16, True, True).passes == 1 and cbo.plan_add(8 * 8192 * 256 + 8, 16, True, True).passes == 2
    assert cbo.plan_add(384, 6, True, True).name == 'add_act_affine_bf16<1>' and cbo.plan_add(384, 6, True, False).name == 'add_act_affine_bf16<8>'


def family_instances():
    fam = re.compile('^(?:%s)$' % '|'.join(arm_coverage.FAMILY_SETS['conv_bf16']))
    found = set()
    for ln in open(os.path.join(ROOT, 'profiles', 'dispatch_arms', 'conv_bf16_kernels.txt')):
        m = re.match(r'(.*?)\s+v\d+\s+s\d+\s+spill\d+', ln)
        if m and fam.match(arm_coverage.norm(m.group(1))):
            found.add(arm_coverage.norm(m.group(1)))
    return found


def test_case_table_names_every_emitted_instance():
    """every conv_bf16 instance of conv_bf16_kernels.txt is named by an id of tests/test_gpu_conv_bf16_arms.py at 256 CUs (none is
    listed as unreachable), every id is what the plans derive for each of its shapes, the ids are distinct, and the arms the file
    exists for are in it"""
    inst = family_instances()
    assert len(inst) == 17 and arm_coverage.UNREACHABLE['conv_bf16'] == [], sorted(inst)
    ids = arms.ALL_IDS
    assert len(set(ids)) == len(ids)
    for cid, c in zip(arms.IDS, arms.CASES):
        for S, rule in c.shapes:
            B, p = arms.case_plan(c, 256, S, rule)
            assert cbo.plan_id(p) + ' ' + c.label == cid, (cid, S, B, p)
            if c.c1:
                assert all(s % u == 0 for s, u in zip(S, c.up))
    named = {k for k in inst if any(cid.startswith(k + ' ') for cid in ids) or ('+ ' + k + ' ') in arms.PACK_ID}
    assert named == inst, sorted(inst - named)
    conv = [cid for cid in arms.IDS if cid.startswith('conv3d_bf16')]

    def has(*parts):
        return any(all(re.search(p, cid) for p in parts) for cid in conv)
    for nt, z in ((1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (3, 1), (4, 1), (4, 2), (4, 3)):
        assert has(r'^conv3d_bf16<%d> z%d ' % (nt, z)), (nt, z)
    assert has(r'^conv3d_bf16<3> .* scalar-store') and has(r'^conv3d_bf16<4> z2 live1 ') and has(r'^conv3d_bf16<4> z1 live4 vec cg4 ')
    for nt in (2, 3, 4):
        assert has(r'^conv3d_bf16<%d> z1 .* vec cg4 chunks1 last2 ' % nt) and has(r'^conv3d_bf16<%d> z1 .* vec cg4 chunks1 last3 ' % nt)
    for part in (r' vec cg4 chunks2 last1 ', r' vec cg4 .* lds>64K', r' vec cg2 chunks1 last2 ', r' vec cg2 chunks3 last1 ', r' vec cg1 chunks3 last1 ',
                 r' scalar cg4 .* src 2 bytes off', r' scalar cg4 .* 12->16', r' scalar cg4 .* last3 .* 20->16', r' dense ks1 ', r' dense ks6 .* 7->16',
                 r' dense .* 2\+4->16', r' vec .* 16\+32->16 up 1x2x3', r' scalar .* 4\+12->16', r' dense ks4 lds>64K .* dil 6', r'k 1x1x1', r'k 2x2x2', r'k 1x3x5',
                 r' valid$', r'chunks8 last4 .* 256->160'):
        assert has(part), part
    assert sum(c.nobias for c in arms.CASES) == 3 and {arms.case_plan(c, 256, *c.shapes[0])[1].loader for c in arms.CASES if c.nobias} == {'vec', 'scalar', 'dense'}
    assert any(cid.startswith('unsupported') for cid in arms.IDS) and any(cid.startswith('invalid') for cid in arms.IDS)
    # every glue instance has a second grid-stride pass, and both of its paths
    for k in inst - {'conv3d_bf16<%d>' % n for n in (1, 2, 3, 4)} - {'conv1x1_bf16<32>', 'conv1x1_bf16<64>', 'conv3d_pack_bf16<unsignedshort>'}:
        assert any(cid.startswith(k + ' ') and ' p2 ' in cid for cid in ids) or k == 'conv3d_pack_bf16<float>', k
    for path in ('vec,store16', 'vec,store2', 'scalar'):
        assert any(cid.startswith('conv1x1_bf16<') and ' %s ' % path in cid for cid in ids)
    # no single buffer above 80 MB
    for label, S, B, ch, pool, same in arms.MP:
        assert 2 * B * int(np.prod(S)) * ch <= 80e6
    for label, L, B, c0, c1, up, off in arms.UC:
        assert 2 * B * int(np.prod(arms._uc_shape(L, up))) * (c0 + c1) <= 80e6
    assert all(2 * rows * ch <= 80e6 for _, rows, ch, *_ in arms.AA) and 2 * arms.SECOND_4096 * 16 <= 80e6
