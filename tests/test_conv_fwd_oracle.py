"""
CPU tests of oracle/conv_fwd_oracle.py (the float64 reference and the restated dispatch behind tests/test_gpu_conv_fwd_arms.py): the
reference against torch.nn.functional.conv3d in float64 on the materialised concatenation, `s2d_taps` against float64 autograd through
UpSampling3D(2) + Conv3D, and the case table of the GPU file against the kernel instances the compiler emitted
(profiles/dispatch_arms/conv_kernels.txt) -- the part of "every arm has an id" that needs no GPU.
"""

import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import conv_fwd_oracle as cfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import arm_coverage                                                                       # noqa: E402
import test_gpu_conv_fwd_arms as arms                                                     # noqa: E402  (the case table; nothing is launched)


def torch_conv(x, w, b, dilation, pb, pa):
    """conv3d of one weight set in float64 on an explicitly padded tensor: [B, X, Y, Z, C] -> [B, OX, OY, OZ, cout]"""
    xt = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 4, 1, 2, 3)
    xt = Fn.pad(xt, (pb[2], pa[2], pb[1], pa[1], pb[0], pa[0]))
    wt = torch.from_numpy(np.asarray(w, np.float64)).permute(4, 3, 0, 1, 2)
    bt = None if b is None else torch.from_numpy(np.asarray(b, np.float64))
    return Fn.conv3d(xt, wt, bt, dilation=dilation).permute(0, 2, 3, 4, 1).numpy()


# c0, c1, up, cout, k, dilation, padding, pad_before, per entry, bias
ORACLE_CASES = {
    'two sources up 2x2x2': (5, 3, (2, 2, 2), 4, (3, 3, 3), 1, 'same', None, False, True),
    'two sources up 3x1x2': (2, 6, (3, 1, 2), 5, (3, 3, 3), 1, 'same', None, False, True),
    'dilation 2': (4, 0, None, 3, (3, 1, 3), 2, 'same', None, False, True),
    'valid': (3, 0, None, 7, (3, 3, 3), 1, 'valid', None, False, False),
    '2x2x2 pad_before 1x0x1': (4, 0, None, 3, (2, 2, 2), 1, 'same', (1, 0, 1), False, True),
    '4x4x4 same': (2, 0, None, 3, (4, 4, 4), 1, 'same', None, False, True),
    'per entry': (4, 0, None, 5, (3, 3, 3), 1, 'same', None, True, True),
}


@pytest.mark.parametrize('name', sorted(ORACLE_CASES))
def test_oracle_against_torch(name):
    c0, c1, up, cout, k, dil, padding, pad, pe, bias = ORACLE_CASES[name]
    rng = np.random.default_rng(len(name))
    B, S = 2, (6, 6, 8)
    x = rng.standard_normal((B,) + S + (c0,))
    lo = rng.standard_normal((B,) + tuple(s // u for s, u in zip(S, up)) + (c1,)) if c1 else None
    w = rng.standard_normal(((B,) if pe else ()) + k + (c0 + c1, cout))
    b = rng.standard_normal(((B,) if pe else ()) + (cout,)) if bias else None
    pre, S_abs, ref = cfo.conv(x, w, b, dil, padding, lo, up, pad, pe, act='elu')
    cat = x if lo is None else np.concatenate([x, lo.repeat(up[0], 1).repeat(up[1], 2).repeat(up[2], 3)], -1)
    ext = [(kk - 1) * dil for kk in k]
    pb = list(pad) if pad is not None else [e // 2 for e in ext] if padding == 'same' else [0, 0, 0]
    pa = [e - p for e, p in zip(ext, pb)] if (padding == 'same' or pad is not None) else [0, 0, 0]
    if pe:
        want = np.concatenate([torch_conv(cat[i:i + 1], w[i], b[i], dil, pb, pa) for i in range(B)])
        wabs = np.concatenate([torch_conv(np.abs(cat[i:i + 1]), np.abs(w[i]), np.abs(b[i]), dil, pb, pa) for i in range(B)])
    else:
        want = torch_conv(cat, w, b, dil, pb, pa)
        wabs = torch_conv(np.abs(cat), np.abs(w), None if b is None else np.abs(b), dil, pb, pa)
    assert pre.shape == want.shape and (padding != 'valid' or pre.shape[1:4] == tuple(s - e for s, e in zip(S, ext)))
    assert np.abs(pre - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(S_abs - wabs).max() <= 1e-12 * np.abs(wabs).max()
    assert np.abs(ref - Fn.elu(torch.from_numpy(want)).numpy()).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(cfo.activate(pre, 'relu'), np.maximum(pre, 0)) and cfo.activate(pre, None) is pre
    assert np.array_equal(cfo.bound(S_abs, 'elu'), 8 * 2.0 ** -24 * S_abs + 3e-6) and np.array_equal(cfo.bound(S_abs), 8 * 2.0 ** -24 * S_abs)


def test_exact_inputs_give_integers():
    rng = np.random.default_rng(1)
    x, w, b = cfo.integers(rng, (1, 4, 5, 6, 8)), cfo.integers(rng, (3, 3, 3, 8, 5)), cfo.integers(rng, (5,))
    pre, S_abs, _ = cfo.conv(x, w, b, with_abs=False)
    assert S_abs is None and np.array_equal(pre, np.round(pre)) and set(np.unique(x)) == set(range(-3, 4))
    cfo.exact_condition(27, 96)
    with pytest.raises(AssertionError):
        cfo.exact_condition(27, 2 ** 24 // 243 + 1)


def test_s2d_taps_against_autograd():
    """the gradient of the low-resolution input of UpSampling3D(2) + Conv3D 3x3x3 'same' by float64 autograd, as
    test_folded_decoder_backward_matrices_cpu derives it, equals s2d_taps of the space-to-depth gradient with
    models._fold_dgrad_weights -- also when every dead tap of those weights is overwritten: s2d_taps does not read them"""
    from neurite_amd import models as nm
    torch.manual_seed(0)
    c1, group, S = 6, 16, (6, 4, 8)
    X1, Y1, Z1 = [v // 2 for v in S]
    lo = torch.randn(2, X1, Y1, Z1, c1, dtype=torch.float64, requires_grad=True)
    W = torch.randn(3, 3, 3, c1, group, dtype=torch.float64)
    upt = lo.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
    y = Fn.conv3d(upt.permute(0, 4, 1, 2, 3), W.permute(4, 3, 0, 1, 2), padding=1).permute(0, 2, 3, 4, 1)
    dpre = torch.randn_like(y)
    (y * dpre).sum().backward()
    s2d = cfo.space_to_depth2(dpre.numpy())
    wf = nm._fold_dgrad_weights(W).numpy()
    assert wf.shape == (3, 3, 3, 8 * group, c1)
    got, S_abs, _ = cfo.s2d_taps(s2d, wf, group)
    assert np.abs(got - lo.grad.numpy()).max() < 1e-12 * np.abs(got).max()
    dead = wf == 0
    assert dead.reshape(27, -1).any(1).sum() == 26                    # every tap but the centre is dead for some parity group
    noisy = np.where(dead, 7.0, wf)
    got2, S2, _ = cfo.s2d_taps(s2d, noisy, group)
    assert np.array_equal(got2, got) and np.array_equal(S2, S_abs)
    full, _, _ = cfo.conv(s2d, wf, None)                                # with the dead taps zero it is the plain convolution
    assert np.abs(full - got).max() < 1e-12 * np.abs(got).max()


def test_batch_rules_at_256_cus():
    assert [cfo.batch_for(r, 256, t) for r, t in (('unsplit', 12), ('split2', 12), ('p27', 27), ('pool', 8), ('up2', 27), (3, 5))] == [43, 22, 24, 82, 48, 3]
    for cus in (64, 104, 256, 304):
        assert cfo.batch_for('unsplit', cus, 12) * 12 >= 2 * cus
        assert cus <= cfo.batch_for('split2', cus, 12) * 12 < 2 * cus
        assert cfo.batch_for('p27', cus, 27) * 27 > 2 * cus and cfo.batch_for('up2', cus, 27) * 27 > 4 * cus


def test_plan_outside_the_family():
    assert cfo.plan('conv3d', 256, (8, 8, 16), 1, 1, 16, variant=1, packed=False).name == 'not conv_fwd: conv3d_c1_mfma'
    assert cfo.plan('conv3d', 256, (8, 8, 16), 1, 1, 8, variant=1, packed=False, dilation=2).name == 'not conv_fwd: conv3d_c1_vec'
    assert cfo.plan('conv3d', 256, (8, 8, 16), 1, 4, 8, variant=2).name.startswith('unsupported')           # cin < 8
    assert cfo.plan('conv3d', 256, (8, 8, 16), 1, 4, 8, variant=0).name == 'conv3d_direct<false>'
    assert cfo.plan('hyperconv3d', 256, (8, 8, 16), 1, 16, 16, ksize=(2, 2, 2), variant=6).name.startswith('unsupported')
    assert cfo.plan('conv3d_pad', 256, (8, 8, 16), 1, 16, 16, ksize=(3, 3, 3), pad_before=(2, 1, 1), variant=2).name.startswith('unsupported')
    # auto: the persistent schedule from two tiles per CU on, the 2x2x2 arm from 4 x 40^3 voxels on, for the CU count given
    assert cfo.plan('conv3d', 256, (5, 9, 17), 43, 16, 16).name == 'conv3d_p27_mfma<1,false,false>'
    assert cfo.plan('conv3d', 304, (5, 9, 17), 43, 16, 16).name == 'conv3d_mfma<1,true,false,false>'
    assert cfo.plan('conv3d', 256, (40, 40, 40), 4, 16, 16, ksize=(2, 2, 2)).name == 'conv3d_mfma_k2<1>'
    assert cfo.plan('conv3d', 256, (40, 40, 39), 4, 16, 16, ksize=(2, 2, 2), weights=True).name == 'conv3d_direct<false>'


def family_instances():
    fam = re.compile('^(?:%s)$' % '|'.join(arm_coverage.FAMILY_SETS['conv_fwd']))
    found = set()
    for ln in open(os.path.join(ROOT, 'profiles', 'dispatch_arms', 'conv_kernels.txt')):
        m = re.match(r'(.*?)\s+v\d+\s+s\d+\s+spill\d+', ln)
        if m and fam.match(arm_coverage.norm(m.group(1))):
            found.add(arm_coverage.norm(m.group(1)))
    return found


def test_case_table_names_every_emitted_instance():
    """every conv_fwd instance of conv_kernels.txt is named by a case of tests/test_gpu_conv_fwd_arms.py at 256 CUs (none is listed as
    unreachable), every id is what `plan` derives for each of the case's shapes, and the ids are distinct"""
    inst = family_instances()
    kernels = {k for k in inst if not re.match(r'space_to_depth2|conv3d_pack_', k)}
    assert len(kernels) == 41 and len(inst) == 46, sorted(inst)
    assert arm_coverage.UNREACHABLE['conv_fwd'] == []
    assert len(set(arms.IDS)) == len(arms.IDS) == len(arms.CASES)
    named = set()
    for cid, c in zip(arms.IDS, arms.CASES):
        for S, rule in c.shapes:
            B, p = arms.case_plan(c, 256, S, rule)
            assert cfo.plan_id(p) + ' ' + c.label == cid, (cid, S, B, p)
            assert p.name in kernels, (cid, p)
            named.add(p.name)
            if c.also0:
                assert cfo.plan(c.entry, 256, S, B, c.c0, c.cout, ksize=c.k, variant=0).name == p.name
    assert named == kernels, sorted(kernels - named)
    # the mechanisms the large-grid shapes are there for
    t = {cid: int(re.search(r' t(\d+)', cid).group(1)) for cid in arms.IDS}
    z = {cid: int(re.search(r' z(\d+)', cid).group(1)) for cid in arms.IDS}
    for fam_re, key in ((r'conv3d_p27_mfma<%d,false,false>', t), (r'conv3d_p27_mfma<%d,false,true>', t), (r'conv3d_up2_mfma<%d,0>', t)):
        for nt in (1, 2, 3, 4):
            assert any(cid.startswith(fam_re % nt) and key[cid] == 3 for cid in arms.IDS), fam_re % nt
    for nt in (2, 3, 4):
        assert any(cid.startswith('conv3d_p27_mfma<%d,true,false>' % nt) and t[cid] == 3 for cid in arms.IDS)
    for hyper in ('false', 'true'):
        for nt in (1, 2, 3, 4):
            for fast in ('true', 'false'):
                assert any(cid.startswith('conv3d_mfma<%d,%s,false,%s> z1 ' % (nt, fast, hyper)) for cid in arms.IDS)
            assert any(cid.startswith('conv3d_mfma<%d,false,false,%s> z1 t1 no-prefetch,lds>64K' % (nt, hyper)) for cid in arms.IDS)
            assert any(cid.startswith('conv3d_mfma<%d,false,false,%s> z1 t1 prefetch' % (nt, hyper)) for cid in arms.IDS)
        assert {z[cid] for cid in arms.IDS if cid.startswith('conv3d_mfma<1,true,false,%s>' % hyper)} == {1, 2, 3, 4}
        assert any(cid.startswith('conv3d_mfma<2,true,false,%s> z2' % hyper) for cid in arms.IDS)
    for nt in (1, 2, 3, 4):
        assert any(cid.startswith('conv3d_mfma<%d,true,true,false> z1' % nt) for cid in arms.IDS)
    assert any(cid.startswith('conv3d_mfma<2,true,true,false> z2') for cid in arms.IDS)
    assert any(cid.startswith('conv3d_direct<false> z1 t2') for cid in arms.IDS)
