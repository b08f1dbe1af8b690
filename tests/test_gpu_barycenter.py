"""
utils.barycenter (csrc/barycenter.hip) on the GPU: coordinates, exact sums against the reference's own outputs
(tests/golden/barycenter_small.npz, made by tests/golden/make_barycenter_golden.py), float data against float64, the dtype / layout
plumbing, the gradient and graph capture.  Every forward call is made twice and the two results are compared bit for bit.

Which case reaches which kernel (float32 storage reads 4 elements per 16-byte group, bfloat16 / float16 read 8):
    int_c5     [2,9,10,33,5]  (1,2,3)   inner arm, per element (5 is no multiple of a group); 23 slabs: 23 partials per output
    int_c8     [2,9,10,33,8]  (1,2,3)   inner arm, 16-byte groups: 2 column lanes (float32), 1 (16-bit)
    int_c8 off the same at a base pointer that is only 4 / 2-byte aligned: inner arm, per element
    int_c68    [3,7,6,5,68]   (1,2,3)   inner arm: 17 groups on 32 column lanes (float32); 68 % 8 != 0: per element, 64 column lanes,
                                        TWO column tiles (16-bit); lines of 5 elements, shorter than the row-lane stride
    int_slabs  [1,40,40,40,4] (1,2,3)   inner arm, one column lane x 256 row lanes, 62 slabs (float32); per element (16-bit)
    int_trail  [3,31,32,33]   (1,2,3)   trailing arm, 16-byte groups; slabs of 4677 / 10912 elements: ragged heads and tails, groups
                                        that straddle a line end (33 % 4 != 0)
    int_trail off                       trailing arm, per element (unaligned base)
    int_2d     [2,3,64,64,7]  (2,3)     inner arm, k = 2, per element, outer = 6
    int_all    [2,5,6,7,3]    None      trailing arm, k = 5, one block
    int_perm   the same       (3,1)     permuted copy, trailing arm, k = 2, outer = 36, a whole reduction shorter than a block
    int_one    the same       (2,)      permuted copy, trailing arm, k = 1, R = 6
    int_long   [2,4100,3]     (1,)      inner arm with a dimension longer than the LDS coordinate table: coordinates computed in place
    [4,70001]  (1,)                     trailing arm, no table, odd length, 17 slabs per row
    eye(v)     (1,)                     trailing arm, outer = v
The second stage adds more than one partial per output wherever a case has more than one slab (int_c5, int_slabs, int_trail,
[4,70001], ...), with one run per slab or several slabs per run (int_slabs, float32: 62 slabs on 16 runs).

Measured on MI355X: the largest |err| / bound over all float cases is 0.18 for the kernels (`f_one`, a reduction over 6 elements;
0.15 for the reference's own fixtures on the same case), below 0.02 for every reduction over a thousand elements or more; gradients are within
1.5e-7 of scale (float32) and a quarter of a bfloat16 ulp of scale.  The bounds are order-free conditions, the ratios (printed by
every test) the evidence of how tight the kernels are.
"""

import numpy as np
import pytest
import torch

import neurite_amd as ne
from conftest import golden_cases, load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GOLD = golden_cases(load_golden('barycenter_small'))
INT_TAGS = sorted(t for t in GOLD if t.startswith('int_') or t.startswith('spike_'))
FLOAT_TAGS = sorted(t for t in GOLD if t.startswith('f_'))
STORAGE = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
_REF = {}


def _axes(case):
    return tuple(int(a) for a in case['axes']) if 'axes' in case else None


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _twice(x, **kw):
    """the op, called twice: run-to-run bit-identical"""
    a = ne.utils.barycenter(x, **kw)
    b = ne.utils.barycenter(x, **kw)
    torch.cuda.synchronize()
    assert a.dtype == b.dtype and np.array_equal(_bits(a.float()), _bits(b.float())), 'not bit-identical run to run'
    return a


def _grid(v, normalize, shift):
    """the reference's float32 grid of a dimension of size v, utils.py:557-561"""
    g = np.arange(v, dtype=np.float32)
    if shift:
        g = g - (v - 1) / 2
    if normalize:
        g = g / v
    assert g.dtype == np.float32
    return g


def _ref64(x, axes, normalize, shift):
    """float64 on the given values and the float32 coordinates: y64 and the bound of test 3, both [*kept, k]"""
    x = np.asarray(x, np.float64)
    nd = x.ndim
    axes = list(range(nd)) if axes is None else [a % nd for a in axes]
    kept = [a for a in range(nd) if a not in axes]
    xt = np.transpose(x, kept + axes)
    red = tuple(range(len(kept), nd))
    n = int(np.prod([xt.shape[a] for a in red]))
    den, aden = xt.sum(axis=red), np.abs(xt).sum(axis=red)
    ys, bounds = [], []
    for j, ax in enumerate(red):
        shp = [1] * nd
        shp[ax] = -1
        g = _grid(xt.shape[ax], normalize, shift).astype(np.float64).reshape(shp)
        num, anum = (xt * g).sum(axis=red), np.abs(xt * g).sum(axis=red)
        safe = np.where(den == 0, 1.0, den)
        y = np.where(den == 0, 0.0, num / safe)
        ys.append(y)
        bounds.append(np.where(den == 0, 0.0, 1.02 * (n + 4) * U * (anum + np.abs(y) * aden) / np.abs(safe)))
    cond = float(((n + 4) * U * aden / np.maximum(np.abs(den), 1e-300)).max())
    return np.stack(ys, -1), np.stack(bounds, -1), cond


def _check_bound(y, y64, bound, what):
    err = np.abs(np.asarray(y, np.float64) - y64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print('%s: worst ratio |err| / bound = %.3g' % (what, ratio))
    assert np.all(err <= bound), '%s: max |err| / bound = %.3g' % (what, ratio)
    return ratio


# ---- 1. coordinates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('v', [7, 160, 161, 1000])
def test_coordinates_are_the_reference_grid_bit_for_bit(dev, v):
    x = torch.eye(v, device=dev)
    for normalize in (False, True):
        for shift in (False, True):
            y = _twice(x, axes=(1,), normalize=normalize, shift_center=shift)
            assert y.shape == (v, 1)
            want = _grid(v, normalize, shift)
            assert np.array_equal(y.cpu().numpy()[:, 0].view(np.uint32), want.view(np.uint32)), (v, normalize, shift)


# ---- 2. exact sums ----------------------------------------------------------------------------------------------------------------
def _unaligned(x):
    """the same contiguous tensor at a base pointer one element past a 16-byte boundary"""
    buf = torch.empty(x.numel() + 8, dtype=x.dtype, device=x.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + x.numel()].view(x.shape)
    out.copy_(x)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


@pytest.mark.parametrize('storage', sorted(STORAGE))
@pytest.mark.parametrize('tag', INT_TAGS)
def test_integer_data_equals_the_reference_bit_for_bit(dev, tag, storage):
    case = GOLD[tag]
    x = torch.tensor(case['x']).to(dev).to(STORAGE[storage])
    forms = [('', x)]
    if tag in ('int_c8', 'int_trail'):
        forms.append((' off', _unaligned(x)))
    for name, xin in forms:
        for shift in (0, 1):
            want = case['y_n0_s%d' % shift]
            y = _twice(xin, axes=_axes(case), shift_center=bool(shift))
            got = y.cpu().numpy()
            assert got.shape == want.shape and got.dtype == np.float32
            assert not np.isnan(got).any()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                '%s%s %s shift %d: max |diff| %.3g' % (tag, name, storage, shift, np.abs(got - want).max())
    if tag.startswith('int_') and 'axes' in case:
        # the all-zero channel the fixture holds: exactly +0.0
        zero = y.cpu().numpy()[(-1,) * (y.dim() - 1)]
        assert np.array_equal(zero.view(np.uint32), np.zeros_like(zero).view(np.uint32))


# ---- 3. float data ------------------------------------------------------------------------------------------------------------------
FLOAT_SHAPES = [(GOLD[t]['x'].shape, _axes(GOLD[t])) for t in INT_TAGS if t.startswith('int_')] + [((4, 70001), (1,))]


def _float_case(i, signed=False):
    key = (i, signed)
    if key not in _REF:
        shape, axes = FLOAT_SHAPES[i]
        rng = np.random.default_rng(7000 + i)
        x = rng.random(shape, dtype=np.float32)
        if signed:
            x = (2 * x - np.float32(0.5)).astype(np.float32)              # uniform on [-0.5, 1.5): sum |x| / |sum x| is about 1.25
        x.setflags(write=False)
        _REF[key] = (x, axes)
    return _REF[key]


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
@pytest.mark.parametrize('i', range(len(FLOAT_SHAPES)), ids=lambda i: 'x'.join(map(str, FLOAT_SHAPES[i][0])) + '_' + str(FLOAT_SHAPES[i][1]))
def test_uniform_data_within_the_order_free_bound(dev, i, storage):
    x, axes = _float_case(i)
    xd = torch.tensor(x).to(dev).to(STORAGE[storage])
    stored = xd.float().cpu().numpy()
    for shift in (False, True):
        y64, bound, cond = _ref64(stored, axes, True, shift)
        assert cond <= 0.01, cond
        y = _twice(xd, axes=axes, normalize=True, shift_center=shift)
        _check_bound(y.cpu().numpy(), y64, bound, '%s %s %s shift %d' % (FLOAT_SHAPES[i][0], axes, storage, shift))


def test_signed_data_within_the_order_free_bound(dev):
    x, axes = _float_case(0, signed=True)
    xd = torch.tensor(x).to(dev)
    for normalize in (False, True):
        for shift in (False, True):
            y64, bound, cond = _ref64(x, axes, normalize, shift)
            assert cond <= 0.01, cond
            y = _twice(xd, axes=axes, normalize=normalize, shift_center=shift)
            _check_bound(y.cpu().numpy(), y64, bound, 'signed n %d s %d' % (normalize, shift))


@pytest.mark.parametrize('tag', FLOAT_TAGS)
def test_reference_fixtures_and_kernels_meet_the_same_bound(dev, tag):
    case = GOLD[tag]
    x, axes = case['x'], _axes(case)
    xd = torch.tensor(x).to(dev)
    for normalize in (0, 1):
        for shift in (0, 1):
            y64, bound, cond = _ref64(x, axes, normalize, shift)
            assert cond <= 0.01
            fixture = case['y_n%d_s%d' % (normalize, shift)]
            assert fixture.shape == y64.shape
            _check_bound(fixture, y64, bound, '%s reference n %d s %d' % (tag, normalize, shift))
            y = _twice(xd, axes=axes, normalize=bool(normalize), shift_center=bool(shift))
            assert tuple(y.shape) == fixture.shape
            _check_bound(y.cpu().numpy(), y64, bound, '%s kernel n %d s %d' % (tag, normalize, shift))


# ---- 4. dtype and layout ----------------------------------------------------------------------------------------------------------------
def test_dtype_casts_the_float32_result(dev):
    x = torch.tensor(GOLD['f_spatial']['x']).to(dev)
    kw = dict(axes=(1, 2, 3), normalize=True, shift_center=True)
    y = _twice(x, **kw)
    assert y.dtype == torch.float32
    for dtype in (torch.float64, torch.bfloat16):
        z = _twice(x, dtype=dtype, **kw)
        assert z.dtype == dtype and torch.equal(z, y.to(dtype))


def test_other_input_dtypes_are_cast_to_float32(dev):
    case = GOLD['int_c5']
    x8 = torch.tensor(case['x']).to(dev)
    want = _twice(x8.float(), axes=(1, 2, 3))
    for dtype in (torch.uint8, torch.int32, torch.int64, torch.float64):
        y = _twice(x8.to(dtype), axes=(1, 2, 3))
        assert y.dtype == torch.float32 and np.array_equal(_bits(y), _bits(want)), dtype


def test_strided_views_give_the_bits_of_their_contiguous_copy(dev):
    x = torch.tensor(_float_case(0)[0]).to(dev)
    views = [x[:, ::2], x[..., 1:4], x.transpose(1, 3), x[:, :, :, ::3, :]]
    for v in views:
        assert not v.is_contiguous()
        for axes in ((1, 2, 3), None, (3, 1)):
            a = _twice(v, axes=axes, normalize=True)
            b = _twice(v.contiguous(), axes=axes, normalize=True)
            assert np.array_equal(_bits(a), _bits(b))
    # negative axes count from the end
    assert np.array_equal(_bits(_twice(x, axes=(-4, -3, -2))), _bits(_twice(x, axes=(1, 2, 3))))
    assert np.array_equal(_bits(_twice(x, axes=-1)), _bits(_twice(x, axes=(4,))))


# ---- 5. gradient ------------------------------------------------------------------------------------------------------------------------
def _torch_restatement(x, axes, normalize, shift):
    """the reference's expression in torch (float64 values, float32 coordinates)"""
    nd = x.dim()
    axes = list(range(nd)) if axes is None else [a % nd for a in axes]
    kept = [a for a in range(nd) if a not in axes]
    xt = x.permute(*kept, *axes)
    red = tuple(range(len(kept), nd))
    grids = [torch.tensor(_grid(xt.shape[a], normalize, shift).astype(np.float64)) for a in red]
    mesh = torch.stack(torch.meshgrid(*grids, indexing='ij'), -1)
    num = (mesh * xt.unsqueeze(-1)).sum(dim=red)
    den = xt.unsqueeze(-1).sum(dim=red)
    return torch.where(den == 0, torch.zeros_like(num), num / torch.where(den == 0, torch.ones_like(den), den))


GRAD_CASES = [((2, 9, 10, 33, 5), (1, 2, 3), True, True), ((4, 70001), (1,), True, False), ((2, 5, 6, 7, 3), (3, 1), False, True)]


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
@pytest.mark.parametrize('shape,axes,normalize,shift', GRAD_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_gradient_against_float64_autograd(dev, shape, axes, normalize, shift, storage):
    rng = np.random.default_rng(sum(shape))
    x = torch.tensor(rng.random(shape, dtype=np.float32)).to(STORAGE[storage])
    x64 = x.to(torch.float64).requires_grad_(True)
    y64 = _torch_restatement(x64, axes, normalize, shift)
    w = torch.tensor(rng.standard_normal(tuple(y64.shape)).astype(np.float32))
    (y64 * w.double()).sum().backward()
    want = x64.grad
    scale = float(want.abs().max())

    grads = []
    for _ in range(2):
        xd = x.to(dev).requires_grad_(True)
        y = ne.utils.barycenter(xd, axes=axes, normalize=normalize, shift_center=shift)
        (y * w.to(dev)).sum().backward()
        assert xd.grad.dtype == STORAGE[storage] and xd.grad.shape == xd.shape
        grads.append(xd.grad)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(grads[0]), _bits(grads[1])), 'gradient not bit-identical run to run'
    got = grads[0].cpu()
    assert torch.isfinite(got.float()).all()
    if storage == 'f32':
        err = float((got.double() - want).abs().max())
        print('gradient %s %s: max |err| / scale = %.3g' % (shape, axes, err / scale))
        assert err <= 2e-4 * scale
    else:
        ulp = 2.0 ** (np.floor(np.log2(scale)) - 7)                      # one bfloat16 ulp at the gradient's largest magnitude
        err = float((got.double() - want.to(torch.bfloat16).double()).abs().max())
        print('gradient %s %s bf16: max |err| / ulp(scale) = %.3g' % (shape, axes, err / ulp))
        assert err <= ulp


def test_gradient_of_an_empty_channel_is_zero(dev):
    rng = np.random.default_rng(11)
    x = rng.random((2, 9, 10, 33, 5), dtype=np.float32)
    x[..., 2] = 0
    x[1, ..., 4] = 0
    xd = torch.tensor(x).to(dev).requires_grad_(True)
    y = ne.utils.barycenter(xd, axes=(1, 2, 3), normalize=True, shift_center=True)
    (y * torch.tensor(rng.standard_normal((2, 5, 3)).astype(np.float32)).to(dev)).sum().backward()
    g = xd.grad.cpu().numpy()
    assert not np.isnan(g).any()
    assert np.all(g[..., 2] == 0) and np.all(g[1, ..., 4] == 0)
    assert np.abs(g[..., 0]).max() > 0
    assert np.all(y.detach().cpu().numpy()[:, 2] == 0)


# ---- 6. graph capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,axes', [((2, 9, 10, 33, 8), (1, 2, 3)), ((3, 31, 32, 33), (1, 2, 3))], ids=['inner', 'trailing'])
def test_forward_and_backward_capture_into_a_graph(dev, shape, axes):
    rng = np.random.default_rng(3)
    first, second = (torch.tensor(rng.random(shape, dtype=np.float32)).to(dev) for _ in range(2))
    w = torch.tensor(rng.standard_normal((shape[0],) + shape[1 + len(axes):] + (len(axes),)).astype(np.float32)).to(dev)
    x = first.clone()

    def step():
        xin = x.detach().requires_grad_(True)                              # a leaf of this step's own stream
        y = ne.utils.barycenter(xin, axes=axes, normalize=True, shift_center=True)
        gx, = torch.autograd.grad((y * w).sum(), xin)
        return y.detach(), gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                             # workspace growth: outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y_g, gx_g = step()
    for values in (second, first, second):
        x.copy_(values)
        g.replay()
        torch.cuda.synchronize()
        got = (_bits(y_g), _bits(gx_g))
        y_e, gx_e = step()
        torch.cuda.synchronize()
        assert np.array_equal(got[0], _bits(y_e)) and np.array_equal(got[1], _bits(gx_e))
