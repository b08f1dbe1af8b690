"""
CPU tests of the bfloat16 inference path (no kernel is launched): the bf16 C entry points are declared, typed and exported,
they validate their arguments, bf16 models refuse what they do not run before touching a device, and the end-to-end check of
tests/test_gpu_unet_bf16.py rejects a network whose reference lost one tap of one layer.
"""

import numpy as np
import pytest
import torch

import neurite_amd as ne
from neurite_amd import _lib
from oracle import unet_oracle as uo

BF16_ENTRY_POINTS = ['nrt_conv3d_packed_weight_bytes_bf16', 'nrt_conv3d_pack_weights_bf16', 'nrt_conv3d_bf16',
                     'nrt_conv1x1_softmax_bf16', 'nrt_softmax_lastdim_bf16', 'nrt_maxpool3d_bf16', 'nrt_upsample_concat_bf16',
                     'nrt_add_act_affine_bf16']


def test_bf16_entry_points_declared_typed_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in BF16_ENTRY_POINTS:
        assert name in declared, '%s is not declared in include/neurite_amd.h' % name
        assert name in _lib._SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'libneurite_amd.so does not export %s' % name


def test_bf16_entry_points_validate_arguments():
    lib = _lib.lib()
    k3, s = _lib.ints([3, 3, 3]), _lib.ints([4, 4, 4])
    # K = 27 taps x 1 channel fits ONE k-step of 32: 1 step x 1 output block x 64 lanes x 8 bf16
    assert lib.nrt_conv3d_packed_weight_bytes_bf16(k3, 1, 16) == 1024
    # Cin >= 8: [8-channel group][27 taps padded to 28]: 2 groups x 7 steps x 2 output blocks
    assert lib.nrt_conv3d_packed_weight_bytes_bf16(k3, 16, 32) == 2 * 7 * 2 * 1024
    assert lib.nrt_conv3d_packed_weight_bytes_bf16(k3, 0, 16) == 0
    assert lib.nrt_conv3d_pack_weights_bf16(None, _lib.DT_BF16, k3, 4, 4, None, None) == -1
    dummy = 16
    assert lib.nrt_conv3d_pack_weights_bf16(dummy, _lib.DT_F16, k3, 4, 4, dummy, None) == -2
    assert lib.nrt_conv3d_bf16(None, 4, None, 0, None, None, None, None, 1, s, k3, 8, 1, 1, 0, None) == -1
    # activations beyond none / elu / relu are not fused into the epilogue
    assert lib.nrt_conv3d_bf16(dummy, 4, None, 0, None, dummy, None, dummy, 1, s, k3, 8, 1, 1, 3, None) == -1
    assert lib.nrt_conv1x1_softmax_bf16(dummy, dummy, None, dummy, 8, 16, 65, 1, 0, None) == -2
    assert lib.nrt_softmax_lastdim_bf16(None, None, 4, 4, None) == -1
    assert lib.nrt_maxpool3d_bf16(None, None, 1, s, 4, s, 1, None) == -1
    assert lib.nrt_upsample_concat_bf16(None, 0, None, 4, None, 1, s, s, None) == -1
    assert lib.nrt_add_act_affine_bf16(dummy, None, None, None, dummy, 8, 4, 0x100, None) == -1


def _unet(dtype):
    return ne.models.unet(4, (8, 8, 8, 1), 2, 3, 3).to(dtype)


def test_bf16_model_refusals_come_before_any_device_use():
    x = torch.zeros(1, 8, 8, 8, 1)                          # a CPU tensor: reaching the device check would raise NeuriteAmdError
    m = _unet(torch.bfloat16).train()
    with pytest.raises(NotImplementedError, match='inference'):
        m(x)
    with pytest.raises(NotImplementedError, match='unet_conv_downarm_0_0'):
        _unet(torch.float16).eval()(x)
    with pytest.raises(NotImplementedError, match='unet_conv_downarm_0_0'):
        _unet(torch.float64).eval()(x)
    mixed = _unet(torch.bfloat16).eval()
    mixed.get_layer('unet_conv_uparm_2_0').float()
    with pytest.raises(NotImplementedError, match='unet_conv_uparm_2_0'):
        mixed(x)
    # a float32 model still reaches the device check (behaviour unchanged)
    with pytest.raises(ne.errors.NeuriteAmdError):
        _unet(torch.float32).eval()(x)


def test_bf16_weight_cache_is_dropped_like_the_float32_one():
    m = _unet(torch.bfloat16)
    c = m.get_layer('unet_conv_downarm_0_0')
    stale = torch.zeros(1)

    def plant():
        c._packs['bf16'] = (c._kernel_key(c.kernel.dtype), stale)

    plant()
    m.eval()
    assert 'bf16' not in c._packs
    plant()
    m.load_state_dict(m.state_dict())
    assert 'bf16' not in c._packs
    plant()
    m.set_weights([np.zeros(tuple(t.shape), np.float32) for _, t, _ in m._weight_tensors()])
    assert 'bf16' not in c._packs
    plant()                                                 # a dtype change moves the key: the entry is rebuilt, not served
    assert c._pack('bf16', c._kernel_key(c.kernel.dtype), lambda: 'fresh') is stale
    m.float()
    assert c._pack('bf16', c._kernel_key(c.kernel.dtype), lambda: 'fresh') == 'fresh'


def test_end_to_end_check_rejects_a_dropped_tap():
    """the end-to-end criterion of the GPU tests separates bf16 rounding from a wrong network: a bf16-rounded copy of the float64
    reference passes, the same copy against the reference of a network with one tap of one convolution removed fails"""
    import test_gpu_unet_bf16 as tb
    rng = np.random.default_rng(0)
    model = ne.models.unet(8, (16, 16, 16, 1), 2, 3, 4, feat_mult=2)
    tb._randomise(model, rng)
    model = model.to(torch.bfloat16)
    weights, _ = tb.bf16_params(model)
    x = tb.bfr(rng.standard_normal((16, 16, 16, 1)))
    ref = uo.unet_forward(x, weights, 2, 1)
    got = tb.bfr(ref)                                       # within rounding of the true network
    tb.check_e2e(got, ref)
    dropped = dict(weights)
    k, b = dropped['unet_conv_uparm_2_0']
    k = k.copy()
    k[1, 1, 2] = 0.0                                        # one tap of the last decoder convolution
    dropped['unet_conv_uparm_2_0'] = (k, b)
    ref_bad = uo.unet_forward(x, dropped, 2, 1)
    with pytest.raises(AssertionError):
        tb.check_e2e(got, ref_bad)
