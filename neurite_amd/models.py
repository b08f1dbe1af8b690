"""
neurite_amd.models -- neurite's U-Net builders on MI355X.

unet      neurite/tf/models.py:88-246
conv_enc  neurite/tf/models.py:1309-1442
conv_dec  neurite/tf/models.py:1445-1617
conv_block: alias of conv_enc (the name BASELINE.json uses for the conv stacks; not in the reference tree)

Same arguments, defaults, layer names ('{prefix}_conv_downarm_{level}_{conv}', '{prefix}_maxpool_{level}',
'{prefix}_up_{n}', '{prefix}_merge_{n}', '{prefix}_conv_uparm_{n}_{conv}', '{prefix}_likelihood',
'{prefix}_prediction' ...) and graph as the Keras builders; the returned object is a torch.nn.Module whose
parameters keep the Keras layouts (Conv kernel [k.., Cin, Cout], bias [Cout]) so trained Keras weights map
one to one.  Forward runs on the HIP kernels of csrc/conv.hip: Conv3D = MFMA implicit GEMM (fp32), with
UpSampling3D + concatenate fused into the following convolution's loader and the final 1x1 conv fused
with the channel softmax.  1-D / 2-D nets are lifted to 3-D with unit leading dimensions.

One interpreter, `ConvNet._interpret`, walks the op list in three modes that differ only in the primitives it is handed:
  float32 inference (eval mode or grad disabled): Dropout is the identity, BatchNormalization uses its moving statistics; with
               `fold_head` the first layer's max-pooling, the last decoder convolution and the soft-max head fold into their neighbours
  float32 training (`model.train()` with grad enabled): every op is recorded through the autograd functions below (csrc/conv_bwd.hip),
               Dropout draws, BatchNormalization uses and updates the batch statistics
  bfloat16 inference: the same glue wrappers, which pick the *_bf16 entry points from the tensor's dtype

bfloat16 inference (csrc/conv_bf16.hip): a ConvNet whose parameters and buffers are all torch.bfloat16 (`net.bfloat16()`,
`net.to(dev, torch.bfloat16)`), in eval mode or with grad disabled, runs on bf16 kernels end to end with the semantics of
Keras' mixed_bfloat16 compute on bf16 variables.  The input op casts the input to bf16; every tensor between kernels, the
output and every tensor of `return_tensors` are bf16.  Rounding points -- each kernel computes in float32 from the stored bf16
values and rounds its result to bf16 once (round-to-nearest-even):
  Conv3D       exact bf16 products, float32 accumulation (v_mfma_f32_16x16x32_bf16), bias and ELU / ReLU in float32, one rounding;
               other activations and a softmax activation run as a pass of their own over the rounded output (a second rounding)
  MaxPooling3D, UpSampling3D, concatenate: exact
  add, Activation, inference BatchNorm (scale and shift formed in float32 from the bf16 parameters), the prior heads: float32, one
               rounding
  likelihood + softmax: float32 logits, float32 softmax, one rounding (fused unless the logits are materialised); a stand-alone
               softmax reads the bf16 logits
Limits: inference only (a bf16 model asked to record a training graph raises NotImplementedError); float16 / float64 parameters
and mixed dtypes raise NotImplementedError; `conv_variant` is ignored; `fold_head = False` materialises every layer; the
float32 folds (pooling, up-sampled decoder half, head) have no bf16 form -- only the up-sample + concatenate in the convolution's
loader and the 1x1 + softmax head are fused.  A float32 model is unchanged for any input dtype.
"""

import functools
import inspect
import json
import math
import sys
import types
import warnings

import numpy as np
import torch
from torch import nn

from . import _lib
from . import layers
from . import utils

__all__ = ['unet', 'conv_enc', 'conv_dec', 'conv_block', 'ConvNet', 'labels_to_image', 'labels_to_image_new', 'SynthStrip', 'add_prior', 'dilation_net', 'load', 'load_config', 'ae', 'single_ae', 'design_dnn', 'EncoderNet']

# element-wise activations, codes of include/neurite_amd.h (nrt_activation); definitions follow tf.keras.activations -- the reference
# hands the string straight to Keras (neurite/tf/models.py:1346, 1429, 1507, 1588)
_ACTS = {None: 0, 'linear': 0, 'elu': 1, 'relu': 2, 'sigmoid': 3, 'tanh': 4, 'softplus': 5, 'softsign': 6, 'selu': 7,
         'exponential': 8, 'hard_sigmoid': 9, 'leaky_relu': 10}  # stand-alone Activation layers (nrt_add_act_affine_*) take the same set
_ACT_MUL_B = 0x100
_ACT_LAST_FUSED = 2          # elu, relu are fused into the conv / LocallyConnected3D epilogues; the others run as an element-wise pass


def _act_code(activation):
    if activation not in _ACTS:
        raise NotImplementedError('activation %r is not implemented by the HIP path (%s are; softmax as a layer activation runs as '
                                  'its own kernel)' % (activation, ', '.join(sorted(str(k) for k in _ACTS))))
    return _ACTS[activation]


def _p32(t):
    """device pointer for a float32 entry point (*_f32): any other dtype is refused -- a bf16 buffer read as float32 would be
    read past its end"""
    if t is not None and t.dtype != torch.float32:
        raise NotImplementedError('a %s tensor cannot go to a float32 kernel (bf16 models run on their own kernels: all '
                                  'parameters bf16, inference)' % t.dtype)
    return _lib.ptr(t)


def _pbf(t):
    """device pointer for a bf16 entry point (*_bf16)"""
    if t is not None and t.dtype != torch.bfloat16:
        raise NotImplementedError('the bf16 kernels take bfloat16 tensors, got %s' % t.dtype)
    return _lib.ptr(t)


# the glue kernels exist once per compute dtype: entry-point suffix and the pointer check of that dtype's tensors
_BY_DTYPE = {torch.float32: ('_f32', _p32), torch.bfloat16: ('_bf16', _pbf)}


def _glue(stem, t):
    """(entry point's name, pointer check) of the glue kernel `stem` for the dtype of tensor `t`; outputs take t's dtype"""
    if t.dtype not in _BY_DTYPE:
        _p32(t)                                   # raises: no kernel family takes this dtype
    suffix, p = _BY_DTYPE[t.dtype]
    return stem + suffix, p


def _triple(v, ndims, what):
    if isinstance(v, (int, np.integer)):
        v = (int(v),) * ndims
    v = tuple(int(x) for x in v)
    if len(v) != ndims:
        raise ValueError('%s must have %d entries, got %r' % (what, ndims, v))
    return (1,) * (3 - ndims) + v


def _lift(x, ndims):
    """[B, *S, C] with len(S) = ndims -> [B, 1.., *S, C] (3 spatial dims)."""
    for _ in range(3 - ndims):
        x = x.unsqueeze(1)
    return x.contiguous()


def _unlift(x, ndims):
    for _ in range(3 - ndims):
        x = x.squeeze(1)
    return x


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    if isinstance(v, tuple):
        return [_jsonable(x) for x in v]
    if isinstance(v, list):
        return [_jsonable(x) for x in v]
    return v


def _store_config(func):
    """
    The builders' counterpart of modelio.store_config_args (neurite/tf/modelio.py:8-45): every argument the network was
    built with (defaults, positionals, keywords) is kept on the returned model as `model.config`, so that
    `model.save(path)` / `models.load(path)` rebuild the same architecture without the caller restating it
    (LoadableModel, modelio.py:78-143).  Graph-valued arguments (input_model, convL, src ...) are not recorded.
    """
    sig = inspect.signature(func)

    @functools.wraps(func)
    def wrapper(*args, **kwargs):
        net = func(*args, **kwargs)
        if isinstance(net, tuple):                     # ae(single_model=False): three models, each with the config of its own builder
            return net
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        params = {}
        loadable = True
        for k, v in bound.arguments.items():
            if k in ('convL', 'src', 'src_input', 'input_model'):
                loadable = loadable and v is None
                continue
            if k == 'enc_lambda_layers':               # callables do not travel in a config
                loadable = loadable and not v
                params[k] = None
                continue
            params[k] = _jsonable(v)
        params['metadata'] = {}
        net.config = {'builder': func.__name__, 'params': params, 'loadable': loadable}
        return net
    return wrapper


def _h5py():
    """h5py where the interpreter has it, else the package's own reader / writer of the same calls (neurite_amd/h5lite.py:
    the HDF5 subset Keras files use, checked against files the HDF5 library wrote -- tests/test_h5lite.py)"""
    try:
        import h5py
        return h5py
    except ImportError:
        from . import h5lite
        return h5lite


def _h5_attr(group, name):
    """Keras splits attributes that would not fit an object header (64512 bytes) into name0, name1, ... (hdf5_format.py:
    save_attributes_to_hdf5_group / load_attributes_from_hdf5_group): read either form"""
    if name in group.attrs:
        return list(group.attrs[name])
    out, k = [], 0
    while '%s%d' % (name, k) in group.attrs:
        out.extend(group.attrs['%s%d' % (name, k)])
        k += 1
    if not k:
        raise KeyError('no attribute %r in %s' % (name, getattr(group, 'name', group)))
    return out


def _h5_set_attr(group, name, data):
    """a list of byte strings as Keras stores it: one attribute, or name0, name1, ... when it would exceed an object header"""
    arr = np.asarray(data)
    chunks, n = [arr], 1
    while any(c.nbytes > 64512 for c in chunks):
        n += 1
        chunks = np.array_split(arr, n)
    if n == 1:
        group.attrs[name] = data
    else:
        for k, c in enumerate(chunks):
            group.attrs['%s%d' % (name, k)] = c


def _is_h5(path):
    return str(path).lower().endswith(('.h5', '.hdf5', '.keras.h5'))


def _h5_str(v):
    return v.decode('utf-8') if isinstance(v, bytes) else str(v)


class _Conv(nn.Module):
    """Keras Conv{N}D (channels-last, stride 1): kernel [k1..kN, Cin, Cout], glorot_uniform; bias zeros."""

    def __init__(self, name, cin, cout, ksize3, dilation=1, padding='same', activation=None):
        super().__init__()
        self.layer_name = name
        self.cin, self.cout = int(cin), int(cout)
        self.ksize3 = tuple(ksize3)
        self.dilation = int(dilation)
        if padding not in ('same', 'valid'):
            raise ValueError('padding must be same or valid')
        self.padding = padding
        self.activation = activation
        # the channel softmax is not element-wise: a linear epilogue, then the softmax kernel
        self.post_softmax = activation == 'softmax'
        self.act = 0 if self.post_softmax else _act_code(activation)
        k = self.ksize3
        fan = k[0] * k[1] * k[2]
        limit = math.sqrt(6.0 / (fan * self.cin + fan * self.cout))
        self.kernel = nn.Parameter((torch.rand(*k, self.cin, self.cout) * 2 - 1) * limit)
        self.bias = nn.Parameter(torch.zeros(self.cout))
        self._packs = {}                             # {slot: (key, tensor)} of the kernel-ready weight copies, see _pack
        self.fold_backward = True                    # decoder form: differentiate the up-sampled channels on the low-resolution grid
        self.max_norm = None                         # Keras kernel_constraint=MaxNorm(max_norm, axis=0); ConvNet.apply_constraints

    def invalidate_packed(self):
        """forget the MFMA-packed copy of the kernel.  The cache key below sees in-place writes through the Parameter
        (`_version`), a new storage and a device move; writes through `.data` (EMA / weight averaging: `p.data.mul_()`)
        bump no version, so the copy is also dropped on every `train()` / `eval()` switch, `set_weights`, `load_weights` and
        `load_state_dict`, and it is never used while the model is in training mode."""
        self._packs.clear()

    def train(self, mode=True):
        self.invalidate_packed()
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_packed()
        return super()._load_from_state_dict(*args, **kwargs)

    def _pack(self, slot, key, build, while_training=False):
        """the tensor cached in `slot` if it was built for `key`, else `build()`, cached under `key`.  The copies derived from this
        layer's kernel are never served in training mode (training loops may write through .data between steps)."""
        if self.training and not while_training:
            self._packs.pop(slot, None)
        hit = self._packs.get(slot)
        if hit is None or hit[0] != key:
            hit = self._packs[slot] = (key, build())
        return hit[1]

    def _kernel_key(self, *more):
        return (self.kernel._version, self.kernel.data_ptr(), self.kernel.device) + more

    def _packed_weights(self):
        def build():
            lib = _lib.lib()
            dev = self.kernel.device
            n = lib.nrt_conv3d_packed_weight_floats(_lib.ints(self.ksize3), self.cin, self.cout)
            packed = torch.empty(int(n), dtype=torch.float32, device=dev)
            _lib.call(dev, 'nrt_conv3d_pack_weights_f32', _p32(self.kernel.detach().contiguous()), _lib.ints(self.ksize3), self.cin,
                      self.cout, _p32(packed))
            return packed
        return self._pack('packed', self._kernel_key(), build)

    def _packed_weights_up2(self, c0):
        """the kernel folded for nrt_conv3d_up2_f32: skip channels [0, c0) keep their 27 taps, the up-sampled channels
        get 8 parity classes x 8 taps of pre-summed weights"""
        def build():
            lib = _lib.lib()
            dev = self.kernel.device
            n = lib.nrt_conv3d_up2_packed_weight_floats(int(c0), self.cin - int(c0), self.cout)
            packed = torch.empty(int(n), dtype=torch.float32, device=dev)
            _lib.call(dev, 'nrt_conv3d_up2_pack_weights_f32', _p32(self.kernel.detach().contiguous()), int(c0), self.cin - int(c0),
                      self.cout, _p32(packed))
            return packed
        return self._pack('up2', self._kernel_key(int(c0)), build)

    def forward(self, x, lo=None, up=None, variant=0):
        """x [B, X, Y, Z, c0]; optional lo [B, X/up, Y/up, Z/up, c1] is nearest-upsampled and concatenated after x.
        bf16 parameters: the bf16 kernels (inference; `variant` is ignored)."""
        if self.kernel.dtype == torch.bfloat16:
            if torch.is_grad_enabled() and (x.requires_grad or (lo is not None and lo.requires_grad)
                                            or self.kernel.requires_grad or self.bias.requires_grad):
                raise NotImplementedError('%s: bf16 convolutions run inference only (call under torch.no_grad())' % self.layer_name)
            return self.run_bf16(x, lo, up)
        if torch.is_grad_enabled() and (x.requires_grad or (lo is not None and lo.requires_grad)
                                        or self.kernel.requires_grad or self.bias.requires_grad):
            y = _ConvFn.apply(x, lo, self.kernel, self.bias, self, up, variant, False)
        else:
            y = self._run(x, lo, up, variant)
        if self.post_softmax:
            return _softmax_with_grad(y) if (torch.is_grad_enabled() and y.requires_grad) else _softmax(y)
        return y

    def pool_foldable(self, x, variant):
        """a 3x3x3 'same' encoder convolution whose 2x2x2 max-pooling can come out of the same kernel: the single-channel first layer
        (csrc/conv.hip: conv3d_c1_mfma<NT, true>) and, round 6, layers over 16 k input channels with 32 .. 64 filters in the persistent
        schedule (csrc/conv_p27.h: conv3d_p27_mfma<NT, true>)"""
        if self.ksize3 != (3, 3, 3) or self.dilation != 1 or x.shape[-1] != self.cin:
            return False
        if self.padding != 'same' or self.act > _ACT_LAST_FUSED or self.post_softmax or x.dtype != torch.float32:
            return False
        if self.cin == 1:
            return variant in (0, 1) and _lib.lib().nrt_conv3d_c1_pool_supported(_lib.ints(list(x.shape[1:4])), self.cout) == 1
        return variant in (0, 5) and _lib.lib().nrt_conv3d_pool_supported(self.cin, self.cout, _lib.ints(list(x.shape[1:4])), int(x.shape[0])) == 1

    def run_with_pool(self, x):
        """(act(conv(x)), MaxPooling3D(2) of it) from one kernel (nrt_conv3d_c1_pool_f32 / nrt_conv3d_pool_f32).  Inference only."""
        dev = _lib.require_device(x, self.kernel)
        x = x.contiguous()
        B, S = x.shape[0], list(x.shape[1:4])
        out = torch.empty([B] + S + [self.cout], dtype=torch.float32, device=dev)
        pooled = torch.empty([B] + [v // 2 for v in S] + [self.cout], dtype=torch.float32, device=dev)
        if self.cin == 1:
            _lib.call(dev, 'nrt_conv3d_c1_pool_f32', _p32(x), _p32(self.kernel.detach().contiguous()), _p32(self.bias.detach()),
                      _p32(out), _p32(pooled), B, _lib.ints(S), self.cout, self.act)
        else:
            _lib.call(dev, 'nrt_conv3d_pool_f32', _p32(x), self.cin, _p32(self._packed_weights()), _p32(self.bias.detach()),
                      _p32(out), _p32(pooled), B, _lib.ints(S), self.cout, self.act)
        return out, pooled

    def _packed_head(self, head_kernel, labels, dev):
        """the head's kernel in matrix-core fragment order, repacked when the parameter changes (version counter)"""
        def build():
            src = head_kernel.detach().reshape(-1, labels).contiguous()
            packed = torch.empty(16 * labels, dtype=torch.float32, device=dev)
            _lib.call(dev, 'nrt_conv3d_up2_head_pack_f32', _p32(src), labels, _p32(packed))
            return packed
        # keyed by the head's kernel, not this layer's: served in any mode (run_with_head is inference only)
        return self._pack('head', (head_kernel.data_ptr(), head_kernel._version, str(dev)), build, while_training=True)

    def run_with_head(self, x, lo, head_kernel, head_bias):
        """softmax(act(this decoder convolution) @ head_kernel + head_bias) in one kernel (nrt_conv3d_up2_head_f32); the caller has
        checked ConvNet._head_foldable.  Inference only."""
        dev = _lib.require_device(x, lo, self.kernel)
        x, lo = x.contiguous(), lo.contiguous()
        c0, c1 = x.shape[-1], lo.shape[-1]
        B, S = x.shape[0], list(x.shape[1:4])
        labels = head_kernel.shape[-1]
        out = torch.empty([B] + S + [labels], dtype=torch.float32, device=dev)
        hw = self._packed_head(head_kernel, labels, dev)
        _lib.call(dev, 'nrt_conv3d_up2_head_f32', _p32(x), c0, _p32(lo), c1, _p32(self._packed_weights_up2(c0)), _p32(self.bias.detach()),
                  _p32(hw), _p32(head_bias.detach()), labels, _p32(out), B, _lib.ints(S), self.cout, self.act)
        return out

    def _packed_weights_bf16(self):
        """the bf16 kernel in the A-operand order of v_mfma_f32_16x16x32_bf16 (nrt_conv3d_pack_weights_bf16); keyed and dropped
        like the 'packed' slot (_pack, invalidate_packed), plus the dtype"""
        def build():
            lib = _lib.lib()
            dev = self.kernel.device
            n = lib.nrt_conv3d_packed_weight_bytes_bf16(_lib.ints(self.ksize3), self.cin, self.cout)
            packed = torch.empty(int(n) // 2, dtype=torch.bfloat16, device=dev)
            _lib.call(dev, 'nrt_conv3d_pack_weights_bf16', _pbf(self.kernel.detach().contiguous()), _lib.DT_BF16, _lib.ints(self.ksize3),
                      self.cin, self.cout, _lib.ptr(packed))
            return packed
        return self._pack('bf16', self._kernel_key(self.kernel.dtype), build)

    def _geometry(self, x, lo, up):
        """what _run and run_bf16 check before they launch: (x, lo) contiguous, their channel counts c0, c1, batch B, input size S
        and output size O"""
        x = x.contiguous()
        c0 = x.shape[-1]
        c1 = 0 if lo is None else lo.shape[-1]
        if c0 + c1 != self.cin:
            raise ValueError('%s expects %d input channels, got %d' % (self.layer_name, self.cin, c0 + c1))
        B, S = x.shape[0], list(x.shape[1:4])
        if lo is not None:
            lo = lo.contiguous()
            if [S[d] // up[d] for d in range(3)] != list(lo.shape[1:4]) or any(S[d] % up[d] for d in range(3)):
                raise ValueError('%s: skip %s and up-sampled %s x %s shapes do not match'
                                 % (self.layer_name, S, list(lo.shape[1:4]), up))
        O = S if self.padding == 'same' else [S[d] - (self.ksize3[d] - 1) * self.dilation for d in range(3)]
        return x, lo, c0, c1, B, S, O

    def run_bf16(self, x, lo=None, up=None):
        """act(conv(concat(x, upsample(lo)))) on bf16 tensors (nrt_conv3d_bf16): exact products, float32 accumulation, bias and
        ELU / ReLU in float32, one rounding; any other activation as a pass of its own, a softmax activation as its own kernel"""
        dev = _lib.require_device(x, lo, self.kernel)
        x, lo, c0, c1, B, S, O = self._geometry(x, lo, up)
        out = torch.empty([B] + O + [self.cout], dtype=torch.bfloat16, device=dev)
        bias = self.bias.detach().to(torch.float32).contiguous()          # exact: every bf16 value is a float32
        _lib.call(dev, 'nrt_conv3d_bf16', _pbf(x), c0, _pbf(lo), c1, _lib.ints(up) if lo is not None else None,
                  _lib.ptr(self._packed_weights_bf16()), _lib.ptr(bias), _lib.ptr(out), B, _lib.ints(S), _lib.ints(self.ksize3), self.cout,
                  self.dilation, int(self.padding == 'same'), self.act if self.act <= _ACT_LAST_FUSED else 0)
        if self.act > _ACT_LAST_FUSED:
            out = _elementwise(out, act=self.act)
        if self.post_softmax:
            out = _softmax(out)
        return out

    def _run(self, x, lo=None, up=None, variant=0):
        dev = _lib.require_device(x, lo, self.kernel)
        if x.dtype != torch.float32:
            raise NotImplementedError('the HIP conv path is float32')
        x, lo, c0, c1, B, S, O = self._geometry(x, lo, up)
        out = torch.empty([B] + O + [self.cout], dtype=torch.float32, device=dev)
        w = self.kernel.detach().contiguous()
        # decoder form (UpSampling3D(2) + concatenate + 3x3x3 SAME): the up-sampled half runs as 8 folded taps on the
        # low-resolution grid (variant 0 = auto, 4 = required; 2 keeps the plain implicit GEMM over all 27 taps)
        # these are all the reasons nrt_conv3d_up2_f32 has to decline (NRT_ERR_UNSUPPORTED): anything outside them takes the plain GEMM
        folded = (variant in (0, 4) and lo is not None and tuple(up) == (2, 2, 2) and self.ksize3 == (3, 3, 3)
                  and self.dilation == 1 and self.padding == 'same'
                  and _lib.lib().nrt_conv3d_up2_supported(c0, c1, self.cout, _lib.ints(S)) == 1
                  # the folded kernel forms 32-bit output offsets over the whole batch (conv_up2.h launch_up2); the shape query
                  # does not see the batch, and nrt_conv3d_f32 has no such limit
                  and B * S[0] * S[1] * S[2] * self.cout < (1 << 30))
        if variant == 4 and not folded:
            raise NotImplementedError('%s: shapes outside the folded decoder kernel' % self.layer_name)
        if folded:
            _lib.call(dev, 'nrt_conv3d_up2_f32', _p32(x), c0, _p32(lo), c1, _p32(self._packed_weights_up2(c0)), _p32(self.bias.detach()),
                      _p32(out), B, _lib.ints(S), self.cout, self.act if self.act <= _ACT_LAST_FUSED else 0)
            if self.act > _ACT_LAST_FUSED:
                out = _elementwise(out, act=self.act)
            return out
        _lib.call(dev, 'nrt_conv3d_f32', _p32(x), c0, _p32(lo), c1, _lib.ints(up) if lo is not None else None, _p32(w),
                  _p32(self._packed_weights()), _p32(self.bias.detach()), _p32(out), B, _lib.ints(S), _lib.ints(self.ksize3), self.cout,
                  self.dilation, int(self.padding == 'same'), self.act if self.act <= _ACT_LAST_FUSED else 0, int(variant))
        if self.act > _ACT_LAST_FUSED:            # activations beyond elu / relu: an element-wise pass over the layer output
            out = _elementwise(out, act=self.act)
        return out


class _Dense(nn.Module):
    """Keras Dense: kernel [in, out] (glorot_uniform) exactly as a .h5 file stores it -- nrt_dense_f32 reads that layout, so there is no
    transposed or packed copy to invalidate -- and bias [out] (zeros)."""

    def __init__(self, name, cin, cout, activation=None):
        super().__init__()
        self.layer_name = name
        self.cin, self.cout = int(cin), int(cout)
        self.activation = activation
        # the softmax is not element-wise: a linear Dense, then the softmax kernel over the units
        self.post_softmax = activation == 'softmax'
        self.act = 0 if self.post_softmax else _act_code(activation)
        limit = math.sqrt(6.0 / (self.cin + self.cout))
        self.kernel = nn.Parameter((torch.rand(self.cin, self.cout) * 2 - 1) * limit)
        self.bias = nn.Parameter(torch.zeros(self.cout))

    def forward(self, x, variant=0):
        y = _dense(x, self.kernel, self.bias, self.act, variant)
        if self.post_softmax:
            return _softmax_with_grad(y) if (torch.is_grad_enabled() and y.requires_grad) else _softmax(y)
        return y


class _LocalBiasWeight(nn.Module):
    """the one weight of layers.LocalBias (neurite/tf/layers.py:762-767): `kernel` of the shape of one batch entry, Keras' default
    RandomNormal (stddev 0.05)"""

    def __init__(self, name, shape):
        super().__init__()
        self.layer_name = name
        self.kernel = nn.Parameter(torch.empty(tuple(int(v) for v in shape)).normal_(0.0, 0.05))


def _dense_workspace(dev, batch, cin, cout, variant):
    n = _lib.lib().nrt_dense_workspace_bytes(batch, cin, cout, variant)
    return (_lib.workspace(dev, n), n) if n else (None, 0)


def _dense_run(x, kernel, bias, act, variant):
    dev = _lib.require_device(x, kernel, bias)
    x = x.contiguous()
    B, cin, cout = x.shape[0], kernel.shape[0], kernel.shape[1]
    if x.dim() != 2 or x.shape[1] != cin:
        raise ValueError('Dense: input of shape %s for a kernel %s' % (tuple(x.shape), tuple(kernel.shape)))
    y = torch.empty((B, cout), dtype=torch.float32, device=dev)
    ws, n = _dense_workspace(dev, B, cin, cout, variant)
    _lib.call(dev, 'nrt_dense_f32', _p32(x), _p32(kernel), _p32(bias), _p32(y), B, cin, cout, int(act), int(variant), _lib.ptr(ws), n)
    return y


class _DenseFn(torch.autograd.Function):
    """y = act(x @ kernel + bias) and its three gradients on csrc/dense.hip; the activation's backward is nrt_act_bwd_f32 on y"""

    @staticmethod
    def forward(ctx, x, kernel, bias, act, variant):
        with torch.no_grad():
            y = _dense_run(x, kernel, bias, act, variant)
        ctx.save_for_backward(x, kernel, y)
        ctx.cfg = (act, variant)
        return y

    @staticmethod
    def backward(ctx, g):
        x, kernel, y = ctx.saved_tensors
        act, variant = ctx.cfg
        dev = g.device
        d = _act_bwd(g, y, act)
        x = x.contiguous()
        B, cin, cout = x.shape[0], kernel.shape[0], kernel.shape[1]
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(kernel) if need_w else None
        gb = torch.empty(cout, dtype=torch.float32, device=dev) if need_b else None
        ws, n = _dense_workspace(dev, B, cin, cout, variant)
        _lib.call(dev, 'nrt_dense_bwd_f32', _p32(d), _p32(x), _p32(kernel), _p32(gx), _p32(gw), _p32(gb), B, cin, cout, int(variant),
                  _lib.ptr(ws), n)
        return gx, gw, gb, None, None


def _dense(x, kernel, bias, act=0, variant=0):
    if torch.is_grad_enabled() and (x.requires_grad or kernel.requires_grad or (bias is not None and bias.requires_grad)):
        return _DenseFn.apply(x, kernel, bias, act, variant)
    return _dense_run(x, kernel.detach(), None if bias is None else bias.detach(), act, variant)


class _BatchNorm(nn.Module):
    """Keras BatchNormalization (axis -1): gamma, beta, moving_mean, moving_variance, epsilon = 1e-3, momentum = 0.99.
    Inference uses the moving statistics; in training mode (`_BatchNormFn`) the batch statistics, and the moving ones are
    updated as moving * momentum + batch * (1 - momentum) with the biased batch variance."""

    def __init__(self, name, channels, epsilon=1e-3, momentum=0.99):
        super().__init__()
        self.layer_name = name
        self.epsilon = epsilon
        self.momentum = momentum
        self.gamma = nn.Parameter(torch.ones(channels))
        self.beta = nn.Parameter(torch.zeros(channels))
        self.register_buffer('moving_mean', torch.zeros(channels))
        self.register_buffer('moving_variance', torch.ones(channels))


# The glue layers, float32 or bf16 by the dtype of their first tensor (_glue; bf16 forms in csrc/conv_bf16.hip: float32 arithmetic
# from the bf16 operands, one rounding; pooling and up-sampling exact).  scale, shift and bias are float32 for both.
def _elementwise(a, b=None, scale=None, shift=None, act=0, mul=False):
    """act(a + b) * scale + shift, or with mul act(a) * b"""
    if mul:
        act = int(act) | _ACT_MUL_B
    dev = _lib.require_device(a, b)
    name, p = _glue('nrt_add_act_affine', a)
    a = a.contiguous()
    b = None if b is None else b.contiguous()
    y = torch.empty_like(a)
    _lib.call(dev, name, p(a), p(b), _p32(scale), _p32(shift), p(y), a.numel(), a.shape[-1], int(act))
    return y


def _global_max_workspace(dev, B, V, C):
    n = _lib.lib().nrt_global_max_workspace_bytes(B, V, C)
    if not n:
        raise NotImplementedError('global max of a [%d, %d, %d] tensor: the kernels index elements with 32 bits' % (B, V, C))
    return _lib.workspace(dev, n), n


class _GlobalMaxFn(torch.autograd.Function):
    """max over everything between the batch axis and the channels (per_channel: Keras GlobalMaxPooling{1,2,3}D, [B, *S, C] ->
    [B, C]) or over everything but the batch axis (design_dnn's flatten-then-max lambda, -> [B, 1]), with tf.reduce_max's gradient:
    the positions that attain the max share it (csrc/globalmax.hip)"""

    @staticmethod
    def forward(ctx, x, per_channel):
        dev = _lib.require_device(x)
        x = x.contiguous()
        B = x.shape[0]
        C = x.shape[-1] if per_channel else 1
        V = x.numel() // (B * C)
        y = torch.empty((B, C), dtype=torch.float32, device=dev)
        count = torch.empty((B, C), dtype=torch.int32, device=dev)
        ws, n = _global_max_workspace(dev, B, V, C)
        _lib.call(dev, 'nrt_global_max_f32', _p32(x), B, V, C, _p32(y), _lib.ptr(count), _lib.ptr(ws), n)
        ctx.save_for_backward(x, y, count)
        ctx.dims = (B, V, C)
        ctx.mark_non_differentiable(count)
        return y, count

    @staticmethod
    def backward(ctx, g, _gcount):
        x, y, count = ctx.saved_tensors
        B, V, C = ctx.dims
        dev = g.device
        g = g.contiguous()
        gx = torch.empty_like(x)
        ws, n = _global_max_workspace(dev, B, V, C)
        _lib.call(dev, 'nrt_global_max_bwd_f32', _p32(x), _p32(y), _lib.ptr(count), _p32(g), B, V, C, _p32(gx), _lib.ptr(ws), n)
        return gx, None


def _global_max(x, per_channel=True, return_count=False):
    if x.dtype != torch.float32:
        raise NotImplementedError('the global max kernels are float32')
    y, count = _GlobalMaxFn.apply(x, bool(per_channel))
    return (y, count) if return_count else y


class _ScaleFn(torch.autograd.Function):
    """y = x * factor (layers.RescaleValues, layers.Negate) on the element-wise kernel; the gradient is the same call"""

    @staticmethod
    def _apply(x, factor):
        C = x.shape[-1]
        scale = torch.full((C,), float(factor), dtype=torch.float32, device=x.device)
        shift = torch.zeros(C, dtype=torch.float32, device=x.device)
        return _elementwise(x, scale=scale, shift=shift)

    @staticmethod
    def forward(ctx, x, factor):
        ctx.factor = float(factor)
        with torch.no_grad():
            return _ScaleFn._apply(x, factor)

    @staticmethod
    def backward(ctx, g):
        return _ScaleFn._apply(g, ctx.factor), None


def _scale_values(x, factor):
    if x.dtype != torch.float32:
        raise NotImplementedError('the element-wise kernel behind RescaleValues / Negate is float32 here')
    if torch.is_grad_enabled() and x.requires_grad:
        return _ScaleFn.apply(x, factor)
    return _ScaleFn._apply(x, factor)


def _maxnorm(w, max_value, eps=1e-7):
    """Keras MaxNorm(max_value, axis=0) in place on a contiguous float32 weight tensor"""
    dev = _lib.require_device(w)
    if not w.is_contiguous():
        raise ValueError('a constrained weight must be contiguous')
    _lib.call(dev, 'nrt_maxnorm_f32', _p32(w), int(w.shape[0]), w.numel() // int(w.shape[0]), float(max_value), float(eps))


def _maxpool(x, pool3, padding):
    dev = _lib.require_device(x)
    name, p = _glue('nrt_maxpool3d', x)
    x = x.contiguous()
    B, S, C = x.shape[0], list(x.shape[1:4]), x.shape[-1]
    same = padding == 'same'
    O = [(S[d] + pool3[d] - 1) // pool3[d] if same else S[d] // pool3[d] for d in range(3)]
    y = torch.empty([B] + O + [C], dtype=x.dtype, device=dev)
    _lib.call(dev, name, p(x), p(y), B, _lib.ints(S), C, _lib.ints(pool3), int(same))
    return y


def _upsample_concat(skip, lo, up3):
    dev = _lib.require_device(skip, lo)
    name, p = _glue('nrt_upsample_concat', lo)
    lo = lo.contiguous()
    B, S1, c1 = lo.shape[0], list(lo.shape[1:4]), lo.shape[-1]
    S = [S1[d] * up3[d] for d in range(3)]
    c0 = 0 if skip is None else skip.shape[-1]
    if skip is not None:
        skip = skip.contiguous()
        if list(skip.shape[1:4]) != S:
            raise ValueError('concatenate: shapes %s and %s do not match' % (list(skip.shape[1:4]), S))
    y = torch.empty([B] + S + [c0 + c1], dtype=lo.dtype, device=dev)
    _lib.call(dev, name, p(skip), c0, p(lo), c1, p(y), B, _lib.ints(S), _lib.ints(up3))
    return y


def _conv1x1_softmax(x, kernel, bias, softmax, act=0):
    """a 1x1x1 convolution (the likelihood layer, cout <= 64) with the channel softmax optionally fused: float32 logits"""
    dev = _lib.require_device(x, kernel)
    name, p = _glue('nrt_conv1x1_softmax', x)
    x = x.contiguous()
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    y = torch.empty(list(x.shape[:-1]) + [cout], dtype=x.dtype, device=dev)
    w = kernel.detach().reshape(cin, cout).contiguous()
    b = bias.detach().to(torch.float32).contiguous()             # (itself for a float32 bias; exact: every bf16 value is a float32)
    fused = int(act) if int(act) <= _ACT_LAST_FUSED else 0       # elu / relu ride in the epilogue, the others as a pass of their own
    if softmax and fused != int(act):
        raise NotImplementedError('a 1x1x1 convolution with a non-fused activation followed by the channel softmax')
    _lib.call(dev, name, p(x), p(w), _p32(b), p(y), x.numel() // cin, cin, cout, int(softmax), fused)
    return y if fused == int(act) else _elementwise(y, act=int(act))


def _softmax(x):
    dev = _lib.require_device(x)
    name, p = _glue('nrt_softmax_lastdim', x)
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.call(dev, name, p(x), p(y), x.numel() // x.shape[-1], x.shape[-1])
    return y


# --------------------------------------------------------------------------------------
# autograd: the backward kernels of csrc/conv_bwd.hip behind torch.autograd.Function
# --------------------------------------------------------------------------------------

def _act_bwd(g, y, act):
    if act == 0:
        return g.contiguous()
    dev = g.device
    g = g.contiguous()
    d = torch.empty_like(g)
    _lib.call(dev, 'nrt_act_bwd_f32', _p32(g), _p32(y), int(act), _p32(d), g.numel())
    return d


def _upsample_sum(g, c_off, c, lo_shape, up3):
    """grad of nearest up-sampling: channels [c_off, c_off + c) of g [B, S, Cg] summed over up^3 blocks -> [B, S/up, c]."""
    dev = g.device
    g = g.contiguous()
    B = g.shape[0]
    d = torch.empty([B] + list(lo_shape) + [c], dtype=torch.float32, device=dev)
    _lib.call(dev, 'nrt_upsample_sum_f32', _p32(g), g.shape[-1], int(c_off), _p32(d), int(c), B, _lib.ints(lo_shape), _lib.ints(up3))
    return d


def _dgrad_pad_before(ksize3, dilation):
    """zero padding before of the transpose of a 'same' convolution: the forward pads p = (k - 1) * dilation // 2 before and
    (k - 1) * dilation - p after, so its transpose pads (k - 1) * dilation - p before.  Odd kernels: the same p; even kernels: one more."""
    return [(k - 1) * int(dilation) - ((k - 1) * int(dilation)) // 2 for k in ksize3]


def _conv_dgrad(dpre, wpart, ksize3, dilation, variant=0):
    """grad wrt the conv input: conv(dpre, weights flipped in space and transposed in the channel axes) on the forward kernel, padded
    as the transpose is (nrt_conv3d_pad_f32)."""
    lib = _lib.lib()
    dev = dpre.device
    cout, cpart = wpart.shape[-1], wpart.shape[-2]
    wt = wpart.flip(0, 1, 2).transpose(3, 4).contiguous()             # [k, k, k, cout, cpart]; a few KB of glue
    if variant == 6 and not (cout >= 8 and cpart <= 64):
        variant = 0                  # the transposed layer swaps the channel counts: outside the 2x2x2 arm's, it is not forced
    if tuple(ksize3) == (1, 1, 1) and cpart % 4 == 0 and cpart <= 64:
        # 1x1x1 (the likelihood layer): a per-voxel matrix product on the streaming kernel, not on the halo-tile convolution
        dpre = dpre.contiguous()
        out = torch.empty(list(dpre.shape[:-1]) + [cpart], dtype=torch.float32, device=dev)
        _lib.call(dev, 'nrt_conv1x1_softmax_f32', _p32(dpre), _p32(wt), None, _p32(out), dpre.numel() // cout, cout, cpart, 0, 0)
        return out
    n = lib.nrt_conv3d_packed_weight_floats(_lib.ints(ksize3), cout, cpart)
    packed = torch.empty(int(n), dtype=torch.float32, device=dev)
    B, S = dpre.shape[0], list(dpre.shape[1:4])
    out = torch.empty([B] + S + [cpart], dtype=torch.float32, device=dev)
    _lib.call(dev, 'nrt_conv3d_pack_weights_f32', _p32(wt), _lib.ints(ksize3), cout, cpart, _p32(packed))
    _lib.call(dev, 'nrt_conv3d_pad_f32', _p32(dpre), cout, None, 0, None, _p32(wt), _p32(packed), None, _p32(out), B, _lib.ints(S),
              _lib.ints(ksize3), cpart, int(dilation), _lib.ints(_dgrad_pad_before(ksize3, dilation)), 0, int(variant))
    return out


# ---- folded backward of a decoder convolution (UpSampling3D(2) + concatenate + Conv3D 3x3x3 'same') -------------------------
# Per axis, output parity p and low-resolution tap t cover the 3x3x3 taps d in S(p, t): S(0,0) = {0}, S(0,1) = {1,2},
# S(1,0) = {0,1}, S(1,1) = {2} (csrc/conv_up2.h).  _FOLD_A[p][t][d] is that membership; _FOLD_B[p][e][d] is the same
# seen from the low-resolution grid in the backward direction (3x3x3 tap e = 2 - p - t of the space-to-depth gradient).
_FOLD_A = ((( 1, 0, 0), (0, 1, 1)), ((1, 1, 0), (0, 0, 1)))
_FOLD_B = (((0, 0, 0), (0, 1, 1), (1, 0, 0)), ((0, 0, 1), (1, 1, 0), (0, 0, 0)))


_FOLD_ON_DEVICE = {}


def _fold_table(table, like):
    """_FOLD_A / _FOLD_B as a tensor on `like`'s device, uploaded once (a host->device copy per step would also keep the training
    step out of a hipGraph: copies from pageable memory are not capturable)"""
    key = (table is _FOLD_A, like.device, like.dtype)
    m = _FOLD_ON_DEVICE.get(key)
    if m is None:
        m = _FOLD_ON_DEVICE[key] = torch.tensor(table, dtype=like.dtype, device=like.device)
    return m


def _fold_dgrad_weights(k_lo):
    """kernel rows of the up-sampled channels [3,3,3,c1,cout] -> the 3x3x3 kernel [3,3,3, 8 * cout, c1] that maps the
    space-to-depth gradient (parity group P = (px*2 + py)*2 + pz, channels P*cout + co) to the gradient of the
    low-resolution tensor; only 2 x 2 x 2 taps per parity group are non-zero."""
    Bm = _fold_table(_FOLD_B, k_lo)
    c1, cout = k_lo.shape[3], k_lo.shape[4]
    return torch.einsum('xea,yfb,zgc,abcio->efgxyzoi', Bm, Bm, Bm, k_lo).reshape(3, 3, 3, 8 * cout, c1).contiguous()


def _unfold_wgrad(dwf):
    """folded weight gradient [8 parity groups, 8 taps, c1, cout] -> [3,3,3,c1,cout]"""
    Am = _fold_table(_FOLD_A, dwf)
    c1, cout = dwf.shape[2], dwf.shape[3]
    return torch.einsum('xta,yub,zvc,xyztuvio->abcio', Am, Am, Am, dwf.reshape(2, 2, 2, 2, 2, 2, c1, cout))


def _fold_backward_ok(mod, x, lo, up):
    return (lo is not None and tuple(up) == (2, 2, 2) and mod.ksize3 == (3, 3, 3) and mod.dilation == 1 and mod.padding == 'same'
            and x.shape[-1] % 16 == 0 and lo.shape[-1] % 16 == 0 and mod.cout % 16 == 0 and mod.cout <= 32 and lo.shape[-1] <= 64
            and all(s % 2 == 0 for s in x.shape[1:4]))


def _space_to_depth2(dpre):
    dev = dpre.device
    dpre = dpre.contiguous()
    B, S, C = dpre.shape[0], list(dpre.shape[1:4]), dpre.shape[-1]
    y = torch.empty([B] + [s // 2 for s in S] + [8 * C], dtype=torch.float32, device=dev)
    _lib.call(dev, 'nrt_space_to_depth2_f32', _p32(dpre), _p32(y), B, _lib.ints(S), C)
    return y


def _conv_dgrad_lo_folded(s2d, k_lo):
    """gradient of the low-resolution input: 2 x 2 x 2 taps per parity group of the space-to-depth gradient (replaces the 27-tap
    dgrad over the up-sampled channels at full resolution + the 2^3 block sum)"""
    lib = _lib.lib()
    dev = s2d.device
    c1, cout = k_lo.shape[3], k_lo.shape[4]
    wf = _fold_dgrad_weights(k_lo)
    k3 = (3, 3, 3)
    n = lib.nrt_conv3d_packed_weight_floats(_lib.ints(k3), 8 * cout, c1)
    packed = torch.empty(int(n), dtype=torch.float32, device=dev)
    B, S1 = s2d.shape[0], list(s2d.shape[1:4])
    out = torch.empty([B] + S1 + [c1], dtype=torch.float32, device=dev)
    _lib.call(dev, 'nrt_conv3d_pack_weights_f32', _p32(wf), _lib.ints(k3), 8 * cout, c1, _p32(packed))
    _lib.call(dev, 'nrt_conv3d_s2d_taps_f32', _p32(s2d), cout, _p32(packed), _p32(out), B, _lib.ints(S1), c1)
    return out


def _conv_wgrad_lo_folded(lo, s2d, cout):
    dev = lo.device
    lo = lo.contiguous()
    c1 = lo.shape[-1]
    dwf = torch.zeros(8, 8, c1, cout, dtype=torch.float32, device=dev)
    _lib.call(dev, 'nrt_conv3d_wgrad_s2d_f32', _p32(lo), _p32(s2d), _p32(dwf), lo.shape[0], _lib.ints(list(lo.shape[1:4])), c1, cout)
    return _unfold_wgrad(dwf)


class _ConvFn(torch.autograd.Function):
    """Conv3D (+ fused up-sample/concat loader, bias, activation) with dgrad / wgrad."""

    @staticmethod
    def forward(ctx, x, lo, kernel, bias, mod, up, variant, one_by_one):
        with torch.no_grad():
            if one_by_one:
                out = _conv1x1_softmax(x, kernel, bias, False, mod.act)
            else:
                out = mod._run(x, lo, up, variant)
        ctx.mod, ctx.up = mod, up
        ctx.dgrad_variant = 6 if variant == 6 else 0          # a forced 2x2x2 matrix-core arm is forced in the input gradient too
        ctx.save_for_backward(x, lo, kernel, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, lo, kernel, out = ctx.saved_tensors
        mod, up = ctx.mod, ctx.up
        dev = g.device
        dpre = _act_bwd(g, out, mod.act)
        if mod.padding != 'same':
            # A 'valid' convolution is the 'same' convolution restricted to the outputs whose window lies inside the volume
            # (output v = same-output v + pb, pb = ((k - 1) * dilation) // 2 as TF pads).  Its backward is therefore the
            # 'same' backward of the output gradient embedded in zeros at those positions (nrt_pad3d): the positions that
            # were never computed contribute nothing, and no window reads outside the input.
            S = list(x.shape[1:4])
            pb = [((mod.ksize3[d] - 1) * mod.dilation) // 2 for d in range(3)]
            padded = torch.empty([dpre.shape[0]] + S + [dpre.shape[-1]], dtype=dpre.dtype, device=dev)
            dpre = dpre.contiguous()
            _lib.call(dev, 'nrt_pad3d', _p32(dpre), _p32(padded), dpre.shape[0], _lib.ints(list(dpre.shape[1:4])), _lib.ints(pb),
                      _lib.ints(S), dpre.shape[-1] * 4, 0)
            dpre = padded
        need_x, need_lo, need_w, need_b = ctx.needs_input_grad[:4]
        dx = dlo = dw = db = None
        c0 = x.shape[-1]
        if mod.fold_backward and _fold_backward_ok(mod, x, lo, up):
            # decoder form: the up-sampled channels are differentiated on the low-resolution grid (8 parity groups x 2x2x2 taps of
            # the space-to-depth gradient: 0.30 of the matrix work of the 27-tap form), the skip channels as a plain convolution
            k5 = kernel.detach()
            s2d = _space_to_depth2(dpre) if (need_lo or need_w) else None
            if need_x:
                dx = _conv_dgrad(dpre, k5[..., :c0, :], mod.ksize3, 1)
            if need_lo:
                dlo = _conv_dgrad_lo_folded(s2d, k5[..., c0:, :])
            if need_w or need_b:
                dw = torch.empty_like(kernel, dtype=torch.float32)
                dws = torch.zeros(3, 3, 3, c0, mod.cout, dtype=torch.float32, device=dev)
                db = torch.zeros(mod.cout, dtype=torch.float32, device=dev)
                xs = x.contiguous()
                _lib.call(dev, 'nrt_conv3d_wgrad_f32', _p32(xs), _p32(dpre), _p32(dws), _p32(db), xs.shape[0],
                          _lib.ints(list(xs.shape[1:4])), c0, mod.cout, _lib.ints(mod.ksize3), 1)
                dw[..., :c0, :] = dws
                dw[..., c0:, :] = _conv_wgrad_lo_folded(lo, s2d, mod.cout)
            return dx, dlo, dw if need_w else None, db if need_b else None, None, None, None, None
        if need_w or need_b:
            dw = torch.zeros_like(kernel, dtype=torch.float32)
            db = torch.zeros(mod.cout, dtype=torch.float32, device=dev)
            xs = x.contiguous()
            lo_c = None if lo is None else lo.contiguous()
            if lo_c is not None and c0 % 4:
                xs, lo_c = _upsample_concat(xs, lo_c, up), None          # a channel quad would straddle the two sources
            B, S = xs.shape[0], list(xs.shape[1:4])
            _lib.call(dev, 'nrt_conv3d_wgrad2_f32', _p32(xs), xs.shape[-1], _p32(lo_c), 0 if lo_c is None else lo_c.shape[-1],
                      _lib.ints(up) if lo_c is not None else None, _p32(dpre), _p32(dw), _p32(db), B, _lib.ints(S), mod.cout,
                      _lib.ints(mod.ksize3), mod.dilation)
        k5 = kernel.detach()
        if lo is not None and need_x and need_lo and mod.cin <= 64:
            # one dgrad for both sources of the fused loader (dpre is staged once, three N-tiles per A fragment)
            full = _conv_dgrad(dpre, k5, mod.ksize3, mod.dilation, ctx.dgrad_variant)
            dx = full[..., :c0]
            dlo = _upsample_sum(full, c0, mod.cin - c0, list(lo.shape[1:4]), up)
        else:
            if need_x:
                dx = _conv_dgrad(dpre, k5[..., :c0, :], mod.ksize3, mod.dilation, ctx.dgrad_variant)
            if lo is not None and need_lo:
                full = _conv_dgrad(dpre, k5[..., c0:, :], mod.ksize3, mod.dilation, ctx.dgrad_variant)
                dlo = _upsample_sum(full, 0, full.shape[-1], list(lo.shape[1:4]), up)
        return dx, dlo, dw if need_w else None, db if need_b else None, None, None, None, None


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pool3, padding):
        with torch.no_grad():
            y = _maxpool(x, pool3, padding)
        ctx.save_for_backward(x)
        ctx.cfg = (tuple(pool3), padding)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        pool3, padding = ctx.cfg
        dev = g.device
        x = x.contiguous()
        g = g.contiguous()
        dx = torch.empty_like(x)
        _lib.call(dev, 'nrt_maxpool3d_bwd_f32', _p32(x), _p32(g), _p32(dx), x.shape[0], _lib.ints(list(x.shape[1:4])), x.shape[-1],
                  _lib.ints(pool3), int(padding == 'same'))
        return dx, None, None


class _MergeFn(torch.autograd.Function):
    """concatenate([skip, UpSampling3D(lo)]) (skip may be None: plain up-sampling)."""

    @staticmethod
    def forward(ctx, skip, lo, up3):
        with torch.no_grad():
            y = _upsample_concat(skip, lo, up3)
        ctx.cfg = (0 if skip is None else skip.shape[-1], lo.shape[-1], list(lo.shape[1:4]), tuple(up3))
        return y

    @staticmethod
    def backward(ctx, g):
        c0, c1, lo_shape, up3 = ctx.cfg
        dskip = g[..., :c0].contiguous() if c0 and ctx.needs_input_grad[0] else None
        dlo = _upsample_sum(g, c0, c1, lo_shape, up3) if ctx.needs_input_grad[1] else None
        return dskip, dlo, None


def _head_grads(x, kernel, mod, dz, needs):
    """(dx, dw, db) of the likelihood conv from dz = d loss / d logits; needs = which of the three are wanted"""
    dev = dz.device
    dx = dw = db = None
    if needs[1] or needs[2]:
        xin = x.contiguous()
        dw = torch.zeros_like(kernel, dtype=torch.float32)
        db = torch.zeros(mod.cout, dtype=torch.float32, device=dev)
        _lib.call(dev, 'nrt_conv3d_wgrad_f32', _p32(xin), _p32(dz), _p32(dw), _p32(db), xin.shape[0], _lib.ints(list(xin.shape[1:4])),
                  mod.cin, mod.cout, _lib.ints(mod.ksize3), 1)
    if needs[0]:
        dx = _conv_dgrad(dz, kernel.detach(), mod.ksize3, 1)
    return dx, dw, db


class SoftmaxSource:
    """
    Stamp (`y._nrt_softmax_src`) on a channel soft-max output that is still its producer's untouched result: `inputs` are the
    autograd inputs of the producer and `grads_from_dz(dz, needs)` turns d loss / d logits into their gradients.  A loss that can
    form dz itself (metrics._SegLossFn: Dice + CCE of the prediction) attaches to `inputs` directly, and the gradient wrt the
    probabilities -- with the separate soft-max backward pass over it -- is never materialised.
    """

    def __init__(self, y, inputs, grads_from_dz):
        self.inputs, self._grads_from_dz = tuple(inputs), grads_from_dz
        self.version = y._version
        # the closure keeps the producer's inputs alive outside save_for_backward: the in-place check autograd would do is done here
        self.input_versions = tuple(None if t is None else t._version for t in self.inputs)

    def valid_for(self, y):
        """The shortcut replaces y's own autograd node: it must not be taken when somebody observes the gradient AT y (a hook on the
        prediction, retain_grad) -- those would silently see nothing -- nor when y was modified since the producer wrote it."""
        if y._version != self.version or not torch.is_grad_enabled() or not y.requires_grad:
            return False
        if y.retains_grad or getattr(y, '_backward_hooks', None):
            return False
        return True

    def grads_from_dz(self, dz, needs):
        for t, v in zip(self.inputs, self.input_versions):
            if t is not None and t._version != v:
                raise RuntimeError('neurite_amd: an input of the soft-max head was modified in place after the forward pass; its '
                                   'gradient through the joint segmentation loss would be computed from the modified values')
        return self._grads_from_dz(dz, needs)


def _stamp_softmax(y, inputs, grads_from_dz):
    if torch.is_grad_enabled() and y.requires_grad:
        y._nrt_softmax_src = SoftmaxSource(y, inputs, grads_from_dz)
    return y


class _HeadFn(torch.autograd.Function):
    """likelihood 1x1 conv + channel softmax in one pass (no logits tensor); backward from the prediction alone."""

    @staticmethod
    def forward(ctx, x, kernel, bias, mod):
        with torch.no_grad():
            y = _conv1x1_softmax(x, kernel, bias, True, 0)
        ctx.mod = mod
        ctx.save_for_backward(x, kernel, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x, kernel, y = ctx.saved_tensors
        dev = g.device
        g = g.contiguous()
        dz = torch.empty_like(y)
        _lib.call(dev, 'nrt_softmax_bwd_f32', _p32(y), _p32(g), _p32(dz), y.numel() // y.shape[-1], y.shape[-1])
        return _head_grads(x, kernel, ctx.mod, dz, ctx.needs_input_grad) + (None,)


def _head(x, kernel, bias, mod):
    y = _HeadFn.apply(x, kernel, bias, mod)
    return _stamp_softmax(y, (x, kernel, bias), lambda dz, needs: _head_grads(x, kernel, mod, dz, needs))


def _softmax_with_grad(z):
    return _stamp_softmax(_SoftmaxFn.apply(z), (z,), lambda dz, needs: (dz,))


class _ChannelScaleFn(torch.autograd.Function):
    """y[b, ..., c] = x[b, ..., c] * scale[b, c]: Keras Dropout with noise_shape [None, 1, .., 1, C] (whole feature maps are
    dropped, models.py:1390-1399) once the mask is drawn; the backward is the same scaling of the gradient."""

    @staticmethod
    def _apply(x, scale):
        x = x.contiguous()
        y = torch.empty_like(x)
        dev = x.device
        zero = torch.zeros(x.shape[-1], dtype=torch.float32, device=dev)
        for b in range(x.shape[0]):
            _lib.call(dev, 'nrt_add_act_affine_f32', _p32(x[b]), None, _p32(scale[b]), _p32(zero), _p32(y[b]), x[b].numel(), x.shape[-1], 0)
        return y

    @staticmethod
    def forward(ctx, x, scale):
        ctx.save_for_backward(scale)
        with torch.no_grad():
            return _ChannelScaleFn._apply(x, scale)

    @staticmethod
    def backward(ctx, g):
        (scale,) = ctx.saved_tensors
        return _ChannelScaleFn._apply(g, scale), None


class _AddActFn(torch.autograd.Function):
    """y = act(a [+ b]): the residual merge (`KL.add`, models.py:1426) and the stand-alone Activation layers"""

    @staticmethod
    def forward(ctx, a, b, act):
        with torch.no_grad():
            y = _elementwise(a, b, act=act)
        ctx.act = act
        ctx.has_b = b is not None
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        d = _act_bwd(g, y, ctx.act)
        return d, (d if ctx.has_b else None), None


class _MulFn(torch.autograd.Function):
    """y = a * b (`KL.multiply` of the prior and the sigmoid likelihood, models.py:412-417)"""

    @staticmethod
    def forward(ctx, a, b):
        with torch.no_grad():
            y = _elementwise(a, b, mul=True)
        ctx.save_for_backward(a, b)
        return y

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = _elementwise(g, b, mul=True) if ctx.needs_input_grad[0] else None
        db = _elementwise(g, a, mul=True) if ctx.needs_input_grad[1] else None
        return da, db


def _channel_sums(a, b=None):
    dev = a.device
    C = a.shape[-1]
    out = torch.zeros(C, dtype=torch.float32, device=dev)
    _lib.call(dev, 'nrt_channel_sums_f32', _p32(a), _p32(b), a.numel() // C, C, _p32(out))
    return out


class _BatchNormFn(torch.autograd.Function):
    """training-mode BatchNormalization over all axes but the last; [C]-sized arithmetic is glue, volume passes are kernels"""

    @staticmethod
    def forward(ctx, x, gamma, beta, mod):
        with torch.no_grad():
            x = x.contiguous()
            C = x.shape[-1]
            n = x.numel() // C
            mean = _channel_sums(x) / n
            var = torch.clamp(_channel_sums(x, x) / n - mean * mean, min=0.0)
            inv = torch.rsqrt(var + mod.epsilon)
            scale = (gamma * inv).contiguous()
            shift = (beta - mean * scale).contiguous()
            y = _elementwise(x, scale=scale, shift=shift)
            mod.moving_mean.mul_(mod.momentum).add_(mean * (1 - mod.momentum))
            mod.moving_variance.mul_(mod.momentum).add_(var * (1 - mod.momentum))
        ctx.save_for_backward(x, gamma, mean, inv)
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, mean, inv = ctx.saved_tensors
        dev = g.device
        g = g.contiguous()
        C = x.shape[-1]
        n = x.numel() // C
        sg = _channel_sums(g)
        sgx = _channel_sums(g, x)
        sgxh = (sgx - mean * sg) * inv                         # sum g * xhat
        dgamma, dbeta = sgxh, sg
        dx = None
        if ctx.needs_input_grad[0]:
            scale = gamma * inv
            m1, m2 = sg / n, sgxh / n
            A = scale.contiguous()
            B = (-scale * inv * m2).contiguous()
            C0 = (-scale * m1 + scale * inv * m2 * mean).contiguous()
            dx = torch.empty_like(x)
            _lib.call(dev, 'nrt_channel_axpby_f32', _p32(g), _p32(x), _p32(A), _p32(B), _p32(C0), _p32(dx), x.numel(), C)
        return dx, dgamma, dbeta, None


class _SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        with torch.no_grad():
            y = _softmax(z)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        dev = g.device
        g = g.contiguous()
        dz = torch.empty_like(y)
        _lib.call(dev, 'nrt_softmax_bwd_f32', _p32(y), _p32(g), _p32(dz), y.numel() // y.shape[-1], y.shape[-1])
        return dz


# the op kinds of the auto-encoder bottleneck (single_ae); float32 only
_AE_KINDS = ('flatten', 'reshape', 'dense', 'resize', 'local_bias', 'sample', 'identity', 'lambda')
# the layers design_dnn / EncoderNet add: GlobalMaxPooling{1,2,3}D, the flatten-then-max lambda, layers.RescaleValues and the plain
# (element-wise) Dropout; float32 only, like the auto-encoder kinds
_CLS_KINDS = ('global_max', 'global_max_all', 'rescale', 'dropout_ew')


class _PendingConv:
    """inputs of a decoder convolution whose only consumer is the soft-max head: both run as one kernel at the head's op"""

    def __init__(self, x, lo):
        self.x, self.lo = x, lo


class ConvNet(nn.Module):
    """
    A built conv_enc / conv_dec / unet graph: an ordered list of named Keras-equivalent layers
    (`self.layer_names`, `self.get_layer(name)`) executed on the HIP kernels.
    """

    def __init__(self, name, ndims, input_shapes, ops, output, modules):
        super().__init__()
        self.name = name
        self.ndims = ndims
        self.input_shapes = input_shapes            # list of per-input shapes (without batch)
        self.ops = ops                              # list of dicts, executed in order
        self.output_name = output
        self.layers_by_name = nn.ModuleDict()
        for k, m in modules.items():
            self.layers_by_name[k] = m
        self.layer_names = [op['name'] for op in ops]
        self._flat = {op['name']: bool(op.get('flat')) for op in ops}      # layers whose Keras tensor is [B, E]
        self._keras_shape = {op['name']: tuple(op['keras_shape']) for op in ops if op.get('keras_shape')}   # any other rank
        self.last_dropout_masks = {}                # {element-wise Dropout layer: the mask / (1 - rate) of the last training forward}
        self.output_shape = ops[-1].get('shape') if ops else None
        self.conv_variant = 0                       # 0 auto, 1 direct, 2 MFMA, 6 the 2x2x2 MFMA arm (tests / tuning); float32 only, bf16 ignores it
        self.fold_head = True                       # inference: last decoder convolution + likelihood + soft-max as ONE kernel where it applies
        self.dense_variant = 0                      # 0 auto, 1 reduce arm, 2 expand arm of csrc/dense.hip (tests / tuning)
        self.last_draws = {}                        # {sampling layer: the N(0, 1) noise of the last forward}
        # {conv layer: the soft-max likelihood that is its ONLY consumer}: candidates for nrt_conv3d_up2_head_f32 (models.py:1545-1605)
        uses = {}
        for op in ops:
            for key in ('src', 'lo', 'skip', 'a', 'b'):
                v = op.get(key)
                for n in (v if isinstance(v, (list, tuple)) else [v]):
                    if isinstance(n, str):
                        uses.setdefault(n, []).append(op)
        # {single-channel first convolution: the 2x2x2 max-pooling that reads it}: candidates for nrt_conv3d_c1_pool_f32 (models.py:1378-1438)
        self._pool_of = {}
        for op in ops:
            if op['kind'] == 'maxpool' and tuple(op.get('pool', ())) == (2, 2, 2) and isinstance(op.get('src'), str):
                src = next((o for o in ops if o['name'] == op['src']), None)
                if src is not None and src['kind'] == 'conv' and not src.get('lo') and op['src'] not in self._pool_of:
                    self._pool_of[op['src']] = op['name']
        self._head_of = {}
        for op in ops:
            if op['kind'] == 'conv' and op.get('lo') and op['name'] != output:
                u = uses.get(op['name'], [])
                if len(u) == 1 and u[0]['kind'] == 'likelihood' and u[0].get('fuse_softmax') and u[0].get('src') == op['name']:
                    self._head_of[op['name']] = u[0]['name']
        self.eval()                                 # Keras predict semantics; model.train() records the graph for autograd

    def _head_foldable(self, conv_name, head_name, x, lo, up):
        """run-time half of the test: shapes and settings the folded kernel takes (csrc/conv_up2.h: up2_head_ok)"""
        c, h = self.layers_by_name[conv_name], self.layers_by_name[head_name]
        if lo is None or up is None or tuple(up) != (2, 2, 2) or self.conv_variant not in (0, 4):
            return False
        if c.ksize3 != (3, 3, 3) or c.dilation != 1 or c.padding != 'same' or c.act > _ACT_LAST_FUSED or c.post_softmax:
            return False
        if tuple(h.ksize3) != (1, 1, 1) or h.cin != c.cout:
            return False
        B, S = x.shape[0], list(x.shape[1:4])
        if B * S[0] * S[1] * S[2] * h.cout >= (1 << 30):
            return False
        return _lib.lib().nrt_conv3d_up2_head_supported(x.shape[-1], lo.shape[-1], c.cout, h.cout, _lib.ints(S)) == 1

    # ---- Keras Model weight API (modelio: neurite/tf/modelio.py:111-143 saves/loads `model.get_weights()` lists) ----
    def _weight_tensors(self):
        """weights in Keras order: layers in graph order; Conv and Dense: kernel, bias; BatchNormalization: gamma, beta, mean, variance;
        LocalBias: kernel"""
        out = []
        for name in self.layer_names:
            if name in self.layers_by_name:
                m = self.layers_by_name[name]
                if isinstance(m, _Conv):
                    out += [(name + '/kernel', m.kernel, getattr(m, 'keras_nd', self.ndims)), (name + '/bias', m.bias, None)]
                elif isinstance(m, _BatchNorm):
                    out += [(name + '/gamma', m.gamma, None), (name + '/beta', m.beta, None),
                            (name + '/moving_mean', m.moving_mean, None), (name + '/moving_variance', m.moving_variance, None)]
                elif isinstance(m, _Dense):
                    out += [(name + '/kernel', m.kernel, None), (name + '/bias', m.bias, None)]
                elif isinstance(m, _LocalBiasWeight):
                    out += [(name + '/kernel', m.kernel, None)]
        return out

    def get_weights(self):
        """list of numpy arrays in Keras `model.get_weights()` order and layout (Conv{N}D kernels [k1..kN, Cin, Cout])."""
        res = []
        for _, t, nd in self._weight_tensors():
            a = t.detach().cpu().numpy()
            if nd is not None and nd < 3:
                a = a.reshape(a.shape[3 - nd:])                  # drop the lifted singleton kernel dims
            res.append(a)
        return res

    def set_weights(self, weights):
        """counterpart of `get_weights` (e.g. the arrays of a Keras-trained neurite unet exported with np.savez)."""
        slots = self._weight_tensors()
        if len(weights) != len(slots):
            raise ValueError('You called `set_weights(weights)` on model "%s" with a weight list of length %d, but the '
                             'model was expecting %d weights.' % (self.name, len(weights), len(slots)))
        with torch.no_grad():
            for (name, t, nd), w in zip(slots, weights):
                w = np.asarray(w, dtype=np.float32)
                if nd is not None and nd < 3:
                    w = w.reshape((1,) * (3 - nd) + w.shape)
                if tuple(w.shape) != tuple(t.shape):
                    raise ValueError('Layer weight shape %s not compatible with provided weight shape %s (%s)'
                                     % (tuple(t.shape), tuple(w.shape), name))
                t.copy_(torch.from_numpy(w))
        for m in self.layers_by_name.values():
            if isinstance(m, _Conv):
                m.invalidate_packed()

    def apply_constraints(self):
        """Apply the kernel constraints the builder attached (design_dnn(conv_maxnorm=m): MaxNorm(m, axis=0) on every convolution,
        nrt_maxnorm_f32 in place).  Call it after `optimizer.step()`: Keras' optimizers apply a variable's constraint themselves,
        torch's do not know about it.  Launches only, so it can be captured in the training step's graph; a no-op on a network
        without constraints.  The packed copies of a constrained kernel are dropped as after any weight write."""
        for name in self.layer_names:
            m = self.layers_by_name[name] if name in self.layers_by_name else None
            if isinstance(m, _Conv) and m.max_norm:
                # Keras' axis 0 is the first kernel axis of the Conv{N}D layer: behind the unit axes a 1-D / 2-D kernel is lifted by
                with torch.no_grad():
                    _maxnorm(m.kernel.data.view(m.kernel.shape[3 - getattr(m, 'keras_nd', self.ndims):]), m.max_norm)
                m.invalidate_packed()

    def _weights_by_layer(self):
        """[(layer name, [(variable name, tensor, conv ndims or None), ...])] in Keras layer order"""
        groups = []
        for name, t, nd in self._weight_tensors():
            layer, var = name.rsplit('/', 1)
            if not groups or groups[-1][0] != layer:
                groups.append((layer, []))
            groups[-1][1].append((var, t, nd))
        return groups

    def save_weights(self, path):
        """
        `.npz` (default; np.savez archive keyed by `layer/variable`) or, for a path ending in .h5 / .hdf5, the Keras
        `save_weights` HDF5 layout (root attrs `layer_names`; per layer a group with attr `weight_names`
        and one dataset per variable, `layer/kernel:0` ...) so that the file loads into the Keras-built neurite unet.
        """
        if _is_h5(path):
            h5py = _h5py()
            with h5py.File(path, 'w') as f:
                self._write_h5_weights(f)
            return
        np.savez(path, **self._npz_dict())

    def _npz_dict(self):
        return {name: a for (name, _, _), a in zip(self._weight_tensors(), self.get_weights())}

    def _write_h5_weights(self, f):
        arrays = dict(zip([n for n, _, _ in self._weight_tensors()], self.get_weights()))
        groups = self._weights_by_layer()
        _h5_set_attr(f, 'layer_names', [l.encode('utf8') for l, _ in groups])
        # (what Keras' loader looks at: without `keras_version` it takes the file for Keras 1 and transposes convolution kernels)
        f.attrs['backend'] = b'tensorflow'
        f.attrs['keras_version'] = b'2.4.0'
        for layer, vs in groups:
            g = f.create_group(layer)
            names = ['%s/%s:0' % (layer, var) for var, _, _ in vs]
            _h5_set_attr(g, 'weight_names', [n.encode('utf8') for n in names])
            for n, (var, _, _) in zip(names, vs):
                g.create_dataset(n, data=arrays[layer + '/' + var])

    def _read_h5_weights(self, f, by_name):
        """Keras HDF5 weights (the file itself for `save_weights`, its `model_weights` group for `model.save`):
        layers are matched by name when every layer of this model is present (or by_name), else in order, as Keras does."""
        if 'layer_names' not in f.attrs and 'layer_names0' not in f.attrs and 'model_weights' in f:
            f = f['model_weights']
        stored = [_h5_str(n) for n in _h5_attr(f, 'layer_names')]
        with_w = [n for n in stored if len(_h5_attr(f[n], 'weight_names'))]
        groups = self._weights_by_layer()
        mine = [l for l, _ in groups]
        if by_name:
            pairs = [(g, g[0]) for g in groups if g[0] in with_w]
        elif all(l in with_w for l in mine):
            pairs = [(g, g[0]) for g in groups]
        else:
            if len(with_w) != len(mine):
                raise ValueError('You are trying to load a weight file containing %d layers into a model with %d layers.'
                                 % (len(with_w), len(mine)))
            pairs = list(zip(groups, with_w))
        out = {}
        for (layer, vs), src in pairs:
            g = f[src]
            wn = [_h5_str(n) for n in _h5_attr(g, 'weight_names')]
            if len(wn) != len(vs):
                raise ValueError('Layer %s expects %d weights, the file holds %d for %s' % (layer, len(vs), len(wn), src))
            for (var, _, _), n in zip(vs, wn):
                out[layer + '/' + var] = np.asarray(g[n])
        return out

    def load_weights(self, path, by_name=False):
        """counterpart of `save_weights`; also reads HDF5 files written by Keras (`model.save_weights` / `model.save`: h5py if
        installed, else neurite_amd.h5lite).  by_name=True loads only the layers found in the file (Keras semantics)."""
        if _is_h5(path):
            h5py = _h5py()
            with h5py.File(path, 'r') as f:
                found = self._read_h5_weights(f, by_name)
        else:
            with np.load(path) as z:
                found = {name: z[name] for name, _, _ in self._weight_tensors() if name in z.files}
        slots = self._weight_tensors()
        if not by_name:
            missing = [n for n, _, _ in slots if n not in found]
            if missing:
                raise ValueError('weight file %s has no entry for %s' % (path, missing))
            self.set_weights([found[n] for n, _, _ in slots])
            return
        current = dict(zip([n for n, _, _ in slots], self.get_weights()))
        current.update(found)
        self.set_weights([current[n] for n, _, _ in slots])

    # ---- LoadableModel (neurite/tf/modelio.py:78-143): architecture arguments travel with the weights ----
    def get_config(self):
        if not hasattr(self, 'config'):
            raise RuntimeError('this network was not built through unet / conv_enc / conv_dec, so it has no stored config')
        return self.config['params']

    @property
    def metadata(self):
        return self.get_config()['metadata']

    def save(self, path):
        """weights + the builder arguments (`model_config`), reloadable with `neurite_amd.models.load(path)`"""
        cfg = json.dumps({'class_name': self.config['builder'] if hasattr(self, 'config') else None,
                          'config': self.get_config()})
        if hasattr(self, 'config') and not self.config['loadable']:
            raise RuntimeError('networks assembled from an input_model are saved part by part (save the encoder and the '
                               'decoder arguments), as their config cannot name the graph they were grafted on')
        if _is_h5(path):
            h5py = _h5py()
            with h5py.File(path, 'w') as f:
                f.attrs['model_config'] = cfg
                self._write_h5_weights(f.create_group('model_weights'))
            return
        np.savez(path, __model_config__=np.array(cfg), **self._npz_dict())

    def get_layer(self, name):
        if name in self.layers_by_name:
            return self.layers_by_name[name]
        if name in self.layer_names:
            return self.ops[self.layer_names.index(name)]
        raise ValueError('No such layer: %s' % name)

    def keras_graph(self):
        """
        The network as the list of Keras layers the reference builders create (neurite/tf/models.py:1309-1617, :378-436):
        per layer `name`, Keras `class`, constructor `config`, producer names of its `inputs`, and `output_shape`
        (batch = None).  Fused ops are expanded (`up_N` + `merge_N` for the in-loader up-sampling/concatenation,
        `likelihood` + `prediction` for the fused head); layers no output depends on are left out, as in a Keras Model.
        tests/test_unet_graph.py compares this with the graphs recorded from the reference's own builders.
        """
        nd = self.ndims
        layers = []

        def shape_of(op):
            sp, c = op['shape']
            if op.get('keras_shape'):
                return [None] + [int(v) for v in op['keras_shape']]
            if op.get('flat'):
                return [None, int(c)]
            return [None] + [int(v) for v in sp[3 - nd:]] + [int(c)]

        def emit(name, cls, config, inputs, out_shape):
            layers.append({'name': name, 'class': cls, 'config': config, 'inputs': list(inputs), 'output_shape': out_shape})

        ndrop = 0
        for op in self.ops:
            kind, name = op['kind'], op['name']
            if kind == 'input':
                emit(name, 'InputLayer', {}, [], shape_of(op))
            elif kind == 'input_concat':
                emit(name, 'Concatenate', {'axis': -1}, op['src'], shape_of(op))
            elif kind in ('conv', 'likelihood'):
                m = self.layers_by_name[name]
                cnd = getattr(m, 'keras_nd', nd)                      # (design_dnn ends a 3-D network in a Conv1D)
                cfg = {'filters': m.cout, 'kernel_size': [int(k) for k in m.ksize3[3 - cnd:]], 'strides': [1] * cnd,
                       'padding': getattr(m, 'keras_padding', m.padding), 'dilation_rate': [m.dilation] * cnd,
                       'activation': m.activation if m.activation is not None else 'linear', 'use_bias': True}
                if m.max_norm:
                    cfg['kernel_constraint'] = {'class': 'MaxNorm', 'max_value': m.max_norm, 'axis': 0}
                emit(name, 'Conv%dD' % cnd, cfg, [op['merge'] if op.get('lo') else op['src']], shape_of(op))
            elif kind == 'dropout':
                sp, c = op['shape']
                auto = 'dropout' if ndrop == 0 else 'dropout_%d' % ndrop
                ndrop += 1
                op_name = auto                                        # the reference passes no name: Keras numbers them
                emit(op_name, 'Dropout', {'rate': float(op['rate']), 'noise_shape': [None] + [1] * nd + [int(c)]},
                     [op['src']], shape_of(op))
                layers[-1]['alias'] = name
            elif kind == 'dropout_ew':
                op_name = name
                if op.get('auto_name'):                               # the reference passes no name: Keras numbers them
                    op_name = 'dropout' if ndrop == 0 else 'dropout_%d' % ndrop
                    ndrop += 1
                emit(op_name, 'Dropout', {'rate': float(op['rate']), 'noise_shape': None}, [op['src']], shape_of(op))
                layers[-1]['alias'] = name
            elif kind == 'global_max':
                emit(name, 'GlobalMaxPooling%dD' % nd, {}, [op['src']], shape_of(op))
            elif kind == 'global_max_all':
                emit(name, 'Lambda', {'function': [['batch_flatten'], ['max', 1, True]]}, [op['src']], shape_of(op))
            elif kind == 'rescale':
                emit(name, 'RescaleValues', {'resize': op['resize']}, [op['src']], shape_of(op))
            elif kind == 'maxpool':
                pool = [int(p) for p in op['pool'][3 - nd:]]
                emit(name, 'MaxPooling%dD' % nd, {'pool_size': pool, 'strides': pool, 'padding': op['padding']}, [op['src']],
                     shape_of(op))
            elif kind == 'upsample':
                emit(name, 'UpSampling%dD' % nd, {'size': [int(p) for p in op['up'][3 - nd:]]}, [op['src']], shape_of(op))
            elif kind == 'merge':
                if not op.get('up_materialised', True):
                    sp, c = self._builder_state['shapes'][op['up_name']]
                    emit(op['up_name'], 'UpSampling%dD' % nd, {'size': [int(p) for p in op['up'][3 - nd:]]}, [op['lo']],
                         [None] + [int(v) for v in sp[3 - nd:]] + [int(c)])
                emit(name, 'Concatenate', {'axis': nd + 1}, [op['skip'], op.get('up_name', op['lo'])], shape_of(op))
            elif kind == 'add':
                emit(name, 'Add', {}, [op['a'], op['b']], shape_of(op))
            elif kind == 'multiply':
                emit(name, 'Multiply', {}, [op['a'], op['b']], shape_of(op))
            elif kind == 'activation':
                emit(name, 'Activation', {'activation': op['activation']}, [op['src']], shape_of(op))
            elif kind == 'bn':
                m = self.layers_by_name[name]
                emit(name, 'BatchNormalization', {'axis': int(op['axis']), 'momentum': float(m.momentum),
                                                  'epsilon': float(m.epsilon)}, [op['src']], shape_of(op))
            elif kind == 'prediction':
                if op['activation'] == 'softmax' and not op.get('as_activation'):
                    emit(name, 'Lambda', {'function': [['softmax', op.get('axis', nd + 1)]]}, [op['src']], shape_of(op))
                else:
                    emit(name, 'Activation', {'activation': op['activation']}, [op['src']], shape_of(op))
            elif kind == 'flatten':
                emit(name, 'Flatten', {}, [op['src']], shape_of(op))
            elif kind == 'reshape':
                emit(name, 'Reshape', {'target_shape': shape_of(op)[1:]}, [op['src']], shape_of(op))
            elif kind == 'dense':
                m = self.layers_by_name[name]
                emit(name, 'Dense', {'units': m.cout, 'activation': m.activation if m.activation is not None else 'linear',
                                     'use_bias': True}, [op['src']], shape_of(op))
            elif kind == 'resize':
                emit(name, 'Resize', {'zoom_factor': [float(z) for z in op['zoom']], 'interp_method': 'linear'}, [op['src']],
                     shape_of(op))
            elif kind == 'local_bias':
                emit(name, 'LocalBias', {'my_initializer': 'RandomNormal', 'biasmult': 1.0}, [op['src']], shape_of(op))
            elif kind == 'sample':
                emit(name, 'SampleNormalLogVar', {}, [op['a'], op['b']], shape_of(op))
            elif kind in ('identity', 'lambda'):
                emit(name, 'Lambda', {'function': []}, [op['src']], shape_of(op))
            else:
                raise RuntimeError('unknown op ' + kind)
        # dropouts are referred to by their builder names inside the op list
        alias = {l['alias']: l['name'] for l in layers if 'alias' in l}
        for l in layers:
            l['inputs'] = [alias.get(i, i) for i in l['inputs']]
            l.pop('alias', None)
        by_name = {l['name']: l for l in layers}
        out = alias.get(self.output_name, self.output_name)
        seen, stack = set(), [out]
        while stack:
            n = stack.pop()
            if n not in seen:
                seen.add(n)
                stack.extend(by_name[n]['inputs'])
        inputs = [op['name'] for op in sorted((o for o in self.ops if o['kind'] == 'input'), key=lambda o: o['index'])]
        return {'name': self.name, 'inputs': inputs, 'outputs': [out], 'layers': [l for l in layers if l['name'] in seen]}

    def _compute_dtype(self):
        """torch.float32 or torch.bfloat16: the dtype every parameter and floating-point buffer shares.  Any other dtype, or a mix,
        raises NotImplementedError naming the first layer (graph order) that breaks the rule."""
        first = None
        for name in self.layer_names:
            m = self.layers_by_name[name] if name in self.layers_by_name else None
            if m is None:
                continue
            for t in list(m.parameters(recurse=False)) + [b for b in m.buffers(recurse=False) if b.is_floating_point()]:
                if t.dtype not in (torch.float32, torch.bfloat16):
                    raise NotImplementedError('%s: %s parameters are not supported (float32, or bfloat16 for inference)'
                                              % (name, t.dtype))
                if first is None:
                    first = t.dtype
                elif t.dtype != first:
                    raise NotImplementedError('%s: %s parameters in a %s network; convert the whole model (net.float() or '
                                              'net.bfloat16())' % (name, t.dtype, first))
        return first or torch.float32

    def forward(self, inputs, return_tensors=None, _noise=None):
        """inputs: [B, *spatial, C] (or a list for multi-input nets).  Returns the prediction tensor
        (or a dict of the named intermediate tensors listed in return_tensors).  _noise: {sampling layer name: tensor} replaces the
        N(0, 1) draw of a SampleNormalLogVar layer (tests, replays); the draws of a call are kept in `last_draws`."""
        if isinstance(inputs, (list, tuple)):
            xs = list(inputs)
        else:
            xs = [inputs]
        if len(xs) != len(self.input_shapes):
            raise ValueError('%s expects %d input(s), got %d' % (self.name, len(self.input_shapes), len(xs)))
        bf16 = self._compute_dtype() == torch.bfloat16
        if bf16:
            for op in self.ops:
                if op['kind'] in _AE_KINDS or op['kind'] in _CLS_KINDS:
                    raise NotImplementedError('%s: %s layers have no bfloat16 kernel; run this network in float32 (net.float())'
                                              % (op['name'], op['kind']))
        self._noise = dict(_noise or {})
        if bf16 and self.training and torch.is_grad_enabled():
            raise NotImplementedError('%s: bfloat16 networks run inference only (model.eval() or torch.no_grad()); train in '
                                      'float32' % self.name)
        for x, shp in zip(xs, self.input_shapes):
            _lib.require_device(x)
            if tuple(x.shape[1:]) != tuple(shp):
                raise ValueError('input shape %s does not match the model input %s' % (tuple(x.shape[1:]), tuple(shp)))
        if bf16:
            mode = _BF16
        elif self.training and torch.is_grad_enabled():
            mode = _TRAIN
        else:
            mode = _F32
        return self._interpret(mode, xs, set(return_tensors or []), return_tensors)

    def _interpret(self, mode, xs, keep, return_tensors):
        """The one walk over the op list.  `mode` (_F32, _BF16 or _TRAIN below the class) holds what differs between float32
        inference, bf16 inference (module docstring: rounding points) and autograd recording: the input dtype, one primitive per glue
        layer, and the conv / likelihood / dropout handlers, which fold, defer or draw in their own ways.  Which tensors an op reads,
        where its result goes and what `keep` (the names in return_tensors) forces to be materialised is decided here."""
        nd = self.ndims
        t = {}
        if mode.recording:
            self.last_dropout_scales = {}
            self.last_dropout_masks = {}
        with torch.set_grad_enabled(mode.recording):
            for op in self.ops:
                kind, name = op['kind'], op['name']
                if kind == 'input':
                    t[name] = _lift(xs[op['index']].to(mode.dtype), nd)
                elif kind == 'input_concat':
                    t[name] = torch.cat([t[s] for s in op['src']], -1).contiguous()      # host glue (rare), exact
                elif kind == 'conv':
                    src, lo = t[op['src']], (t[op['lo']] if op.get('lo') else None)
                    if mode.conv_reads_merge and lo is not None and t.get(op['merge']) is not None:
                        src, lo = t[op['merge']], None                                    # the materialised concatenation
                    mode.conv(self, op, src, lo, t, keep)
                elif kind == 'dropout':
                    t[name] = mode.dropout(self, op, t[op['src']])
                elif kind == 'maxpool':
                    if t.get(name) is None:                                               # (else: produced by the convolution in front of it)
                        t[name] = mode.maxpool(t[op['src']], op['pool'], op['padding'])
                elif kind == 'upsample':
                    t[name] = mode.merge(None, t[op['src']], op['up'])
                elif kind == 'merge':
                    if op.get('fused') and name not in keep and (self.fold_head or not mode.merge_needs_fold_head):
                        t[name] = None            # consumed by the next conv's loader (skip + lo), never materialised
                    else:
                        t[name] = mode.merge(t[op['skip']], t[op['lo']], op['up'])
                elif kind == 'add':
                    t[name] = mode.add_act(t[op['a']], t[op['b']], 0)
                elif kind == 'activation':
                    t[name] = mode.add_act(t[op['src']], None, _ACTS[op['activation']])
                elif kind == 'multiply':
                    t[name] = mode.mul(t[op['a']], t[op['b']])
                elif kind == 'bn':
                    t[name] = mode.bn(t[op['src']], self.layers_by_name[name])
                elif kind == 'likelihood':
                    mode.likelihood(self, op, t, keep)
                elif kind == 'prediction':
                    if t.get(name) is not None:
                        pass                                    # produced by the fused likelihood
                    elif op['activation'] == 'softmax':
                        t[name] = mode.softmax(t[op['src']])
                    elif mode.recording and op['activation'] in (None, 'linear'):
                        t[name] = t[op['src']]                  # (inference copies instead: the prediction is a tensor of its own)
                    else:
                        t[name] = mode.add_act(t[op['src']], None, _act_code(op['activation']))
                elif kind in _AE_KINDS:
                    self._ae_op(op, t)
                elif kind in _CLS_KINDS:
                    self._cls_op(op, t, mode.recording)
                elif mode.recording:
                    raise NotImplementedError('neurite_amd: training through %r layers (%s) is not implemented' % (kind, name))
                else:
                    raise RuntimeError('unknown op ' + kind)
        # (bf16 included: every builder that marks an op 'flat' or gives it a 'keras_shape' also adds an auto-encoder or classifier
        # op, and forward() refuses those for a bf16 network)
        if return_tensors:
            return {k: self._unlift_named(k, t[k]) for k in keep}
        return self._unlift_named(self.output_name, t[self.output_name])

    def _unlift_named(self, name, x):
        """the tensor of layer `name` in its Keras shape: [B, *spatial, C], or [B, E] behind a Flatten / Dense"""
        if name in self._keras_shape:
            return x.reshape((x.shape[0],) + self._keras_shape[name])
        if self._flat.get(name):
            return x.reshape(x.shape[0], -1)
        return _unlift(x, self.ndims)

    def _ae_op(self, op, t):
        """the bottleneck layers of single_ae (models.py:438-646), inference and autograd recording alike: every kernel behind them
        records itself when gradients are enabled.  A [B, E] tensor rides as [B, 1, 1, 1, E]."""
        kind, name = op['kind'], op['name']
        nd = self.ndims
        if kind == 'identity':
            t[name] = t[op['src']]
        elif kind == 'lambda':
            src = t[op['src']]
            t[name] = op['fn'](self._unlift_named(op['src'], src)).reshape(src.shape)
        elif kind == 'flatten':
            src = t[op['src']]
            t[name] = src.reshape(src.shape[0], 1, 1, 1, -1)        # channels-last row-major: Keras' Flatten, a view
        elif kind == 'reshape':
            sp, c = op['shape']
            t[name] = t[op['src']].reshape((-1,) + tuple(sp) + (c,))
        elif kind == 'dense':
            src = t[op['src']]
            y = self.layers_by_name[name](src.reshape(src.shape[0], -1), variant=self.dense_variant)
            t[name] = y.view(y.shape[0], 1, 1, 1, -1)
        elif kind == 'resize':
            t[name] = _lift(self.layers_by_name[name](_unlift(t[op['src']], nd)), nd)
        elif kind == 'local_bias':
            src, k = t[op['src']], self.layers_by_name[name].kernel
            t[name] = layers._local_affine('LocalBias', src.reshape((-1,) + tuple(k.shape)), None, k, 1.0).reshape(src.shape)
        elif kind == 'sample':
            mu, lv = t[op['a']], t[op['b']]
            noise = self._noise.get(name)
            if noise is not None:
                noise = noise.to(torch.float32).reshape(mu.shape)
            lay = self.layers_by_name[name]
            t[name] = lay([mu, lv], _noise=noise)
            self.last_draws[name] = lay.last_draws['noise']
        else:
            raise RuntimeError('unknown op ' + kind)

    def _cls_op(self, op, t, recording):
        """the layers design_dnn / EncoderNet add to the conv stacks (neurite/tf/models.py:1620-1848), inference and autograd
        recording alike; a [B, E] tensor rides as [B, 1, 1, 1, E].  recording: model.train() with gradients enabled -- the only
        state in which Dropout draws."""
        kind, name = op['kind'], op['name']
        src = t[op['src']]
        if kind in ('global_max', 'global_max_all'):
            y = _global_max(src, per_channel=kind == 'global_max')
            t[name] = y.view(y.shape[0], 1, 1, 1, -1)
        elif kind == 'rescale':
            t[name] = _scale_values(src, op['resize'])
        elif kind == 'dropout_ew':
            rate = float(op.get('rate', 0))
            if recording and rate > 0:
                # KL.Dropout(rate) without a noise_shape: one draw per element.  The draw is plumbing, the multiply the kernel
                mask = ((torch.rand(src.shape, device=src.device) >= rate).to(torch.float32) / (1.0 - rate)).contiguous()
                self.last_dropout_masks[name] = mask
                t[name] = _MulFn.apply(src, mask)
            else:
                t[name] = src
        else:
            raise RuntimeError('unknown op ' + kind)

    # ---- the ops that differ per mode: handlers of _F32 / _BF16 / _TRAIN, called from _interpret ----
    def _conv_f32(self, op, src, lo, t, keep):
        name, m = op['name'], self.layers_by_name[op['name']]
        head = self._head_of.get(name) if self.fold_head and name not in keep else None
        pool = self._pool_of.get(name) if self.fold_head else None
        if head is not None and head not in keep and self._head_foldable(name, head, src, lo, op.get('up')):
            t[name] = _PendingConv(src, lo)               # runs inside the likelihood op: one kernel, no feature tensor
        elif pool is not None and lo is None and m.pool_foldable(src, self.conv_variant):
            t[name], t[pool] = m.run_with_pool(src)       # the pooled tensor from the same kernel
        else:
            t[name] = m(src, lo=lo, up=op.get('up'), variant=self.conv_variant)

    def _conv_bf16(self, op, src, lo, t, keep):
        t[op['name']] = self.layers_by_name[op['name']].run_bf16(src, lo, op.get('up'))

    def _conv_train(self, op, src, lo, t, keep):
        m = self.layers_by_name[op['name']]
        t[op['name']] = _ConvFn.apply(src, lo, m.kernel, m.bias, m, op.get('up'), self.conv_variant, False)

    def _likelihood_f32(self, op, t, keep):
        name, m, src = op['name'], self.layers_by_name[op['name']], t[op['src']]
        if isinstance(src, _PendingConv):
            t[name] = None
            t[op['pred_name']] = self.layers_by_name[op['src']].run_with_head(src.x, src.lo, m.kernel, m.bias)
            t[op['src']] = None
        elif op.get('fuse_softmax'):
            t[name] = _conv1x1_softmax(src, m.kernel, m.bias, False) if name in keep else None
            t[op['pred_name']] = _conv1x1_softmax(src, m.kernel, m.bias, True)
        else:
            t[name] = _conv1x1_softmax(src, m.kernel, m.bias, False) if m.cout <= 64 else m(src)

    def _likelihood_bf16(self, op, t, keep):
        """with fold_head the likelihood + softmax run as one kernel; without it every layer is materialised"""
        name, m, src = op['name'], self.layers_by_name[op['name']], t[op['src']]
        if op.get('fuse_softmax') and self.fold_head and name not in keep:
            t[name] = None
            t[op['pred_name']] = _conv1x1_softmax(src, m.kernel, m.bias, True)
        elif m.cout <= 64 and tuple(m.ksize3) == (1, 1, 1):
            t[name] = _conv1x1_softmax(src, m.kernel, m.bias, False)
        else:
            t[name] = m.run_bf16(src)

    def _likelihood_train(self, op, t, keep):
        """the fused head has its own backward from the prediction alone (_HeadFn); kept logits run unfused"""
        name, m, src = op['name'], self.layers_by_name[op['name']], t[op['src']]
        if op.get('fuse_softmax') and name not in keep and m.cout <= 64 and tuple(m.ksize3) == (1, 1, 1):
            t[name] = None
            t[op['pred_name']] = _head(src, m.kernel, m.bias, m)
        elif m.cout <= 64:
            t[name] = _ConvFn.apply(src, None, m.kernel, m.bias, m, None, 0, True)
        else:
            t[name] = _ConvFn.apply(src, None, m.kernel, m.bias, m, None, self.conv_variant, False)

    def _dropout_train(self, op, src):
        rate = float(op.get('rate', 0))
        if rate <= 0:
            return src
        kept = (torch.rand((src.shape[0], src.shape[-1]), device=src.device) >= rate).to(torch.float32)
        scale = (kept / (1.0 - rate)).contiguous()          # [B, C] numbers: the draw is plumbing, the scaling a kernel
        self.last_dropout_scales[op['name']] = scale
        return _ChannelScaleFn.apply(src, scale)


def _affine(bn):
    """inference BatchNormalization as a per-channel scale and shift, formed in float32 from parameters of either dtype"""
    scale = bn.gamma.detach().float() / torch.sqrt(bn.moving_variance.float() + bn.epsilon)
    shift = bn.beta.detach().float() - bn.moving_mean.float() * scale
    return scale.contiguous(), shift.contiguous()


def _bn_inference(x, bn):
    scale, shift = _affine(bn)
    return _elementwise(x, scale=scale, shift=shift)


# The three modes of ConvNet._interpret.  Inference takes the glue wrappers, which pick the float32 or bf16 kernel from the tensor;
# recording takes the autograd functions.  bf16 materialises every merge unless fold_head, and its convolutions read a materialised
# merge instead of repeating it in their loader.
_INFERENCE = dict(recording=False, maxpool=_maxpool, merge=_upsample_concat, bn=_bn_inference, softmax=_softmax,
                  add_act=lambda a, b, act: _elementwise(a, b, act=act), mul=lambda a, b: _elementwise(a, b, mul=True),
                  dropout=lambda net, op, src: src)
_F32 = types.SimpleNamespace(dtype=torch.float32, merge_needs_fold_head=False, conv_reads_merge=False,
                             conv=ConvNet._conv_f32, likelihood=ConvNet._likelihood_f32, **_INFERENCE)
_BF16 = types.SimpleNamespace(dtype=torch.bfloat16, merge_needs_fold_head=True, conv_reads_merge=True,
                              conv=ConvNet._conv_bf16, likelihood=ConvNet._likelihood_bf16, **_INFERENCE)
_TRAIN = types.SimpleNamespace(dtype=torch.float32, merge_needs_fold_head=False, conv_reads_merge=False, recording=True,
                               maxpool=_MaxPoolFn.apply, merge=_MergeFn.apply, add_act=_AddActFn.apply, mul=_MulFn.apply,
                               bn=lambda x, bn: _BatchNormFn.apply(x, bn.gamma, bn.beta, bn), softmax=_softmax_with_grad,
                               dropout=ConvNet._dropout_train, conv=ConvNet._conv_train, likelihood=ConvNet._likelihood_train)


# --------------------------------------------------------------------------------------
# builders
# --------------------------------------------------------------------------------------

class _Builder:
    def __init__(self, ndims):
        self.ndims = ndims
        self.ops = []
        self.modules = {}
        self.shapes = {}        # name -> (spatial3 tuple, channels)

    def add(self, op, shape):
        self.ops.append(op)
        self.shapes[op['name']] = shape
        op['shape'] = shape
        return op['name']


def _encoder(bld, nb_features, input_shape, nb_levels, conv_size, prefix, feat_mult, pool_size, dilation_rate_mult,
             padding, activation, layer_nb_feats, use_residuals, nb_conv_per_level, conv_dropout, batch_norm,
             src_name):
    """neurite/tf/models.py:1360-1438.  Returns the name of the last tensor."""
    ndims = bld.ndims
    pool3 = _triple(pool_size, ndims, 'pool_size')
    k3 = _triple(conv_size, ndims, 'conv_size')
    last = src_name
    lfidx = 0
    for level in range(nb_levels):
        lvl_first = last
        if isinstance(nb_features, list):                                        # :1367-1373
            lfidx = 0
            if isinstance(nb_features[level], list):
                layer_nb_feats = nb_features[level]
                nb_conv_per_level = len(layer_nb_feats)
            else:
                nb_lvl_feats = nb_conv_per_level * [nb_features[level]]
        else:
            nb_lvl_feats = int(np.round(nb_features * feat_mult ** level))      # :1375
        dil = dilation_rate_mult ** level                                        # :1376
        for conv in range(nb_conv_per_level):
            if layer_nb_feats is not None:                                       # :1379-1381
                nb_lvl_feats = layer_nb_feats[lfidx]
                lfidx += 1
            name = '%s_conv_downarm_%d_%d' % (prefix, level, conv)
            # with residuals the last conv of a level is built WITHOUT conv_kwargs: no activation and dilation_rate 1  :1384-1388
            tail = use_residuals and conv == nb_conv_per_level - 1
            act, cdil = (None, 1) if tail else (activation, dil)
            sp, cin = bld.shapes[last]
            bld.modules[name] = _Conv(name, cin, int(nb_lvl_feats), k3, cdil, padding, act)
            last = bld.add({'kind': 'conv', 'name': name, 'src': last}, (_conv_out(sp, k3, cdil, padding), int(nb_lvl_feats)))
            if conv_dropout > 0:                                                 # :1390-1399
                name = '%s_dropout_downarm_%d_%d' % (prefix, level, conv)
                last = bld.add({'kind': 'dropout', 'name': name, 'src': last, 'rate': conv_dropout}, bld.shapes[last])
        if use_residuals:                                                        # :1401-1429
            convarm = last
            nb_in, nb_out = bld.shapes[lvl_first][1], bld.shapes[convarm][1]
            add_layer = lvl_first
            if nb_in > 1 and nb_out > 1 and nb_in != nb_out:
                name = '%s_expand_down_merge_%d' % (prefix, level)
                sp, cin = bld.shapes[lvl_first]
                bld.modules[name] = _Conv(name, cin, int(nb_lvl_feats), k3, dil, padding, activation)
                add_layer = bld.add({'kind': 'conv', 'name': name, 'src': lvl_first},
                                    (_conv_out(sp, k3, dil, padding), int(nb_lvl_feats)))
                # :1412-1423 builds a Dropout on this tensor too, but its output is overwritten by the KL.add below before
                # anything reads it (add_layer was bound before the dropout): the layer is not part of the Keras model
            name = '%s_res_down_merge_%d' % (prefix, level)
            last = bld.add({'kind': 'add', 'name': name, 'a': add_layer, 'b': convarm}, bld.shapes[convarm])
            name = '%s_res_down_merge_act_%d' % (prefix, level)
            last = bld.add({'kind': 'activation', 'name': name, 'src': last, 'activation': activation}, bld.shapes[last])
        if batch_norm is not None:                                               # :1431-1433
            name = '%s_bn_down_%d' % (prefix, level)
            bld.modules[name] = _BatchNorm(name, bld.shapes[last][1])
            last = bld.add({'kind': 'bn', 'name': name, 'src': last, 'axis': batch_norm}, bld.shapes[last])
        if level < (nb_levels - 1):                                              # :1436-1438
            name = '%s_maxpool_%d' % (prefix, level)
            sp, c = bld.shapes[last]
            osp = tuple((sp[d] + pool3[d] - 1) // pool3[d] if padding == 'same' else sp[d] // pool3[d] for d in range(3))
            last = bld.add({'kind': 'maxpool', 'name': name, 'src': last, 'pool': pool3, 'padding': padding}, (osp, c))
    return last


def _conv_out(sp, k3, dil, padding):
    if padding == 'same':
        return tuple(sp)
    return tuple(sp[d] - (k3[d] - 1) * dil for d in range(3))


def _decoder(bld, nb_features, nb_levels, conv_size, nb_labels, prefix, feat_mult, pool_size, use_skip_connections,
             padding, dilation_rate_mult, activation, use_residuals, final_pred_activation, nb_conv_per_level,
             layer_nb_feats, batch_norm, conv_dropout, last, enc_conv_per_level):
    """neurite/tf/models.py:1510-1613."""
    ndims = bld.ndims
    pool3 = _triple(pool_size, ndims, 'pool_size')
    k3 = _triple(conv_size, ndims, 'conv_size')
    lfidx = 0
    for level in range(nb_levels - 1):
        if isinstance(nb_features, list):                                        # :1517-1524
            lfidx = 0
            lindex = nb_levels - level - 2
            if isinstance(nb_features[lindex], list):
                layer_nb_feats = nb_features[lindex]
                nb_conv_per_level = len(layer_nb_feats)
            else:
                nb_lvl_feats = nb_features[lindex]
        else:
            nb_lvl_feats = int(np.round(nb_features * feat_mult ** (nb_levels - 2 - level)))   # :1526
        dil = dilation_rate_mult ** (nb_levels - 2 - level)                     # :1527
        up_name = '%s_up_%d' % (prefix, nb_levels + level)                      # :1530-1532
        lo = last
        sp_lo, c_lo = bld.shapes[lo]
        sp_up = tuple(sp_lo[d] * pool3[d] for d in range(3))
        need_up_tensor = use_residuals or not use_skip_connections
        if need_up_tensor:
            last = bld.add({'kind': 'upsample', 'name': up_name, 'src': lo, 'up': pool3}, (sp_up, c_lo))
        up_tensor = last
        fused = None
        if use_skip_connections:                                                 # :1536-1542
            ncpl = enc_conv_per_level[nb_levels - 2 - level] if isinstance(enc_conv_per_level, list) else enc_conv_per_level
            conv_name = '%s_conv_downarm_%d_%d' % (prefix, nb_levels - 2 - level, ncpl - 1)
            if conv_name not in bld.shapes:
                raise ValueError('No such layer: %s' % conv_name)
            sp_s, c_s = bld.shapes[conv_name]
            if tuple(sp_s) != tuple(sp_up):
                raise ValueError('A `Concatenate` layer requires inputs with matching shapes except for the concat axis. '
                                 'Got inputs shapes: %s, %s' % (sp_s, sp_up))
            name = '%s_merge_%d' % (prefix, nb_levels + level)
            if not need_up_tensor:
                bld.shapes[up_name] = (sp_up, c_lo)      # UpSampling3D happens inside the next conv's loader
            fused = {'skip': conv_name, 'lo': lo, 'up': pool3, 'name': name}
            last = bld.add({'kind': 'merge', 'name': name, 'skip': conv_name, 'lo': lo, 'up': pool3, 'fused': True,
                            'up_name': up_name, 'up_materialised': need_up_tensor}, (sp_up, c_s + c_lo))
        for conv in range(nb_conv_per_level):                                    # :1545-1555
            if layer_nb_feats is not None:
                nb_lvl_feats = layer_nb_feats[lfidx]
                lfidx += 1
            name = '%s_conv_uparm_%d_%d' % (prefix, nb_levels + level, conv)
            tail = use_residuals and conv == nb_conv_per_level - 1                # :1552-1555, as in the encoder
            act, cdil = (None, 1) if tail else (activation, dil)
            sp, cin = bld.shapes[last]
            bld.modules[name] = _Conv(name, cin, int(nb_lvl_feats), k3, cdil, padding, act)
            op = {'kind': 'conv', 'name': name, 'src': last}
            if conv == 0 and fused is not None:
                op.update({'src': fused['skip'], 'lo': fused['lo'], 'up': fused['up'], 'merge': fused['name']})
            last = bld.add(op, (_conv_out(sp, k3, cdil, padding), int(nb_lvl_feats)))
            if conv_dropout > 0:
                name = '%s_dropout_uparm_%d_%d' % (prefix, level, conv)
                last = bld.add({'kind': 'dropout', 'name': name, 'src': last, 'rate': conv_dropout}, bld.shapes[last])
        if use_residuals:                                                        # :1568-1588
            add_layer = up_tensor
            nb_in, nb_out = bld.shapes[add_layer][1], bld.shapes[last][1]
            if nb_in > 1 and nb_out > 1 and nb_in != nb_out:
                name = '%s_expand_up_merge_%d' % (prefix, level)
                sp, cin = bld.shapes[add_layer]
                bld.modules[name] = _Conv(name, cin, int(nb_lvl_feats), k3, dil, padding, activation)
                add_layer = bld.add({'kind': 'conv', 'name': name, 'src': add_layer},
                                    (_conv_out(sp, k3, dil, padding), int(nb_lvl_feats)))
                if conv_dropout > 0:                                             # :1579-1582: a second Dropout on the conv arm
                    name = '%s_dropout_up_merge_%d_%d' % (prefix, level, nb_conv_per_level - 1)
                    last = bld.add({'kind': 'dropout', 'name': name, 'src': last, 'rate': conv_dropout}, bld.shapes[last])
            name = '%s_res_up_merge_%d' % (prefix, level)
            last = bld.add({'kind': 'add', 'name': name, 'a': last, 'b': add_layer}, bld.shapes[add_layer])
            name = '%s_res_up_merge_act_%d' % (prefix, level)
            last = bld.add({'kind': 'activation', 'name': name, 'src': last, 'activation': activation}, bld.shapes[last])
        if batch_norm is not None:                                               # :1590-1592
            name = '%s_bn_up_%d' % (prefix, level)
            bld.modules[name] = _BatchNorm(name, bld.shapes[last][1])
            last = bld.add({'kind': 'bn', 'name': name, 'src': last, 'axis': batch_norm}, bld.shapes[last])

    # likelihood (1x1 conv, no activation) and prediction  :1594-1613
    name = '%s_likelihood' % prefix
    sp, cin = bld.shapes[last]
    bld.modules[name] = _Conv(name, cin, int(nb_labels), (1, 1, 1), 1, 'same', None)
    bld.modules[name].keras_padding = 'valid'     # convL(nb_labels, 1, activation=None): Keras' default; identical at 1x1x1
    pred = '%s_prediction' % prefix
    fuse = final_pred_activation == 'softmax' and nb_labels <= 64
    last = bld.add({'kind': 'likelihood', 'name': name, 'src': last, 'fuse_softmax': fuse, 'pred_name': pred},
                   (sp, int(nb_labels)))
    if final_pred_activation == 'softmax':
        print("using final_pred_activation %s for %s" % (final_pred_activation, prefix))
        act = 'softmax'
    else:
        act = 'linear' if final_pred_activation is None else final_pred_activation
        _act_code(act)
    last = bld.add({'kind': 'prediction', 'name': pred, 'src': name, 'activation': act}, (sp, int(nb_labels)))
    return last


def _fix_residual_adds(bld):
    # the decoder's `add` takes (conv arm, add_layer); keep explicit operands consistent
    for op in bld.ops:
        if op['kind'] == 'add' and op['a'] == op['b']:
            raise RuntimeError('degenerate residual add in ' + op['name'])


def _append_prior(bld, last, model_name, prefix, spatial, nb_labels, ndims, input_index, use_logp, final_pred_activation):
    """the layers of models.add_prior (models.py:378-436) appended to a graph under construction; returns the output name"""
    sp = (1,) * (3 - ndims) + tuple(spatial)
    prior = bld.add({'kind': 'input', 'name': '%s-input' % prefix, 'index': input_index}, (sp, nb_labels))
    if use_logp:                                                                 # :401-406
        print("Breaking change: use_logp option now requires log input!", file=sys.stderr)
        post = bld.add({'kind': 'add', 'name': '%s_posterior' % prefix, 'a': prior, 'b': last}, (sp, nb_labels))
    else:                                                                        # :408-414: sigmoid likelihood x prior
        like = bld.add({'kind': 'activation', 'name': '%s_likelihood_sigmoid' % prefix, 'src': last, 'activation': 'sigmoid'},
                       (sp, nb_labels))
        post = bld.add({'kind': 'multiply', 'name': '%s_posterior' % prefix, 'a': prior, 'b': like}, (sp, nb_labels))
    if final_pred_activation == 'softmax':
        assert use_logp, 'cannot do softmax when adding prior via P()'
        print("using final_pred_activation %s for %s" % (final_pred_activation, model_name))
        return bld.add({'kind': 'prediction', 'name': '%s_prediction' % prefix, 'src': post, 'activation': 'softmax', 'axis': -1},
                       (sp, nb_labels))
    return bld.add({'kind': 'prediction', 'name': '%s_prediction' % prefix, 'src': post, 'activation': 'linear'}, (sp, nb_labels))


def add_prior(input_model, prior_shape, name='prior_model', prefix=None, use_logp=True, final_pred_activation='softmax',
              add_prior_layer_reg=0):
    """
    Append the post-prior layers to a built network (models.py:378-436): a second input `prior` [B, *prior_shape] is added
    to (use_logp: log-prior + log-likelihood, then softmax) or multiplied with (prior x sigmoid(likelihood)) the model output.
    """
    if not isinstance(input_model, ConvNet):
        raise TypeError('add_prior expects a network built by unet / conv_enc / conv_dec')
    model_name = name
    if prefix is None:
        prefix = model_name
    prior_shape = tuple(int(s) for s in prior_shape)
    ndims = input_model.ndims
    out_sp, out_c = input_model._builder_state['shapes'][input_model.output_name]
    if tuple(out_sp[3 - ndims:]) != prior_shape[:-1] or out_c != prior_shape[-1]:
        raise ValueError('prior shape %s does not match the model output %s' % (prior_shape, tuple(out_sp[3 - ndims:]) + (out_c,)))
    bld = _Builder(ndims)
    bld.ops = list(input_model.ops)
    bld.modules = dict(input_model.layers_by_name.items())
    bld.shapes = dict(input_model._builder_state['shapes'])
    last = _append_prior(bld, input_model.output_name, model_name, prefix, prior_shape[:-1], prior_shape[-1], ndims,
                         len(input_model.input_shapes), use_logp, final_pred_activation)
    net = ConvNet(model_name, ndims, list(input_model.input_shapes) + [prior_shape], bld.ops, last, bld.modules)
    net._builder_state = dict(shapes=bld.shapes)
    return net


def dilation_net(nb_features, input_shape, nb_levels, conv_size, nb_labels, name='dilation_net', prefix=None, feat_mult=1,
                 pool_size=2, use_logp=True, padding='same', dilation_rate_mult=1, activation='elu', use_residuals=False,
                 final_pred_activation='softmax', nb_conv_per_level=1, add_prior_layer=False, add_prior_layer_reg=0,
                 layer_nb_feats=None, batch_norm=None):
    """models.py:45-85: as the reference, a unet that takes only `dilation_rate_mult` from these arguments (every other
    option is passed to unet at its default)."""
    return unet(nb_features, input_shape, nb_levels, conv_size, nb_labels, name='unet', prefix=None, feat_mult=1, pool_size=2,
                use_logp=True, padding='same', activation='elu', use_residuals=False, dilation_rate_mult=dilation_rate_mult,
                final_pred_activation='softmax', nb_conv_per_level=1, add_prior_layer=False, add_prior_layer_reg=0,
                layer_nb_feats=None, batch_norm=None)


@_store_config
def conv_enc(nb_features, input_shape, nb_levels, conv_size, name=None, prefix=None, feat_mult=1, pool_size=2,
             dilation_rate_mult=1, padding='same', activation='elu', layer_nb_feats=None, use_residuals=False,
             nb_conv_per_level=2, conv_dropout=0, batch_norm=None, convL=None, src=None, src_input=None):
    """Fully convolutional encoder (neurite/tf/models.py:1309-1442)."""
    if convL is not None or src is not None or src_input is not None:
        raise NotImplementedError('convL / src / src_input are Keras-graph arguments; pass input_shape (or a list of '
                                  'input shapes to unet) instead')
    model_name = name
    if prefix is None:
        prefix = model_name
    ndims = len(input_shape) - 1
    if ndims < 1 or ndims > 3:
        raise NotImplementedError('1-, 2- and 3-D networks are supported')
    input_shape = tuple(int(s) for s in input_shape)
    bld = _Builder(ndims)
    in_name = '%s_input' % prefix
    sp3 = (1,) * (3 - ndims) + input_shape[:-1]
    bld.add({'kind': 'input', 'name': in_name, 'index': 0}, (sp3, input_shape[-1]))
    last = _encoder(bld, nb_features, input_shape, nb_levels, conv_size, prefix, feat_mult, pool_size,
                    dilation_rate_mult, padding, activation, layer_nb_feats, use_residuals, nb_conv_per_level,
                    conv_dropout, batch_norm, in_name)
    net = ConvNet(model_name, ndims, [input_shape], bld.ops, last, bld.modules)
    net._builder_state = dict(shapes=bld.shapes, nb_conv_per_level=nb_conv_per_level, nb_levels=nb_levels,
                              nb_features=nb_features)
    return net


conv_block = conv_enc


@_store_config
def conv_dec(nb_features, input_shape, nb_levels, conv_size, nb_labels, name=None, prefix=None, feat_mult=1,
             pool_size=2, use_skip_connections=False, padding='same', dilation_rate_mult=1, activation='elu',
             use_residuals=False, final_pred_activation='softmax', nb_conv_per_level=2, layer_nb_feats=None,
             batch_norm=None, conv_dropout=0, convL=None, input_model=None):
    """Fully convolutional decoder (neurite/tf/models.py:1445-1617); with input_model = an encoder built by
    conv_enc and use_skip_connections it is the U-Net."""
    if convL is not None:
        raise NotImplementedError('convL is a Keras-graph argument')
    model_name = name
    if prefix is None:
        prefix = model_name
    if use_skip_connections:                                                     # :1479-1480
        assert input_model is not None, "is using skip connections, tensors dictionary is required"
    if input_model is None:
        ndims = len(input_shape) - 1
        input_shape = tuple(int(s) for s in input_shape)
        bld = _Builder(ndims)
        in_name = '%s_input' % prefix
        bld.add({'kind': 'input', 'name': in_name, 'index': 0}, ((1,) * (3 - ndims) + input_shape[:-1], input_shape[-1]))
        last = in_name
        input_shapes = [input_shape]
        enc_ncpl = nb_conv_per_level
    else:
        ndims = input_model.ndims
        bld = _Builder(ndims)
        bld.ops = list(input_model.ops)
        bld.modules = dict(input_model.layers_by_name.items())
        bld.shapes = dict(input_model._builder_state['shapes'])
        last = input_model.output_name
        input_shapes = input_model.input_shapes
        enc_ncpl = nb_conv_per_level
        if isinstance(nb_features, list):
            enc_ncpl = [len(f) if isinstance(f, list) else nb_conv_per_level for f in nb_features]
    last = _decoder(bld, nb_features, nb_levels, conv_size, nb_labels, prefix, feat_mult, pool_size,
                    use_skip_connections, padding, dilation_rate_mult, activation, use_residuals,
                    final_pred_activation, nb_conv_per_level, layer_nb_feats, batch_norm, conv_dropout, last, enc_ncpl)
    _fix_residual_adds(bld)
    net = ConvNet(model_name, ndims, input_shapes, bld.ops, last, bld.modules)
    net._builder_state = dict(shapes=bld.shapes)
    return net


@_store_config
def unet(nb_features, input_shape, nb_levels, conv_size, nb_labels, name='unet', prefix=None, feat_mult=1,
         pool_size=2, use_logp=True, padding='same', dilation_rate_mult=1, activation='elu', use_residuals=False,
         final_pred_activation='softmax', nb_conv_per_level=1, add_prior_layer=False, add_prior_layer_reg=0,
         layer_nb_feats=None, conv_dropout=0, batch_norm=None):
    """unet-style model with the reference's parametrisation (neurite/tf/models.py:88-246)."""
    model_name = name
    if prefix is None:
        prefix = model_name
    if add_prior_layer and not use_logp:                                         # models.py:423
        assert final_pred_activation != 'softmax', 'cannot do softmax when adding prior via P()'
    multi = isinstance(input_shape[0], (tuple, list, np.ndarray))
    if multi:                                                                    # :155-170
        shapes = [tuple(int(v) for v in s) for s in input_shape]
        for s in shapes:
            if not np.array_equal(s[:-1], shapes[0][:-1]):
                raise ValueError('spatial dimensions must match if multiple input shapes '
                                 'are provided, but got shapes '
                                 f'{shapes[0][:-1]} and {s[:-1]}')
        first = shapes[0]
    else:
        shapes = [tuple(int(v) for v in input_shape)]
        first = shapes[0]
    ndims = len(first) - 1
    if isinstance(nb_features, list):                                            # :179-190
        if nb_levels is not None:
            warnings.warn('nb_levels is not None while ' + 'nb_features list of lists specified - overriding')
        if feat_mult is not None:
            warnings.warn('feat_mult is not None while ' + 'nb_features list of lists specified - overriding')
        nb_levels = len(nb_features)
        assert isinstance(nb_features[0], list), \
            'nb_features must be a scalar or a list of lists (not a list of scalars)'

    if ndims < 1 or ndims > 3:
        raise NotImplementedError('1-, 2- and 3-D networks are supported')
    bld = _Builder(ndims)
    if multi:
        names = []
        for i, s in enumerate(shapes):
            n = f'{prefix}_input_{i}'
            bld.add({'kind': 'input', 'name': n, 'index': i}, ((1,) * (3 - ndims) + s[:-1], s[-1]))
            names.append(n)
        src = bld.add({'kind': 'input_concat', 'name': f'{prefix}_input_concat', 'src': names},
                      ((1,) * (3 - ndims) + first[:-1], sum(s[-1] for s in shapes)))
    else:
        src = bld.add({'kind': 'input', 'name': '%s_input' % prefix, 'index': 0},
                      ((1,) * (3 - ndims) + first[:-1], first[-1]))
    last = _encoder(bld, nb_features, first, nb_levels, conv_size, prefix, feat_mult, pool_size, dilation_rate_mult,
                    padding, activation, layer_nb_feats, use_residuals, nb_conv_per_level, conv_dropout, batch_norm, src)
    lnf = layer_nb_feats[(nb_levels * nb_conv_per_level):] if layer_nb_feats is not None else None      # :214
    enc_ncpl = nb_conv_per_level
    if isinstance(nb_features, list):
        enc_ncpl = [len(f) for f in nb_features]
    last = _decoder(bld, nb_features, nb_levels, conv_size, nb_labels, prefix, feat_mult, pool_size, 1, padding,
                    dilation_rate_mult, activation, use_residuals, 'linear' if add_prior_layer else final_pred_activation,
                    nb_conv_per_level, lnf, batch_norm, conv_dropout, last, enc_ncpl)
    _fix_residual_adds(bld)
    if add_prior_layer:                                                          # models.add_prior, :378-436
        pname = model_name + '_prior'
        last = _append_prior(bld, last, pname, pname, tuple(first[:-1]), int(nb_labels), ndims, len(shapes), use_logp,
                             final_pred_activation)
        shapes = shapes + [tuple(first[:-1]) + (int(nb_labels),)]
        model_name = pname
    net = ConvNet(model_name, ndims, shapes, bld.ops, last, bld.modules)
    net._builder_state = dict(shapes=bld.shapes)
    return net


def _keras_shape(bld, name):
    """shape (without batch) of the Keras tensor behind op `name`: [*spatial, C], or [E] behind a Flatten / Dense"""
    sp, c = bld.shapes[name]
    op = next(o for o in bld.ops if o['name'] == name)
    if op.get('flat'):
        return [int(c)]
    return [int(v) for v in sp[3 - bld.ndims:]] + [int(c)]


def _last_axis_only(name, axis, rank):
    """Keras BatchNormalization(axis=...) on a tensor of `rank` axes (batch included): the kernels normalise over the last one"""
    a = int(axis)
    if a < 0:
        a += rank
    if a != rank - 1:
        raise NotImplementedError('%s: BatchNormalization over axis %r of a rank-%d tensor is not implemented (the last axis is)'
                                  % (name, axis, rank))


def _single_ae_layers(bld, last, prefix, enc_size, ae_type, conv_size, enc_lambda_layers, batch_norm, padding, activation,
                      include_mu_shift_layer, do_vae):
    """the layers of models.single_ae (neurite/tf/models.py:476-642) appended behind tensor `last`; returns the output name"""
    ndims = bld.ndims
    input_shape = _keras_shape(bld, last)                                        # :472
    input_nb_feats = input_shape[-1]
    one3 = (1, 1, 1)                                                             # a [B, E] tensor rides as [B, 1, 1, 1, E]

    def add(op, sp3, c, flat):
        if flat:
            op['flat'] = True
        return bld.add(op, (tuple(sp3), int(c)))

    def same(op, src):
        sp3, c = bld.shapes[src]
        return add(op, sp3, c, next(o for o in bld.ops if o['name'] == src).get('flat'))

    def conv(name, src, filters):
        sp, cin = bld.shapes[src]
        bld.modules[name] = _Conv(name, cin, int(filters), k3, 1, padding, activation)
        return add({'kind': 'conv', 'name': name, 'src': src}, _conv_out(sp, k3, 1, padding), int(filters), False)

    def resize(name, src, target):
        sp, c = bld.shapes[src]
        cur = list(sp[3 - ndims:])
        zf = [target[f] / cur[f] for f in range(ndims)]                           # :516-517, 572-573, 632
        bld.modules[name] = layers.Resize(zoom_factor=list(zf), name=name)
        out = (1,) * (3 - ndims) + tuple(int(cur[f] * zf[f]) for f in range(ndims))     # Resize.compute_output_shape
        return add({'kind': 'resize', 'name': name, 'src': src, 'zoom': zf}, out, c, False)

    def local_bias(name, src):
        bld.modules[name] = _LocalBiasWeight(name, _keras_shape(bld, src))
        return same({'kind': 'local_bias', 'name': name, 'src': src}, src)

    def bn(name, src):
        _last_axis_only(name, batch_norm, len(_keras_shape(bld, src)) + 1)
        bld.modules[name] = _BatchNorm(name, bld.shapes[src][1])
        return same({'kind': 'bn', 'name': name, 'src': src, 'axis': batch_norm}, src)

    def clean_up(which, src):                                                     # :535-547, 590-602
        for layer_fcn in enc_lambda_layers:
            name = '%s_ae_%s_%s' % (prefix, which, layer_fcn.__name__)
            src = same({'kind': 'lambda', 'name': name, 'src': src, 'fn': layer_fcn}, src)
        if batch_norm is not None:
            src = bn('%s_ae_%s_bn' % (prefix, which), src)
        return same({'kind': 'identity', 'name': '%s_ae_%s' % (prefix, which), 'src': src}, src)

    if ae_type == 'conv':                                                        # :476-479
        if len(input_shape) - 1 != ndims or ndims < 1:
            raise ValueError('a convolutional auto-encoder needs a [*spatial, features] input, got %s' % (input_shape,))
        assert conv_size is not None, 'with conv ae, need conv_size'
        k3 = _triple(conv_size, ndims, 'conv_size')
    if ae_type == 'dense' and len(input_shape) > 1:                              # :486-488
        last = add({'kind': 'flatten', 'name': '%s_ae_%s_down_flat' % (prefix, ae_type), 'src': last}, one3,
                   int(np.prod(input_shape)), True)
    pre_enc = last

    if ae_type == 'dense':                                                       # :494-499
        assert len(enc_size) == 1, "enc_size should be of length 1 for dense layer"
        enc_size_str = ''.join(['%d_' % d for d in enc_size])[:-1]

        def dense_enc(which):
            name = '%s_ae_%s_enc_dense_%s' % (prefix, which, enc_size_str)
            bld.modules[name] = _Dense(name, bld.shapes[pre_enc][1], int(enc_size[0]))
            return add({'kind': 'dense', 'name': name, 'src': pre_enc}, one3, int(enc_size[0]), True)
        last = dense_enc('mu')
    else:                                                                        # :501-528
        assert len(enc_size) == len(input_shape), \
            "encoding size does not match input shape %d %d" % (len(enc_size), len(input_shape))
        resized = list(enc_size)[:-1] != list(input_shape)[:-1] and all(f is not None for f in input_shape[:-1]) and \
            all(f is not None for f in enc_size[:-1])
        if resized:
            last = conv('%s_ae_mu_enc_conv' % prefix, pre_enc, enc_size[-1])
            last = resize('%s_ae_mu_enc' % prefix, last, list(enc_size[:-1]))
        elif enc_size[-1] is None:
            last = same({'kind': 'identity', 'name': '%s_ae_mu_enc' % prefix, 'src': pre_enc}, pre_enc)
        else:
            last = conv('%s_ae_mu_enc' % prefix, pre_enc, enc_size[-1])

    if include_mu_shift_layer:                                                   # :530-533
        last = local_bias('%s_ae_mu_shift' % prefix, last)
    last = clean_up('mu', last)

    if do_vae:                                                                   # :550-608
        mu = last
        if ae_type == 'dense':
            last = dense_enc('sigma')
        elif resized:
            last = conv('%s_ae_sigma_enc_conv' % prefix, pre_enc, enc_size[-1])
            last = resize('%s_ae_sigma_enc' % prefix, last, list(enc_size[:-1]))
        elif enc_size[-1] is None:
            last = conv('%s_ae_sigma_enc' % prefix, pre_enc, bld.shapes[pre_enc][1])
        else:
            last = conv('%s_ae_sigma_enc' % prefix, pre_enc, enc_size[-1])
        logvar = clean_up('sigma', last)
        name = '%s_ae_sample' % prefix
        bld.modules[name] = layers.SampleNormalLogVar(name=name)
        op = {'kind': 'sample', 'name': name, 'a': mu, 'b': logvar}
        last = same(op, mu)

    if include_mu_shift_layer:                                                   # :610-613
        last = local_bias('%s_ae_sample_shift' % prefix, last)

    if ae_type == 'dense':                                                       # :616-623
        name = '%s_ae_%s_dec_flat_%s' % (prefix, ae_type, enc_size_str)
        units = int(np.prod(input_shape))
        bld.modules[name] = _Dense(name, bld.shapes[last][1], units)
        last = add({'kind': 'dense', 'name': name, 'src': last}, one3, units, True)
        if len(input_shape) > 1:
            sp3 = (1,) * (4 - len(input_shape)) + tuple(input_shape[:-1])
            last = add({'kind': 'reshape', 'name': '%s_ae_%s_dec' % (prefix, ae_type), 'src': last}, sp3, input_shape[-1], False)
    else:                                                                        # :625-638
        if resized:
            last = resize('%s_ae_mu_dec' % prefix, last, list(input_shape[:-1]))
        last = conv('%s_ae_%s_dec' % (prefix, ae_type), last, input_nb_feats)

    if batch_norm is not None:                                                   # :640-642
        last = bn('%s_bn_ae_%s_dec' % (prefix, ae_type), last)
    return last


@_store_config
def single_ae(enc_size, input_shape, name='single_ae', prefix=None, ae_type='dense', conv_size=None, input_model=None,
              enc_lambda_layers=None, batch_norm=True, padding='same', activation=None, include_mu_shift_layer=False,
              do_vae=False):
    """
    Single-layer (variational) auto-encoder, input - encoding - output (neurite/tf/models.py:438-646): `ae_type='dense'` is
    Flatten - Dense(enc_size) - Dense(prod(input_shape)) - Reshape on csrc/dense.hip, `ae_type='conv'` a convolution (with a Resize
    where the encoding's spatial size differs, a pass-through where enc_size[-1] is None).  do_vae adds the sigma branch and
    layers.SampleNormalLogVar; include_mu_shift_layer a LocalBias before and after it; enc_lambda_layers are callables on torch
    tensors, named by their __name__; batch_norm is the BatchNormalization axis (it must be the tensor's last one).
    """
    model_name = name
    if prefix is None:
        prefix = model_name
    if enc_lambda_layers is None:
        enc_lambda_layers = []
    if ae_type not in ('dense', 'conv'):
        raise ValueError("ae_type must be 'dense' or 'conv', got %r" % (ae_type,))
    if input_model is None:
        assert input_shape is not None, 'input_shape of input_model is necessary'
        input_shape = tuple(int(s) for s in input_shape)
        ndims = len(input_shape) - 1
        if ndims > 3:
            raise NotImplementedError('inputs of up to 3 spatial dimensions are supported')
        bld = _Builder(ndims)
        op = {'kind': 'input', 'name': '%s_input' % prefix, 'index': 0}
        if ndims == 0:
            op['flat'] = True
        last = bld.add(op, ((1,) * (3 - ndims) + input_shape[:-1], input_shape[-1]))
        input_shapes = [input_shape]
    else:
        if not isinstance(input_model, ConvNet):
            raise TypeError('input_model must be a network built by this module')
        bld = _Builder(input_model.ndims)
        bld.ops = list(input_model.ops)
        bld.modules = dict(input_model.layers_by_name.items())
        bld.shapes = dict(input_model._builder_state['shapes'])
        last = input_model.output_name
        input_shapes = input_model.input_shapes
    last = _single_ae_layers(bld, last, prefix, enc_size, ae_type, conv_size, enc_lambda_layers, batch_norm, padding, activation,
                             include_mu_shift_layer, do_vae)
    net = ConvNet(model_name, bld.ndims, input_shapes, bld.ops, last, bld.modules)
    net._builder_state = dict(shapes=bld.shapes)
    return net


@_store_config
def ae(nb_features, input_shape, nb_levels, conv_size, nb_labels, enc_size, name='ae', prefix=None, feat_mult=1, pool_size=2,
       padding='same', activation='elu', use_residuals=False, nb_conv_per_level=1, batch_norm=None, enc_batch_norm=None,
       ae_type='conv', enc_lambda_layers=None, add_prior_layer=False, add_prior_layer_reg=0, use_logp=True, conv_dropout=0,
       include_mu_shift_layer=False, single_model=False, final_pred_activation='softmax', src=None, src_input=None,
       do_vae=False):
    """
    Convolutional (optionally variational, optionally dense-bottleneck) auto-encoder (neurite/tf/models.py:249-375):
    conv_enc - single_ae - conv_dec [- add_prior].  Returns (dec_model, mid_ae_model, enc_model), three stackable networks, or with
    single_model=True the one chained network.
    """
    model_name = name
    ndims = len(input_shape) - 1
    if isinstance(pool_size, int):
        pool_size = (pool_size,) * ndims
    enc_model = conv_enc(nb_features, input_shape, nb_levels, conv_size, name=model_name, feat_mult=feat_mult,
                         pool_size=pool_size, padding=padding, activation=activation, use_residuals=use_residuals,
                         nb_conv_per_level=nb_conv_per_level, conv_dropout=conv_dropout, batch_norm=batch_norm, src=src,
                         src_input=src_input)

    def out_shape(model):
        sp, c = model._builder_state['shapes'][model.output_name]
        return [int(v) for v in sp[3 - model.ndims:]] + [int(c)]

    if single_model:                                                             # :321-326
        in_input_shape, in_model = None, enc_model
    else:
        in_input_shape, in_model = out_shape(enc_model), None
    mid_ae_model = single_ae(enc_size, in_input_shape, conv_size=conv_size, name=model_name, ae_type=ae_type,
                             input_model=in_model, batch_norm=enc_batch_norm, enc_lambda_layers=enc_lambda_layers,
                             include_mu_shift_layer=include_mu_shift_layer, do_vae=do_vae)
    if single_model:                                                             # :339-344
        in_input_shape, in_model = None, mid_ae_model
    else:
        in_input_shape, in_model = out_shape(mid_ae_model), None
    dec_model = conv_dec(nb_features, in_input_shape, nb_levels, conv_size, nb_labels, name=model_name, feat_mult=feat_mult,
                         pool_size=pool_size, use_skip_connections=False, padding=padding, activation=activation,
                         use_residuals=use_residuals, final_pred_activation=final_pred_activation,
                         nb_conv_per_level=nb_conv_per_level, batch_norm=batch_norm, conv_dropout=conv_dropout,
                         input_model=in_model)
    if add_prior_layer:                                                          # :363-370
        dec_model = add_prior(dec_model, [*input_shape[:-1], nb_labels], name=model_name, prefix=model_name + '_prior',
                              use_logp=use_logp, final_pred_activation=final_pred_activation,
                              add_prior_layer_reg=add_prior_layer_reg)
    if single_model:
        return dec_model
    return (dec_model, mid_ae_model, enc_model)


def _flat_tail(bld):
    """helpers that append [B, E] layers (riding as [B, 1, 1, 1, E]) behind a builder's last tensor"""
    one3 = (1, 1, 1)

    def flatten(name, src):
        sp, c = bld.shapes[src]
        op = {'kind': 'flatten', 'name': name, 'src': src, 'flat': True}
        return bld.add(op, (one3, int(np.prod(sp)) * int(c)))

    def dense(name, src, units, activation=None):
        bld.modules[name] = _Dense(name, bld.shapes[src][1], int(units), activation)
        return bld.add({'kind': 'dense', 'name': name, 'src': src, 'flat': True}, (one3, int(units)))

    def dropout(name, src, rate, auto_name=False):
        op = {'kind': 'dropout_ew', 'name': name, 'src': src, 'rate': float(rate), 'auto_name': auto_name}
        srcop = next(o for o in bld.ops if o['name'] == src)
        for k in ('flat', 'keras_shape'):
            if srcop.get(k):
                op[k] = srcop[k]
        return bld.add(op, bld.shapes[src])

    return flatten, dense, dropout


@_store_config
def design_dnn(nb_features, input_shape, nb_levels, conv_size, nb_labels, feat_mult=1, pool_size=2, padding='same',
               activation='elu', final_layer='dense-sigmoid', conv_dropout=0, conv_maxnorm=0, nb_input_features=1,
               batch_norm=False, name=None, prefix=None, use_strided_convolution_maxpool=True, nb_conv_per_level=2):
    """
    "Deep" CNN that ends in a number per volume (neurite/tf/models.py:1620-1775): nb_levels x (nb_conv_per_level convolutions, then a
    stride-1 convolution of kernel size pool_size -- it does not down-sample -- or, with use_strided_convolution_maxpool=False, a
    max-pooling), then `final_layer`:
      'dense-sigmoid'       Flatten - Dense(1, sigmoid)
      'dense-softmax'       Flatten - Dense(nb_labels, softmax)
      'myglobalmaxpooling'  BatchNormalization(axis=batch_norm) - max over everything but the batch axis - Reshape((1, 1)) -
                            Conv1D(1, 1, sigmoid).  batch_norm IS the axis here, as in the reference: the last axis runs, the default
                            False is axis 0, which Keras refuses (ValueError)
      'globalmaxpooling'    Conv3D(2, 1, relu) - GlobalMaxPooling3D - softmax (3-D inputs only)
      'dense-tanh'          raises TypeError, as the reference does ('%s_%s_tanh' % prefix)
      anything else         the model ends at the last convolution or pooling
    input_shape is the SPATIAL shape; nb_input_features the channels.  conv_dropout is a plain element-wise Dropout in front of every
    convolution (it draws in model.train() only; the mask of the last draw is in `last_dropout_masks`).  conv_maxnorm > 0 attaches
    MaxNorm(conv_maxnorm) to every convolution of the levels: call `apply_constraints()` after each optimizer step.
    """
    model_name = name
    if model_name is None:
        model_name = 'model_1'
    if prefix is None:
        prefix = model_name
    ndims = len(input_shape)
    if ndims < 1 or ndims > 3:
        raise NotImplementedError('1-, 2- and 3-D networks are supported')
    input_shape = tuple(int(v) for v in input_shape)
    if not use_strided_convolution_maxpool and ndims == 1:
        raise ValueError('design_dnn pools with MaxPooling2D unless the input is 3-D: a 1-D input cannot be pooled')
    pool3 = _triple(pool_size, ndims, 'pool_size')
    k3 = _triple(conv_size, ndims, 'conv_size')
    bld = _Builder(ndims)
    flatten, dense, dropout = _flat_tail(bld)
    in_name = '%s_input' % prefix
    last = bld.add({'kind': 'input', 'name': in_name, 'index': 0}, ((1,) * (3 - ndims) + input_shape, int(nb_input_features)))

    def conv(name, src, filters, ksize):
        sp, cin = bld.shapes[src]
        m = bld.modules[name] = _Conv(name, cin, int(filters), ksize, 1, padding, activation)
        if conv_maxnorm > 0:
            m.max_norm = conv_maxnorm
        return bld.add({'kind': 'conv', 'name': name, 'src': src}, (_conv_out(sp, ksize, 1, padding), int(filters)))

    for level in range(nb_levels):
        for ci in range(nb_conv_per_level):
            if conv_dropout > 0:                                                  # :1675-1678, no name: Keras numbers them
                last = dropout('%s_dropout_%d_%d' % (prefix, level, ci), last, conv_dropout, auto_name=True)
            nb_lvl_feats = int(np.round(nb_features * feat_mult ** level))
            last = conv('%s_conv_%d_%d' % (prefix, level, ci), last, nb_lvl_feats, k3)
        if use_strided_convolution_maxpool:                                       # :1687-1691
            last = conv('%s_strided_conv_%d' % (prefix, level), last, nb_lvl_feats, pool3)
        else:
            sp, c = bld.shapes[last]
            osp = tuple((sp[d] + pool3[d] - 1) // pool3[d] if padding == 'same' else sp[d] // pool3[d] for d in range(3))
            last = bld.add({'kind': 'maxpool', 'name': '%s_maxpool_%d' % (prefix, level), 'src': last, 'pool': pool3,
                            'padding': padding}, (osp, c))

    if final_layer == 'dense-sigmoid':
        last = flatten('%s_flatten' % prefix, last)
        last = dense('%s_dense' % prefix, last, 1, 'sigmoid')
    elif final_layer == 'dense-tanh':
        last = flatten('%s_flatten' % prefix, last)
        last = dense('%s_dense' % prefix, last, 1)
        tanh_name = '%s_%s_tanh' % prefix                                          # :1725 -- TypeError, as in the reference
        op = {'kind': 'activation', 'name': tanh_name, 'src': last, 'activation': 'tanh', 'flat': True}
        last = bld.add(op, bld.shapes[last])
    elif final_layer == 'dense-softmax':
        last = flatten('%s_flatten' % prefix, last)
        last = dense('%s_dense' % prefix, last, nb_labels, 'softmax')
    elif final_layer == 'myglobalmaxpooling':
        name = '%s_batch_norm' % prefix
        if int(batch_norm) == 0:
            raise ValueError('%s: BatchNormalization(axis=%r): axis 0 is the batch axis (pass the feature axis as batch_norm)'
                             % (name, batch_norm))
        _last_axis_only(name, batch_norm, ndims + 2)
        bld.modules[name] = _BatchNorm(name, bld.shapes[last][1])
        last = bld.add({'kind': 'bn', 'name': name, 'src': last, 'axis': int(batch_norm)}, bld.shapes[last])
        one3 = (1, 1, 1)
        last = bld.add({'kind': 'global_max_all', 'name': '%s_global_max_pool' % prefix, 'src': last, 'flat': True}, (one3, 1))
        last = bld.add({'kind': 'reshape', 'name': '%s_global_max_pool_reshape' % prefix, 'src': last, 'keras_shape': (1, 1)},
                       (one3, 1))
        name = '%s_global_max_pool_sigmoid' % prefix
        m = bld.modules[name] = _Conv(name, 1, 1, one3, 1, 'valid', 'sigmoid')
        m.keras_nd = 1                                                            # KL.Conv1D(1, 1) on [B, 1, 1]
        last = bld.add({'kind': 'conv', 'name': name, 'src': last, 'keras_shape': (1, 1)}, (one3, 1))
    elif final_layer == 'globalmaxpooling':
        if ndims != 3:
            raise ValueError("final_layer='globalmaxpooling' is Conv3D + GlobalMaxPooling3D: it needs a 3-D input, got %d-D" % ndims)
        name = '%s_conv_to_featmaps' % prefix
        sp, cin = bld.shapes[last]
        bld.modules[name] = _Conv(name, cin, 2, (1, 1, 1), 1, 'valid', 'relu')
        last = bld.add({'kind': 'conv', 'name': name, 'src': last}, (sp, 2))
        last = bld.add({'kind': 'global_max', 'name': '%s_global_max_pool' % prefix, 'src': last, 'flat': True}, ((1, 1, 1), 2))
        last = bld.add({'kind': 'prediction', 'name': '%s_global_max_pool_softmax' % prefix, 'src': last, 'activation': 'softmax',
                        'as_activation': True, 'flat': True}, ((1, 1, 1), 2))
    net = ConvNet(model_name, ndims, [input_shape + (int(nb_input_features),)], bld.ops, last, bld.modules)
    net._builder_state = dict(shapes=bld.shapes)
    return net


@_store_config
def EncoderNet(nb_features, input_shape, nb_levels, conv_size, name=None, prefix=None, feat_mult=1, pool_size=2,
               dilation_rate_mult=1, padding='same', activation='elu', layer_nb_feats=None, use_residuals=False,
               nb_conv_per_level=2, conv_dropout=0, dense_size=256, nb_labels=2, final_activation=None, rescale=None, dropout=None,
               batch_norm=None):
    """
    Convolutional encoder with a classifier or regressor on top (neurite/tf/models.py:1782-1848): conv_enc - Flatten - [Dropout] -
    Dense(dense_size) - [Dropout] - [layers.RescaleValues(rescale)] - Dense(nb_labels, final_activation).  nb_labels <= 0 is a
    one-unit regressor (final_activation None: linear); otherwise final_activation None is softmax.  As in the reference, `prefix`,
    `dilation_rate_mult` and `layer_nb_feats` are accepted and not passed on to the encoder.
    """
    enc = conv_enc(nb_features, input_shape, nb_levels, conv_size, name=name, feat_mult=feat_mult, pool_size=pool_size,
                   padding=padding, activation=activation, use_residuals=use_residuals, nb_conv_per_level=nb_conv_per_level,
                   conv_dropout=conv_dropout, batch_norm=batch_norm)
    bld = _Builder(enc.ndims)
    bld.ops = list(enc.ops)
    bld.modules = dict(enc.layers_by_name.items())
    bld.shapes = dict(enc._builder_state['shapes'])
    flatten, dense, drop = _flat_tail(bld)
    last = flatten('flatten', enc.output_name)
    if dropout is not None and dropout > 0:
        last = drop('dropout_flat', last, dropout)
    last = dense('dense', last, dense_size)
    if dropout is not None and dropout > 0:
        last = drop('dropout_dense', last, dropout)
    if nb_labels <= 0:                                                             # a regression net
        nb_labels = 1
        if final_activation is None:
            final_activation = 'linear'
    elif final_activation is None:
        final_activation = 'softmax'
    if rescale is not None:
        last = bld.add({'kind': 'rescale', 'name': 'rescale_values', 'src': last, 'resize': rescale, 'flat': True}, bld.shapes[last])
    last = dense('output_dense', last, nb_labels, final_activation)
    net = ConvNet(None, enc.ndims, enc.input_shapes, bld.ops, last, bld.modules)
    net._builder_state = dict(shapes=bld.shapes)
    return net


def load_config(path):
    """builder name and arguments stored by `ConvNet.save` (LoadableModel.load_config, neurite/tf/modelio.py:125-143)"""
    if _is_h5(path):
        h5py = _h5py()
        with h5py.File(path, 'r') as f:
            cfg = f.attrs['model_config']
    else:
        with np.load(path) as z:
            if '__model_config__' not in z.files:
                raise ValueError('%s holds weights only (written by save_weights); build the model and call load_weights' % path)
            cfg = z['__model_config__'].item()
    cfg = json.loads(_h5_str(cfg))
    return cfg['class_name'], cfg['config']


def load(path, by_name=False, **kwargs):
    """
    LoadableModel.load (neurite/tf/modelio.py:111-123): rebuild the network from the arguments saved with it (keyword
    arguments override them), then load its weights.
    """
    builder, config = load_config(path)
    builders = {'unet': unet, 'conv_enc': conv_enc, 'conv_dec': conv_dec, 'ae': ae, 'single_ae': single_ae,
                'design_dnn': design_dnn, 'EncoderNet': EncoderNet}
    if builder not in builders:
        raise ValueError('%s was not saved from a unet / conv_enc / conv_dec / ae / single_ae / design_dnn / EncoderNet network (class_name %r)'
                         % (path, builder))
    config.update(kwargs)
    metadata = config.pop('metadata', {})
    model = builders[builder](**config)
    model.metadata.update(metadata)
    model.load_weights(path, by_name=by_name)
    return model


def labels_to_image(*args, **kwargs):
    """neurite/tf/models.py:649-918; implemented in neurite_amd.synthesis."""
    from . import synthesis
    return synthesis.labels_to_image(*args, **kwargs)


def labels_to_image_new(*args, **kwargs):
    """neurite/tf/models.py:920-1300; implemented in neurite_amd.synthesis."""
    from . import synthesis
    return synthesis.labels_to_image_new(*args, **kwargs)


class SynthStrip(nn.Module):
    """
    SynthStrip (neurite/tf/models.py:1888-1967): a label map is turned into a synthetic image by `labels_to_image`
    (integer output labels), a unet with one linear output channel is applied to it, and the model returns the unet output
    concatenated with the warped label map, [B, *inshape, 2], for a brain / non-brain loss.  Constructor arguments are
    recorded as `modelio.store_config_args` does (`get_config`, `save`, `SynthStrip.load`).
    """

    def __init__(self, inshape, labels_in, labels_out, nb_unet_features=None, nb_unet_levels=None, unet_feat_mult=1,
                 nb_unet_conv_per_level=1, src_feats=1, gen_args={}):
        super().__init__()
        ndims = len(inshape)
        assert ndims in [1, 2, 3], 'ndims should be one of 1, 2, or 3. found: %d' % ndims
        inshape = tuple(int(s) for s in inshape)
        self.config = {'builder': 'SynthStrip', 'loadable': True,
                       'params': dict(inshape=list(inshape), labels_in=_jsonable(labels_in), labels_out=_jsonable(labels_out),
                                      nb_unet_features=_jsonable(nb_unet_features), nb_unet_levels=nb_unet_levels,
                                      unet_feat_mult=unet_feat_mult, nb_unet_conv_per_level=nb_unet_conv_per_level,
                                      src_feats=src_feats, gen_args=_jsonable(dict(gen_args)), metadata={})}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                       # the reference builds the deprecated generator here too
            self.gen_model = labels_to_image(inshape, labels_in, labels_out, id=0, return_def=False, one_hot=False, **gen_args)
        self.unet = unet(nb_unet_features, (*inshape, 1), nb_unet_levels, ndims * (3,), 1, feat_mult=unet_feat_mult,
                         nb_conv_per_level=nb_unet_conv_per_level, final_pred_activation='linear')
        self.name = 'synthstrip'

    def get_config(self):
        return self.config['params']

    @property
    def metadata(self):
        return self.config['params']['metadata']

    def get_strip_model(self):
        """the stripping model (just the U-Net)"""
        return self.unet

    def train(self, mode=True):
        super().train(mode)
        self.unet.train(mode)                                    # ConvNet defaults to eval(); follow the wrapper's mode
        return self

    def forward(self, labels):
        synth_image, synth_labels = self.gen_model(labels)[:2]
        self.synth_image = synth_image
        out = self.unet(synth_image)
        return torch.cat([out, synth_labels.to(torch.float32)], -1)

    def brain_mask(self, image, border=1.0, connectivity=1, normalize=False):
        """
        The brain mask of an image: the stripping model predicts a signed distance to the brain boundary, and the mask is
        `sdt < border` (border in voxels, outwards), its largest connected component, with the holes of that component filled.  This is the
        post-processing of FreeSurfer's mri_synthstrip, restated, not recorded: FreeSurfer is not in the reference tree.

        image: [B, *inshape] or [B, *inshape, 1] float32, already at the model's resolution (nothing is resampled) and, with
        normalize=False, at its intensity range.  normalize=True applies mri_synthstrip's intensity step first, per batch entry:
        the minimum subtracted, divided by the 99th percentile of the result, clipped to [0, 1]
        (utils.percentile_norm(image, 0, 99, clip=True, batched=True); also restated, not recorded).
        Returns bool [B, *inshape].  Runs under no_grad, entirely on the device (utils.percentile_norm, utils.largest_component,
        utils.fill_holes).
        """
        inshape = tuple(self.config['params']['inshape'])
        if not isinstance(image, torch.Tensor):
            raise TypeError('SynthStrip.brain_mask: expected a torch.Tensor, got %s' % type(image).__name__)
        if tuple(image.shape[1:]) == inshape:
            image = image.unsqueeze(-1)
        if image.dim() != len(inshape) + 2 or tuple(image.shape[1:]) != inshape + (1,):
            raise ValueError('SynthStrip.brain_mask: expected [B, %s] or [B, %s, 1], got shape %s'
                             % (', '.join(map(str, inshape)), ', '.join(map(str, inshape)), tuple(image.shape)))
        with torch.no_grad():
            if normalize:
                image = utils.percentile_norm(image, 0, 99, clip=True, batched=True)
            sdt = self.get_strip_model()(image)[..., 0]
            mask = utils.largest_component(sdt < float(border), connectivity, batched=True)
            return utils.fill_holes(mask, connectivity, batched=True)

    def save(self, path):
        """unet weights + constructor arguments (npz), reloadable with SynthStrip.load"""
        cfg = json.dumps({'class_name': 'SynthStrip', 'config': self.get_config()})
        np.savez(path, __model_config__=np.array(cfg), **self.unet._npz_dict())

    @classmethod
    def load(cls, path, **kwargs):
        builder, config = load_config(path)
        if builder != 'SynthStrip':
            raise ValueError('%s was not saved from a SynthStrip model (class_name %r)' % (path, builder))
        config.update(kwargs)
        metadata = config.pop('metadata', {})
        for key in ('labels_in', 'labels_out'):               # JSON turned integer label keys into strings
            if isinstance(config.get(key), dict):
                config[key] = {(int(k) if isinstance(k, str) and k.lstrip('-').isdigit() else k): v for k, v in config[key].items()}
        model = cls(**config)
        model.metadata.update(metadata)
        model.unet.load_weights(path)
        return model
