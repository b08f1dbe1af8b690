"""ConvNet forward / training-step times where the host side shows: the config-3 forward of tools/unet_small.py, timed, and 16^3 nets
(float32, bf16, return_tensors, training with and without batch norm + residuals + dropout) whose kernels are a few microseconds each.
Device events per call, median / min / max.  One JSON line.

    python tools/convnet_host_bench.py [TREE]      # TREE: root of another checkout to import neurite_amd from (NEURITE_AMD_LIB: its library)
"""
import contextlib, io, json, os, sys, warnings
root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
import numpy as np
import torch
import neurite_amd as ne
assert os.path.abspath(ne.__file__).startswith(root), ne.__file__
dev = torch.device('cuda:0')


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return {'median': round(float(np.median(out)), 4), 'min': round(float(np.min(out)), 4), 'max': round(float(np.max(out)), 4)}


res = {'models_lines': sum(1 for _ in open(os.path.join(root, 'neurite_amd', 'models.py')))}
with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
    warnings.simplefilter('ignore')
    torch.manual_seed(0)
    net = ne.models.unet(16, (160, 160, 160, 1), 3, 3, 32, feat_mult=2).to(dev)
    small = ne.models.unet(4, (16, 16, 16, 1), 2, 3, 4, feat_mult=2).to(dev)
    small_res = ne.models.unet(4, (16, 16, 16, 4), 2, 3, 4, feat_mult=2, batch_norm=-1, use_residuals=True, conv_dropout=0.25,
                               nb_conv_per_level=2).to(dev)
x = torch.randn(1, 160, 160, 160, 1, device=dev)
res['unet_small.py config (cfg3 fwd f32)'] = timed(lambda: net(x), 20, 5)
del net, x
xs = torch.randn(2, 16, 16, 16, 1, device=dev)
xr = torch.randn(2, 16, 16, 16, 4, device=dev)
res['16^3 fwd f32'] = timed(lambda: small(xs), 300, 30)
res['16^3 fwd f32 return_tensors'] = timed(lambda: small(xs, return_tensors=['unet_merge_2', 'unet_likelihood', 'unet_prediction']), 300, 30)
res['16^3 bn+res fwd f32'] = timed(lambda: small_res(xr), 300, 30)


def step(m, xs=xs):
    m.zero_grad(set_to_none=True)
    m(xs).sum().backward()


small.train(); small_res.train()
res['16^3 train fwd+bwd'] = timed(lambda: step(small), 100, 10)
res['16^3 bn+res+dropout train fwd+bwd'] = timed(lambda: step(small_res, xr), 100, 10)
small.eval(); small_res.eval()
b = small.bfloat16(); br = small_res.bfloat16()
res['16^3 fwd bf16'] = timed(lambda: b(xs), 300, 30)
res['16^3 bn+res fwd bf16'] = timed(lambda: br(xr), 300, 30)
print(json.dumps(res))
