"""SHA-256 of what small ConvNet models compute on seeded weights and inputs, in every mode of ConvNet._interpret: run once per tree
(a fresh process each, the library held fixed with NEURITE_AMD_LIB) and compare the lists -- an edit of the host code that keeps
every launch and its arguments keeps every digest.

    python tools/convnet_bits.py out.json                       # digests of this tree (gradient values go to out.npz)
    python tools/convnet_bits.py --dry out.json                 # no device: builds every network and lists its op kinds per case
    python tools/convnet_bits.py --compare a.json b.json [--merged m.json]    # prints the keys that differ; exit 1 if there are any
    python tools/convnet_bits.py --compare a.json b.json --unstable a2.json a3.json ... [--unstable-b b2.json ...]
        a2 ...: further runs of a's tree.  The weight-gradient and channel-sum kernels accumulate with float atomics, so digests behind
        them move between runs of one tree.  An entry that differs among a, a2 ... (or among b, b2 ...) is taken out of the digest comparison and listed by
        name; a gradient among them is compared by value (out.npz) with the bound of tests/test_gpu_conv_backward.py -- or, where
        the first tree's own runs are further apart than that, with 3 x their largest distance.

Per case: the output, every tensor asked for through return_tensors and, in training mode, every parameter gradient after
out.sum().backward() (`grad/`; `grad/input_i` is the gradient of input i, which no atomic touches in a net without
BatchNormalization) and after (out * ramp).sum().backward() (`wgrad/`: a soft-max output sums to a constant), the dropout
draws (`last_dropout_scales`, `last_dropout_masks`) and the sampling noise.  `paths` records which folds the float32 networks took.
Shapes are the smallest that reach each branch: 16^3 with 4 features for the plain paths; 16 features and 16 labels where the
first layer's pooling (nrt_conv3d_c1_pool_f32: 16 or 32 filters, z a multiple of 16) and the head (nrt_conv3d_up2_head_f32: 16 or 32
labels) fold.
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL = 2e-4                                               # tests/test_gpu_conv_backward.py: max |a - b| / max |b|


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def run(out_path, dry=False):
    import neurite_amd as ne
    from neurite_amd import models as nm
    dev = torch.device('cpu' if dry else 'cuda:0')
    res = {'library_build_id': ne._lib.lib().nrt_build_id().decode()}
    values = {}

    def build(fn, *args, seed=0, **kw):
        """the network on the device: glorot kernels of the builder under `seed`, every other parameter and buffer random too"""
        torch.manual_seed(seed)
        with contextlib.redirect_stdout(sys.stderr), contextlib.redirect_stderr(open(os.devnull, 'w')):
            net = fn(*args, **kw)
        with torch.no_grad():
            for name, p in list(net.named_parameters()) + list(net.named_buffers()):
                if name.endswith('moving_variance'):
                    p.copy_(torch.rand(p.shape) + 0.5)
                elif not name.endswith('kernel') and p.is_floating_point():
                    p.copy_(torch.randn(p.shape) * 0.1 + (1.0 if name.endswith('gamma') else 0.0))
        return net.to(dev)

    def inputs(net, seed=1, batch=2):
        torch.manual_seed(seed)
        return [torch.randn((batch,) + tuple(s)).to(dev) for s in net.input_shapes]

    def case(key, net, xs, rt=None, train=False, noise=None, out_name=None):
        if dry:
            res[key] = [op['kind'] for op in net.ops]
            return
        net.train(train)
        for tag in (('grad', 'wgrad') if train else ('',)):
            torch.manual_seed(7)                                           # the dropout draws of this call
            net.zero_grad(set_to_none=True)
            xs = [x.detach().requires_grad_(train) for x in xs]
            with torch.set_grad_enabled(train):
                got = net(xs if len(xs) > 1 else xs[0], return_tensors=rt, _noise=noise)
            outs = got if isinstance(got, dict) else {'out': got}
            if tag != 'wgrad':
                for k, v in outs.items():
                    res['%s/%s' % (key, k)] = sha(v)
                for what in ('last_dropout_scales', 'last_dropout_masks', 'last_draws'):
                    for k, v in (getattr(net, what, None) or {}).items() if train or what == 'last_draws' else ():
                        res['%s/%s/%s' % (key, what, k)] = sha(v)
            if train:
                y = outs[out_name or 'out']
                w = torch.linspace(0.5, 1.5, y.numel(), device=dev).reshape(y.shape) if tag == 'wgrad' else 1.0
                (y * w).sum().backward()
                for k, p in list(net.named_parameters()) + [('input_%d' % i, x) for i, x in enumerate(xs)]:
                    if p.grad is not None:
                        name = '%s/%s/%s' % (key, tag, k)
                        res[name] = sha(p.grad)
                        values[name] = p.grad.detach().cpu().numpy()
        net.eval()

    def unet(feats=4, labels=4, shape=(16, 16, 16, 1), **kw):
        return build(nm.unet, feats, shape, 2, 3, labels, feat_mult=2, **kw)

    merge, like, pool = 'unet_merge_2', 'unet_likelihood', 'unet_maxpool_0'
    keeps = {'plain': None, 'keep_merge': [merge, 'unet_prediction'], 'keep_likelihood': [like, 'unet_prediction'],
             'keep_pool_conv': [pool, 'unet_conv_downarm_0_0', 'unet_conv_uparm_2_0', 'unet_prediction'],
             'keep_all3': [merge, like, pool, 'unet_prediction']}

    # float32 inference: the plain net (no pool or head fold at 4 features) and the net whose first pooling and head fold
    for tag, net in (('unet4', unet()), ('unet16', unet(16, 16))):
        xs = inputs(net)
        first, last = net.layers_by_name['unet_conv_downarm_0_0'], 'unet_conv_uparm_2_0'
        t = dry or net(xs[0], return_tensors=['unet_input', 'unet_conv_downarm_0_0', 'unet_conv_downarm_1_0'])
        res['paths/%s' % tag] = dry or {'pool_fold': bool(first.pool_foldable(t['unet_input'], 0)),
                                 'head_fold': bool(net._head_foldable(last, like, t['unet_conv_downarm_0_0'],
                                                                      t['unet_conv_downarm_1_0'], (2, 2, 2)))}
        for fold in (True, False):
            net.fold_head = fold
            for kname, rt in keeps.items():
                case('f32/%s/fold%d/%s' % (tag, fold, kname), net, xs, rt)
        net.fold_head = True
        # bf16 inference of the same weights
        b16 = net.bfloat16()
        for fold in (True, False):
            b16.fold_head = fold
            for kname in ('plain', 'keep_merge', 'keep_likelihood'):
                case('bf16/%s/fold%d/%s' % (tag, fold, kname), b16, xs, keeps[kname])

    # training: batch norm, residual adds, dropout; also with the merge and the logits kept
    for tag, feats, labels in (('unet4', 4, 4), ('unet16', 16, 16)):
        # (4 input channels: the residual add of a level does not broadcast a single-channel input over the level's features)
        net = unet(feats, labels, (16, 16, 16, 4), batch_norm=-1, use_residuals=True, conv_dropout=0.25, nb_conv_per_level=2)
        xs = inputs(net)
        case('train/%s_bn_res_drop' % tag, net, xs, train=True)
        case('train/%s_bn_res_drop/keep' % tag, net, xs, rt=[merge, like, 'unet_prediction'], train=True, out_name='unet_prediction')
        case('f32/%s_bn_res_drop' % tag, net, xs)
        case('bf16/%s_bn_res_drop' % tag, net.bfloat16(), xs)
    net = unet()
    case('train/unet4', net, inputs(net), train=True)

    # 2-D (lift / unlift), also with a linear prediction: a copy in inference, the logits themselves in training
    for act in ('softmax', 'linear'):
        net = unet(shape=(16, 16, 1), final_pred_activation=act)
        xs = inputs(net)
        case('f32/unet2d_%s' % act, net, xs, ['unet_merge_2', 'unet_prediction'])
        case('f32/unet2d_%s/plain' % act, net, xs)
        case('train/unet2d_%s' % act, net, xs, train=True)
        case('bf16/unet2d_%s' % act, net.bfloat16(), xs)

    # conv_dec (up-sampling without a skip), alone and with a non-fused activation
    for act in ('elu', 'tanh'):
        net = build(nm.conv_dec, 4, (4, 4, 4, 3), 3, 3, 4, name='dec', nb_conv_per_level=1, activation=act)
        xs = inputs(net)
        case('f32/conv_dec_%s' % act, net, xs)
        case('train/conv_dec_%s' % act, net, xs, train=True)
        case('bf16/conv_dec_%s' % act, net.bfloat16(), xs)

    # add_prior: log-prior + softmax, and prior x sigmoid (multiply)
    for logp in (True, False):
        net = unet(add_prior_layer=True, use_logp=logp, final_pred_activation='softmax' if logp else 'linear')
        xs = inputs(net)
        case('f32/prior_logp%d' % logp, net, xs)
        case('train/prior_logp%d' % logp, net, xs, train=True)
        case('bf16/prior_logp%d' % logp, net.bfloat16(), xs)
    base = unet()
    net = nm.add_prior(base, (16, 16, 16, 4), use_logp=False, final_pred_activation='linear')
    case('f32/add_prior_fn', net, inputs(net))

    net = build(nm.dilation_net, 4, (16, 16, 16, 1), 2, 3, 4, dilation_rate_mult=2)
    xs = inputs(net)
    case('f32/dilation_net', net, xs)
    case('train/dilation_net', net, xs, train=True)
    case('bf16/dilation_net', net.bfloat16(), xs)

    # single_ae with the noise supplied; ae as one model
    for ae_type, enc, shape in (('dense', [6], (4, 4, 4, 3)), ('conv', [2, 2, 2, 5], (4, 4, 4, 3))):
        net = build(nm.single_ae, enc, shape, ae_type=ae_type, conv_size=3, do_vae=True, include_mu_shift_layer=True, batch_norm=-1)
        xs = inputs(net)
        torch.manual_seed(3)
        noise = {'single_ae_ae_sample': torch.randn((2,) + tuple(enc)).to(dev)}
        names = [n for n in net.layer_names if n in net.layers_by_name]
        case('f32/single_ae_%s' % ae_type, net, xs, rt=names + [net.output_name], noise=noise)
        case('train/single_ae_%s' % ae_type, net, xs, train=True, noise=noise)
    net = build(nm.ae, 4, (8, 8, 8, 1), 2, 3, 4, [2, 2, 2, 3], single_model=True)
    xs = inputs(net)
    case('f32/ae_single_model', net, xs)
    case('train/ae_single_model', net, xs, train=True)

    # design_dnn / EncoderNet, with the element-wise dropout
    for final in ('dense-sigmoid', 'dense-softmax', 'myglobalmaxpooling', 'globalmaxpooling'):
        net = build(nm.design_dnn, 4, (8, 8, 8), 2, 3, 3, final_layer=final, conv_dropout=0.25, conv_maxnorm=2.0, batch_norm=-1,
                    nb_conv_per_level=1)
        xs = inputs(net)
        case('f32/design_dnn_%s' % final, net, xs)
        case('train/design_dnn_%s' % final, net, xs, train=True)
    net = build(nm.EncoderNet, 4, (8, 8, 8, 1), 2, 3, name='enc', nb_conv_per_level=1, conv_dropout=0.25, dense_size=8, nb_labels=3,
                rescale=0.5, dropout=0.25, batch_norm=-1)
    xs = inputs(net)
    case('f32/encoder_net', net, xs, rt=['dense', 'rescale_values', 'output_dense'])
    case('train/encoder_net', net, xs, train=True)

    json.dump(res, open(out_path, 'w'), indent=1, sort_keys=True)
    np.savez_compressed(os.path.splitext(out_path)[0] + '.npz', **values)
    print(len(res) - 1, 'entries ->', out_path)


def compare(pa, pb, reruns=(), reruns_b=(), out_path=None):
    """a: the first tree, b: the second, reruns / reruns_b: further runs of the first / second tree"""
    a, b = json.load(open(pa)), json.load(open(pb))
    again = [json.load(open(p)) for p in reruns]
    keys = sorted((set(a) | set(b)) - {'library_build_id'})
    again_b = [json.load(open(p)) for p in reruns_b]
    unstable = [k for k in keys if any(a.get(k) != r.get(k) for r in again) or any(b.get(k) != r.get(k) for r in again_b)]
    is_grad = lambda k: '/grad/' in k or '/wgrad/' in k                      # noqa: E731
    bad = [k for k in keys if a.get(k) != b.get(k) and k not in unstable]
    forward = [k for k in unstable if not is_grad(k)]
    by_value, over = [], []
    if unstable:
        va, vb = (np.load(os.path.splitext(p)[0] + '.npz') for p in (pa, pb))
        vr = [np.load(os.path.splitext(p)[0] + '.npz') for p in reruns]
        pass_max = {}
        for k in va.files:
            pass_max[k.rsplit('/', 1)[0]] = max(pass_max.get(k.rsplit('/', 1)[0], 0.0), float(np.abs(va[k]).max()))
        for k in unstable:
            if is_grad(k):
                if k not in vb.files:
                    bad.append(k)
                    continue
                ref = va[k].astype(np.float64)
                # the test's scale, max |g|; a gradient that cancels to zero (a bias in front of a batch norm) is rounding noise of
                # its backward pass, so not below 1e-3 of the largest gradient of that pass
                scale = max(float(np.abs(ref).max()), 1e-3 * pass_max[k.rsplit('/', 1)[0]], 1e-30)
                err = float(np.abs(vb[k] - ref).max()) / scale
                own = max([float(np.abs(v[k] - ref).max()) / scale for v in vr] or [0.0])
                by_value.append({'key': k, 'err_over_scale': err, 'largest_between_runs_of_first_tree': own, 'max_abs': scale})
                # the bound of the test where the first tree meets it itself; else 3 x its own largest deviation
                if err >= max(TOL, 3 * own):
                    over.append(k)
    print('%d entries; %d stable within each tree, of which %d differ; %d not stable within a tree (%d of them no gradients), '
          'gradients among them compared by value: %d outside' % (len(keys), len(keys) - len(unstable), len(bad), len(unstable),
                                                                  len(forward), len(over)))
    for k in bad:
        print('   differs:', k)
    for k in forward:
        print('   not stable within a tree, no gradient:', k)
    for r in by_value:
        if r['key'] in over or r['err_over_scale'] >= TOL:
            print('   by value%s: %s  %.3g (between runs of the first tree %.3g, bound %g, max |g| %.3g)'
                  % (' OUTSIDE' if r['key'] in over else '', r['key'], r['err_over_scale'], r['largest_between_runs_of_first_tree'], TOL,
                     r['max_abs']))
    if out_path:
        json.dump({'libraries': [a['library_build_id'], b['library_build_id']], 'entries': len(keys), 'mismatches': bad + over,
                   'runs_of_first_tree': 1 + len(again), 'runs_of_second_tree': 1 + len(again_b), 'not_stable_within_a_tree_forward': forward,
                   'not_stable_within_a_tree_gradients': by_value,
                   'digests': {k: a[k] for k in keys if k not in unstable and k not in bad}}, open(out_path, 'w'), indent=1, sort_keys=True)
    return 1 if bad or over else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('out', nargs='?')
    ap.add_argument('--dry', action='store_true')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--merged', metavar='FILE', help='with --compare: write the comparison here')
    ap.add_argument('--unstable', nargs='+', default=[], metavar='A2', help='further runs of the tree that wrote A')
    ap.add_argument('--unstable-b', nargs='+', default=[], metavar='B2', help='further runs of the tree that wrote B')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.unstable, args.unstable_b, args.merged))
    run(args.out, dry=args.dry)
