"""
Timing of the per-voxel parameter layers and the stream layers (csrc/local.hip) against the torch-eager expression of the same
math on the same tensors -- the only yardstick there is, the layers being new.

    python tools/local_layers_bench.py [--reps 30] [--out profiles/local_layers/local_layers_bench.jsonl] [--cases NAME,...]
    python tools/local_layers_bench.py --dry       # CPU rehearsal: arguments, shapes, byte counts; measures nothing

The driver starts one child process per case (`--case NAME`), each under a time limit of its own, and stops at the first child
that fails or runs out of time.  A child times, with device events, the layer's forward (nothing recorded) and its backward
(torch.autograd.grad on a graph built once) alternated with the eager forms inside every repetition after a warm-up of both, and
appends one JSON line: median / min / max in ms per variant, the algorithmic bytes of the pass (every tensor read or written
once; parameters once for the whole batch), the share of the 8 TB/s HBM peak those bytes over the median time come to, the ratio
kernel / eager and the library build id.  The outputs of the two variants are compared first (relative error in the record).
A time needs a GPU: without one the tool fails.
"""

import argparse
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurite_amd import _lib                                                                       # noqa: E402
from neurite_amd import layers as L                                                                # noqa: E402

HBM_PEAK = 8.0e12
CASE_TIMEOUT_S = 150

# name: (kind, batch, spatial shape, channels in, channels out)
CASES = {
    'param_with_input_160_c1': ('param', 4, (160, 160, 160), 1, 1),
    'param_with_input_160_c3': ('param', 4, (160, 160, 160), 3, 3),
    'mean_stream_160_c1': ('mean', 4, (160, 160, 160), 1, 1),
    'mean_stream_160_c3': ('mean', 4, (160, 160, 160), 3, 3),
    'local_linear_160_c32': ('linear', 4, (160, 160, 160), 32, 32),
    'cross_linear_64_8to8': ('cross', 4, (64, 64, 64), 8, 8),
    'cross_linear_64_1to16': ('cross', 4, (64, 64, 64), 1, 16),
    'cov_stream_v4096': ('cov', 4, (4096,), 1, 1),
}


def algorithmic_bytes(kind, B, S, cin, cout):
    """(forward, backward) bytes: every tensor of the pass once, float32"""
    V = int(np.prod(S))
    if kind == 'param':
        n = V * cin
        return 4 * (n + B * n), 4 * (B * n + n)
    if kind == 'mean':
        n = V * cin
        return 4 * (B * n + 2 * n + B * n), 4 * (2 * B * n)
    if kind == 'linear':
        n = V * cin
        return 4 * (2 * B * n + 2 * n), 4 * (3 * B * n + 3 * n)
    if kind == 'cross':
        w, xb, yb, bb = V * cin * cout, B * V * cin, B * V * cout, V * cout
        return 4 * (xb + w + bb + yb), 4 * ((yb + w + xb) + (xb + yb + w + bb))
    if kind == 'cov':
        return 4 * (2 * V * V + B * V * V + B * V), None
    raise ValueError(kind)


def build_case(kind, B, S, cin, cout, dev):
    """returns (kernel forward, eager forward, tensors to differentiate [kernel side], [eager side]); forward(grad) -> output"""
    g = torch.Generator(device='cpu').manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)                                          # noqa: E731
    if kind == 'param':
        shape = tuple(S) + (cin,)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            layer = L.LocalParamWithInput(shape, mult=2.5)
        x = rnd(B, 8, 8, 1)
        layer(x)
        k2 = layer.kernel.detach().clone().requires_grad_()

        def eager():
            e = x.flatten(1)[:, 0:1] * 0 + 1
            return (e @ (k2 * 2.5).reshape(1, -1)).reshape((B,) + shape)
        return (lambda: layer(x)), eager, [layer.kernel], [k2]
    if kind == 'mean':
        shape = tuple(S) + (cin,)
        layer = L.MeanStream(cap=100)
        layer.train()
        x = rnd(B, *shape).requires_grad_()
        x2 = x.detach().clone().requires_grad_()
        layer(x.detach())
        state = {'mean': torch.zeros(shape, device=dev), 'count': torch.zeros(1, device=dev)}
        cap = torch.tensor(100.0, device=dev)
        one = torch.tensor(1.0, device=dev)

        def eager():
            new_count = state['count'] + B
            alpha = B / torch.minimum(new_count, cap)
            new_mean = state['mean'] * (1 - alpha) + (x2.sum(0) / B) * alpha
            state['count'], state['mean'] = new_count, new_mean.detach()
            return (torch.minimum(one, new_count / cap) * new_mean).unsqueeze(0).repeat((B,) + (1,) * len(shape))
        return (lambda: layer(x)), eager, [x], [x2]
    if kind == 'linear':
        shape = tuple(S) + (cin,)
        layer = L.LocalLinear()
        x = rnd(B, *shape).requires_grad_()
        layer(x.detach())
        x2 = x.detach().clone().requires_grad_()
        m2, b2 = layer.mult.detach().clone().requires_grad_(), layer.bias.detach().clone().requires_grad_()
        return (lambda: layer(x)), (lambda: x2 * m2 + b2), [x, layer.mult, layer.bias], [x2, m2, b2]
    if kind == 'cross':
        layer = L.LocalCrossLinear(cout)
        x = rnd(B, *S, cin).requires_grad_()
        layer(x.detach())
        x2 = x.detach().clone().requires_grad_()
        V = int(np.prod(S))
        w2 = layer.mult.detach().clone().requires_grad_()
        b2 = layer.bias.detach().clone().requires_grad_()

        def eager():
            y = torch.einsum('bvc,vco->bvo', x2.reshape(B, V, cin), w2.reshape(V, cin, cout))
            return y.reshape((B,) + tuple(S) + (cout,)) + b2
        return (lambda: layer(x)), eager, [x, layer.mult, layer.bias], [x2, w2, b2]
    if kind == 'cov':
        v = int(np.prod(S))
        layer = L.CovStream(cap=100)
        layer.train()
        x = rnd(B, v) * 0.1
        layer(x)
        state = {'mean': torch.zeros(v, device=dev), 'count': torch.zeros(1, device=dev), 'cov': torch.zeros(v, v, device=dev)}
        cap = torch.tensor(100.0, device=dev)
        one = torch.tensor(1.0, device=dev)

        def eager():
            new_count = state['count'] + B
            alpha = B / torch.minimum(new_count, cap)
            new_mean = state['mean'] * (1 - alpha) + (x.sum(0) / B) * alpha
            prev_cap = torch.minimum(state['count'], cap)
            c = state['cov'] * (prev_cap - 1) + x.t() @ x
            new_cov = c / (prev_cap + B - 1)
            state['count'], state['mean'], state['cov'] = new_count, new_mean, new_cov
            return (torch.minimum(one, new_count / cap) * new_cov).unsqueeze(0).repeat(B, 1, 1)
        return (lambda: layer(x)), eager, None, None
    raise ValueError(kind)


def time_alternating(fns, reps, warm=3):
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    for r in range(reps):
        for k, f in fns.items():
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    out = {}
    for k, v in ev.items():
        t = sorted(a.elapsed_time(b) for a, b in v)
        out[k] = {'median_ms': float(np.median(t)), 'min_ms': t[0], 'max_ms': t[-1]}
    return out


def rel_err(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def run_case(name, reps, out_path):
    if not torch.cuda.is_available():
        raise SystemExit('local_layers_bench: no GPU -- a time cannot be produced here (use --dry for a rehearsal)')
    dev = torch.device('cuda:0')
    _lib.require_device(torch.empty(1, device=dev))
    kind, B, S, cin, cout = CASES[name]
    fwd_k, fwd_e, diff_k, diff_e = build_case(kind, B, S, cin, cout, dev)
    bytes_f, bytes_b = algorithmic_bytes(kind, B, S, cin, cout)
    rec = {'case': name, 'kind': kind, 'batch': B, 'shape': list(S), 'cin': cin, 'cout': cout, 'reps': reps,
           'build_id': _lib.lib().nrt_build_id().decode()}

    def fk():
        with torch.no_grad():
            return fwd_k()

    def fe():
        with torch.no_grad():
            return fwd_e()
    if kind not in ('mean', 'cov'):                        # the stream layers' two variants hold states of their own
        rec['forward_rel_diff'] = rel_err(fk(), fe())
    t = time_alternating({'kernel': fk, 'eager': fe}, reps)
    rec['forward'] = {'ms': t, 'algorithmic_MB': bytes_f / 1e6,
                      'share_of_hbm_peak_kernel': bytes_f / (t['kernel']['median_ms'] * 1e-3) / HBM_PEAK,
                      'share_of_hbm_peak_eager': bytes_f / (t['eager']['median_ms'] * 1e-3) / HBM_PEAK,
                      'kernel_over_eager': t['kernel']['median_ms'] / t['eager']['median_ms'],
                      'kernel_not_slower': t['kernel']['median_ms'] <= t['eager']['median_ms']}
    if diff_k is not None:
        yk, ye = fwd_k(), fwd_e()
        g = torch.randn(yk.shape, generator=torch.Generator(device='cpu').manual_seed(1)).to(dev)
        bk = lambda: torch.autograd.grad(yk, diff_k, g, retain_graph=True)                        # noqa: E731
        be = lambda: torch.autograd.grad(ye, diff_e, g, retain_graph=True)                        # noqa: E731
        rec['backward_rel_diff'] = max(rel_err(a, b) for a, b in zip(bk(), be()))
        t = time_alternating({'kernel': bk, 'eager': be}, reps)
        rec['backward'] = {'ms': t, 'algorithmic_MB': bytes_b / 1e6,
                           'share_of_hbm_peak_kernel': bytes_b / (t['kernel']['median_ms'] * 1e-3) / HBM_PEAK,
                           'share_of_hbm_peak_eager': bytes_b / (t['eager']['median_ms'] * 1e-3) / HBM_PEAK,
                           'kernel_over_eager': t['kernel']['median_ms'] / t['eager']['median_ms'],
                           'kernel_not_slower': t['kernel']['median_ms'] <= t['eager']['median_ms']}
    line = json.dumps(rec)
    print(line)
    with open(out_path, 'a') as f:
        f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=os.path.join('profiles', 'local_layers', 'local_layers_bench.jsonl'))
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--case', default=None, help='run this one case in this process (what the driver starts)')
    ap.add_argument('--dry', action='store_true')
    a = ap.parse_args()
    names = [a.case] if a.case else [n for n in a.cases.split(',') if n]
    for n in names:
        if n not in CASES:
            ap.error('unknown case %r (known: %s)' % (n, ', '.join(CASES)))
    if a.dry:
        for n in names:
            kind, B, S, cin, cout = CASES[n]
            bf, bb = algorithmic_bytes(kind, B, S, cin, cout)
            print(json.dumps({'dry': True, 'case': n, 'kind': kind, 'batch': B, 'shape': list(S), 'cin': cin, 'cout': cout,
                              'forward_MB': bf / 1e6, 'backward_MB': None if bb is None else bb / 1e6, 'time': 'not measured'}))
        return
    if a.reps < 20:
        ap.error('--reps must be at least 20')
    out_path = os.path.abspath(a.out)
    if a.case:
        run_case(a.case, a.reps, out_path)
        return
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, 'w').close()
    for n in names:
        cmd = [sys.executable, os.path.abspath(__file__), '--case', n, '--reps', str(a.reps), '--out', out_path]
        try:
            rc = subprocess.run(cmd, timeout=CASE_TIMEOUT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit('local_layers_bench: case %s ran out of its %d s; stopping' % (n, CASE_TIMEOUT_S))
        if rc != 0:
            raise SystemExit('local_layers_bench: case %s failed with status %d; stopping' % (n, rc))


if __name__ == '__main__':
    main()
