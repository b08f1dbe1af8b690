"""
Timing of the hyper-convolution entry points (one weight set per batch entry) against what the same work costs without them.

    python tools/hyperconv_bench.py [--batch 4] [--reps 20] [--out profiles/hyperconv/hyperconv_bench.jsonl] [--shapes NAME,...]
    python tools/hyperconv_bench.py --dry          # CPU rehearsal: arguments, shapes, operation counts, float64 reference at a tiny size

For forward, input gradient and weight gradient of a 3x3x3 'same' convolution it times, with device events, per repetition, the
variants alternated inside every repetition (one process, one warm-up per shape and variant):
  (1)  the one-launch entry points: nrt_hyperconv3d_pack_weights_f32 + nrt_hyperconv3d_f32 (packing happens on every call: the kernels
       are inputs), nrt_hyperconv3d_wgrad_f32; (1n) is (1) without its pack launch
  (2)  the loop over the batch that the shared-weight entry points force: per entry nrt_conv3d_pack_weights_f32 + nrt_conv3d_f32 with
       batch 1, nrt_conv3d_wgrad_f32 with batch 1 (the flipped / transposed kernels of the input gradient are prepared outside the
       timed region, in (2)'s favour)
  (3)  the shared-weight call on the whole batch (nrt_conv3d_f32 / nrt_conv3d_wgrad_f32, packed once outside the timed region): the
       floor -- same flops, batch - 1 fewer weight sets to read, one gradient slice instead of `batch`
(2) and (3) are the yardsticks.  One JSON line per shape: median / min / max per variant in ms, the spread of (3) over its own
repetitions ((max - min) / median), the ratios (1)/(2) and (1n)/(3), whether (1) <= (2) and whether (1n) lies within (3)'s spread,
the forward's flops over the fp32 matrix-core peak, the library build id.  A time needs a GPU: without one the tool fails (--dry
measures nothing).
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurite_amd import _lib                                                                       # noqa: E402

FP32_MFMA_PEAK = 157.3e12            # MI355X, v_mfma_f32_16x16x4_f32: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz

# config 3's U-Net levels (cin -> cout at size^3) and the launch-bound end
SHAPES = {
    'l0_48to16_160': (48, 16, 160), 'l1_16to32_80': (16, 32, 80), 'l2_32to64_40': (32, 64, 40),
    'l3_32to32_20': (32, 32, 20), 'l4_32to32_10': (32, 32, 10),
}
K3 = (3, 3, 3)


def flops(batch, size, cin, cout):
    return 2.0 * batch * size ** 3 * 27 * cin * cout


def reference64(x, kern, bias):
    """float64 per-entry convolution (torch CPU), the definition every variant computes"""
    import torch.nn.functional as Fn
    outs = []
    for b in range(x.shape[0]):
        w = torch.from_numpy(kern[b]).double().permute(4, 3, 0, 1, 2)
        y = Fn.conv3d(torch.from_numpy(x[b:b + 1]).double().permute(0, 4, 1, 2, 3), w, torch.from_numpy(bias[b]).double(), padding=1)
        outs.append(y.permute(0, 2, 3, 4, 1))
    return torch.cat(outs, 0).numpy()


class Case:
    def __init__(self, dev, batch, size, cin, cout, seed=0):
        g = torch.Generator(device='cpu').manual_seed(seed)
        self.dev, self.B, self.S, self.cin, self.cout = dev, batch, [size] * 3, cin, cout
        self.x = torch.randn([batch] + self.S + [cin], generator=g).to(dev)
        self.dp = torch.randn([batch] + self.S + [cout], generator=g).to(dev)
        self.kern = (torch.randn([batch] + list(K3) + [cin, cout], generator=g) / np.sqrt(27 * cin)).to(dev)
        self.bias = (torch.randn(batch, cout, generator=g) * 0.1).to(dev)
        self.kern_t = self.kern.flip(1, 2, 3).transpose(4, 5).contiguous()                 # input-gradient kernels for (2), (3)
        lib = _lib.lib()
        self.n_f = int(lib.nrt_conv3d_packed_weight_floats(_lib.ints(K3), cin, cout))
        self.n_b = int(lib.nrt_conv3d_packed_weight_floats(_lib.ints(K3), cout, cin))
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)                    # noqa: E731
        self.out, self.dx = e([batch] + self.S + [cout]), e([batch] + self.S + [cin])
        self.pk_f, self.pk_b = e(batch * self.n_f), e(batch * self.n_b)
        self.pk1_f, self.pk1_b = e(self.n_f), e(self.n_b)
        self.gk, self.gb = e([batch] + list(K3) + [cin, cout]), e(batch, cout)
        self.st = _lib.stream_ptr(dev)
        # (3): packed once, outside the timed region
        self._pack1(self.kern[0], cin, cout, self.pk1_f)
        self._pack1(self.kern_t[0], cout, cin, self.pk1_b)

    def _pack1(self, w, cin, cout, dst):
        _lib.check(_lib.lib().nrt_conv3d_pack_weights_f32(_lib.ptr(w), _lib.ints(K3), cin, cout, _lib.ptr(dst), self.st), 'pack')

    def _conv(self, src, cin, w, packed, bias, out, batch, cout):
        _lib.check(_lib.lib().nrt_conv3d_f32(_lib.ptr(src), cin, None, 0, None, _lib.ptr(w), _lib.ptr(packed), _lib.ptr(bias),
                                             _lib.ptr(out), batch, _lib.ints(self.S), _lib.ints(K3), cout, 1, 1, 0, 0, self.st), 'conv')

    def _hyper(self, src, cin, w, packed, bias, out, cout):
        _lib.check(_lib.lib().nrt_hyperconv3d_f32(_lib.ptr(src), cin, _lib.ptr(w), _lib.ptr(packed), _lib.ptr(bias), _lib.ptr(out),
                                                  self.B, _lib.ints(self.S), _lib.ints(K3), cout, 1, 1, 0, 0, self.st), 'hyperconv')

    def _hpack(self, flip, dst):
        _lib.check(_lib.lib().nrt_hyperconv3d_pack_weights_f32(_lib.ptr(self.kern), self.B, _lib.ints(K3), self.cin, self.cout, flip,
                                                               _lib.ptr(dst), self.st), 'hyper pack')

    # ---- forward
    def fwd_1(self):
        self._hpack(0, self.pk_f)
        self._hyper(self.x, self.cin, self.kern, self.pk_f, self.bias, self.out, self.cout)

    def fwd_1n(self):
        self._hyper(self.x, self.cin, self.kern, self.pk_f, self.bias, self.out, self.cout)

    def fwd_2(self):
        for b in range(self.B):
            self._pack1(self.kern[b], self.cin, self.cout, self.pk_f[:self.n_f])
            self._conv(self.x[b], self.cin, self.kern[b], self.pk_f[:self.n_f], self.bias[b], self.out[b], 1, self.cout)

    def fwd_3(self):
        self._conv(self.x, self.cin, self.kern[0], self.pk1_f, self.bias[0], self.out, self.B, self.cout)

    # ---- input gradient
    def dgrad_1(self):
        self._hpack(1, self.pk_b)
        self._hyper(self.dp, self.cout, None, self.pk_b, None, self.dx, self.cin)

    def dgrad_1n(self):
        self._hyper(self.dp, self.cout, None, self.pk_b, None, self.dx, self.cin)

    def dgrad_2(self):
        for b in range(self.B):
            self._pack1(self.kern_t[b], self.cout, self.cin, self.pk_b[:self.n_b])
            self._conv(self.dp[b], self.cout, self.kern_t[b], self.pk_b[:self.n_b], None, self.dx[b], 1, self.cin)

    def dgrad_3(self):
        self._conv(self.dp, self.cout, self.kern_t[0], self.pk1_b, None, self.dx, self.B, self.cin)

    # ---- weight gradient (the zero-fill of the outputs is part of every variant: the entry points accumulate)
    def wgrad_1(self):
        self.gk.zero_(); self.gb.zero_()
        _lib.check(_lib.lib().nrt_hyperconv3d_wgrad_f32(_lib.ptr(self.x), _lib.ptr(self.dp), _lib.ptr(self.gk), _lib.ptr(self.gb), self.B,
                                                        _lib.ints(self.S), self.cin, self.cout, _lib.ints(K3), 1, self.st), 'hyper wgrad')

    wgrad_1n = wgrad_1                                                                     # no pack in the weight gradient

    def wgrad_2(self):
        self.gk.zero_(); self.gb.zero_()
        for b in range(self.B):
            _lib.check(_lib.lib().nrt_conv3d_wgrad_f32(_lib.ptr(self.x[b]), _lib.ptr(self.dp[b]), _lib.ptr(self.gk[b]), _lib.ptr(self.gb[b]),
                                                       1, _lib.ints(self.S), self.cin, self.cout, _lib.ints(K3), 1, self.st), 'wgrad')

    def wgrad_3(self):
        self.gk[0].zero_(); self.gb[0].zero_()
        _lib.check(_lib.lib().nrt_conv3d_wgrad_f32(_lib.ptr(self.x), _lib.ptr(self.dp), _lib.ptr(self.gk[0]), _lib.ptr(self.gb[0]), self.B,
                                                   _lib.ints(self.S), self.cin, self.cout, _lib.ints(K3), 1, self.st), 'wgrad')


def time_alternating(fns, reps, warm=3):
    """fns: {name: callable}; every repetition runs each variant once, each between its own pair of device events"""
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
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def summarise(times):
    out = {}
    for k, v in times.items():
        v = sorted(v)
        out[k] = {'median_ms': float(np.median(v)), 'min_ms': v[0], 'max_ms': v[-1]}
    return out


def check_small(dev):
    """the three variants compute the definition (float64, per entry) at a tiny size; (1) and (2) agree bit for bit"""
    c = Case(dev, 3, 12, 16, 16, seed=1)
    want = reference64(c.x.cpu().numpy(), c.kern.cpu().numpy(), c.bias.cpu().numpy())
    c.fwd_1()
    a = c.out.clone()
    c.fwd_2()
    b = c.out.clone()
    torch.cuda.synchronize()
    err = float(np.abs(a.cpu().numpy() - want).max() / np.abs(want).max())
    if err > 1e-5 or not torch.equal(a, b):
        raise SystemExit('hyperconv_bench: variants disagree at the check size (err %.3g, bit-equal %s)' % (err, torch.equal(a, b)))
    return err


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'hyperconv', 'hyperconv_bench.jsonl'))
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--dry', action='store_true')
    a = ap.parse_args()
    if a.reps < 20 and not a.dry:
        ap.error('--reps must be at least 20')
    names = [n for n in a.shapes.split(',') if n]
    for n in names:
        if n not in SHAPES:
            ap.error('unknown shape %r (known: %s)' % (n, ', '.join(SHAPES)))
    if a.dry:
        rng = np.random.default_rng(0)
        x = rng.standard_normal((2, 5, 6, 7, 4)).astype(np.float32)
        k = rng.standard_normal((2, 3, 3, 3, 4, 3)).astype(np.float32)
        b = rng.standard_normal((2, 3)).astype(np.float32)
        y = reference64(x, k, b)
        assert y.shape == (2, 5, 6, 7, 3)
        for n in names:
            cin, cout, size = SHAPES[n]
            print(json.dumps({'dry': True, 'shape': n, 'batch': a.batch, 'cin': cin, 'cout': cout, 'size': size,
                              'gflop_per_pass': flops(a.batch, size, cin, cout) / 1e9,
                              'activation_MB': a.batch * size ** 3 * (cin + cout) * 4 / 1e6,
                              'weight_set_KB': 27 * cin * cout * 4 / 1e3, 'time': 'not measured'}))
        return
    if not torch.cuda.is_available():
        raise SystemExit('hyperconv_bench: no GPU -- a time cannot be produced here (use --dry for a rehearsal)')
    dev = torch.device('cuda:0')
    _lib.require_device(torch.empty(1, device=dev))
    build_id = _lib.lib().nrt_build_id().decode()
    check_err = check_small(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for n in names:
            cin, cout, size = SHAPES[n]
            c = Case(dev, a.batch, size, cin, cout)
            rec = {'shape': n, 'batch': a.batch, 'cin': cin, 'cout': cout, 'size': size, 'reps': a.reps, 'build_id': build_id,
                   'check_rel_err': check_err, 'gflop_per_pass': flops(a.batch, size, cin, cout) / 1e9}
            for op in ('fwd', 'dgrad', 'wgrad'):
                keys = ['1', '1n', '2', '3'] if op != 'wgrad' else ['1', '2', '3']
                t = summarise(time_alternating({k: getattr(c, '%s_%s' % (op, k)) for k in keys}, a.reps))
                if op == 'wgrad':
                    t['1n'] = t['1']
                spread3 = (t['3']['max_ms'] - t['3']['min_ms']) / t['3']['median_ms']
                rec[op] = {
                    'ms': t, 'spread_3': spread3,
                    'ratio_1_over_2': t['1']['median_ms'] / t['2']['median_ms'],
                    'ratio_1n_over_3': t['1n']['median_ms'] / t['3']['median_ms'],
                    'not_slower_than_loop': t['1']['median_ms'] <= t['2']['median_ms'],
                    'within_spread_of_3': t['1n']['median_ms'] - t['3']['median_ms'] <= t['3']['max_ms'] - t['3']['min_ms'],
                    'share_of_fp32_mfma_peak_1n': flops(a.batch, size, cin, cout) / (t['1n']['median_ms'] * 1e-3) / FP32_MFMA_PEAK,
                }
            line = json.dumps(rec)
            print(line)
            f.write(line + '\n')
            f.flush()
            del c
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
