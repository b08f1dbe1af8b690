"""SHA-256 of every result of the fused warp + Dice register kernels and their backward on seeded inputs: run once per library
(NEURITE_AMD_LIB, a fresh process each) and compare the two lists -- an edit that keeps the operation order keeps every digest.

    python tools/warp_dice_bits.py out.json            # digests of the loaded library
    python tools/warp_dice_bits.py --compare a.json b.json merged.json

Cases: random float maps (no lane multiplies zeros) and a random field at 2 x 48^3 for 4 ... 252 labels on the default schedule and
two tile shapes, with and without the warped volume, with a fill value, bf16 storage, grad wrt the field; the ragged 6 x (36, 50, 61)
shape that takes the x-march at 24 labels; synth.cfg2_batch at 48^3 and, for 24 and 32 labels, at 4 x 160^3.  32 labels run with
tune bit 30 (the register kernel instead of the wave-cache kernel).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LABELS = (4, 12, 16, 24, 28, 32, 36, 64, 100, 252)
TILES = (3 | (3 << 4) | (4 << 8), 1 | (1 << 4) | (3 << 8) | (1 << 12))
NO_WC = 1 << 30


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def run(out_path):
    import neurite_amd as ne
    from neurite_amd import synth
    dev = torch.device('cuda:0')
    res = {'library_build_id': ne._lib.lib().nrt_build_id().decode()}

    def case(key, mov, trf, fix, tune, fill=None, warped=True, grad=True):
        tune |= NO_WC if mov.shape[-1] == 32 else 0
        if warped:
            d, w, s = ne.fused.warp_dice(mov, trf, fix, fill_value=fill, return_warped=True, return_sums=True, _tune=tune)
            res[key + '/warped'] = sha(w)
            res[key + '/store/dice'], res[key + '/store/sums'] = sha(d), sha(s)
        d, s = ne.fused.warp_dice(mov, trf, fix, fill_value=fill, return_sums=True, _tune=tune)
        res[key + '/dice'], res[key + '/sums'] = sha(d), sha(s)
        if grad:
            f = trf.clone().requires_grad_()
            wl = torch.linspace(0.5, 1.5, d.numel(), device=dev).reshape(d.shape)
            (ne.fused.warp_dice(mov, f, fix, fill_value=fill, laplace_smoothing=0.1, _tune=tune) * wl).sum().backward()
            res[key + '/grad_loc'] = sha(f.grad)

    def random_maps(B, S, L, seed):
        rng = np.random.default_rng(seed)
        g = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)      # noqa: E731
        return g(rng.random((B,) + S + (L,))), g(rng.normal(0, 2.5, (B,) + S + (3,))), g(rng.random((B,) + S + (L,)))

    for L in LABELS:
        mov, trf, fix = random_maps(2, (48, 48, 48), L, 1000 + L)
        for name, tune in (('default', 0), ('tile8x8x16', TILES[0]), ('tile2x2x8z', TILES[1])):
            case('rand48/L%d/%s' % (L, name), mov, trf, fix, tune, grad=(tune == 0))
        case('rand48/L%d/default/fill' % L, mov, trf, fix, 0, fill=0.0)
        for name, tune in (('default', 0), ('tile8x8x16', TILES[0])):
            case('rand48/L%d/%s/bf16' % (L, name), mov.bfloat16(), trf, fix.bfloat16(), tune, warped=False, grad=False)
        mov, fix, trf = synth.cfg2_batch(2, 48, L, device=dev, seed0=5)
        case('cfg2_48/L%d' % L, mov, trf, fix, 0)
        case('cfg2_48/L%d/bf16' % L, mov.bfloat16(), trf, fix.bfloat16(), 0, warped=False, grad=False)
        print('L', L, flush=True)
    mov, trf, fix = random_maps(6, (36, 50, 61), 24, 78)
    case('xmarch_ragged/L24', mov, trf, fix, 0)
    case('xmarch_ragged/L24/fill', mov, trf, fix, 0, fill=0.0)
    del mov, trf, fix
    for L in (24, 32):
        mov, fix, trf = synth.cfg2_batch(4, 160, L, device=dev, seed0=1)
        case('cfg2_4x160/L%d' % L, mov, trf, fix, 0)
        del mov, fix, trf
        torch.cuda.empty_cache()
        print('160^3 L', L, flush=True)
    json.dump(res, open(out_path, 'w'), indent=1, sort_keys=True)
    print(len(res) - 1, 'digests ->', out_path)


def compare(pa, pb, out_path):
    a, b = json.load(open(pa)), json.load(open(pb))
    keys = sorted((set(a) | set(b)) - {'library_build_id'})
    bad = [k for k in keys if a.get(k) != b.get(k)]
    json.dump({'libraries': [a['library_build_id'], b['library_build_id']], 'cases': len(keys), 'mismatches': bad,
               'digests': {k: a[k] for k in keys if k not in bad}}, open(out_path, 'w'), indent=1, sort_keys=True)
    print('%d digests, %d differ' % (len(keys), len(bad)))
    for k in bad:
        print('  ', k)
    return 1 if bad or a['library_build_id'] == b['library_build_id'] else 0


if __name__ == '__main__':
    if len(sys.argv) == 5 and sys.argv[1] == '--compare':
        sys.exit(compare(*sys.argv[2:]))
    run(sys.argv[1])
