#!/usr/bin/env python3
"""CPU model of a wave-private, direct-mapped LDS row cache for the 32-channel linear gather (no GPU needed).

A wave handles 8 output voxels per pass (a px x py x pz patch) and marches along x; each voxel needs the 8 corner rows of
floor(loc).  The model counts, on the BENCH field (synth.smooth_displacement, sigma 3), per voxel:
  distinct  rows a pass needs after de-duplication inside the pass (what per-pass de-duplication alone would fetch)
  fetched   rows that miss in the wave's cache (direct-mapped, `slots` rows, hash of the low bits of the row coordinates)
  orphans   corner references whose slot is claimed by a different row of the SAME pass (they bypass the cache)
    python tools/wc_sim.py [--waves 400] [--hist] [--exchange]

--exchange: the claim rule of fused_wc.h since the tag exchange instead of "every distinct row that misses stores its
tag, the last store wins": the 64 references of a pass, one per lane, swap their row id into tags[slot] one after the other and read the
word back.  miss = the id that came back differs, orphan = the id read afterwards differs, loader = miss and not orphan -- so the
sequence r1, r2, r1 in one slot makes BOTH r1 lanes loaders (`dup_loaders`: fetched twice, same bytes to the same LDS row).  The order of
the lanes inside an exchange is the hardware's: every figure is given with the lowest and with the highest lane first.  A pass with more
than 16 orphans forgets the cache and fetches its 64 references as they are (the kernel's fallback).
"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurite_amd import synth        # noqa: E402

S = 160
nw = int(sys.argv[sys.argv.index('--waves') + 1]) if '--waves' in sys.argv else 300
trf = synth.smooth_displacement(102, S).numpy()
grid = np.stack(np.meshgrid(*[np.arange(S, dtype=np.float32)] * 3, indexing='ij'), -1)
loc = grid + trf
mx = np.float32(S - 1)
l0 = np.clip(np.floor(loc), 0, mx)
l1 = np.clip(l0 + 1, 0, mx)
i0 = l0.astype(np.int32)
i1 = l1.astype(np.int32)
rng = np.random.default_rng(0)


def lane_refs(x0, y0, z0, patch):
    """the (voxel, corner) references of a pass in LANE order: lane = 8 g + p, voxel g (z offsets 0, 2, 3, 1 inside a row of four, as the
    kernel deals them), corner p = 4 cx + 2 cy + cz"""
    px, py, pz = patch
    zo = (0, 2, 3, 1) if pz == 4 else tuple(range(pz))
    rows = []
    for (x, y, z) in [(x0 + a, y0 + b, z0 + c) for a in range(px) for b in range(py) for c in zo]:
        for cx, cy, cz in itertools.product((0, 1), repeat=3):
            rows.append((int((i1 if cx else i0)[x, y, z, 0]), int((i1 if cy else i0)[x, y, z, 1]), int((i1 if cz else i0)[x, y, z, 2])))
    return rows


def exchange_pass(tags, hs, rids, lowest_first):
    """one pass of the exchange rule on the tags of a wave (updated in place) -> loaders, orphans, duplicate loaders, fallback"""
    k = len(hs)
    old = [0] * k
    for i in (range(k) if lowest_first else range(k - 1, -1, -1)):
        old[i] = tags[hs[i]]
        tags[hs[i]] = rids[i]
    orphan = [tags[hs[i]] != rids[i] for i in range(k)]
    loaders = [rids[i] for i in range(k) if old[i] != rids[i] and not orphan[i]]
    no = sum(orphan)
    if no > 16:
        tags[:] = -1
        return k, 0, 0, True
    return len(loaders), no, len(loaders) - len(set(loaders)), False


def run_exchange(patch, hbits, lowest_first, xlen=160):
    px, py, pz = patch
    bx, by, bz = hbits
    slots = 1 << (bx + by + bz)
    wrng = np.random.default_rng(0)
    tot_vox = tot_fetch = tot_orph = tot_dup = tot_fb = passes = 0
    for _ in range(nw):
        y0 = int(wrng.integers(0, S // py)) * py
        z0 = int(wrng.integers(0, S // pz)) * pz
        tags = np.full(slots, -1, np.int64)
        for x0 in range(0, xlen, px):
            rows = lane_refs(x0, y0, z0, patch)
            hs = [((r[0] & ((1 << bx) - 1)) << (by + bz)) | ((r[1] & ((1 << by) - 1)) << bz) | (r[2] & ((1 << bz) - 1)) for r in rows]
            rids = [(r[0] * S + r[1]) * S + r[2] for r in rows]
            nl, no, dup, fb = exchange_pass(tags, hs, rids, lowest_first)
            tot_vox += px * py * pz
            tot_fetch += nl
            tot_orph += no
            tot_dup += dup
            tot_fb += fb
            passes += 1
    return {'rule': 'exchange', 'first_lane': 'lowest' if lowest_first else 'highest', 'patch': patch, 'hash_bits': hbits, 'slots': slots,
            'fetched_per_voxel': round(tot_fetch / tot_vox, 3), 'orphan_refs_per_voxel': round(tot_orph / tot_vox, 3),
            'dup_loaders_per_pass': round(tot_dup / passes, 4), 'fallback_passes': tot_fb, 'passes': passes}


def run(patch, hbits, xlen=160):
    px, py, pz = patch
    bx, by, bz = hbits
    slots = 1 << (bx + by + bz)
    tot_vox = tot_distinct = tot_fetch = tot_orph = 0
    for _ in range(nw):
        y0 = int(rng.integers(0, S // py)) * py
        z0 = int(rng.integers(0, S // pz)) * pz
        tags = np.full(slots, -1, np.int64)
        for x0 in range(0, xlen, px):
            vs = [(x0 + a, y0 + b, z0 + c) for a in range(px) for b in range(py) for c in range(pz)]
            rows = []
            for (x, y, z) in vs:
                for cx, cy, cz in itertools.product((0, 1), repeat=3):
                    ix = (i1 if cx else i0)[x, y, z, 0]
                    iy = (i1 if cy else i0)[x, y, z, 1]
                    iz = (i1 if cz else i0)[x, y, z, 2]
                    rows.append((int(ix), int(iy), int(iz)))
            uniq = set(rows)
            tot_vox += len(vs)
            tot_distinct += len(uniq)
            # phase 1: every distinct row that misses writes its tag; the LAST writer of a slot wins (any fixed order will do)
            claim = {}
            for r in sorted(uniq):
                h = ((r[0] & ((1 << bx) - 1)) << (by + bz)) | ((r[1] & ((1 << by) - 1)) << bz) | (r[2] & ((1 << bz) - 1))
                rid = (r[0] * S + r[1]) * S + r[2]
                if tags[h] != rid:
                    claim[h] = rid
            for h, rid in claim.items():
                tags[h] = rid
                tot_fetch += 1
            # phase 2: a reference whose slot now holds another row is an orphan (fetched past the cache)
            for r in rows:
                h = ((r[0] & ((1 << bx) - 1)) << (by + bz)) | ((r[1] & ((1 << by) - 1)) << bz) | (r[2] & ((1 << bz) - 1))
                rid = (r[0] * S + r[1]) * S + r[2]
                if tags[h] != rid:
                    tot_orph += 1
    return {'patch': patch, 'hash_bits': hbits, 'slots': slots, 'distinct_per_voxel': round(tot_distinct / tot_vox, 3),
            'fetched_per_voxel': round(tot_fetch / tot_vox, 3), 'orphan_refs_per_voxel': round(tot_orph / tot_vox, 3)}


import ast
cases = ast.literal_eval(os.environ.get('WC_CASES', '[((1,2,4),(2,2,3))]'))
EXCHANGE = '--exchange' in sys.argv
for patch, hb in cases:
    if EXCHANGE:
        for lowest_first in (True, False):
            print(json.dumps(run_exchange(tuple(patch), tuple(hb), lowest_first)), flush=True)
    else:
        print(json.dumps(run(tuple(patch), tuple(hb))), flush=True)


def histogram(patch=(1, 2, 4), hbits=(2, 2, 3), waves=60, exchange=False, lowest_first=True):
    """distribution of the fetch-list length n = loaders + orphans per pass (what the kernel's rare paths see); exchange: under the
    exchange rule (a fallback pass counts n = 64), with the duplicate loaders it fetches"""
    px, py, pz = patch
    bx, by, bz = hbits
    slots = 1 << (bx + by + bz)
    ns, orph = [], []
    dups = fbs = 0
    hrng = np.random.default_rng(1) if exchange else rng      # (both lane orders over the same waves)
    for _ in range(waves):
        y0 = int(hrng.integers(0, S // py)) * py
        z0 = int(hrng.integers(0, S // pz)) * pz
        tags = np.full(slots, -1, np.int64)
        for x0 in range(0, S, px):
            if exchange:
                rows = lane_refs(x0, y0, z0, patch)
                hs = [((r[0] & ((1 << bx) - 1)) << (by + bz)) | ((r[1] & ((1 << by) - 1)) << bz) | (r[2] & ((1 << bz) - 1)) for r in rows]
                rids = [(r[0] * S + r[1]) * S + r[2] for r in rows]
                nl, no, dup, fb = exchange_pass(tags, hs, rids, lowest_first)
                ns.append(nl + no)
                orph.append(17 if fb else no)
                dups += dup
                fbs += fb
                continue
            rows = []
            for (x, y, z) in [(x0 + a, y0 + b, z0 + c) for a in range(px) for b in range(py) for c in range(pz)]:
                for cx, cy, cz in itertools.product((0, 1), repeat=3):
                    rows.append((int((i1 if cx else i0)[x, y, z, 0]), int((i1 if cy else i0)[x, y, z, 1]), int((i1 if cz else i0)[x, y, z, 2])))
            hs = [((r[0] & ((1 << bx) - 1)) << (by + bz)) | ((r[1] & ((1 << by) - 1)) << bz) | (r[2] & ((1 << bz) - 1)) for r in rows]
            rids = [(r[0] * S + r[1]) * S + r[2] for r in rows]
            claim = {}
            for h, rid in zip(hs, rids):
                if tags[h] != rid:
                    claim[h] = rid                      # last writer wins
            for h, rid in claim.items():
                tags[h] = rid
            no = sum(1 for h, rid in zip(hs, rids) if tags[h] != rid)
            ns.append(len(claim) + no)
            orph.append(no)
    ns, orph = np.array(ns), np.array(orph)
    extra = {'rule': 'exchange', 'first_lane': 'lowest' if lowest_first else 'highest', 'dup_loaders_per_pass': round(dups / ns.size, 4),
             'fallback_passes': fbs} if exchange else {}
    return {**extra, 'mean_n': float(ns.mean()), 'p_n_gt16': float((ns > 16).mean()), 'p_n_gt24': float((ns > 24).mean()), 'p_n_gt32': float((ns > 32).mean()),
            'p_n_gt40': float((ns > 40).mean()), 'p_orph_gt8': float((orph > 8).mean()), 'p_orph_gt16': float((orph > 16).mean()), 'max_n': int(ns.max()),
            'p_groups_of_8': [round(float(x), 4) for x in np.bincount(-(-ns // 8), minlength=9) / ns.size]}    # P(ceil(n / 8) = 0 .. 8)


if '--hist' in sys.argv:
    if EXCHANGE:
        for lowest_first in (True, False):
            print(json.dumps(histogram(exchange=True, lowest_first=lowest_first)))
    else:
        print(json.dumps(histogram()))
