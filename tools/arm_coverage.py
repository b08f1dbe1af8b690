"""Which template instances of the U-Net head and glue kernels (or, --families warp_bwd, of the warp backward; --families
conv_wgrad, of the conv weight gradient; --families conv_fwd, of the conv forward) did a traced run never launch?

    hipcc <build.FLAGS> --cuda-device-only -S neurite_amd/csrc/conv.hip -o conv.s          (the same for conv_bwd.hip)
    python tools/kernel_digest.py conv.s > conv_kernels.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d out -o arms -- python -m pytest tests/test_gpu_dispatch_arms.py ...
    python tools/arm_coverage.py --kernels conv_kernels.txt conv_bwd_kernels.txt --stats out/arms_kernel_stats.csv

The kernel tables (tools/kernel_digest.py) list every instance the compiler emitted; the stats file lists every kernel that ran,
with its number of launches.  Prints one line per instance of the families below that the run never launched -- nothing when
every arm ran -- and exits 1 if there is one.  --all lists the launched instances with their launch counts too.

--families warp_bwd checks the dispatch arms of nrt_interpn_bwd_f32 and nrt_interpn_nearest_bwd_f32 instead (csrc/backward.hip,
tests/test_gpu_warp_backward_arms.py; kernel table profiles/dispatch_arms/backward_kernels.txt).

--families conv_wgrad checks the weight-gradient kernels of csrc/conv_bwd.hip (tests/test_gpu_conv_wgrad_arms.py; kernel table
profiles/dispatch_arms/conv_bwd_kernels.txt).  Instances that no call within the contract can launch are named by --unreachable
REGEX (default for this family: the six per-parity-group folded instances conv3d_wgrad<NA,NB,3,2,false>, see
profiles/dispatch_arms/README.md): they are listed as such and do not count towards the exit status -- unless the run DID launch
one, which is reported and exits 1.

--families conv_fwd checks the convolution forward kernels of csrc/conv.hip, conv_p27.h and conv_up2.h with space_to_depth2 and the
weight-pack kernels (tests/test_gpu_conv_fwd_arms.py; kernel table profiles/dispatch_arms/conv_kernels.txt).  Every instance is
reachable.

--families lc3d checks the LocallyConnected3D kernels of csrc/lc3d.hip and pad3d_rows (tests/test_gpu_lc3d_arms.py; kernel table
profiles/dispatch_arms/lc3d_kernels.txt).  The four bfloat16 lc3d_fwd_mfma<..., NPC = 2> instances are unreachable.

--families conv_bf16 checks the bfloat16 inference kernels of csrc/conv_bf16.hip (tests/test_gpu_conv_bf16_arms.py; kernel table
profiles/dispatch_arms/conv_bf16_kernels.txt): 17 instances, every one reachable.

--families warp_fwd checks the warp forward kernels of csrc/interpn.hip, interpn_lean.hip and interpn_any.hip
(tests/test_gpu_warp_forward_arms.py; kernel tables profiles/dispatch_arms/interpn_kernels.txt, interpn_lean_kernels.txt and
interpn_any_kernels.txt): 210 instances.  The 18 instances interpn_lean<C, VPL, ABSOLUTE | SHIFT> are unreachable.

--families dice checks the Dice reductions of csrc/dice.hip and csrc/dice_reduce.h, --families cce the weighted cross-entropy of
csrc/cce.hip (tests/test_gpu_dice_cce_arms.py; kernel tables profiles/dispatch_arms/dice_kernels.txt and cce_kernels.txt): 107 and 60
instances, every one reachable.

--families warp_dice checks the fused warp + soft Dice forward of csrc/fused.hip and csrc/fused_wc.h (tests/test_gpu_warp_dice_arms.py;
kernel table profiles/dispatch_arms/fused_kernels.txt): 168 warp_dice_tile, 144 warp_dice_tile_pad and 60 warp_dice_wc instances.  96
are unreachable: the 78 with STORE = true on bfloat16 storage and the other 18 of warp_dice_tile_pad<2, ...>.
"""
import argparse
import csv
import re
import subprocess
import sys

# the dispatchers of nrt_conv1x1_softmax_f32, nrt_softmax_lastdim_f32, nrt_softmax_bwd_f32, nrt_conv3d_wgrad2_f32 (its two
# streaming arms), the single-channel arms of nrt_conv3d_f32 with shared weights and without the folded pooling, and the
# element-wise / pooling / batch-norm kernels
FAMILIES = [r'conv1x1_rows<\d+,\d+>', r'conv1x1_vec<\d+,0>', r'conv1x1_softmax<\d+>', r'softmax_lastdim', r'softmax_lastdim_vec<\d+>',
            r'softmax_bwd', r'softmax_bwd_vec<\d+>', r'conv1x1_wgrad16<\d+>', r'conv3d_c1_wgrad<\d+>', r'conv3d_c1_mfma<\d+,false,false>',
            r'conv3d_c1_vec<\d+,false>', r'act_bwd', r'act_bwd_tail', r'maxpool_bwd', r'add_act_affine', r'add_act_affine_v4',
            r'channel_sums', r'channel_axpby']
# the dispatchers of nrt_interpn_bwd_f32 and nrt_interpn_nearest_bwd_f32 (the x-march kernels interpn_bwd_vol_sort and warp_dice_bwd_xm
# are the benchmark path and have their own tests)
WARP_BWD_FAMILIES = [r'interpn_bwd_rows<\d+,\d+>', r'interpn_bwd_generic<\d+,\d+>', r'interpn_bwd_vol_elems<\d+,\d+>',
                     r'interpn_bwd_vol_sort_any<\d+>', r'interpn_nearest_bwd<\d+,\d+>']
# the dispatchers of nrt_conv3d_wgrad2_f32 / nrt_conv3d_wgrad_f32, nrt_hyperconv3d_wgrad_f32, nrt_conv3d_wgrad_s2d_f32 and
# nrt_upsample_sum_f32 (the two streaming arms are in FAMILIES as well: here they make the weight-gradient table whole)
CONV_WGRAD_FAMILIES = [r'conv3d_wgrad<\d+,\d+,\d+,\d+,(?:false|true)>', r'conv3d_wgrad_fold<\d+>', r'upsample_sum', r'conv1x1_wgrad16<\d+>',
                       r'conv3d_c1_wgrad<\d+>']
# the dispatchers of nrt_conv3d_f32 / nrt_conv3d_pad_f32, nrt_hyperconv3d_f32 / nrt_hyperconv3d_pad_f32, nrt_conv3d_pool_f32, nrt_conv3d_up2_f32
# and nrt_conv3d_s2d_taps_f32, with nrt_space_to_depth2_f32 and the four weight-pack kernels their tests go through (the head forms
# conv3d_up2_mfma<1,1> and <1,2> and the single-channel first-layer kernels have their own tests and are outside this family)
CONV_FWD_FAMILIES = [r'conv3d_mfma<\d+,(?:false|true),(?:false|true),(?:false|true)>', r'conv3d_p27_mfma<\d+,(?:false|true),(?:false|true)>',
                     r'conv3d_up2_mfma<\d+,0>', r'conv3d_mfma_k2<\d+>', r'conv3d_direct<(?:false|true)>', r'space_to_depth2',
                     r'conv3d_pack_weights', r'conv3d_pack_weights_batched<(?:false|true)>', r'conv3d_pack_weights_up2']
# the dispatchers of nrt_lc3d_f, nrt_lc3d_bwd_f and nrt_pad3d (csrc/lc3d.hip): the whole translation unit but nrt_zero_words
_T = r'(?:float|unsignedshort)'
LC3D_FAMILIES = [r'lc3d_fwd<%s,\d+,\d+,(?:false|true),\d+>' % _T, r'lc3d_bwd<%s,\d+,\d+,(?:false|true),\d+>' % _T,
                 r'lc3d_fwd_mfma<%s,\d+,\d+,\d+,\d+>' % _T, r'lc3d_fwd_mfma_blk<%s,\d+,\d+,\d+,\d+>' % _T, r'lc3d_generic<%s>' % _T,
                 r'pad3d_rows<(?:unsignedint|unsignedshort)>']
# the dispatchers of nrt_conv3d_bf16, nrt_conv3d_pack_weights_bf16, nrt_conv1x1_softmax_bf16, nrt_softmax_lastdim_bf16, nrt_maxpool3d_bf16,
# nrt_upsample_concat_bf16 and nrt_add_act_affine_bf16 (csrc/conv_bf16.hip): the whole translation unit but nrt_zero_words
CONV_BF16_FAMILIES = [r'conv3d_bf16<\d+>', r'conv3d_pack_bf16<%s>' % _T, r'conv1x1_bf16<\d+>', r'softmax_lastdim_bf16<(?:false|true)>',
                      r'maxpool3d_bf16<\d+>', r'upsample_concat_bf16<\d+>', r'add_act_affine_bf16<\d+>']
# the dispatchers of nrt_interpn_f32_ex / nrt_interpn_f32, nrt_interpn_add_f32, nrt_interpn_nearest_i32 and nrt_interpn_any (the wave-cache
# kernel of variant 10 and the fused warp + Dice kernels live in other translation units and have their own tests)
_A = r'(?:float|double|HalfTag|Bf16Tag)'
WARP_FWD_FAMILIES = [r'interpn_generic<\d+,\d+,\d+,(?:float|int)>', r'interpn_rows<\d+,\d+,\d+>', r'interpn_tile<\d+,\d+>',
                     r'interpn_zrun_c32<\d+,\d+,\d+>', r'interpn_lean_tile<\d+,\d+,\d+>', r'interpn_lean<\d+,\d+,\d+>',
                     r'interpn_any_nd<%s,(?:false|true),\d+,\d+>' % _A, r'interpn_any<%s,(?:false|true)>' % _A, r'interpn_any_nearest_i32']
# the dispatchers of nrt_dice_soft / nrt_dice_soft_f32 / nrt_sqdiff_sums_f32, nrt_dice_hard_prob / _f32 / _minmax_f32, nrt_dice_hard_label_i32,
# nrt_dice_from_sums_f32 and nrt_dice_mean_pair_f32 / nrt_dice_mean_f32 (csrc/dice.hip with the second stage of csrc/dice_reduce.h): the
# whole translation unit but nrt_zero_words
_ST = r'(?:float|DiceBf16|_Float16)'
DICE_FAMILIES = [r'dice_soft_vec<\d+,(?:false|true),%s>' % _ST, r'dice_soft_generic<(?:false|true),%s>' % _ST,
                 r'dice_hard_vec<\d+,(?:false|true),%s>' % _ST, r'dice_hard_prob_generic<%s>' % _ST, r'dice_hard_prob_direct<%s>' % _ST,
                 r'dice_hard_label<(?:false|true)>', r'dice_hard_label_private', r'reduce_rows<(?:float,double|unsignedint,longlong)>',
                 r'dice_soft_finalize', r'dice_counts_reduce', r'dice_from_counts', r'dice_from_sums', r'dice_mean_pair', r'minmax_rows']
# the dispatcher of nrt_wcce / nrt_wcce_mean (csrc/cce.hip): the whole translation unit but nrt_zero_words
CCE_FAMILIES = [r'wcce_vec<\d+,%s,(?:false|true),(?:false|true)>' % _T, r'wcce_generic<%s,(?:false|true)>' % _T]
# the dispatchers of nrt_warp_dice_soft_f32 / nrt_warp_dice_soft_bf16 (csrc/fused.hip, csrc/fused_wc.h) and, for the wave-cache kernel without
# its Dice half, of nrt_interpn_f32_ex variant 10 (the backward warp_dice_wc_bwd is another family)
_B = r'(?:false|true)'
WARP_DICE_FAMILIES = [r'warp_dice_tile<\d+,\d+,%s,\d+,%s>' % (_B, _T), r'warp_dice_tile_pad<\d+,\d+,%s,\d+,%s>' % (_B, _T),
                      r'warp_dice_wc<\d+,%s,%s,%s,%s,%s>' % (_B, _B, _B, _B, _B)]
FAMILY_SETS = {'conv': FAMILIES, 'warp_dice': WARP_DICE_FAMILIES, 'dice': DICE_FAMILIES, 'cce': CCE_FAMILIES, 'warp_bwd': WARP_BWD_FAMILIES, 'conv_wgrad': CONV_WGRAD_FAMILIES, 'conv_fwd': CONV_FWD_FAMILIES,
               'lc3d': LC3D_FAMILIES, 'conv_bf16': CONV_BF16_FAMILIES, 'warp_fwd': WARP_FWD_FAMILIES}
# instances no contract-conforming call can launch: the per-parity-group folded form is only taken when a pointer is not 16-byte
# aligned, which include/neurite_amd.h rules out; a bfloat16 patch the matrix-core forward accepts has at most 56 16-byte pieces, so
# its two-pieces-per-lane form (NPC = 2, more than 64) never runs; nrt_lean_launch sends every call with per-voxel locations (ABSOLUTE = 0,
# SHIFT = 1) to interpn_lean_tile, so the row form interpn_lean only runs in LINSPACE mode; nrt_warp_dice_soft_bf16 has no `warped`
# parameter and the implementation refuses `warped` for 16-bit storage, so STORE = true never meets unsigned short, and fused_group
# gives G = 2 for 8 labels only, which is no padded count, so warp_dice_tile_pad<2, ...> is never chosen (profiles/dispatch_arms/README.md)
UNREACHABLE = {'warp_dice': [r'warp_dice_tile(?:_pad)?<\d+,\d+,true,\d+,unsignedshort>', r'warp_dice_tile_pad<2,.*>'], 'conv': [], 'warp_bwd': [], 'conv_wgrad': [r'conv3d_wgrad<\d+,\d+,3,2,false>'], 'conv_fwd': [],
               'lc3d': [r'lc3d_fwd_mfma<unsignedshort,\d+,\d+,\d+,2>'], 'conv_bf16': [], 'dice': [], 'cce': [], 'warp_fwd': [r'interpn_lean<\d+,\d+,[01]>']}
FAMILY = re.compile('^(?:%s)$' % '|'.join(FAMILIES))


def norm(name):
    """`void (anonymous namespace)::f<1, 2>(args)` and `f<1, 2>` -> `f<1,2>`"""
    name = name.strip().strip('"')
    if name.endswith('.kd'):
        name = name[:-3]
    name = name.replace('(anonymous namespace)::', '')
    name = re.sub(r'^void\s+', '', name)
    depth = 0
    for i, ch in enumerate(name):                 # cut the argument list: the first '(' outside the template brackets
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            name = name[:i]
            break
    return name.replace(' ', '')


def instances(paths):
    found = set()
    for p in paths:
        for ln in open(p):
            m = re.match(r'(.*?)\s+v\d+\s+s\d+\s+spill\d+', ln)
            if m and FAMILY.match(norm(m.group(1))):
                found.add(norm(m.group(1)))
    return sorted(found)


def demangle(name):
    """a name the profiler left mangled: instances over _Float16 (DF16_, which neither it nor an older c++filt knows; Dh, the same builtin
    type before clang 15, prints as `half` -- tools/kernel_digest.py does the same)"""
    out = subprocess.run(['c++filt', name.replace('DF16_', 'Dh')], capture_output=True, text=True).stdout.strip()
    return re.sub(r'\bhalf\b', '_Float16', out) if 'DF16_' in name else out


def launches(path):
    calls = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            n = norm(demangle(row['Name']) if row['Name'].startswith('_Z') else row['Name'])
            calls[n] = calls.get(n, 0) + int(row['Calls'])
    return calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--kernels', nargs='+', required=True, help='tables written by tools/kernel_digest.py')
    ap.add_argument('--stats', required=True, help='kernel stats CSV of a rocprofv3 --kernel-trace --stats run')
    ap.add_argument('--all', action='store_true', help='list the launched instances and their launch counts as well')
    ap.add_argument('--families', choices=sorted(FAMILY_SETS), default='conv', help='which dispatchers (default: the head and glue kernels)')
    ap.add_argument('--unreachable', nargs='*', default=None, metavar='REGEX',
                    help='instances no call within the contract can launch (default: those documented for the family)')
    args = ap.parse_args()
    global FAMILY
    FAMILY = re.compile('^(?:%s)$' % '|'.join(FAMILY_SETS[args.families]))
    inst, calls = instances(args.kernels), launches(args.stats)
    if not inst:
        raise SystemExit('no instance of the families in %s' % ', '.join(args.kernels))
    unreachable = re.compile('^(?:%s)$' % '|'.join((UNREACHABLE[args.families] if args.unreachable is None else args.unreachable) or ['(?!)']))
    expected = [k for k in inst if unreachable.match(k)]
    missing = [k for k in inst if not calls.get(k) and k not in expected]
    surprise = [k for k in expected if calls.get(k)]
    if args.all:
        for k in inst:
            if calls.get(k):
                print('%8d launches  %s' % (calls[k], k))
    for k in missing:
        print('never launched: %s' % k)
    for k in expected:
        if k in surprise:
            print('launched although named unreachable: %s' % k)
        else:
            print('never launched (unreachable within the contract): %s' % k)
    if args.all:
        print('%d instances, %d never launched%s' % (len(inst), len(missing) + len(expected) - len(surprise),
                                                    ', %d of them unreachable within the contract' % (len(expected) - len(surprise)) if expected else ''))
    return 1 if missing or surprise else 0


if __name__ == '__main__':
    sys.exit(main())
