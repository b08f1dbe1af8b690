/*
 * neurite_amd.h -- C ABI of libneurite_amd.so, the MI355X (gfx950 / CDNA4) implementation of
 * neurite's 3-D volume hot path.
 *
 * The reference (adalca/neurite) is pure Python on TensorFlow and has no FFI of its own
 * (SURVEY.md section 8b); its boundary is a set of Python call signatures.  Each entry point below
 * replaces the TensorFlow op sequence that one reference function issues, and is what a
 * `neurite/torch/` backend (the dormant switch at neurite/__init__.py:33-42) would bind.
 * INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *  - All tensor pointers are DEVICE pointers (HIP), row-major, channels-last, exactly the
 *    reference layout [B, *spatial, C].
 *  - The spelling of a parameter says where its memory lives: `T name[]` is a HOST array that is
 *    read during the call (shapes, kernel sizes, voxel spacings, percentile positions); `T *name`
 *    is DEVICE memory or an opaque handle (`void *stream`).  The Python binding derives its
 *    argument types from these declarations (neurite_amd/_lib.py).
 *  - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *    stream), allocates nothing and never synchronises.  Scratch memory is supplied by the
 *    caller: ask nrt_*_workspace_bytes() and pass a device buffer of at least that size.
 *  - Return value: NRT_OK or a negative nrt_status; nothing throws across the ABI.
 *    nrt_status_string() describes a code.
 *  - Inputs are never written.  Pointers must be 16-byte aligned (torch allocations are).
 */
#ifndef NEURITE_AMD_H
#define NEURITE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    NRT_OK = 0,
    NRT_ERR_INVALID_ARG = -1,   /* NULL pointer, bad rank, non-positive size ...            */
    NRT_ERR_UNSUPPORTED = -2,   /* combination not implemented by the HIP path              */
    NRT_ERR_LAUNCH = -3,        /* hipLaunchKernel / hipGetLastError reported a failure     */
    NRT_ERR_WORKSPACE = -4      /* workspace missing or too small                           */
} nrt_status;

const char *nrt_status_string(int status);
/* ABI version, bumped when a signature changes. */
int nrt_abi_version(void);
/* Identity of the sources the library was built from (16 hex digits of a sha256 over flags, headers and kernels; "unknown" for a
 * build outside neurite_amd/build.py).  The reference is pure Python and has no counterpart; __graft_entry__.build() uses it to
 * refuse a shipped binary that does not match the tree. */
const char *nrt_build_id(void);
/* Name of the GPU architecture the library was compiled for ("gfx950"). */
const char *nrt_target_arch(void);
/* Library state on the CURRENT device (no reference counterpart: TensorFlow owns its runtime state, neurite/tf has none).
 * Kernels that coordinate their blocks through atomic counters (the persistent gather's work lists, the one-launch weighted
 * cross-entropy) keep them in a device-resident pool of self-cleaning slots: one slot per stream for eager launches, a slot of its own
 * for every launch recorded during stream capture (a captured graph may be replayed beside any eager work).
 *   nrt_init            resolves the pool's address; optional (the first launch does it), but call it once per device BEFORE the first
 *                       stream capture so that nothing but launches happens inside the capture.
 *   nrt_counters_reset  zero-fills the pool on `stream`: recovery after a kernel was aborted mid-flight (nothing else leaves a slot
 *                       dirty); not needed in normal operation, must not run beside launches of this library.
 *   nrt_counters_slot_index   index of the slot a launch on `stream` would use right now (-1: more streams than the pool has stream
 *                       slots); diagnostic / tests. */
int nrt_init(void);
int nrt_counters_reset(void *stream);
int nrt_counters_slot_index(void *stream);

/* ------------------------------------------------------------------------------------------
 * interpn / SpatialTransformer / Resize
 * replaces: neurite/tf/utils/utils.py:73-220 (interpn), :223-265 (resize -> interpn on a
 * linspace grid), :333-476 (identity grids), and voxelmorph's transform()/SpatialTransformer
 * (call sites neurite/tf/models.py:806-807, 1157-1159).
 * ------------------------------------------------------------------------------------------ */
typedef enum {
    NRT_LOC_ABSOLUTE = 0,  /* loc[b, q, 0:D] are sampling locations (interpn's own contract)   */
    NRT_LOC_SHIFT = 1,     /* loc[b, q, 0:D] are displacements, location = float(q_d) + loc    */
                           /* (SpatialTransformer: identity 'ij' grid never materialised)      */
    NRT_LOC_LINSPACE = 2   /* loc == NULL; location_d = tf.linspace(0, S_d-1, out_d)[q_d]      */
                           /* (resize()/Resize: align-corners grid computed in registers)      */
} nrt_loc_mode;

typedef enum { NRT_INTERP_LINEAR = 0, NRT_INTERP_NEAREST = 1 } nrt_interp_method;

/*
 * out[b, q, c] = interpn(vol[b], location(b, q))     q over out_shape, c < channels
 *   vol  [batch, vol_shape[0..ndim-1], channels]  (vol_batch_stride elements between volumes;
 *                                                  0 re-uses one volume for every b)
 *   loc  [batch, out_shape[0..ndim-1], ndim]      (loc_batch_stride elements between fields;
 *                                                  0 = single_transform)
 *   out  [batch, out_shape..., channels]           dense
 * ndim in {1,2,3}.  Linear: 2^ndim corners blended in itertools.product order with separately
 * rounded multiplies/adds (bit-identical to the reference's float32 op sequence); nearest:
 * round-half-even, pure data movement; fill: out*(!oob) + oob*fill on the UNCLIPPED location.
 */
int nrt_interpn_f32(const float *vol, const float *loc, float *out,
                    int ndim, const int vol_shape[], const int out_shape[], int channels,
                    int batch, long long vol_batch_stride, long long loc_batch_stride,
                    int loc_mode, int method, int has_fill, float fill_value, void *stream);

/* Same, selecting a specific kernel (for tuning / benchmarking).  variant:
 *   0 auto | 1 generic element-per-thread | 2 row-per-lane-group (C%4==0)
 *   3 z-run with register reuse of the shared corner rows (ndim 3, C==32; the auto choice on regular grids: NRT_LOC_LINSPACE)
 *   5 3-D tiles with a depth-2 software pipeline (C%4==0, linear)
 *   8 few-channel kernel: one voxel per lane, z corners of a row by one load (ndim 3, C<=4; the auto choice there)
 *   10 wave-private LDS row cache on the x-march schedule (ndim 3, C==32, linear; the auto choice for displacement fields and
 *      absolute locations since round 5: at least as fast as variant 3 on every field measured)
 *   any other value: NRT_ERR_INVALID_ARG
 * tune: variant-specific knob (variant 3: z-chunk length | order | patch | region bits; variant 5: tile geometry). */
int nrt_interpn_f32_ex(const float *vol, const float *loc, float *out,
                       int ndim, const int vol_shape[], const int out_shape[], int channels,
                       int batch, long long vol_batch_stride, long long loc_batch_stride,
                       int loc_mode, int method, int has_fill, float fill_value,
                       int variant, int tune, void *stream);

/* Nearest-neighbour lookup on int32 volumes (label maps); fill arithmetic done in int32. */
int nrt_interpn_nearest_i32(const int32_t *vol, const float *loc, int32_t *out,
                            int ndim, const int vol_shape[], const int out_shape[], int channels,
                            int batch, long long vol_batch_stride, long long loc_batch_stride,
                            int loc_mode, int has_fill, int32_t fill_value, void *stream);

/* interpn for every other dtype / rank the reference accepts (neurite/tf/utils/utils.py:106-127, 137-213 are dtype- and
 * rank-generic): float16, bfloat16 and float64 volumes in 1..8 dimensions, float32 and (nearest only) int32 volumes in
 * 4..8 dimensions (TensorFlow itself stops at rank-8 tensors).  `dtype` is an nrt_dtype value (below).  loc is cast to the volume dtype and the arithmetic runs in that
 * dtype, one rounding per operation, as TensorFlow evaluates it.  loc: float32 [batch, out_shape, ndim] (float64 when
 * loc_is_f64, float64 volumes with NRT_LOC_ABSOLUTE only), NULL for NRT_LOC_LINSPACE.  vol / out are `dtype`. */
int nrt_interpn_any(const void *vol, const void *loc, void *out, int dtype, int ndim, const int vol_shape[],
                    const int out_shape[], int channels, int batch, long long vol_batch_stride,
                    long long loc_batch_stride, int loc_mode, int loc_is_f64, int method, int has_fill,
                    double fill_value, void *stream);

/* out = addend + interpn_linear(vol, loc): the update of voxelmorph's compose() (curr + transform(nxt, curr)) and of
 * integrate_vec() (vec += transform(vec, vec); scaling and squaring) in one pass -- call sites
 * neurite/tf/models.py:802-804, 1131, 1149-1154 (VecInt / ComposeTransform next to SpatialTransformer).
 * addend [batch, out_shape, channels]; same rounding as the two separate TF ops (interp, then one add). */
int nrt_interpn_add_f32(const float *vol, const float *loc, const float *addend, float *out, int ndim,
                        const int vol_shape[], const int out_shape[], int channels, int batch,
                        long long vol_batch_stride, long long loc_batch_stride, long long addend_batch_stride,
                        int loc_mode, int has_fill, float fill_value, void *stream);

/* voxelmorph.utils.affine_to_dense_shift ('ij' indexing; called on affine inputs of SpatialTransformer / AffineToDenseShift and by
 * the synthesis models, neurite/tf/models.py:1131-1154): out[b, q, :] = A_b [q - c; 1] - (q - c), c = (shape - 1) / 2 when
 * shift_center else 0.  matrix [batch, ndim, ndim + 1], out [batch, *shape, ndim]; ndim 2 or 3. */
int nrt_affine_to_dense_shift_f32(const float *matrix, int batch, int ndim, const int shape[], int shift_center, float *out,
                                  void *stream);

/* ------------------------------------------------------------------------------------------
 * Dice
 * replaces: neurite/tf/metrics.py:415-482 (Dice.dice) incl. the optional renormalisation
 * (:434-436), the range asserts (:439-444, returned as min/max) and the hard path (:450-468).
 * ------------------------------------------------------------------------------------------ */
size_t nrt_dice_workspace_bytes(long long nvox, int nlabels, int batch);

/*
 * Soft Dice.  y_true, y_pred [batch, nvox, nlabels] float32.
 *   sums   [batch, 3, nlabels] float32 : sum_v t*p, sum_v t*t, sum_v p*p
 *   dice   [batch, nlabels]    float32 : laplace>0 ? (2*tp+eps)/(tt+pp+eps) : divide_no_nan(2*tp, tt+pp)
 *   minmax [4] float32 (may be NULL)   : min t, max t, min p, max p over the whole call
 *                                        (after normalisation if normalize = 1)
 *   normalize 0 or 1 (y / sum_l y first, :434-436); any other value is NRT_ERR_INVALID_ARG.
 * Deterministic: wavefront shuffles -> LDS -> per-block partials -> fixed-order second stage.
 */
int nrt_dice_soft_f32(const float *y_true, const float *y_pred, long long nvox, int nlabels, int batch,
                      int normalize, float laplace_smoothing,
                      float *sums, float *dice, float *minmax,
                      void *workspace, size_t workspace_bytes, void *stream);
/* The same for maps STORED as float32, bfloat16 or float16 (dtype: NRT_DT_F32 / NRT_DT_BF16 / NRT_DT_F16, both maps alike): the
 * values are widened to float32 in registers and every sum is a float32 sum, as TensorFlow's reductions of 16-bit tensors
 * accumulate; sums / dice / minmax are float32.  (neurite/tf/metrics.py:415-482 is dtype-agnostic.) */
int nrt_dice_soft(const void *y_true, const void *y_pred, int dtype, long long nvox, int nlabels, int batch, int normalize,
                  float laplace_smoothing, float *sums, float *dice, float *minmax, void *workspace, size_t workspace_bytes,
                  void *stream);
/* Sums of the squared difference of two label maps, per batch entry and label, in ONE pass over the two maps: what
 * MeanSquaredErrorProb (neurite/tf/metrics.py:653-692: mean of w_l (y_true - y_pred)^2) reduces.  The difference is formed in
 * registers (exact, no t^2 - 2 t p + p^2 expansion), squared and summed by the nrt_dice_soft_f32 kernels in their order.
 *   a, b [batch, nvox, nlabels]; sums [batch, 3, nlabels] float32, every one of the three rows = sum_v (a - b)^2;
 *   scratch [batch, nlabels] float32 (overwritten); workspace as nrt_dice_soft_f32. */
int nrt_sqdiff_sums_f32(const float *a, const float *b, long long nvox, int nlabels, int batch, float *sums, float *scratch,
                        void *workspace, size_t workspace_bytes, void *stream);


/*
 * Hard Dice from probabilistic maps: argmax over labels (ties -> lowest index) then one-hot.
 *   counts [batch, 3, nlabels] int64 : #(a_t==l && a_p==l), #(a_t==l), #(a_p==l)   (exact)
 *   dice   [batch, nlabels] float32
 */
int nrt_dice_hard_prob_f32(const float *y_true, const float *y_pred, long long nvox, int nlabels, int batch,
                           float laplace_smoothing, long long *counts, float *dice,
                           void *workspace, size_t workspace_bytes, void *stream);
/* the same with minmax [4] = min t, max t, min p, max p of the inputs from the same pass (the range asserts of
 * neurite/tf/metrics.py:439-444); nlabels a multiple of 4 up to 256 and 16-byte aligned maps, else NRT_ERR_UNSUPPORTED */
int nrt_dice_hard_prob_minmax_f32(const float *y_true, const float *y_pred, long long nvox, int nlabels, int batch,
                                  float laplace_smoothing, long long *counts, float *dice, float *minmax,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* Hard Dice of probability maps stored as float32 / bfloat16 / float16 (arg-max of the stored values: exact in any of them);
 * minmax [4] may be NULL. */
int nrt_dice_hard_prob(const void *y_true, const void *y_pred, int dtype, long long nvox, int nlabels, int batch,
                       float laplace_smoothing, long long *counts, float *dice, float *minmax, void *workspace,
                       size_t workspace_bytes, void *stream);


/* Hard Dice from label maps [batch, nvox] int32; labels outside [0, nlabels) match nothing.  workspace: NULL, or
 * nrt_dice_workspace_bytes(nvox, nlabels, batch) bytes (then the block histograms are reduced without global atomics). */
int nrt_dice_hard_label_i32(const int32_t *y_true, const int32_t *y_pred, long long nvox, int nlabels,
                            int batch, float laplace_smoothing, long long *counts, float *dice,
                            void *workspace, size_t workspace_bytes, void *stream);

/* dice[b,l] from externally reduced sums (e.g. after an RCCL all-reduce of `sums`). */
int nrt_dice_from_sums_f32(const float *sums, int nlabels, int batch, float laplace_smoothing,
                           float *dice, void *stream);

/* out2[0] = sum over the [batch, nlabels] entries of dice * weights, out2[1] = batch * nlabels: the pair a rank
 * contributes to the single all-reduce behind Dice.mean_dice over a batch sharded across GPUs
 * (neurite/tf/metrics.py:499-510, K.mean(dice * weights)).  weights: NULL, [nlabels], or with
 * weights_per_batch != 0 [batch, nlabels].  One launch, fixed summation order. */
int nrt_dice_mean_pair_f32(const float *dice, const float *weights, int nlabels, int batch,
                           int weights_per_batch, float *out2, void *stream);

/* The same launch writing three floats: [sum, count, sum / count] -- a process that is alone (no collective to wait for) reads the mean
 * K.mean(dice * weights) of neurite/tf/metrics.py:499-510 from out3[2] without launching the division. */
int nrt_dice_mean_f32(const float *dice, const float *weights, int nlabels, int batch, int weights_per_batch, float *out3,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused SpatialTransformer + soft Dice  (the BASELINE "interpn+Dice" pipeline in one pass)
 * replaces: SpatialTransformer (see nrt_interpn_f32, NRT_LOC_SHIFT) immediately followed by
 * Dice.dice(fixed, warped) (neurite/tf/metrics.py:415-482) without materialising `warped`.
 *   moving [batch, vol_shape, nlabels], loc [batch, out_shape, 3] (or NULL for NRT_LOC_LINSPACE),
 *   fixed  [batch, out_shape, nlabels];  warped [batch, out_shape, nlabels] or NULL (not written).
 *   sums / dice / minmax as nrt_dice_soft_f32 with y_true = fixed, y_pred = warped.
 * 3-D only, nlabels a multiple of 4 in [4, 256] (4 * 2^k labels: lane groups of nlabels / 4 lanes; any other count: lane groups
 * of the next power of two, the lanes past nlabels / 4 idle).  tune: tile shape knob (0 = default): log2 of the tile extents
 * along x, y, z in bits 0-3, 4-7, 8-11, bit 14 the x-march schedule ((y,z) patches of 2^lty x 2^ltz voxels marched along x).  Extents
 * too small for a block are widened, never refused: z to a wave's run of 64 / G voxels, y until a tile -- on the x-march the
 * (y,z) patch -- holds the 256 / G voxels of a pass (G = lanes per voxel, above).
 * Size limits (NRT_ERR_UNSUPPORTED beyond them; use nrt_interpn_f32 + nrt_dice_soft_f32): one batch entry of moving /
 * fixed / warped below 4 GiB, shape[0] * shape[1] and shape[2] below 2^24 for both shapes (32-bit row offsets, 24-bit
 * index multiplies).
 * ------------------------------------------------------------------------------------------ */
size_t nrt_warp_dice_workspace_bytes(const int out_shape[], int nlabels, int batch, int tune);
int nrt_warp_dice_soft_f32(const float *moving, const float *loc, const float *fixed, float *warped,
                           const int vol_shape[], const int out_shape[], int nlabels, int batch,
                           long long loc_batch_stride, int loc_mode, int has_fill, float fill_value,
                           float laplace_smoothing, float *sums, float *dice, float *minmax,
                           int tune, void *workspace, size_t workspace_bytes, void *stream);

/* The same with the two label maps STORED as bfloat16 (moving [batch, vol_shape, nlabels], fixed [batch, out_shape, nlabels]):
 * half the bytes per row (a 32-label row is 64 B, two z-neighbours share a cache line).  The rows are widened to float32 in
 * registers and the arithmetic is the float32 kernel's, so for maps whose values are bfloat16 numbers (one-hot label maps)
 * sums / dice are bit-identical to nrt_warp_dice_soft_f32 on the widened maps.  An extension of this package (the reference
 * has no fused form; TensorFlow would blend bfloat16 tensors in bfloat16 -- nrt_interpn_any does that for interpn).
 * No `warped` output. */
int nrt_warp_dice_soft_bf16(const void *moving, const float *loc, const void *fixed, const int vol_shape[],
                            const int out_shape[], int nlabels, int batch, long long loc_batch_stride, int loc_mode,
                            int has_fill, float fill_value, float laplace_smoothing, float *sums, float *dice,
                            float *minmax, int tune, void *workspace, size_t workspace_bytes, void *stream);

/* Name of the kernel instantiation nrt_warp_dice_soft_f32 launches for these arguments, as a profiler prints it (e.g.
 * "warp_dice_tile<8, 1, false, 3, float>", "warp_dice_tile_pad<8, 1, false, 3, float>" for 24 labels); "" for arguments the entry
 * point rejects.  The returned buffer is thread-local.
 * Measurement plumbing (bench.py joins its timing with the counter passes under profiles/ by this name); no reference counterpart. */
const char *nrt_warp_dice_kernel_name(const int out_shape[], const int vol_shape[], int nlabels, int batch, int loc_mode, int has_fill,
                                      int store, int want_minmax, int tune);

/* ------------------------------------------------------------------------------------------
 * Fused SpatialTransformer + soft Dice on integer LABEL MAPS  (csrc/warp_labels.hip)
 * An extension of this package: the reference has no fused form and no soft Dice on label ids.  With M = one_hot(moving, nlabels)
 * and F = one_hot(fixed, nlabels) in float32 (an id outside [0, nlabels) gives an all-zero row, as tf.one_hot does) the results
 * are those of nrt_warp_dice_soft_f32 on M and F, without the one-hot tensors: the tri-linear warp of a one-hot map has at most
 * 8 non-zero values per voxel, the sums of the weights of the corners that carry each label.
 *   moving [batch, vol_shape] int32, loc [batch, out_shape, 3], fixed [batch, out_shape] int32;
 *   warped [batch, out_shape, nlabels] float32 or NULL (not written): bit-identical to nrt_interpn_f32 on M;
 *   sums [batch, 3, nlabels] (sum t p, sum t^2, sum p^2), dice [batch, nlabels] as nrt_dice_soft_f32.
 * nlabels 1 ... 256 (no multiple-of-4 rule).  loc_mode NRT_LOC_SHIFT or NRT_LOC_ABSOLUTE (NRT_LOC_LINSPACE: NRT_ERR_INVALID_ARG);
 * loc_batch_stride = 0: one transform for every batch entry.  has_fill: fill_value must be 0 (an out-of-bounds voxel contributes
 * p = 0 for every label).  No atomics: results are run-to-run bit-identical.  No host synchronisation.
 * Size limits (NRT_ERR_UNSUPPORTED beyond them): 3-D, batch <= 65535, fewer than 2^31 voxels per volume and per output, one batch
 * entry of `warped` below 4 GiB.
 * The backward is wrt loc only: grad_loc [batch, out_shape, 3] from the forward's sums and grad_dice [batch, nlabels]; it is 0 for
 * out-of-bounds voxels when has_fill is set, and for a label whose denominator is 0.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_warp_dice_labels_workspace_bytes(const int out_shape[], int nlabels, int batch);
int nrt_warp_dice_labels_f32(const int32_t *moving, const float *loc, const int32_t *fixed, float *warped /* or NULL */,
                             const int vol_shape[], const int out_shape[], int nlabels, int batch,
                             long long loc_batch_stride, int loc_mode, int has_fill, float fill_value,
                             float laplace_smoothing, float *sums, float *dice,
                             void *workspace, size_t workspace_bytes, void *stream);
int nrt_warp_dice_labels_bwd_f32(const int32_t *moving, const float *loc, const int32_t *fixed, const float *sums,
                                 const float *grad_dice, float *grad_loc, const int vol_shape[], const int out_shape[],
                                 int nlabels, int batch, long long loc_batch_stride, int loc_mode, int has_fill,
                                 float laplace_smoothing, void *stream);

/* ------------------------------------------------------------------------------------------
 * Warp integer LABEL MAPS by linear interpolation + arg-max, and fuse several of them by a weighted vote  (csrc/warp_argmax.hip)
 * An extension of this package (the reference warps one-hot maps and takes tf.argmax).  With M = one_hot(moving, nlabels) in float32
 * the ids are argmax_l and prob is max_l of nrt_interpn_f32's tri-linear warp of M, without M: per label l the warped value is
 *   p_l = the float32 sum, starting from 0, of the weights fl(fl(wx wy) wz) of the corners that carry l, added in corner order
 *         000 ... 111 (at most 8 labels per voxel have p_l != 0).
 * The winner is the label with the largest p_l > 0; an exact tie goes to the smaller id; no label with p_l > 0: id 0, prob 0 (what
 * np.argmax of the dense row gives).
 *   moving [batch, vol_shape] int32; out_ids [batch, out_shape] int32; out_prob [batch, out_shape] float32 or NULL (not written;
 *   the ids are the same either way).  3-D only.
 * nlabels = L in 1 ... 2^31 - 1: an id outside [0, L) is an all-zero row, as tf.one_hot has it: it never wins and is never used as an
 * index.  nlabels = 0: every int32 value is a label (ids compare as signed integers).
 * has_fill: a voxel whose unclipped location lies outside the volume gets fill_label and prob 0 (with nlabels >= 1 and fill_label 0
 * that is the one-hot pipeline under fill_value = 0); without has_fill the edge is clamped, as everywhere else.
 *   nrt_warp_labels_argmax_i32         loc [batch, out_shape, 3] with loc_mode NRT_LOC_SHIFT or NRT_LOC_ABSOLUTE (loc_batch_stride in
 *                                      floats, 0: one transform for every batch entry), or loc = NULL with NRT_LOC_LINSPACE: the
 *                                      align-corners grid of resize.
 *   nrt_affine_warp_labels_argmax_i32  matrix [matrix_batch, 3, 4] float32, matrix_batch = batch or 1; the location of output voxel q
 *                                      is formed in registers exactly as nrt_affine_warp_f32 forms it: p = (float)q - c (c =
 *                                      (out_shape - 1) / 2 when shift_center, else 0), s_i = (((M_i0 p_0 + M_i1 p_1) + M_i2 p_2) +
 *                                      M_i3) - p_i, loc_i = (float)q_i + s_i, one rounding per operation.
 *   nrt_fuse_labels_i32                atlases [n_atlases, vol_shape] int32, loc [n_atlases, out_shape, 3] displacements
 *                                      (NRT_LOC_SHIFT; loc_atlas_stride in floats, 0: one field for every atlas), weights [n_atlases]
 *                                      float32, finite and >= 0, or NULL for all ones.  V_l = the float32 sum, starting from 0, over
 *                                      the atlases in order n = 0 ... of fl(w_n p_{n,l}); a label absent from atlas n adds +0.
 *                                      out_ids [out_shape] = the label with the largest V_l > 0, ties and the all-zero case as
 *                                      above; out_votes [out_shape] = its V_l (not normalised) or NULL.  has_fill: an atlas whose
 *                                      location is out of bounds adds nothing; every atlas out of bounds: fill_label, votes 0.
 *                                      Exact for every input, 8 n_atlases distinct ids at one voxel included (a voxel with more
 *                                      than 32 candidates leaves the in-LDS list for a slower list-free pass with the same sums).
 * Non-finite locations: every gather index stays inside the volume; the values are unspecified.
 * No atomics, no workspace, no host synchronisation; results are run-to-run bit-identical.
 * Checked before any launch: NRT_ERR_INVALID_ARG for a NULL moving / atlases, out_ids, matrix, shape or (unless NRT_LOC_LINSPACE) loc,
 * an extent, batch or n_atlases < 1, nlabels < 0, an unknown loc_mode, NRT_LOC_LINSPACE given with a loc, a negative stride, a
 * matrix_batch that is neither 1 nor batch; NRT_ERR_UNSUPPORTED for 2^31 or more voxels in a map, batch > 65535, n_atlases > 16.
 * ------------------------------------------------------------------------------------------ */
int nrt_warp_labels_argmax_i32(const int32_t *moving, const float *loc /* NULL for NRT_LOC_LINSPACE */, int32_t *out_ids,
                               float *out_prob /* or NULL */, const int vol_shape[], const int out_shape[], int nlabels, int batch,
                               long long loc_batch_stride, int loc_mode, int has_fill, int fill_label, void *stream);
int nrt_affine_warp_labels_argmax_i32(const int32_t *moving, const float *matrix, int32_t *out_ids, float *out_prob /* or NULL */,
                                      const int vol_shape[], const int out_shape[], int nlabels, int batch, int matrix_batch,
                                      int shift_center, int has_fill, int fill_label, void *stream);
int nrt_fuse_labels_i32(const int32_t *atlases, const float *loc, const float *weights /* or NULL */, int32_t *out_ids,
                        float *out_votes /* or NULL */, const int vol_shape[], const int out_shape[], int nlabels, int n_atlases,
                        long long loc_atlas_stride, int has_fill, int fill_label, void *stream);

/* ------------------------------------------------------------------------------------------
 * Label-weighted categorical cross-entropy
 * replaces: neurite/tf/metrics.py:640-650 + tf.keras.losses.CategoricalCrossentropy
 * ------------------------------------------------------------------------------------------ */
typedef enum { NRT_DT_F32 = 0, NRT_DT_BF16 = 1, NRT_DT_F16 = 2, NRT_DT_F64 = 3, NRT_DT_I32 = 4, NRT_DT_U8 = 5 } nrt_dtype;

size_t nrt_wcce_workspace_bytes(long long nvox_total, int channels);

/*
 * y_true, y_pred [nvox_total, channels] of `dtype`; label_weights [channels] float32 or NULL.
 *   t' = w*t; [t' = t'*(1-s) + s/C]; from_logits ? -sum t' log_softmax(z)
 *                                               : q = clip(p/sum p, 1e-7, 1-1e-7), -sum t' log q
 *   loss_sum  [1] float32 : sum over all voxels (the caller divides by nvox_total)
 *   per_voxel [nvox_total] float32 or NULL
 * Arithmetic in float32 regardless of the input dtype.
 */
int nrt_wcce(const void *y_true, const void *y_pred, int dtype, const float *label_weights,
             long long nvox_total, int channels, int from_logits, float label_smoothing,
             float *loss_sum, float *per_voxel,
             void *workspace, size_t workspace_bytes, void *stream);
/* The same with the division of the default reduction ('sum_over_batch_size': metrics.py:650 -> Keras CategoricalCrossentropy) done by
 * the block that finishes the sum: loss_mean[0] = float32(sum) / float32(divide_by); one launch, nothing for the caller to divide. */
int nrt_wcce_mean(const void *y_true, const void *y_pred, int dtype, const float *label_weights,
                  long long nvox_total, int channels, int from_logits, float label_smoothing, double divide_by,
                  float *loss_mean, float *per_voxel,
                  void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * unet layers
 * replaces the Keras layers that neurite/tf/models.py instantiates: Conv3D (:1378-1388, :1545-1555,
 * :1596), MaxPooling3D (:1436-1438), UpSampling3D + concatenate (:1531-1542), the channel softmax
 * (:1601-1605) and the residual add / activation / BatchNormalization (:1401-1433).
 * All tensors channels-last float32 [batch, X, Y, Z, C]; `shape`, `ksize`, `pool`, `up` are host int[3].
 * ------------------------------------------------------------------------------------------ */
/* element-wise activations as tf.keras.activations defines them (elu alpha 1, hard_sigmoid = clip(0.2 x + 0.5, 0, 1), leaky_relu slope
 * 0.2).  The convolution / LocallyConnected3D entry points (nrt_conv3d_f32, nrt_conv3d_up2_f32, nrt_conv1x1_softmax_f32,
 * nrt_lc3d_f) fuse NONE / ELU / RELU into their epilogues and return NRT_ERR_INVALID_ARG for the other codes: run those as an
 * element-wise pass over the layer output (nrt_add_act_affine_f32, which accepts all of them, as do nrt_act_bwd_f32 and the
 * backward entry points).  The channel softmax is a kernel of its own (nrt_softmax_lastdim_f32). */
typedef enum { NRT_ACT_NONE = 0, NRT_ACT_ELU = 1, NRT_ACT_RELU = 2, NRT_ACT_SIGMOID = 3, NRT_ACT_TANH = 4, NRT_ACT_SOFTPLUS = 5,
               NRT_ACT_SOFTSIGN = 6, NRT_ACT_SELU = 7, NRT_ACT_EXPONENTIAL = 8, NRT_ACT_HARD_SIGMOID = 9, NRT_ACT_LEAKY_RELU = 10 } nrt_activation;
/* nrt_add_act_affine_f32 only: or-ed into `activation`, y = act(a) * b instead of act(a + b) (models.add_prior, use_logp=False) */
#define NRT_ACT_MUL_B 0x100

/* Weights re-ordered for the MFMA kernel ("packed"): query the size, pack once per layer. */
size_t nrt_conv3d_packed_weight_floats(const int ksize[], int cin, int cout);
int nrt_conv3d_pack_weights_f32(const float *weights /* Keras [kx,ky,kz,cin,cout] */, const int ksize[],
                                int cin, int cout, float *packed, void *stream);

/*
 * y = act(conv3d(concat(src0, upsample_nearest(src1, up)), W) + bias), cross-correlation, stride 1,
 * dilation `dilation`, SAME (output = shape) or VALID padding.
 *   src0 [batch, shape, c0]; src1 [batch, shape/up, c1] or NULL with c1 = 0 (plain convolution);
 *   weights Keras layout [kx,ky,kz,c0+c1,cout] (direct kernel), packed_weights from
 *   nrt_conv3d_pack_weights_f32 (MFMA kernel; may be NULL => direct kernel); bias [cout] or NULL.
 * variant 0 = auto (MFMA implicit GEMM when k in {1,3}^3, SAME, dilation <= 2, cout <= 64, cin >= 8; its persistent LDS-DMA
 * schedule for 3x3x3, dilation 1, cin % 16 == 0 when there is more than one tile per CU), 1 = direct, 2 = MFMA (one tile per
 * block), 5 = MFMA in the persistent schedule, 6 = the 2x2x2 MFMA arm (2x2x2 kernel, dilation 1, SAME, cin >= 8, cout <= 64,
 * c0 % 4 == 0 with a second source, 16-byte aligned sources; anything else is NRT_ERR_UNSUPPORTED).  An even kernel runs on the
 * direct kernel under variant 0, except that the 2x2x2 arm is taken where it has been measured faster (profiles/conv_even: 16 .. 64
 * channels on both sides and at least 4 * 40^3 output voxels over the batch).
 */
int nrt_conv3d_f32(const float *src0, int c0, const float *src1, int c1, const int up[],
                   const float *weights, const float *packed_weights, const float *bias, float *out,
                   int batch, const int shape[], const int ksize[], int cout, int dilation,
                   int padding_same, int activation, int variant, void *stream);

/*
 * The single-channel first encoder convolution with the 2x2x2 MaxPooling3D behind it (neurite/tf/models.py:1378-1388 and
 * :1436-1438) in one kernel: `out` [batch, shape, cout] exactly as nrt_conv3d_f32 writes it (the decoder's skip connection reads
 * it), and `pool_out` [batch, shape / 2, cout] = MaxPooling3D(2)(out) in addition -- the pooled values are taken from the tile
 * while it is in LDS instead of reading the full-resolution tensor back.  3x3x3 SAME, weights in Keras layout [3,3,3,1,cout],
 * cout 16 or 32, shape a multiple of (4, 4, 16); bit-identical to nrt_conv3d_f32 followed by nrt_maxpool3d_f32.
 */
int nrt_conv3d_c1_pool_supported(const int shape[], int cout);
int nrt_conv3d_c1_pool_f32(const float *src /* [batch, shape, 1] */, const float *weights, const float *bias, float *out,
                           float *pool_out, int batch, const int shape[], int cout, int activation, void *stream);
/*
 * The same pattern below the first level (round 6): a 3x3x3 SAME convolution over c0 = 16 k input channels (packed weights of
 * nrt_conv3d_pack_weights_f32) and the MaxPooling3D(2) of its activated output from one kernel (models.py:1378-1388 + 1436-1438) --
 * `out` [batch, shape, cout] as nrt_conv3d_f32 (variant 5) writes it, `pool_out` [batch, shape / 2, cout] in addition.  cout 32, 48 or
 * 64, shape a multiple of (4, 4, 16); bit-identical to nrt_conv3d_f32 followed by nrt_maxpool3d_f32.
 */
int nrt_conv3d_pool_supported(int c0, int cout, const int shape[], int batch);
int nrt_conv3d_pool_f32(const float *src /* [batch, shape, c0] */, int c0, const float *packed_weights, const float *bias, float *out,
                        float *pool_out, int batch, const int shape[], int cout, int activation, void *stream);

/*
 * The decoder convolution of models.unet (neurite/tf/models.py:1531-1555: UpSampling3D(2) -> concatenate([skip, up]) ->
 * Conv3D 3x3x3 SAME) with the up-sampled half FOLDED: on a nearest-up-sampled tensor the 27 taps collapse to 8 taps
 * on the low-resolution grid, with one of 8 pre-summed weight sets chosen by the parity of the output voxel
 * (K = 27 c0 + 8 c1 instead of 27 (c0 + c1)).  Same result as nrt_conv3d_f32(skip, c0, lo, c1, up = {2,2,2}, ...)
 * up to float32 rounding of the weight sums.  c0 % 16 == 0, c1 % 16 == 0, cout <= 64, activation none / elu / relu.
 *   nrt_conv3d_up2_supported            1 when the shapes qualify (otherwise use nrt_conv3d_f32)
 *   nrt_conv3d_up2_packed_weight_floats size of the folded, fragment-ordered weights
 *   nrt_conv3d_up2_pack_weights_f32     weights Keras layout [3,3,3,c0+c1,cout] -> packed
 */
int nrt_conv3d_up2_supported(int c0, int c1, int cout, const int shape[]);
size_t nrt_conv3d_up2_packed_weight_floats(int c0, int c1, int cout);
int nrt_conv3d_up2_pack_weights_f32(const float *weights, int c0, int c1, int cout, float *packed, void *stream);
int nrt_conv3d_up2_f32(const float *skip /* [batch, shape, c0] */, int c0, const float *lo /* [batch, shape/2, c1] */, int c1,
                       const float *packed_weights, const float *bias, float *out, int batch, const int shape[], int cout,
                       int activation, void *stream);
/*
 * The LAST decoder convolution of models.unet with the network's head folded in (neurite/tf/models.py:1545-1555 the convolution,
 * :1596 the 1x1x1 "likelihood" convolution, :1601-1605 the channel soft-max): out = softmax(act(conv_up2(skip, lo)) @ head_weights
 * + head_bias) [batch, shape, labels]; the 16-channel feature tensor between the two convolutions is never written.  Inference
 * only (the backward of a training step needs that tensor).  cout == 16, labels 16 or 32, shape a multiple of (4, 4, 16), c0 < c1;
 * the head's kernel packed by nrt_conv3d_up2_head_pack_f32 (Keras layout [16, labels] -> 16 * labels floats in matrix-core
 * fragment order), both head arrays 16-byte aligned.  Same values as nrt_conv3d_up2_f32 followed by nrt_conv1x1_softmax_f32 up
 * to the float32 summation order of the 16-term head products.
 */
int nrt_conv3d_up2_head_supported(int c0, int c1, int cout, int labels, const int shape[]);
int nrt_conv3d_up2_head_pack_f32(const float *head_weights /* [16, labels] */, int labels, float *packed /* [16 * labels] */, void *stream);
int nrt_conv3d_up2_head_f32(const float *skip, int c0, const float *lo, int c1, const float *packed_weights, const float *bias,
                            const float *packed_head_weights, const float *head_bias /* [labels] */, int labels,
                            float *out /* [batch, shape, labels] */, int batch, const int shape[], int cout, int activation,
                            void *stream);

/*
 * Backward of the folded decoder convolution with respect to its low-resolution input (what tf.GradientTape derives through
 * UpSampling3D + concatenate + Conv3D, neurite/tf/models.py:1531-1555): the gradient of the up-sampled tensor summed over
 * the 2^3 blocks is a 4x4x4 stride-2 convolution of dpre = 8 parity sub-lattices x 2x2x2 taps on the low-resolution grid.
 *   nrt_space_to_depth2_f32   y[b][q][P * channels + c] = x[b][2 q + p][c], P = (px * 2 + py) * 2 + pz (shape = x's, even)
 *   nrt_conv3d_s2d_taps_f32   3x3x3 SAME convolution of x [batch, shape, 8 * group] in which the channels of parity group P only
 *                             use the taps e = (p ? 1 : 2) - t, t in {0, 1}, per axis (all other weights are taken as zero);
 *                             packed_weights = nrt_conv3d_pack_weights_f32 of [3,3,3, 8 * group, cout]; group % 16 == 0
 */
int nrt_space_to_depth2_f32(const float *x, float *y, int batch, const int shape[], int channels, void *stream);
int nrt_conv3d_s2d_taps_f32(const float *x, int group, const float *packed_weights, float *out, int batch, const int shape[],
                            int cout, void *stream);

/* 1x1 convolution with the channel softmax (or an activation) fused; cout <= 64. x [nvox, cin]. */
int nrt_conv1x1_softmax_f32(const float *x, const float *weights /* [cin, cout] */, const float *bias,
                            float *y, long long nvox, int cin, int cout, int softmax, int activation,
                            void *stream);
int nrt_softmax_lastdim_f32(const float *x, float *y, long long n, int channels, void *stream);
/* MaxPooling3D, stride = pool; SAME keeps partial windows (output ceil(n/p)), VALID drops them. */
int nrt_maxpool3d_f32(const float *x, float *y, int batch, const int shape[], int channels,
                      const int pool[], int padding_same, void *stream);
/* y = concat(skip [batch, shape, c0] (may be NULL with c0 = 0), upsample_nearest(lo [batch, shape/up, c1])) */
int nrt_upsample_concat_f32(const float *skip, int c0, const float *lo, int c1, float *y, int batch,
                            const int shape[], const int up[], void *stream);
/* y = act(a + b) * scale[c] + shift[c]   (b, scale/shift optional): residual merge / inference BatchNorm */
int nrt_add_act_affine_f32(const float *a, const float *b, const float *scale, const float *shift,
                           float *y, long long n, int channels, int activation, void *stream);

/* ------------------------------------------------------------------------------------------
 * bfloat16 inference forms of the conv stack (csrc/conv_bf16.hip; models.ConvNet with bf16 parameters).  Tensors are bf16,
 * channels-last, as the float32 entry points above; biases, BatchNorm scale / shift are float32.  Every kernel computes in
 * float32 from the stored bf16 values and rounds its result to bf16 once, round-to-nearest-even.
 *   nrt_conv3d_packed_weight_bytes_bf16  size of the packed weights (bytes)
 *   nrt_conv3d_pack_weights_bf16         Keras-layout weights [kx,ky,kz,cin,cout] of `dtype` (NRT_DT_F32: rounded to bf16, or
 *                                        NRT_DT_BF16) -> the A-operand order of v_mfma_f32_16x16x32_bf16, K zero-padded to 32
 *   nrt_conv3d_bf16                      semantics of nrt_conv3d_f32 (nearest up-sampling + concatenate of src1, any kernel size
 *                                        and dilation, SAME / VALID; none / ELU / RELU fused, NRT_ERR_INVALID_ARG for other
 *                                        codes): exact bf16 products, float32 accumulation, bias and activation in float32.
 *                                        out 8-byte aligned.
 *   nrt_conv1x1_softmax_bf16             weights bf16 [cin, cout], cout <= 64
 *   nrt_softmax_lastdim_bf16, nrt_maxpool3d_bf16, nrt_upsample_concat_bf16, nrt_add_act_affine_bf16: as the float32 forms
 *   (pooling and up-sampling are exact).  No atomics: results are run-to-run bit-identical. */
size_t nrt_conv3d_packed_weight_bytes_bf16(const int ksize[], int cin, int cout);
int nrt_conv3d_pack_weights_bf16(const void *weights, int dtype, const int ksize[], int cin, int cout, void *packed, void *stream);
int nrt_conv3d_bf16(const void *src0, int c0, const void *src1, int c1, const int up[], const void *packed_weights,
                    const float *bias, void *out, int batch, const int shape[], const int ksize[], int cout, int dilation,
                    int padding_same, int activation, void *stream);
int nrt_conv1x1_softmax_bf16(const void *x, const void *weights, const float *bias, void *y, long long nvox, int cin, int cout,
                             int softmax, int activation, void *stream);
int nrt_softmax_lastdim_bf16(const void *x, void *y, long long n, int channels, void *stream);
int nrt_maxpool3d_bf16(const void *x, void *y, int batch, const int shape[], int channels, const int pool[], int padding_same,
                       void *stream);
int nrt_upsample_concat_bf16(const void *skip, int c0, const void *lo, int c1, void *y, int batch, const int shape[],
                             const int up[], void *stream);
int nrt_add_act_affine_bf16(const void *a, const void *b, const float *scale, const float *shift, void *y, long long n,
                            int channels, int activation, void *stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the conv stack (what tf.GradientTape derives for neurite/tf/models.py:1345-1347, 1385, 1438,
 * 1506-1508, 1531, 1604; float32, channels-last, stride 1)
 *   nrt_act_bwd_f32        grad_pre = grad_out * act'(y), from the layer OUTPUT y (ELU: y > 0 ? 1 : y + 1)
 *   nrt_conv3d_wgrad_f32   grad_weights [kx,ky,kz,cin,cout] += sum_v x[v + off(tap)] (x) grad_pre[v] (SAME padding) and
 *                          grad_bias [cout] += sum_v grad_pre[v]; both must be ZERO-FILLED by the caller (float
 *                          atomics, one per weight and block); x is the conv input as the layer saw it
 *                          (the concatenation, if any, materialised); ksize entries 1 .. 4 (SAME padding as the forward pads
 *                          it: floor((k - 1) * dilation / 2) before; kernels of more than 28 taps take a launch per 28),
 *                          dilation <= 2
 *   (grad_x = nrt_conv3d_pad_f32(grad_pre, weights flipped in space and transposed in the channel axes, pad_before =
 *   (k - 1) * dilation - floor((k - 1) * dilation / 2)); for odd kernels that is nrt_conv3d_f32 with SAME padding)
 *   nrt_maxpool3d_bwd_f32  stride == pool: the window's gradient goes to its first maximum
 *   nrt_upsample_sum_f32   nearest up-sampling: grad_lo[v] = sum over the up^3 fine voxels of channels
 *                          [channel_offset, channel_offset + channels) of grad_up [.., grad_channels]
 *   nrt_softmax_bwd_f32    grad_in = y * (grad_out - sum_c grad_out_c y_c)
 * ------------------------------------------------------------------------------------------ */
int nrt_act_bwd_f32(const float *grad_out, const float *y, int activation, float *grad_pre, long long n, void *stream);
int nrt_conv3d_wgrad_f32(const float *x, const float *grad_pre, float *grad_weights, float *grad_bias, int batch,
                         const int shape[], int cin, int cout, const int ksize[], int dilation, void *stream);
/* the same with the forward kernel's fused loader: the layer input was concat(x [.., c0], UpSampling3D(x_lo [.., c1])), which
 * is read from its two sources and never materialised (c0 % 4 == 0; x_lo may be NULL with c1 = 0) */
int nrt_conv3d_wgrad2_f32(const float *x, int c0, const float *x_lo, int c1, const int up[], const float *grad_pre,
                          float *grad_weights, float *grad_bias, int batch, const int shape[], int cout, const int ksize[],
                          int dilation, void *stream);
/* folded form for the up-sampled channels of a decoder convolution (see nrt_conv3d_up2_f32): x_lo [batch, shape, cin] is the
 * low-resolution tensor, grad_pre_s2d [batch, shape, 8 * group] = nrt_space_to_depth2_f32 of the layer's grad_pre (group = cout);
 * grad_folded [8 parity groups][8 taps (tx, ty, tz)][cin][group] += sum_q x_lo[q + p + t - 1] (x) grad_pre_s2d[q][P], ZERO-FILLED by
 * the caller; the 27-tap gradient is dW[d] = sum over the (p, t) with d in S(p, t) per axis (S(0,0) = {0}, S(0,1) = {1,2},
 * S(1,0) = {0,1}, S(1,1) = {2}) -- a 27 x 64 matrix product over cin * group values (host side) */
int nrt_conv3d_wgrad_s2d_f32(const float *x_lo, const float *grad_pre_s2d, float *grad_folded, int batch, const int shape[], int cin,
                             int group, void *stream);
int nrt_maxpool3d_bwd_f32(const float *x, const float *grad_out, float *grad_x, int batch, const int shape[],
                          int channels, const int pool[], int padding_same, void *stream);
int nrt_upsample_sum_f32(const float *grad_up, int grad_channels, int channel_offset, float *grad_lo, int channels,
                         int batch, const int lo_shape[], const int up[], void *stream);
int nrt_softmax_bwd_f32(const float *y, const float *grad_out, float *grad_in, long long nvox, int channels, void *stream);
/* BatchNormalization in training mode (Keras axis -1; models.py:1431-1434, 1585-1588): per-channel sums over [rows, channels],
 * out[c] += sum_r a[r][c] * (b ? b[r][c] : 1)  (ZERO-FILLED by the caller), and y = coef_a[c] a + coef_b[c] b + coef_c[c] */
int nrt_channel_sums_f32(const float *a, const float *b, long long rows, int channels, float *out, void *stream);
int nrt_channel_axpby_f32(const float *a, const float *b, const float *coef_a, const float *coef_b, const float *coef_c, float *y,
                          long long n, int channels, void *stream);

/* ------------------------------------------------------------------------------------------
 * Hyper-convolution: a convolution whose kernel and bias ARRIVE WITH THE BATCH, one set per batch entry
 * replaces: neurite/tf/layers.py:2515-2665 (HyperConv / HyperConv2D / HyperConv3D: call :2571-2590, the per-entry tf.map_fn of
 * _convolve_batch :2592-2612), :2668-2822 (the FromDense forms, whose dense maps stay host plumbing) and :2825-3033 (HyperDense /
 * HyperDenseFromDense: the 1x1x1 case with the rows of x[b] as voxels).  float32, channels-last, stride 1.  One launch serves the whole
 * batch: the kernels of nrt_conv3d_f32 / nrt_conv3d_wgrad_f32 with the weight and bias base advanced by the batch entry.
 * ------------------------------------------------------------------------------------------ */
/* neurite/tf/layers.py:2592-2612 has no packing step (tf.nn.convolution takes the Keras layout); the matrix-core kernels read fragments.
 * weights [batch, kx,ky,kz, cin, cout] -> packed [batch, nrt_conv3d_packed_weight_floats(ksize, cin, cout)], all entries in ONE launch.
 * transpose_flip != 0: per entry the kernel flipped in space and transposed in its channel axes is packed instead -- the weights of the
 * input gradient (what tf.GradientTape derives for :2607-2611), a convolution from cout to cin channels: packed
 * [batch, nrt_conv3d_packed_weight_floats(ksize, cout, cin)]. */
int nrt_hyperconv3d_pack_weights_f32(const float *weights, int batch, const int ksize[], int cin, int cout, int transpose_flip,
                                     float *packed, void *stream);
/* 1 when nrt_hyperconv3d_f32 (variant 0) runs these arguments on the matrix cores and therefore reads `packed_weights` (then `weights`
 * may be NULL); 0 when it reads `weights` in the Keras layout.  The rule of nrt_conv3d_f32; no reference counterpart. */
int nrt_hyperconv3d_uses_packed(const int shape[], const int ksize[], int cin, int cout, int dilation, int padding_same);
/* out[b] = act(conv3d(src[b], W[b]) + bias[b]), cross-correlation, SAME or VALID: neurite/tf/layers.py:2592-2612 with the bias and
 * activation of call (:2580-2590).
 *   src [batch, shape, cin]; weights [batch, kx,ky,kz, cin, cout] or NULL; packed_weights from nrt_hyperconv3d_pack_weights_f32 or NULL
 *   (at least one of the two; the kernel that is chosen must find its form: NRT_ERR_INVALID_ARG / NRT_ERR_UNSUPPORTED otherwise, as
 *   nrt_conv3d_f32); bias [batch, cout] or NULL; out [batch, out shape, cout].
 * Kernel choice, variants (0 auto | 1 direct and single-input-channel kernels | 2 MFMA | 5 persistent MFMA), activation codes (none / ELU /
 * ReLU, NRT_ERR_INVALID_ARG beyond) and limits are those of nrt_conv3d_f32; there is no second source and no pool / head fold.
 * No atomics: run-to-run bit-identical, and bit-identical to nrt_conv3d_f32 per entry when every entry carries the same set. */
int nrt_hyperconv3d_f32(const float *src, int cin, const float *weights, const float *packed_weights, const float *bias, float *out,
                        int batch, const int shape[], const int ksize[], int cout, int dilation, int padding_same, int activation,
                        int variant, void *stream);
/* Per-entry weight and bias gradient (what tf.GradientTape derives for neurite/tf/layers.py:2580-2612 with respect to the kernel and
 * bias inputs): grad_weights [batch, kx,ky,kz, cin, cout] and grad_bias [batch, cout] (or NULL), NOT summed over the batch.  Contract of
 * nrt_conv3d_wgrad_f32 otherwise: SAME padding, both outputs ZERO-FILLED by the caller (float atomics, one per weight and block: the sums
 * are not run-to-run bit-identical), ksize entries 1 .. 4, dilation <= 2.  A block only accumulates tiles of one batch entry. */
int nrt_hyperconv3d_wgrad_f32(const float *x, const float *grad_pre, float *grad_weights, float *grad_bias, int batch,
                              const int shape[], int cin, int cout, const int ksize[], int dilation, void *stream);

/* ------------------------------------------------------------------------------------------
 * LocallyConnected3D, implementation 1 ('valid' padding, channels-last)
 * replaces: neurite/tf/layers.py:1126-1197 (local_conv: O slice ops + concat + K.batch_dot) and the
 * bias / activation of :1098-1101.
 *   x [batch, in_shape, cin]; kernel [O, kr*kc*kz*cin, cout] (feature order kr,kc,kz,cin; O = output
 *   positions row-major); bias [O, cout] or NULL; y [batch, out_shape, cout]; all of `dtype`
 *   (NRT_DT_F32 or NRT_DT_BF16), accumulation in float32.  Weights are read exactly once per 1-2 batch entries (vector kernel) or per
 *   <= 8 entries (batches of 3 and more: matrix-core kernel, v_mfma_f32_4x4x1; 16-channel 3x3x3 layers stage their patches per block).
 * variant 0 auto | 1 generic | 2 weight-streaming wave-per-position kernels.
 * ------------------------------------------------------------------------------------------ */
int nrt_lc3d_f(const void *x, const void *kernel, const void *bias, void *y, int dtype, int batch,
               const int in_shape[], int cin, const int ksize[], const int strides[], int cout,
               int activation, int variant, void *stream);
/* Backward of the same layer (autodiff of the batch_dot of layers.py:1189 + bias/activation :1098-1101):
 *   grad_kernel [O, F, cout] and grad_bias [O, cout] (`dtype`, written once, may be NULL), grad_x float32
 *   [batch, in_shape, cin] accumulated with float atomics (ZERO-FILLED by the caller, may be NULL);
 *   y = the layer output (needed when activation != 0), grad_out [batch, out_shape, cout].
 *   cout * itemsize must be a multiple of 16 (the weight-streaming lane layout). */
int nrt_lc3d_bwd_f(const void *x, const void *kernel, const void *y, const void *grad_out, void *grad_kernel,
                   void *grad_bias, float *grad_x, int dtype, int batch, const int in_shape[], int cin,
                   const int ksize[], const int strides[], int cout, int activation, void *stream);

/* Zero-pad (crop == 0) a channels-last volume [batch, in_shape, row] into [batch, out_shape, row] with pad_before voxels
 * in front of every axis, or (crop != 0) copy the interior of a padded volume back out -- `in` is then the padded
 * [batch, out_shape, row] tensor and `out` the [batch, in_shape, row] one.  row_bytes = channels * itemsize (even).
 * padding='same' of LocallyConnected3D implementations 2 / 3 (neurite/tf/layers.py:934-936, 1474-1482: the window is
 * clipped at the border) is the 'valid' layer on the input padded by kernel_size // 2; the crop is its gradient. */
int nrt_pad3d(const void *in, void *out, int batch, const int in_shape[], const int pad_before[], const int out_shape[],
              int row_bytes, int crop, void *stream);

/* ------------------------------------------------------------------------------------------
 * Backward passes (what tf.GradientTape derives from the reference graphs; float32)
 *
 * nrt_interpn_bwd_f32: gradients of linear interpn / transform (neurite/tf/utils/utils.py:137-191, :206-213).
 *   grad_out [batch, out_shape, C]; grad_vol [batch, vol_shape, C] must be ZERO-FILLED by the caller and is
 *   accumulated with float atomics (tf.gather's scatter-add gradient), or NULL; grad_loc [batch, out_shape, D]
 *   is overwritten (gradient wrt loc == gradient wrt the displacement in NRT_LOC_SHIFT mode), or NULL.
 *   The location gradient flows only through clipped_loc (:142; tf.floor has none) on the closed range
 *   [0, size-1]; with has_fill the gradient is zero at out-of-bounds voxels (:209-213).
 * nrt_dice_soft_bwd_f32: d dice[b,l] / d y_pred and / d y_true from the saved sums [batch, 3, L]
 *   (neurite/tf/metrics.py:476-482; divide_no_nan => zero gradient where the denominator is 0).
 * nrt_wcce_bwd_f32: d loss / d y_pred of the weighted CCE (metrics.py:648-650 + Keras normalise/clip/log);
 *   upstream gradient either one device scalar (grad_scalar) or per voxel (grad_per_voxel), times `scale`.
 * ------------------------------------------------------------------------------------------ */
int nrt_interpn_bwd_f32(const float *vol, const float *loc, const float *grad_out, float *grad_vol,
                        float *grad_loc, int ndim, const int vol_shape[], const int out_shape[], int channels,
                        int batch, long long vol_batch_stride, long long loc_batch_stride, int loc_mode,
                        int has_fill, void *stream);

/* Backward of nearest-neighbour interpn (neurite/tf/utils/utils.py:193-204) wrt the volume: tf.gather's scatter-add of
 * grad_out [batch, out_shape, channels] into grad_vol [batch, vol_shape, channels] (ZERO-FILLED by the caller; float atomics),
 * masked where a fill value applies.  The location has no gradient (tf.round). */
int nrt_interpn_nearest_bwd_f32(const float *loc, const float *grad_out, float *grad_vol, int ndim, const int vol_shape[],
                                const int out_shape[], int channels, int batch, long long vol_batch_stride,
                                long long loc_batch_stride, int loc_mode, int has_fill, void *stream);
int nrt_dice_soft_bwd_f32(const float *y_true, const float *y_pred, const float *sums, const float *grad_dice,
                          long long nvox, int nlabels, int batch, float laplace_smoothing, float *grad_pred,
                          float *grad_true, void *stream);

/* The same for Dice(normalize=True) (neurite/tf/metrics.py:434-436): `sums` are those of the per-voxel normalised maps, the
 * gradient is pulled back through t <- divide_no_nan(t, sum_l t) (and p likewise) to the RAW maps y_true / y_pred. */
int nrt_dice_soft_bwd_norm_f32(const float *y_true, const float *y_pred, const float *sums, const float *grad_dice,
                               long long nvox, int nlabels, int batch, float laplace_smoothing, float *grad_pred,
                               float *grad_true, void *stream);
/* Fused backward of nrt_warp_dice_soft_f32 wrt the displacement / location field: rebuilds the warped row in
 * registers, forms d dice / d warped from `sums` (as returned by the forward) and grad_dice [batch, L], and writes
 * grad_loc [batch, out_shape, 3] only.  `warped` and its gradient never touch HBM.  At 32 float32 labels on volumes that take the
 * forward's x-march schedule it runs on the forward's wave-cache gather (csrc/fused_wc.h, BWD; environment NRT_BWD_WC=0 selects the
 * register-pipelined kernel of rounds 2-4: same bits); the grad_loc of nrt_interpn_bwd_f32 at 32 channels likewise.  nlabels: the
 * forward's counts (a multiple of 4 in [4, 256]); counts that are not 4 * 2^k run on padded lane groups, without atomics. */
int nrt_warp_dice_bwd_f32(const float *moving, const float *loc, const float *fixed, const float *sums,
                          const float *grad_dice, float *grad_loc, const int vol_shape[], const int out_shape[],
                          int nlabels, int batch, long long loc_batch_stride, int loc_mode, int has_fill,
                          float laplace_smoothing, void *stream);
int nrt_wcce_bwd_f32(const float *y_true, const float *y_pred, const float *label_weights,
                     const float *grad_scalar, const float *grad_per_voxel, long long nvox_total, int channels,
                     int from_logits, float label_smoothing, float scale, float *grad_pred, void *stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation training loss: soft Dice (neurite/tf/metrics.py:415-482) AND the label-weighted categorical cross-entropy
 * (metrics.py:619-650, probabilities, not logits) of the same pair of maps [batch, nvox, nlabels] float32 in one pass per direction --
 * what neurite/tf/losses.py:225-246 (multiple_losses_decorator) evaluates as two losses over the unet's soft-max output
 * (models.py:1545-1555).  nlabels = 4, 8, ..., 256 (a power of two; nrt_seg_loss_supported), 16-byte aligned maps.
 *   nrt_seg_loss_f32       sums [batch, 3, L], dice [batch, L], minmax [4] or NULL exactly as nrt_dice_soft_f32 (normalize = 0);
 *                          cce_sum [1] exactly as nrt_wcce (from_logits = 0, no per-voxel output).
 *   nrt_seg_loss_bwd_f32   grad = d( sum_bl grad_dice[b,l] dice[b,l] + grad_cce[0] cce_sum ) / d y_pred (either upstream pointer may
 *                          be NULL = 0); through_softmax != 0: y_pred = softmax(z) over the labels and grad = d / d z (what the
 *                          head's nrt_softmax_bwd_f32 would make of it).
 * ------------------------------------------------------------------------------------------ */
int nrt_seg_loss_supported(int nlabels);
size_t nrt_seg_loss_workspace_bytes(long long nvox, int nlabels, int batch);
int nrt_seg_loss_f32(const float *y_true, const float *y_pred, const float *label_weights, long long nvox, int nlabels, int batch,
                     float label_smoothing, float laplace_smoothing, float *sums, float *dice, float *minmax, float *cce_sum,
                     void *workspace, size_t workspace_bytes, void *stream);
int nrt_seg_loss_bwd_f32(const float *y_true, const float *y_pred, const float *label_weights, const float *sums,
                         const float *grad_dice, const float *grad_cce, long long nvox, int nlabels, int batch,
                         float label_smoothing, float laplace_smoothing, int through_softmax, float *grad, void *stream);

/* ------------------------------------------------------------------------------------------
 * The same segmentation loss with an integer LABEL MAP as y_true  (csrc/segloss_labels.hip)
 * An extension of this package: the reference builds the float one-hot map on the host (neurite/tf/generators.py:1024-1049).  With
 * T = one_hot(labels, nlabels) in float32 -- an id outside [0, nlabels) gives an all-zero row, as tf.one_hot does; an id is compared
 * with the labels and never used as an index -- the results are those of nrt_seg_loss_f32 / nrt_seg_loss_bwd_f32 on T and y_pred,
 * without T: 4 bytes of id per voxel stand in for 4 nlabels bytes of row.
 *   labels [batch, nvox] int32, y_pred [batch, nvox, nlabels] float32; nlabels 1 ... 256 (nrt_seg_loss_labels_supported).
 *   Multiples of 4 with 16-byte aligned rows run on lane groups (padded to the next power of two), everything else on a generic kernel.
 *   want: NRT_SEG_WANT_DICE, NRT_SEG_WANT_CCE or both; the kernel of a single loss does no work for the other.
 *     Dice:  sums [batch, 3, L] (the counts sum t^2 are exact), dice [batch, L], minmax [4] or NULL = (0, 1, min y_pred, max y_pred):
 *            the first two are the bounds of a one-hot row.  Without NRT_SEG_WANT_DICE sums and dice may be NULL and minmax must be.
 *     CCE:   cce_sum [1]; may be NULL without NRT_SEG_WANT_CCE.
 *   nrt_seg_loss_labels_bwd_f32: as nrt_seg_loss_bwd_f32; grad_dice or grad_cce may be NULL (that loss is then left out of the
 *   kernel), not both; sums is needed with grad_dice only.
 * NRT_ERR_INVALID_ARG: NULL pointers, nvox < 1, batch < 1, nlabels outside 1 ... 256, want outside 1 ... 3; NRT_ERR_UNSUPPORTED:
 * batch > 65535; NRT_ERR_WORKSPACE: workspace missing or short.  Every refusal comes before any launch.  No atomics: results are
 * run-to-run bit-identical.  No host synchronisation.
 * ------------------------------------------------------------------------------------------ */
#define NRT_SEG_WANT_DICE 1
#define NRT_SEG_WANT_CCE 2
int nrt_seg_loss_labels_supported(int nlabels);
size_t nrt_seg_loss_labels_workspace_bytes(long long nvox, int nlabels, int batch);
int nrt_seg_loss_labels_f32(const int32_t *labels, const float *y_pred, const float *label_weights, long long nvox, int nlabels,
                            int batch, int want, float label_smoothing, float laplace_smoothing, float *sums, float *dice,
                            float *minmax, float *cce_sum, void *workspace, size_t workspace_bytes, void *stream);
int nrt_seg_loss_labels_bwd_f32(const int32_t *labels, const float *y_pred, const float *label_weights, const float *sums,
                                const float *grad_dice, const float *grad_cce, long long nvox, int nlabels, int batch,
                                float label_smoothing, float laplace_smoothing, int through_softmax, float *grad, void *stream);

/* ------------------------------------------------------------------------------------------
 * Synthesis front-end: separable filtering and min-max normalisation
 *   nrt_conv1d_axis_f32   one pass of utils.separable_conv (neurite/tf/utils/utils.py:665-751) / layers.GaussianBlur
 *                         (layers.py:251-364): the tensor viewed as [outer, axis_len, inner] around the filtered axis,
 *                         y[o, a, i] = sum_t kernel[t] * x[o, a*stride + t*dilation - pad_before, i], zero outside
 *                         (cross-correlation, as tf.nn.convolution); y is [outer, out_len, inner]
 *   nrt_minmax_norm_f32   utils.minmax_norm (utils.py:953-968) over a contiguous run of axes: x viewed as
 *                         [outer, reduce_len, inner]; y = div_no_nan(x - min, max - min) per (outer, inner)
 * ------------------------------------------------------------------------------------------ */
int nrt_conv1d_axis_f32(const float *x, const float *kernel, float *y, long long outer, int axis_len, long long inner,
                        int out_len, int width, int stride, int dilation, int pad_before, void *stream);
size_t nrt_minmax_workspace_bytes(long long outer, int inner);
int nrt_minmax_norm_f32(const float *x, float *y, long long outer, long long reduce_len, int inner, void *workspace,
                        size_t workspace_bytes, void *stream);
/* Backward of the two, float32, no atomics (two runs give the same bits), no host synchronisation.
 *   nrt_conv1d_axis_bwd_f32   grad_x [outer, axis_len, inner] from grad_y [outer, out_len, inner]:
 *                             grad_x[o, p, i] = sum_t kernel[t] * grad_y[o, (p + pad_before - t*dilation) / stride, i] over the t whose
 *                             quotient is an integer in [0, out_len); from +0, terms in DESCENDING t, one rounding per multiply and
 *                             per add, absent terms skipped.  stride 1 runs on the kernels of nrt_conv1d_axis_f32 (taps reversed).
 *   nrt_conv1d_axis_bwd_kernel_f32   grad_kernel[t] = sum_{o, a, i} grad_y[o, a, i] * x[o, a*stride + t*dilation - pad_before, i];
 *                             float32 products summed over at most 16 terms per lane, float64 above that; the workspace
 *                             (8-byte aligned, >= nrt_conv1d_axis_bwd_kernel_workspace_bytes) holds the block partials
 *   nrt_minmax_norm_bwd_f32   per group with m = min, M = max, r = M - m: grad_x = 0 if r == 0 (div_no_nan), else
 *                             grad_x_i = g_i / r + [x_i == m] (Sgy - Sg) / (r n_min) - [x_i == M] Sgy / (r n_max), Sg = sum g,
 *                             Sgy = sum g y; ties by float equality share evenly.  Same limits as nrt_minmax_norm_f32; the
 *                             workspace is 8-byte aligned and >= nrt_minmax_norm_bwd_workspace_bytes */
int nrt_conv1d_axis_bwd_f32(const float *grad_y, const float *kernel, float *grad_x, long long outer, int axis_len, long long inner,
                            int out_len, int width, int stride, int dilation, int pad_before, void *stream);
size_t nrt_conv1d_axis_bwd_kernel_workspace_bytes(long long outer, int out_len, long long inner, int width);
int nrt_conv1d_axis_bwd_kernel_f32(const float *x, const float *grad_y, float *grad_kernel, long long outer, int axis_len,
                                   long long inner, int out_len, int width, int stride, int dilation, int pad_before,
                                   void *workspace, size_t workspace_bytes, void *stream);
size_t nrt_minmax_norm_bwd_workspace_bytes(long long outer, long long reduce_len, int inner);
int nrt_minmax_norm_bwd_f32(const float *x, const float *grad_y, float *grad_x, long long outer, long long reduce_len, int inner,
                            void *workspace, size_t workspace_bytes, void *stream);
/* out2 = {min, max} of x[0..n) on the device (no host synchronisation); workspace >= nrt_minmax_workspace_bytes(1, 1) */
int nrt_minmax_f32(const float *x, long long n, float *out2, void *workspace, size_t workspace_bytes, void *stream);
/* centers[0..nb_bins) = tf.linspace(min(x), max(x), nb_bins), the bin centres of utils.soft_quantize / MutualInformation
 * (neurite/tf/utils/utils.py:1152-1154), on the device; workspace as nrt_minmax_f32 */
int nrt_bin_centers_f32(const float *x, long long n, int nb_bins, float *centers, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * Soft quantisation and mutual information (neurite/tf/utils/utils.py:1099-1172, neurite/tf/metrics.py:41-336)
 *   nrt_soft_quantize_f32   out[v, b] = exp(-alpha (clip(x_v) - centers_b)^2)  (or its log)
 *   nrt_mi_joint_f32        x, y [batch, nvox, channels]; per item (b, c): joint[i][j] += sum_v wx_i(v) wy_j(v),
 *                           sum_x[i] += sum_v wx_i(v), sum_y likewise -- the contraction of MutualInformation.channelwise
 *                           without the [V, nb] maps (fp32 MFMA, weights formed in registers); nb_bins <= 32;
 *                           outputs are accumulated with float atomics and must be ZERO-FILLED by the caller
 *   nrt_mi_joint_bwd_f32    gradient wrt x / y given d loss / d joint, d sum_x, d sum_y (bin centres held constant)
 *   nrt_colsum_f32          out[item, c] += sum_r x[item, r, c]  (marginals of probability maps; zero-filled by the caller)
 * ------------------------------------------------------------------------------------------ */
int nrt_soft_quantize_f32(const float *x, const float *centers, float alpha, float min_clip, float max_clip, int return_log,
                          float *out, long long n, int nb_bins, void *stream);

/* Backward of soft_quantize wrt x (bin centres held constant): grad_x [n] from grad_out [n, nb_bins]. */
int nrt_soft_quantize_bwd_f32(const float *x, const float *centers, float alpha, float min_clip, float max_clip,
                              int return_log, const float *grad_out, float *grad_x, long long n, int nb_bins, void *stream);
int nrt_mi_joint_f32(const float *x, const float *y, const float *centers_x, const float *centers_y, float alpha, float min_clip,
                     float max_clip, int batch, long long nvox, int channels, int nb_bins, float *joint, float *sum_x,
                     float *sum_y, void *stream);
int nrt_mi_joint_bwd_f32(const float *x, const float *y, const float *centers_x, const float *centers_y, float alpha,
                         float min_clip, float max_clip, int batch, long long nvox, int channels, int nb_bins,
                         const float *grad_joint, const float *grad_sum_x, const float *grad_sum_y, float *grad_x, float *grad_y,
                         void *stream);
int nrt_colsum_f32(const float *x, int items, long long rows, int cols, float *out, void *stream);
/* mi[item] from joint [items, nb, nb] and the marginal sums [items, nb] (neurite/tf/metrics.py:262-281); nb_bins <= 64 */
int nrt_mi_from_joint_f32(const float *joint, const float *sum_x, const float *sum_y, int items, int nb_bins, float eps, float *mi,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise stages of the label-to-image synthesis model (neurite/tf/models.py:649-918); random numbers are inputs
 *   nrt_synth_relabel_i32     out[i] = lut[labels[i]] (labels -> dense indices, :778-784)
 *   nrt_synth_intensity_f32   labels, noise [B, V] (indices; one draw per voxel), out [B, V, C], mean/std [B, C, L], bg_zero [B, C] or NULL:
 *                             out = noise * std[label] + mean[label], zeroed where label == 0 and bg_zero (:819-849)
 *   nrt_synth_bias_clip_f32   out = clip(image * exp(bias), lo, hi); image [n, C], bias [n] or NULL (:860-874)
 *   nrt_synth_gamma_dc_f32    out = image ^ exp(gamma[b, c]) + dc[b, c]; gamma / dc [B, C] or NULL (:877-888)
 *   nrt_synth_labels_out      indices -> lut (int32 out) or its one-hot encoding [n, depth] (-1 = dropped label) (:890-918)
 * ------------------------------------------------------------------------------------------ */
int nrt_synth_relabel_i32(const int *labels, const float *lut, int lut_len, float *out, long long n, void *stream);
int nrt_synth_intensity_f32(const float *labels, const float *noise, const float *mean, const float *stdv, const float *bg_zero,
                            float *out, int batch, long long nvox, int channels, int nlabels, void *stream);
int nrt_synth_bias_clip_f32(const float *image, const float *bias, float *out, long long n, int channels, float lo, float hi,
                            void *stream);
int nrt_synth_gamma_dc_f32(const float *image, const float *gamma, const float *dc, float *out, int batch, long long nvox,
                           int channels, void *stream);
int nrt_synth_labels_out(const float *idx, const int *lut, int lut_len, int depth, float *onehot, int *out_i32, long long n,
                         void *stream);
/* Stages of labels_to_image_new (neurite/tf/models.py:920-1300) and of the augmentation layers it instantiates:
 *   nrt_synth_axis_mask_f32    x viewed [outer, axis_len, inner]: y = x * mask[a]   (layers.RandomCrop, layers.py:446-519)
 *   nrt_synth_axis_gather_f32  y[o, j, i] = x[o, index[j], i], j < out_len        (layers.Subsample, layers.py:367-443)
 *   nrt_synth_noise_add_f32    y[b, v, c] = x + sd[b * sd_batch_stride + c * sd_channel_stride] * noise   (layers.GaussianNoise, :2305-2403)
 *   nrt_synth_bg_clear_f32     y[b, v, c] = image * (labels[b, v] == 0 && flag[b] ? 0 : 1)   (models.py:1213-1223) */
int nrt_synth_axis_mask_f32(const float *x, const float *mask, float *y, long long outer, int axis_len, long long inner,
                            void *stream);
int nrt_synth_axis_gather_f32(const float *x, const int *index, float *y, long long outer, int axis_len, int out_len,
                              long long inner, void *stream);
/* gradient of nrt_synth_axis_gather_f32 for a non-decreasing index list: run_start [axis_len + 1], the outputs that read slice a
 * are [run_start[a], run_start[a + 1]); grad_x[o, a, i] = their sum, ascending from +0 (zeros for an empty run); no atomics */
int nrt_synth_axis_gather_bwd_f32(const float *grad_y, const int *run_start, float *grad_x, long long outer, int axis_len,
                                  int out_len, long long inner, void *stream);
int nrt_synth_noise_add_f32(const float *x, const float *noise, const float *sd, float *y, int batch, long long nvox,
                            int channels, int sd_batch_stride, int sd_channel_stride, void *stream);
int nrt_synth_bg_clear_f32(const float *image, const float *labels, const float *flag, float *y, int batch, long long nvox,
                           int channels, void *stream);

/* ------------------------------------------------------------------------------------------
 * Local and stream layers (neurite/tf/layers.py:746-808, 1535-1607, 1711-1844, 1915-2073): one parameter, or one small matrix, per
 * voxel, and the running mean / covariance of a stream of batches.  float32, any spatial rank: the tensors are the flat views
 * [batch, n] (n = every axis but the batch) or [batch, nvox, channels].  Every product and sum is rounded on its own (no fma), a
 * parameter is read once for all batch entries, and every parameter gradient is written once by the thread that owns the element,
 * summing b = 0 .. batch-1 in that order: no atomics, run-to-run bit-identical.  16-byte accesses where n (cout, v) is a multiple
 * of 4 and the pointers are 16-byte aligned, 4-byte ones otherwise.  NRT_ERR_INVALID_ARG: a NULL tensor that is not optional,
 * batch < 1, n / nvox / v < 1.  NRT_ERR_UNSUPPORTED: element counts beyond 2^62 or a grid beyond the launch limits.
 *
 *   nrt_local_affine_f32      params mult, bias [n].  x given:  y[b, i] = x[b, i] * mult[i] + bias[i] * bias_scale   (LocalLinear;
 *                             mult NULL: y = x + bias * bias_scale, LocalBias with bias = kernel, bias_scale = biasmult).
 *                             x NULL (mult must be NULL too):  y[b, i] = e[b] * (bias[i] * bias_scale), where e[b] = 1 if probe is
 *                             NULL (LocalParamLayer, batch 1) and e[b] = probe[b * probe_stride] * 0 + 1 otherwise
 *                             (LocalParamWithInput, :1837-1841: probe = the first element of input entry b; NaN / Inf there turns
 *                             entry b into NaN).  x and probe together: NRT_ERR_INVALID_ARG.
 *   nrt_local_affine_bwd_f32  gx[b, i] = g[b, i] * mult[i] (needs mult);  gmult[i] = sum_b g[b, i] * x[b, i] (needs x);
 *                             gbias[i] = bias_scale * sum_b e[b] * g[b, i] (e as above, 1 without a probe).  Each output is optional.
 *   nrt_local_cross_linear_f32      x [batch, nvox, cin], w [nvox, cin, cout], bias [nvox, cout] or NULL:
 *                             y[b, v, o] = sum_c x[b, v, c] * w[v, c, o] (+ bias[v, o]), c ascending.  1 <= cin, cout <= 64, else
 *                             NRT_ERR_UNSUPPORTED.  w[v] is read once per 8 batch entries.
 *   nrt_local_cross_linear_bwd_f32  gx[b, v, c] = sum_o g[b, v, o] * w[v, c, o];  gw[v, c, o] = sum_b x[b, v, c] * g[b, v, o];
 *                             gbias[v, o] = sum_b g[b, v, o].  Each output is optional (gx needs w, gw needs x).
 *   nrt_stream_mean_f32       mean [n] and count [1] are device state.  training != 0 (_mean_update, :2059-2073): new_count =
 *                             count + batch, alpha = batch / min(new_count, cap), mean <- mean * (1 - alpha) + (sum_b x[b] / batch)
 *                             * alpha, count <- new_count, y[b] = min(1, new_count / cap) * mean, and coef[0] (optional) = min(1,
 *                             new_count / cap) * alpha / batch.  training == 0: y[b] = min(1, count / cap) * mean, nothing else is
 *                             written (x may be NULL).  count never travels to the host: the voxel kernel reads the old value and a
 *                             one-thread kernel that follows it in stream order writes the new one; capturable into a hipGraph.
 *   nrt_stream_mean_bwd_f32   gx[b, i] = coef[0] * sum_b' g[b', i]  (the assigned variables are not differentiated through)
 *   nrt_stream_cov_f32        x [batch, v], cov [v, v], mean [v], count [1] (:2014-2052): prev_cap = min(count, cap), cov <- (cov *
 *                             (prev_cap - 1) + sum_b x[b] x[b]^T) / (prev_cap + batch - 1) by IEEE division (a first call with
 *                             batch 1 divides by zero, as the reference does), mean and count as above, y[b] = min(1, new_count /
 *                             cap) * cov.  training == 0: y[b] = min(1, count / cap) * cov.  cov is read and written once, in 16-row
 *                             tiles with the rows of x for the tile in LDS.
 * ------------------------------------------------------------------------------------------ */
int nrt_local_affine_f32(const float *x, const float *probe, long long probe_stride, const float *mult, const float *bias,
                         float bias_scale, float *y, int batch, long long n, void *stream);
int nrt_local_affine_bwd_f32(const float *g, const float *x, const float *probe, long long probe_stride, const float *mult,
                             float bias_scale, float *gx, float *gmult, float *gbias, int batch, long long n, void *stream);
int nrt_local_cross_linear_f32(const float *x, const float *w, const float *bias, float *y, int batch, long long nvox, int cin,
                               int cout, void *stream);
int nrt_local_cross_linear_bwd_f32(const float *g, const float *x, const float *w, float *gx, float *gw, float *gbias, int batch,
                                   long long nvox, int cin, int cout, void *stream);
int nrt_stream_mean_f32(const float *x, float *mean, float *count, float cap, float *y, float *coef, int batch, long long n,
                        int training, void *stream);
int nrt_stream_mean_bwd_f32(const float *g, const float *coef, float *gx, int batch, long long n, void *stream);
int nrt_stream_cov_f32(const float *x, float *mean, float *cov, float *count, float cap, float *y, int batch, int v, int training,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * Dense layer on one shared weight matrix (the bottleneck of models.ae / single_ae, neurite/tf/models.py:499, 558, 618).  float32;
 * x [batch, in], w [in, out] row-major (the Keras `Dense` kernel as stored), bias [out] or NULL, y [batch, out].  Memory bound at the
 * batch sizes these models run at: w is read once per call for up to 16 batch entries (a larger batch runs in chunks of 16).
 *   nrt_dense_f32       y[b, o] = act(sum_i x[b, i] w[i, o] + bias[o]); act: any element-wise code of csrc/activations.h (0 = none).
 *                       variant 0 chooses between the reduce arm (blocks own slabs of `in`, partials in the workspace, summed by a
 *                       second kernel in slab order) and the expand arm (a thread owns adjacent columns and walks `in`); 1 / 2 force
 *                       the reduce / expand arm, each correct at every shape.
 *   nrt_dense_bwd_f32   g [batch, out] = the gradient wrt the pre-activation.  gx[b, i] = sum_o g[b, o] w[i, o] (needs w);
 *                       gw[i, o] = sum_b x[b, i] g[b, o] (needs x); gbias[o] = sum_b g[b, o].  Each output is optional (NULL).
 *                       variant 0 / 2: gx straight from the row-dot kernel where a block spans a row, through partials otherwise;
 *                       1: always through partials.
 *   nrt_dense_workspace_bytes   what both calls need at most under `variant` (0: none); a smaller or missing workspace is
 *                       NRT_ERR_WORKSPACE.
 * No atomics: every sum has a fixed order given the shapes, results are run-to-run bit-identical.  Base pointers need 4-byte
 * alignment only (16-byte loads are used where out % 4 == 0 and the pointers allow).  NRT_ERR_INVALID_ARG: a NULL tensor that is not
 * optional, batch / in / out < 1, an unknown act or variant.  NRT_ERR_UNSUPPORTED: in * out >= 2^31.  Checked before any launch.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_dense_workspace_bytes(int batch, int in, int out, int variant);
int nrt_dense_f32(const float *x, const float *w, const float *bias, float *y, int batch, int in, int out, int act, int variant,
                  void *workspace, size_t workspace_bytes, void *stream);
int nrt_dense_bwd_f32(const float *g, const float *x, const float *w, float *gx, float *gw, float *gbias, int batch, int in, int out,
                      int variant, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Barycenter (centre of mass) of feature maps, neurite/tf/utils/utils.py:512-573, in one pass, and its gradient (csrc/barycenter.hip).
 * x [outer, r_0, ..., r_{k-1}, inner] contiguous, stored as `dtype` (NRT_DT_F32 / NRT_DT_BF16 / NRT_DT_F16) and widened to float32 in
 * registers; red_shape = {r_0 .. r_{k-1}} (host memory), 1 <= k <= 8.  The coordinate of index i along a reduced dimension of size v
 * is the reference's float32 grid value ((float)i, minus (v - 1) / 2 if shift_center, divided by v if normalize), bit for bit.
 *   nrt_barycenter       sums [outer, inner, k + 1] float32: the k numerators sum_r g_d(r) x and the denominator D = sum_r x;
 *                        y [outer, inner, k] float32 = numerator / D, exactly 0 where D == 0 (tf.math.divide_no_nan).
 *   nrt_barycenter_bwd   gy, y [outer, inner, k] and sums as the forward left them -> gx (the layout and dtype of x):
 *                        gx[o, r, i] = sum_d gy[o, i, d] (g_d(r) - y[o, i, d]) / D[o, i], 0 where D == 0.
 *   nrt_barycenter_workspace_bytes   what both calls need at most; 0 for a shape they refuse.
 * No atomics: every sum has a fixed partition and order given the shapes and pointer alignment, results are run-to-run bit-identical.
 * Base pointers need the alignment of their element type only (16-byte accesses are used where inner == 1 or inner is a multiple of
 * 16 bytes and the pointer allows).  Checked before any launch: NRT_ERR_INVALID_ARG for a NULL tensor or red_shape, outer / inner / a
 * reduced size < 1, k outside 1 .. 8; NRT_ERR_UNSUPPORTED for another dtype, a reduced size >= 2^24 (coordinates stop being exact in
 * float32) and outer * R * inner >= 2^31 elements; NRT_ERR_WORKSPACE for a missing or short workspace.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_barycenter_workspace_bytes(int dtype, long long outer, const int red_shape[], int k, long long inner);
int nrt_barycenter(const void *x, int dtype, long long outer, const int red_shape[], int k, long long inner, int normalize,
                   int shift_center, float *y, float *sums, void *workspace, size_t workspace_bytes, void *stream);
int nrt_barycenter_bwd(const float *gy, const float *y, const float *sums, int dtype, long long outer, const int red_shape[], int k,
                       long long inner, int normalize, int shift_center, void *gx, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * Global max over the spatial axes and its gradient (csrc/globalmax.hip): Keras GlobalMaxPooling{1,2,3}D and, with channels = 1
 * and v = V * C, the flatten-then-max lambda of design_dnn (neurite/tf/models.py:1640-1642, 1764).  float32, channels-last.
 *   nrt_global_max_f32       x [batch, v, channels] -> y [batch, channels] = max over v, count [batch, channels] (int32) = how many
 *                            positions attain it.  One pass over x; per-block (max, count) pairs in the workspace are merged by a
 *                            second kernel (the larger max wins, equal maxima add their counts: exact and order-independent).
 *                            The accumulator starts at -inf; a NaN anywhere in a slice gives y = NaN, count = 0.
 *   nrt_global_max_bwd_f32   x, y, count as the forward left them, g [batch, channels] -> gx [batch, v, channels] =
 *                            x == y ? (1.0f / count) * g : 0 (tf.reduce_max: ties share the gradient; the reciprocal is rounded
 *                            first); a slice whose max is NaN gets NaN throughout.  One read of x, one write of gx.
 *   nrt_global_max_workspace_bytes   what both calls need: batch * blocks * max(channels, 4) * 8 bytes, where blocks = the number of
 *                            first-stage blocks per batch entry, min(ceil(v * channels / 16384), max(1, 2048 / batch), v); 0 for a
 *                            shape the calls refuse.  Monotone in v.
 * No atomics and no host synchronisation (both calls capture into a graph); run-to-run bit-identical.  Base pointers need 4-byte
 * alignment only: 16-byte accesses are used where channels % 4 == 0 (or channels <= 2 and v * channels % 4 == 0) and the pointers allow.
 * Checked before any launch: NRT_ERR_INVALID_ARG for a NULL tensor or batch / v / channels < 1; NRT_ERR_UNSUPPORTED for
 * batch * v * channels >= 2^31 or batch > 65535; NRT_ERR_WORKSPACE for a missing or short workspace.
 *
 *   nrt_maxnorm_f32          Keras constraints.MaxNorm(max_value, axis=0) in place on w [k0, rest] (a convolution kernel
 *                            [k0, ..., cin, cout]): n = sqrt(sum_k0 w^2), w <- w * (clip(n, 0, max_value) / (eps + n)); Keras' eps is
 *                            1e-7.  NRT_ERR_INVALID_ARG: NULL w, k0 / rest < 1, max_value <= 0 or NaN, eps < 0 or NaN;
 *                            NRT_ERR_UNSUPPORTED: k0 * rest >= 2^31.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_global_max_workspace_bytes(int batch, long long v, int channels);
int nrt_global_max_f32(const float *x, int batch, long long v, int channels, float *y, int *count, void *workspace,
                       size_t workspace_bytes, void *stream);
int nrt_global_max_bwd_f32(const float *x, const float *y, const int *count, const float *g, int batch, long long v, int channels,
                           float *gx, void *workspace, size_t workspace_bytes, void *stream);
int nrt_maxnorm_f32(float *w, int k0, long long rest, float max_value, float eps, void *stream);

/* ------------------------------------------------------------------------------------------
 * Convolution with an explicit zero padding BEFORE (csrc/conv.hip): nrt_conv3d_f32 / nrt_hyperconv3d_f32 with padding_same = 1,
 * except that pad_before[d] (0 .. (k_d - 1) * dilation) zeros precede the input along axis d and (k_d - 1) * dilation - pad_before[d]
 * follow it; the output keeps the input's shape.  'same' pads floor((k - 1) * dilation / 2) before, so the transpose of a 'same'
 * convolution -- its input gradient -- pads (k - 1) * dilation - floor((k - 1) * dilation / 2) before: the two differ for even
 * kernels.  Where pad_before is what 'same' pads, the call IS the 'same' call (every variant); otherwise the direct kernel runs
 * (variant 0 or 1) or, for nrt_conv3d_pad_f32, the 2x2x2 MFMA arm (variant 6, under the conditions stated at nrt_conv3d_f32;
 * its halo follows pad_before); another variant is NRT_ERR_UNSUPPORTED.  A pad_before outside its range or NULL: NRT_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------------------------ */
int nrt_conv3d_pad_f32(const float *src0, int c0, const float *src1, int c1, const int up[], const float *weights,
                       const float *packed_weights, const float *bias, float *out, int batch, const int shape[], const int ksize[],
                       int cout, int dilation, const int pad_before[], int activation, int variant, void *stream);
int nrt_hyperconv3d_pad_f32(const float *src, int cin, const float *weights, const float *packed_weights, const float *bias,
                            float *out, int batch, const int shape[], const int ksize[], int cout, int dilation,
                            const int pad_before[], int activation, int variant, void *stream);

/* ------------------------------------------------------------------------------------------
 * Patch-wise volume prediction, neurite/tf/utils/seg.py (csrc/seg.hip): the arg-max of a probability map with the probability of a
 * label in the same pass, a label lookup, patch extraction and its inverse, the quilt.  Four streaming kernels: no atomics, no
 * workspace, no host synchronisation (all capture into a graph); run-to-run bit-identical.  Base pointers need the alignment of their
 * element type only (wider accesses are used where the shape and the pointers allow).  Checked before any launch, by every call:
 * NRT_ERR_INVALID_ARG for a NULL tensor or shape array that is not optional and for a size < 1; NRT_ERR_UNSUPPORTED for a dtype
 * outside the ones named and for 2^31 or more elements in any one tensor.
 *
 *   nrt_seg_argmax     pred [n_vox, channels] (NRT_DT_F32 / NRT_DT_BF16), 1 <= channels <= 256 (more: NRT_ERR_UNSUPPORTED).
 *                      labels [n_vox] (int64 if labels_i64 else int32; may be NULL) = np.argmax(pred, -1): the first index wins a tie,
 *                      a NaN counts as the maximum (the first NaN wins).  prob [n_vox] float32 (may be NULL) =
 *                      pred[v, l] / sum_c pred[v, c] (float32 sum), where l = of_labels[v] (int64 if of_labels_i64 else int32) or,
 *                      with of_labels NULL, the arg-max itself; an l outside [0, channels) gives NaN and reads nothing.  labels and
 *                      prob both NULL, or of_labels without prob: NRT_ERR_INVALID_ARG.  channels % 4 == 0: a group of lanes shares a
 *                      voxel's channels with 8- / 16-byte loads and merges (value, index) pairs across lanes; else a thread per voxel.
 *   nrt_seg_recode     out[v] = lookup[seg[v]] for v < n; seg int64 if seg_i64 else int32, lookup [n_lookup] and out float32.
 *                      An index outside [0, n_lookup) writes 0 and reads nothing.
 *   nrt_patch_extract  vol [*vol_shape, channels] (rank ndim 1 .. 3; NRT_DT_F32 / NRT_DT_BF16) -> patches [count, *patch_size,
 *                      channels]: the patches n0 .. n0 + count - 1 of the grid; patch n has the grid index unravel_index(n, grid_size)
 *                      (C order) and starts at index * patch_stride.  NRT_ERR_INVALID_ARG: ndim outside 1 .. 3, a stride < 1, a grid
 *                      that does not fit ((grid - 1) * stride + patch > vol on an axis), n0 < 0 or n0 + count > prod(grid_size).
 *   nrt_patch_quilt    patches [prod(grid_size), *patch_size, channels] (NRT_DT_F32 / NRT_DT_I32, converted to float32) ->
 *                      vol [*((grid - 1) * stride + patch), channels] float32.  An output element reduces the patch values that cover
 *                      it, read in ascending patch index, NaN values skipped (np.nanmean / np.nanmedian over the stack of patches):
 *                      NRT_QUILT_MEAN    float32 sum in that order / the number of values; any cover count.
 *                      NRT_QUILT_MEDIAN  exact selection, (a + b) / 2 of the two middle values of an even count; up to 64 covering
 *                                        patches: prod(ceil(patch / stride)) > 64 is NRT_ERR_UNSUPPORTED.
 *                      No cover (stride > patch) or only NaN values: NaN.  Another `reduce`: NRT_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------------------------ */
typedef enum { NRT_QUILT_MEAN = 0, NRT_QUILT_MEDIAN = 1 } nrt_quilt_reduce;
int nrt_seg_argmax(const void *pred, int dtype, long long n_vox, int channels, void *labels, int labels_i64, const void *of_labels,
                   int of_labels_i64, float *prob, void *stream);
int nrt_seg_recode(const void *seg, int seg_i64, long long n, const float *lookup, long long n_lookup, float *out, void *stream);
int nrt_patch_extract(const void *vol, int dtype, int ndim, const int vol_shape[], int channels, const int patch_size[],
                      const int patch_stride[], const int grid_size[], long long n0, long long count, void *patches, void *stream);
int nrt_patch_quilt(const void *patches, int dtype, int ndim, const int patch_size[], const int patch_stride[], const int grid_size[],
                    int channels, int reduce, float *vol, void *stream);

/* ------------------------------------------------------------------------------------------
 * The registration losses of VoxelMorph (csrc/vxmloss.hip): the windowed normalised cross-correlation of two images (vxm.losses.NCC)
 * and the smoothness penalty on a displacement field (vxm.losses.Grad), each with its gradient.  voxelmorph is not in the reference
 * tree: the semantics are restated, not pinned.  float32, channels-last [batch, *shape, channels]; shape has three extents,
 * a spatial rank below 3 arrives with leading extents of 1 (and window 1).  An extent smaller than the window is legal.
 *   nrt_ncc_f32        n = prod(win) * channels.  Box sums S_I, S_J, S_II, S_JJ, S_IJ of I, J, I I, J J, I J over the window and all channels,
 *                      stride 1, zero padded as TensorFlow's 'SAME' pads ((w - 1) / 2 zeros in front; even windows allowed); each is a plain
 *                      sum of its terms (no running add-and-subtract: exact on small-integer images).  Then, one float32 rounding per
 *                      operation:  uI = S_I / n, uJ = S_J / n, cross = max(((S_IJ - uJ S_I) - uI S_J) + (uI uJ) n, eps),
 *                      Ivar = max((S_II - (2 uI) S_I) + (uI uI) n, eps), Jvar likewise, cc = (cross / Ivar) (cross / Jvar).
 *                      sums [batch, V, 5] (the five sums as the epilogue sees them), cc [batch, V], loss [batch] = -mean(cc): each may be
 *                      NULL, not all three.  One launch, and a tiny second one for `loss`.
 *   nrt_ncc_bwd_f32    gcc [batch, V] (the upstream gradient of cc) and / or gloss [batch] (that of loss): at least one.  gI, gJ (the
 *                      layout of I, J): either may be NULL, not both.  max passes its gradient where the unclamped value >= eps and
 *                      nothing below.  Two launches of the forward's box-sum kernel; nothing of the forward is kept but I and J.
 *   nrt_ncc_workspace_bytes   what both calls need at most (the backward: 20 bytes per voxel); 0 for a geometry they refuse.  The
 *                      forward needs a workspace only for `loss`.
 *   nrt_grad_loss_f32  d_i = y[.., 1:, ..] - y[.., :-1, ..] along each of the last nd (1 .. 3) extents of shape; m_i = the mean over everything
 *                      but the batch of |d_i| (penalty 1) or d_i^2 (penalty 2); loss [batch] = ((m_0 + m_1) + m_2) / nd * loss_mult (pass 1
 *                      for none).  An axis of extent 1 has no differences: its mean is 0 / 0.  Workspace: batch * 6144 bytes.
 *   nrt_grad_loss_bwd_f32   gy_q = sum_i s_i (phi(y_q - y_{q - e_i}) - phi(y_{q + e_i} - y_q)), phi = sign (penalty 1, sign(0) = 0) or 2 d
 *                      (penalty 2), s_i = gloss[b] loss_mult / (nd count_i).  One pass, no workspace.
 * No atomics, no host synchronisation (every call captures into a graph); every sum has a fixed partition and order: run-to-run
 * bit-identical.  Base pointers and the workspace need 4-byte alignment only (the Grad kernels use 16-byte accesses where
 * channels % 4 == 0 and the pointers allow).  Checked before any launch: NRT_ERR_INVALID_ARG for a NULL tensor, shape or win that is not
 * optional, batch or an extent < 1, a NaN or negative eps, nd outside 1 .. 3 or a leading extent != 1 beyond nd, another penalty;
 * NRT_ERR_UNSUPPORTED for a window outside 1 .. 15, channels outside 1 .. 16 (NCC) and 2^31 or more elements in a tensor;
 * NRT_ERR_WORKSPACE for a missing or short workspace.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_ncc_workspace_bytes(int batch, const int shape[], int channels, const int win[]);
int nrt_ncc_f32(const float *I, const float *J, int batch, const int shape[], int channels, const int win[], float eps, float *sums,
                float *cc, float *loss, void *workspace, size_t workspace_bytes, void *stream);
int nrt_ncc_bwd_f32(const float *I, const float *J, const float *gcc, const float *gloss, int batch, const int shape[], int channels,
                    const int win[], float eps, float *gI, float *gJ, void *workspace, size_t workspace_bytes, void *stream);
int nrt_grad_loss_f32(const float *y, int batch, const int shape[], int nd, int channels, int penalty, float loss_mult, float *loss,
                      void *workspace, size_t workspace_bytes, void *stream);
int nrt_grad_loss_bwd_f32(const float *y, const float *gloss, int batch, const int shape[], int nd, int channels, int penalty,
                          float loss_mult, float *gy, void *stream);

/* ------------------------------------------------------------------------------------------
 * Warp by an affine matrix in one kernel, and the gradient wrt the matrix (csrc/affine_warp.hip): SpatialTransformer on an affine
 * input ('ij' indexing) without the dense displacement field between nrt_affine_to_dense_shift_f32 and nrt_interpn_f32.
 * float32, channels-last: vol [batch, *vol_shape, channels], matrix [matrix_batch, ndim, ndim + 1] with matrix_batch = batch, or 1 for
 * one transform shared by the batch; out / grad_out [batch, *out_shape, channels]; ndim 2 or 3; method NRT_INTERP_LINEAR / _NEAREST.
 *   nrt_affine_warp_f32      the location of output voxel q is formed in registers with the roundings of the two-kernel path:
 *                            p = (float)q - c (c = (out_shape - 1) / 2 when shift_center, else 0), s_i = (((M_i0 p_0 + M_i1 p_1) + ..) +
 *                            M_iD) - p_i, loc_i = (float)q_i + s_i, one rounding per operation; then the corner arithmetic, blend order
 *                            and fill of nrt_interpn_f32.  out is bit for bit what that kernel gives on the materialised field.
 *   nrt_affine_warp_bwd_f32  grad_matrix [matrix_batch, ndim, ndim + 1] = sum_q gloc_i(q) p_j(q) (p_D = 1; summed over the batch as well
 *                            when matrix_batch == 1), gloc = d (sum_c grad_out_c out_c) / d loc as nrt_interpn_bwd_f32 defines it (through
 *                            the clipped location, closed range, masked by 1 - oob under a fill value); all zeros for nearest.  No
 *                            gradient field is written: every block leaves one row of partial sums in the workspace, a second launch
 *                            adds the rows in index order in float64.  The gradient wrt vol is nrt_interpn_bwd_f32's on the field.
 *   nrt_affine_warp_workspace_bytes   what the backward needs; 0 for a geometry it refuses.
 * No atomics, no host synchronisation (both calls capture into a graph); the grid and the order of every sum depend on the shapes only:
 * run-to-run bit-identical.  Base pointers need 4-byte alignment only (16-byte accesses are used where channels % 4 == 0 and the
 * pointers allow).  Checked before any launch: NRT_ERR_INVALID_ARG for a NULL tensor or shape, batch, channels or an extent < 1, a
 * matrix_batch that is neither 1 nor batch, another method; NRT_ERR_UNSUPPORTED for ndim outside {2, 3}, 2^31 or more elements in a
 * tensor and batch > 65535; NRT_ERR_WORKSPACE for a missing or short workspace.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_affine_warp_workspace_bytes(int ndim, const int out_shape[], int channels, int batch);
int nrt_affine_warp_f32(const float *vol, const float *matrix, float *out, int ndim, const int vol_shape[], const int out_shape[],
                        int channels, int batch, int matrix_batch, int shift_center, int method, int has_fill, float fill_value,
                        void *stream);
int nrt_affine_warp_bwd_f32(const float *vol, const float *matrix, const float *grad_out, float *grad_matrix, int ndim,
                            const int vol_shape[], const int out_shape[], int channels, int batch, int matrix_batch, int shift_center,
                            int method, int has_fill, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The Jacobian determinant of a displacement field and its gradient (csrc/jacobian.hip): vxm.py.utils.jacobian_determinant.
 * voxelmorph is not in the reference tree: the semantics are restated, not pinned; the oracle is np.gradient.
 * float32, channels-last disp [batch, *shape, nd]: `shape` holds exactly nd extents, nd 2 or 3, 'ij' coordinates.
 *   nrt_jacdet_f32      G[a][c] = the np.gradient difference of disp[.., c] along spatial axis a: (f[i + 1] - f[i - 1]) * 0.5 inside,
 *                       f[1] - f[0] and f[n - 1] - f[n - 2] at the two ends; J[a][c] = G[a][c] + (a == c);
 *                       3-D det = J0[0] (J1[1] J2[2] - J1[2] J2[1]) - J0[1] (J1[0] J2[2] - J1[2] J2[0]) + J0[2] (J1[0] J2[1] - J1[1] J2[0]),
 *                       2-D det = J0[0] J1[1] - J1[0] J0[1]; one float32 rounding per operation, in this order.  One pass over disp
 *                       writes any of (each may be NULL, not all three):
 *                         det   [batch, V] float32, the map;
 *                         stats [batch, 5] 8-byte slots (8-byte aligned): the count of det <= 0 as int64, then min, max, sum det and
 *                               sum det^2 as float64 (min and max are the float32 values; the sums are formed in float64);
 *                         loss  [batch] float32 = float32(sum max(0, -det) / V), the sum in float64.
 *                       stats and loss need the workspace (a tiny second launch adds the per-block rows in block order); the map is
 *                       not needed for them.
 *   nrt_jacdet_bwd_f32  gdisp (the layout of disp) = sum_a sum_p coef_a(p, q) w[p] cof[p][a][c]: cof the cofactor matrix of J at p,
 *                       coef the stencil weight with which q enters G[a] at p (+-1/2 from an interior p, +-1 from p = 0 and p = n - 1),
 *                       w[p] = gdet[p] (the upstream gradient of det, [batch, V]) and / or -gloss[b] / V [det[p] < 0] (that of loss,
 *                       [batch]; the sub-gradient at det == 0 is 0): at least one.  One gather pass that rebuilds J from disp: nothing of
 *                       the forward is kept, no workspace.
 *   nrt_jacdet_workspace_bytes   what the forward needs for stats or loss; 0 for a geometry the calls refuse.
 * No atomics, no host synchronisation (both calls capture into a graph), no memset; every sum has a fixed partition and order: run-to-run
 * bit-identical.  Base pointers and the workspace need 4-byte alignment only.  Checked before any launch: NRT_ERR_INVALID_ARG for a NULL
 * disp, shape or gdisp, no output or no upstream gradient at all, batch < 1, an extent < 2, a stats pointer off 8 bytes;
 * NRT_ERR_UNSUPPORTED for nd outside {2, 3}, 2^31 or more elements in a tensor and batch > 65535; NRT_ERR_WORKSPACE for a missing or
 * short workspace.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_jacdet_workspace_bytes(int batch, const int shape[], int nd);
int nrt_jacdet_f32(const float *disp, int batch, const int shape[], int nd, float *det, void *stats, float *loss, void *workspace,
                   size_t workspace_bytes, void *stream);
int nrt_jacdet_bwd_f32(const float *disp, const float *gdet, const float *gloss, int batch, const int shape[], int nd, float *gdisp,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * Exact Euclidean distance transforms and surface-distance reductions (csrc/edt.hip).  They replace a copy of every
 * volume to the host, scipy.ndimage.distance_transform_edt there (what VoxelMorph's dist_trf / signed_dist_trf call; voxelmorph is not
 * in the reference tree: restated, not pinned; the oracle is the definition, brute force) and a copy back.
 * out [batch, *shape, channels] float32, `shape` holds nd extents (2 or 3), each at most 1024.  The feature set comes from exactly one of
 *   mask   [batch, *shape] uint8: nonzero voxels (nlabels 1, labels NULL, channels 1), or
 *   ids    [batch, *shape] int32 with labels [nlabels] int32 on the device: channel l holds the transform of ids == labels[l]
 *          (channels = nlabels); with NRT_EDT_ANY_OF the set is "ids in labels" and channels = 1.
 * flags: NRT_EDT_SURFACE  (ids only) the features are the set's voxels with a face neighbour (2 nd of them) outside the set, the
 *                         outside of the volume counting as outside the set: m & ~binary_erosion(m), border_value 0;
 *        NRT_EDT_INVERT   the complement of the feature set;
 *        NRT_EDT_SQUARED  squared distances (no root);
 *        NRT_EDT_SIGNED   +d(p, set) outside the set, -d(p, complement) inside it (VoxelMorph's signed_dist_trf; with SQUARED the
 *                         squares carry the sign): two transforms, the first kept in `workspace` (one float volume of out's size,
 *                         nrt_edt_workspace_bytes); not with SURFACE.
 * sampling: NULL (unit voxels) or nd voxel sizes ON THE HOST, finite and positive.
 *   nrt_edt_f32   out = min over the feature voxels q of sqrt(sum_a (s_a (p_a - q_a))^2), 0 on the set, by one pass per axis on out in
 *                 place: f[i] = min_j fl(g[j] + fl(fl(s |i - j|)^2)), float32, no fused multiply-add, then the correctly rounded root.
 *                 At unit spacing every intermediate is an integer below 2^24: the squares are exact and the result is the correctly
 *                 rounded root of the exact squared distance.  An empty feature set gives +inf everywhere (SIGNED of a full set: -inf);
 *                 scipy returns arbitrary finite values there.
 *   nrt_surface_stats_f32   t [batch, *shape] int32, d2 [batch, *shape, nlabels] (a SQUARED transform, from the other map's surfaces):
 *                 over the surface voxels (as above) of label l in entry b, stats[b][l] = three 8-byte slots (8-byte aligned): their
 *                 count (int64), max d2 and sum sqrt(d2) (float64; the root is the correctly rounded float32 one, the sum is formed in
 *                 float64 from per-block partials added in block order; max is -inf where the count is 0).  hist, if given: [batch, nlabels, nbins] uint32, bin (int) d2 is
 *                 incremented for every such voxel with 0 <= d2 < nbins (the caller zeroes it, and may run both directions into one).
 * No float atomics (the histogram's integer adds commute), no host synchronisation (the calls capture into a graph), no allocation:
 * run-to-run bit-identical.  Pointers need their type's alignment only.  Checked before any launch: NRT_ERR_INVALID_ARG for a NULL out,
 * t, labels (with ids), d2, stats or shape, both or neither of mask and ids, mask with labels / nlabels != 1 / SURFACE / ANY_OF, SURFACE
 * with SIGNED, an unknown flag, batch or an extent < 1, a sampling value that is not finite and positive, hist with nbins < 1;
 * NRT_ERR_UNSUPPORTED for nd outside {2, 3}, an extent above 1024, nlabels outside 1 .. 256, batch > 65535, 2^31 or more elements in
 * out (or in hist; nbins above 2^24); NRT_ERR_WORKSPACE for a missing or short workspace.
 * ------------------------------------------------------------------------------------------ */
#define NRT_EDT_SURFACE 1
#define NRT_EDT_INVERT 2
#define NRT_EDT_SIGNED 4
#define NRT_EDT_SQUARED 8
#define NRT_EDT_ANY_OF 16
size_t nrt_edt_workspace_bytes(int batch, const int shape[], int nd, int channels);
int nrt_edt_f32(const void *mask, const int *ids, const int *labels, int nlabels, int batch, const int shape[], int nd,
                const float sampling[], int flags, float *out, void *workspace, size_t workspace_bytes, void *stream);
size_t nrt_surface_stats_workspace_bytes(int batch, const int shape[], int nd, int nlabels);
int nrt_surface_stats_f32(const int *t, const int *labels, int nlabels, const float *d2, int batch, const int shape[], int nd,
                          void *stats, unsigned *hist, long long nbins, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Connected-component labelling and the mask clean-up built on it (csrc/ccl.hip, csrc/ccl_core.h).  They replace a copy
 * of every volume to the host, scipy.ndimage.label / binary_fill_holes there, and a copy back.
 * The input is [batch, *shape], `shape` holds nd extents (2 or 3), and comes from exactly one of
 *   mask   [batch, *shape] uint8: nonzero voxels are foreground (nlabels 1, labels NULL), or
 *   ids    [batch, *shape] int32 with labels [nlabels] int32 (1 .. 256 distinct ids) on the device: ids outside the list are background.
 * Two neighbouring voxels belong to one component when both are foreground and carry the same id; the neighbourhood is scipy's
 * generate_binary_structure(nd, connectivity), connectivity 1 .. nd (4 / 8 neighbours in 2-D, 6 / 18 / 26 in 3-D).
 *   nrt_ccl_label_i32   components [batch, *shape] int32: 0 on the background, else the number of the voxel's component; the
 *                 components of an entry are numbered 1, 2, ... in raster (C) order of their first voxel, per entry: the numbering of
 *                 scipy.ndimage.label.  count [batch] int32: the components of each entry.
 *   nrt_ccl_select      the components are sized and tested, per (entry, label slot; one slot for a mask).  mode is a sum of
 *                 NRT_CCL_LARGEST      keep the largest component of each (entry, slot); ties go to the lowest component number;
 *                 NRT_CCL_MIN_SIZE     keep components of at least min_size voxels;
 *                 NRT_CCL_BORDER_FREE  keep components without a voxel at the border of the volume (first or last along an axis);
 *                 NRT_CCL_INVERT       (mask only) the foreground is the ZERO voxels, and the voxels of the set itself are written
 *                                      as kept: with BORDER_FREE the output is binary_fill_holes(mask, structure);
 *                 a component is kept when it passes every test asked for (mode 0 keeps all).  out, if given: for a mask
 *                 [batch, *shape] uint8, 1 where the voxel is kept, else 0; for ids [batch, *shape] int32, the id map with the voxels
 *                 of rejected components set to `fill` (ids outside the list pass through).  table, if given: [batch, nlabels, 2]
 *                 int32, the number of components and the size of the largest (0 0 where the slot is empty).  One of the two at least.
 * workspace: nrt_ccl_workspace_bytes (nlabels 1 for a mask), 8-byte aligned; the call initialises what it uses of it, every time.
 * Integer atomics only, no workgroup waits for another, no host synchronisation (the calls capture into a graph), no allocation;
 * the results do not depend on the schedule: bit-identical run to run.  Checked before any launch, in this order:
 * NRT_ERR_INVALID_ARG for a NULL components, count or shape, table and out both NULL, both or neither of mask and ids, ids without
 * labels, mask with labels or nlabels != 1, an unknown mode bit, min_size < 0, INVERT with ids, batch < 1, nd outside {2, 3}, an extent
 * < 1, connectivity outside 1 .. nd, nlabels outside 1 .. 256; NRT_ERR_UNSUPPORTED for batch > 65535 or 2^31 or more voxels
 * (32-bit indexing); last, NRT_ERR_WORKSPACE for a missing, misaligned or short workspace.
 * ------------------------------------------------------------------------------------------ */
#define NRT_CCL_LARGEST 1
#define NRT_CCL_MIN_SIZE 2
#define NRT_CCL_BORDER_FREE 4
#define NRT_CCL_INVERT 8
size_t nrt_ccl_workspace_bytes(int batch, const int shape[], int nd, int nlabels);
int nrt_ccl_label_i32(const void *mask, const int *ids, const int *labels, int nlabels, int batch, const int shape[], int nd,
                      int connectivity, int *components, int *count, void *workspace, size_t workspace_bytes, void *stream);
int nrt_ccl_select(const void *mask, const int *ids, const int *labels, int nlabels, int batch, const int shape[], int nd,
                   int connectivity, int mode, int min_size, int fill, int *table, void *out, void *workspace, size_t workspace_bytes,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Exact percentiles of every batch entry of a volume and the percentile intensity normalisation (csrc/select.hip,
 * csrc/select_core.h).  They replace torch.quantile (a sort and a sorted copy of every volume, no mask) or a round trip
 * through the host.
 *   nrt_percentile   x [batch, voxels] stored as `dtype` (NRT_DT_F32 / NRT_DT_BF16 / NRT_DT_F16); mask NULL or [batch, voxels] uint8
 *                 (nonzero = selected).  The population of an entry is its selected and, with NRT_PCT_IGNORE_NAN, non-NaN elements:
 *                 n of them, sorted ascending as s (-0.0 == +0.0, NaN last).  positions: nq (1 .. 8) fractions f in [0, 1], float64,
 *                 on the HOST (read during the call).  pos = (n - 1) f in float64, a = s[floor(pos)], b = s[ceil(pos)],
 *                 t = pos - floor(pos), and with a, b widened to float64 and the result rounded to float32 once
 *                   NRT_PCT_LINEAR    a + (b - a) t  if t < 0.5, else  b - (b - a)(1 - t)      (NumPy's formula)
 *                   NRT_PCT_LOWER     a            NRT_PCT_HIGHER  b            NRT_PCT_MIDPOINT  (a + b) / 2
 *                 out [batch, nq] float32; out_lower, out_upper [batch, nq] float32 (a and b) and out_count [batch] int32 (n) may
 *                 be NULL.  An empty population gives NaN; so does, without NRT_PCT_IGNORE_NAN, a population with a NaN in it (all
 *                 three outputs).  +-inf are ordinary values (inf - inf in the interpolation is NaN, as in NumPy).
 *   nrt_rescale_clip_f32   y [batch, voxels] float32 = (x - lo) / (hi - lo) in float32 with lo = lo[b * stride], hi = hi[b * stride]
 *                 read on the device; 0 where hi == lo; with clip != 0 clipped to [0, 1] (a NaN stays); then, unless
 *                 (out_min, out_max) is (0, 1), out_min + y * (out_max - out_min); NaN where lo or hi is NaN.
 * workspace: nrt_select_workspace_bytes, 16-byte aligned; the call initialises what it uses of it, every time.  A radix select on the
 * monotone key of the floats: three counting passes over x (two for the 16-bit types), integer atomics only, no workgroup waits for
 * another, no host synchronisation (the calls capture into a graph), no allocation; the results do not depend on the schedule:
 * bit-identical run to run.  Checked before any launch, in this order: NRT_ERR_INVALID_ARG for a NULL x, positions, out (lo, hi, y), an
 * unknown dtype, method or flag, batch < 1, voxels < 1, nq outside 1 .. 8, a position outside [0, 1] or NaN (stride < 1, a NaN
 * out_min / out_max); NRT_ERR_UNSUPPORTED for batch > 65535 or batch * voxels >= 2^31 (32-bit indexing); last, NRT_ERR_WORKSPACE for a
 * missing, misaligned or short workspace.
 * ------------------------------------------------------------------------------------------ */
#define NRT_PCT_LINEAR 0
#define NRT_PCT_LOWER 1
#define NRT_PCT_HIGHER 2
#define NRT_PCT_MIDPOINT 3
#define NRT_PCT_IGNORE_NAN 1
size_t nrt_select_workspace_bytes(int batch, long long voxels, int nq);
int nrt_percentile(const void *x, int dtype, const void *mask, int batch, long long voxels, const double positions[], int nq, int method,
                   int flags, float *out, float *out_lower, float *out_upper, int *out_count, void *workspace, size_t workspace_bytes,
                   void *stream);
int nrt_rescale_clip_f32(const void *x, int dtype, int batch, long long voxels, const float *lo, const float *hi, int stride, int clip,
                         float out_min, float out_max, float *y, void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-label region statistics of an integer id map and the confusion matrix of two id maps (csrc/labelstats.hip,
 * csrc/labelstats_core.h).  They replace a [batch, *shape, nlabels] one-hot tensor and its reductions, torch.bincount /
 * scatter_add (float atomics: sums that change from run to run), or a copy to the host and scipy.ndimage.sum / center_of_mass /
 * find_objects there.
 * The label slots: labels [nlabels] int32 on the device, 1 .. 256 distinct ids of any int32 value; slot l collects the voxels with
 * ids == labels[l].  With labels NULL slot l is the id l, and ids outside [0, nlabels) belong to no slot.  An id that is in no slot is
 * never used as an index.
 *   nrt_label_stats   ids [batch, *shape] int32, `shape` holds nd extents (2 or 3); image NULL or [batch, *shape, channels], channels
 *                 last, 1 .. 4 channels, stored as `dtype` (NRT_DT_F32 / NRT_DT_BF16 / NRT_DT_F16) and widened to float32.  Outputs,
 *                 each but counts may be NULL:
 *                   counts     [batch, nlabels] int64          the voxels of the slot
 *                   coord_sums [batch, nlabels, nd] int64      the sum of the voxel index along each axis
 *                   bbox       [batch, nlabels, 2, nd] int32   the smallest and the largest index along each axis, both inclusive;
 *                                                              an empty slot holds (shape[a], -1)
 *                   sums       [batch, nlabels, channels, 2] float64   the sum of x and of x * x (float32 products); a NaN propagates
 *                   minmax     [batch, nlabels, channels, 2] float32   min and max as fminf / fmaxf form them: a NaN is skipped, and
 *                                                              an empty or all-NaN slot holds (+inf, -inf)
 *                 sums and minmax need the image.  The integer outputs are exact.  The float sums: every wave adds its voxels of a slot
 *                 in a fixed lane order and its 64-voxel steps in their order in float32, a block adds its four waves and the call the
 *                 blocks of an entry (32 runs of consecutive blocks, then the runs) in a fixed order in float64; the shares follow
 *                 from the geometry alone.
 *   nrt_label_confusion_i32   a, b [batch, voxels] int32; counts [batch, nlabels + 1, nlabels + 1] int64, zeroed by the call:
 *                 counts[e, i, j] = the voxels of entry e whose a is in slot i and whose b is in slot j; the last row and column
 *                 collect the ids that are in no slot, so every voxel is counted exactly once.
 * workspace: nrt_label_stats_workspace_bytes (channels 0 without an image) / nrt_label_confusion_workspace_bytes, 16-byte aligned; the
 * call initialises what it uses of it, every time.  No float atomics; integer atomics where they commute; no workgroup waits for
 * another, no host synchronisation (the calls capture into a graph), no allocation; the results do not depend on the schedule:
 * bit-identical run to run.  Checked before any launch, in this order: NRT_ERR_INVALID_ARG for a NULL ids (a, b), counts or shape, sums
 * or minmax without an image, an unknown dtype with an image, batch < 1, nd outside {2, 3}, an extent (voxels) < 1, channels outside
 * 1 .. 4 with an image, nlabels outside 1 .. 256; NRT_ERR_UNSUPPORTED for batch > 65535 or batch * voxels >= 2^31 (32-bit indexing);
 * last, NRT_ERR_WORKSPACE for a missing, misaligned or short workspace.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_label_stats_workspace_bytes(int batch, const int shape[], int nd, int nlabels, int channels);
int nrt_label_stats(const int *ids, const int *labels, int nlabels, const void *image, int dtype, int channels, int batch,
                    const int shape[], int nd, long long *counts, long long *coord_sums, int *bbox, double *sums, float *minmax,
                    void *workspace, size_t workspace_bytes, void *stream);
size_t nrt_label_confusion_workspace_bytes(int batch, long long voxels, int nlabels);
int nrt_label_confusion_i32(const int *a, const int *b, const int *labels, int nlabels, int batch, long long voxels, long long *counts,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Binary morphology, box minimum / maximum filters and box rank filters of 2-D and 3-D volumes (csrc/morph.hip, csrc/morph_core.h;
 * DESIGN 4.6o): scipy.ndimage.binary_erosion / binary_dilation, minimum_filter / maximum_filter (grey erosion / dilation by a flat
 * box) and rank_filter / median_filter / percentile_filter without a copy to the host.  Exact integer and order-statistic results.
 * Common to the three: x and out [batch, *shape], `shape` holds nd extents (2 or 3), out is not x.
 *   nrt_binary_morph   x stored as `dtype` (NRT_DT_U8: one byte per voxel, also a bool tensor; NRT_DT_I32; NRT_DT_F32); a voxel is set
 *                 where x != 0 (read in the kernel).  out: one byte per voxel, 0 or 1.  `structure`: the 3 x 3 (x 3) structuring
 *                 element as 27 bits, bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) its entry at the offset (dz, dy, dx); with nd = 2 only
 *                 the plane dz = 0 (bits 9 .. 17) may be set.  Any structure is taken: asymmetric, without its centre, empty.
 *                 dilate 0: out[p] = AND over the set entries o of m[p + o] (erosion); dilate 1: out[p] = OR of m[p - o].  Every voxel
 *                 outside the volume holds border_value (0 or 1).  `iterations` >= 1 single steps are composed.  One launch runs up to
 *                 4 steps on bit-packed rows in LDS; more steps are further launches through the workspace
 *                 (nrt_binary_morph_workspace_bytes: one byte per voxel above 4 iterations, else 0).  The last extent may be up to 1024.
 *   nrt_minmax_filter  x and out stored as `dtype` (NRT_DT_F32 or NRT_DT_I32).  size [nd]: the box, every entry odd and 1 .. 31.
 *                 want_max 0: the minimum over the box, 1: the maximum; one pass per axis whose size is above 1.  The workspace
 *                 (nrt_minmax_filter_workspace_bytes: 4 bytes per voxel when two or more sizes are above 1) needs 4-byte alignment.
 *   nrt_rank_filter    x and out as for nrt_minmax_filter.  size [nd]: the box, every entry odd, at most 27 samples in all.  out = the
 *                 rank-th smallest (0 <= rank < samples) of the samples of the box, compared by value.
 *   mode (both filters): how an index outside [0, n) is read.  0 reflect (d c b a | a b c d | d c b a), 1 mirror (d c b | a b c d |
 *                 c b a), 2 nearest (a a a | a b c d | d d d), 3 constant (cval, converted to `dtype` by truncation); the fold holds
 *                 for a window wider than the axis.  A window that holds a NaN has an unspecified result; +-inf and both zeros are
 *                 ordinary values (-0.0 == 0.0, either may be returned).
 * No atomics, no workgroup waits for another, no host synchronisation (the calls capture into a graph), no allocation; bit-identical
 * run to run.  Checked before any launch, in this order: NRT_ERR_INVALID_ARG for a NULL x, out, shape or size, an unknown dtype,
 * batch < 1, nd outside {2, 3}, an extent < 1, a structure beyond its bits, iterations < 1, a border_value / dilate / want_max that is
 * neither 0 nor 1, an even or non-positive size, an unknown mode, a NaN cval (or one that int32 does not hold, for NRT_DT_I32), a rank
 * outside the box; NRT_ERR_UNSUPPORTED for a size above 31 (27 samples for the rank filter), batch > 65535, batch * voxels >= 2^31
 * (32-bit indexing), a last extent above 1024 and, with nd = 3, a first extent above 524280 (binary); last, NRT_ERR_WORKSPACE for a missing, misaligned or short workspace.
 * ------------------------------------------------------------------------------------------ */
size_t nrt_binary_morph_workspace_bytes(int batch, const int shape[], int nd, int iterations);
int nrt_binary_morph(const void *x, int dtype, int batch, const int shape[], int nd, int structure, int iterations, int border_value,
                     int dilate, void *out, void *workspace, size_t workspace_bytes, void *stream);
size_t nrt_minmax_filter_workspace_bytes(int batch, const int shape[], int nd, const int size[]);
int nrt_minmax_filter(const void *x, int dtype, int batch, const int shape[], int nd, const int size[], int mode, double cval,
                      int want_max, void *out, void *workspace, size_t workspace_bytes, void *stream);
int nrt_rank_filter(const void *x, int dtype, int batch, const int shape[], int nd, const int size[], int rank, int mode, double cval,
                    void *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NEURITE_AMD_H */
