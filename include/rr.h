/*
 * rr.h — C-ABI of librr, the MI355X (gfx950) embed+search library.
 *
 * The reference (Mak-GIBA/research_image_retrieval, src/benchmark) is pure
 * Python/PyTorch and has no FFI of its own: its "operator API" is duck-typed
 * Python.  Every entry point below replaces one torch/numpy
 * call site on the reference's extract-and-rank hot path; the citation in
 * each comment names that site (paths relative to src/benchmark/).  The
 * Python mirror of the reference API (research_image_retrieval_amd/) binds
 * these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - All tensors are caller-owned DEVICE pointers (e.g. torch data_ptr()).
 *     Dense row-major, fp32 unless stated.  Images/activations are NHWC.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Every call is stream-ordered and asynchronous: no host sync inside,
 *     except the explicit *_collect / *_sync helpers.
 *   - Return value: 0 on success, a negative RR_E* code on error; the message
 *     is available from rr_last_error(h).  The library never aborts.
 *   - One handle per device; handles are independent across threads.  Every
 *     entry point runs on its handle's device: the calling thread's current
 *     HIP device is switched to it for the call and restored afterwards.
 */
#ifndef RR_H_
#define RR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_OK 0
#define RR_EINVAL (-1)    /* bad argument / unsupported shape */
#define RR_EHIP (-2)      /* HIP runtime error */
#define RR_EWORKSPACE (-3) /* workspace too small */
#define RR_EOVERFLOW (-4) /* candidate buffer overflow (see rr_cosine_topk) */

/* Words of an activation's max-|x| record (rr_conv2d_h2, rr_amax_f32): the
 * float bit patterns of per-wave maxima, hashed over this many words so no
 * single address takes every atomic.  Zero them before the producing call. */
#define RR_AMAX_SLOTS 64

typedef struct rr_handle_s* rr_handle_t;

/* ABI revision of this header.  Bumped when an existing entry changes its
 * arguments under the same name (a caller built against an older header would
 * pass shifted arguments): 2 = rr_alpha_qe gained n_rows (round 2); 3 = the
 * f16x2 entries rr_conv2d_h2 / rr_bottleneck_out_h2 / rr_stem_pool_h2 /
 * rr_split2_f16 / rr_amax_f32 were added (no existing entry changed); 4 =
 * rr_linear_bf16_ln / rr_ln_partials_bf16 were added (round 4; the ViT
 * LayerNorm fold); 5 = rr_bottleneck_seam_h2 was added and the tuning keys
 * RR_TUNE_SWEEP_ORDER (6), RR_TUNE_SWEEP_PF (7) and RR_TUNE_LP_IL (12)
 * were retired (round 5: they lost their A/Bs; rr_set_tuning returns
 * RR_EINVAL for them, and their numbers are not reused); RR_TUNE_LP_CFG value
 * 6 (the gallery-in-VGPR sweep) was retired then too, and the number was
 * REDEFINED in the same revision as the tests' hook for the three-A-stage
 * persistent bf16 tile (a caller of the old value 6 now gets that tile on
 * stored-C GEMMs and the cost-based pick on sweeps); and rr_linear_bf16_ln /
 * rr_ln_partials_bf16 now centre the bf16 rows on their 256-column tile
 * means with colsum per k tile (same arguments, new layout); 6 = entries
 * REMOVED: rr_bottleneck_seam_h2 (round 5's block seam, measured slower
 * than the two launches it fused) and the split-bf16 core's rr_conv2d_s3 /
 * rr_linear_s3 / rr_split3_bf16 (superseded by the f16x2 core in round 3);
 * the tuning keys RR_TUNE_SWEEP_FORM (14) and RR_TUNE_HALO_2D (15) were
 * added (round 6); 7 = entries ADDED: rr_dolg_local_pool and
 * rr_dolg_orth_fuse (the DOLG head; no existing entry changed);
 * rr_soa_attention (SOLAR's second-order attention block) was ADDED under 7
 * as well: no existing entry changed, so a caller built against the earlier
 * revision-7 header still passes the right arguments everywhere; likewise
 * rr_attention_hd128, rr_token_pool and rr_gelu (the Token head), and
 * rr_how_vlad and rr_how_asmk (the HOW head's aggregations), rr_sos_cov and
 * rr_linear_splitk (the SoSNet head: added, no existing entry changed),
 * rr_cls_attn_pool and rr_linear_splitk_ex (the token aggregator's folded last
 * layer: added, no existing entry changed), rr_spp_regions, rr_spp_max,
 * rr_spoc_refine and rr_linear_groupmax (the SpoC head: added, no existing
 * entry changed), rr_se_squeeze and rr_se_apply (the SE-ResNet trunk's gate:
 * added, no existing entry changed), and the native
 * trunk plan's rr_trunk_h2_* entries, rr_timing_collect_ex and the tuning key
 * RR_TUNE_TRUNK_PARTS (16); rr_timing_collect keeps its arguments and now
 * returns the UNION of the class's launch intervals (equal to the former sum
 * on one stream; see below); 8 = rr_h2_route was ADDED (which kernel
 * instance serves an rr_conv2d_h2 shape; no existing entry changed); 9 =
 * rr_gemm_route was ADDED (which kernel instance serves an fp32, bf16 or fp8
 * GEMM; no existing entry changed).
 * Bindings compare rr_abi_version() with the RR_ABI_VERSION they were
 * written against.                                                          */
#define RR_ABI_VERSION 9
int rr_abi_version(void);

/* ---- handle ------------------------------------------------------------ */
const char* rr_version(void);
int rr_create(int device, rr_handle_t* out);
int rr_destroy(rr_handle_t h);
const char* rr_last_error(rr_handle_t h);

/* Per-kernel-class HIP-event timing (used by bench.py for the roofline).
 * When enabled, every launch of a timed class is bracketed by hipEvents on
 * the launch stream; rr_timing_collect synchronises those events and returns
 * the accumulated milliseconds and launch count for `cls`, then resets it.
 * Classes: 0 = cosine GEMM with the fused top-k filter epilogue,
 *          1 = conv/linear GEMM, 2 = top-k select/merge,
 *          3 = elementwise (preprocess/resize/pool/norm),
 *          4 = dense cosine GEMM (top-k threshold seed, rr_cosine_scores),
 *          5 = fused attention (ViT).
 * The milliseconds are the length of the UNION of the class's launch
 * intervals: every launch's [start, stop] event pair is placed on one time
 * axis, as offsets from the class's first start event, and overlapping
 * intervals count once.  On one stream the intervals are disjoint and this is
 * the sum of the per-launch durations, as before; when launches of a class
 * co-run on several streams (the two-part trunk plan below) it is the time
 * during which the class occupied the chip, so a class time never exceeds the
 * wall time of the window.  The launch count is the number of launches.
 * rr_timing_collect_ex returns, from the same events, the union and the plain
 * sum of the per-launch durations (sum_ms >= union_ms; equal on one stream up
 * to the float rounding of the offsets); either pointer may be NULL. */
int rr_timing_enable(rr_handle_t h, int enable);
int rr_timing_collect(rr_handle_t h, int cls, double* ms, long long* launches);
int rr_timing_collect_ex(rr_handle_t h, int cls, double* union_ms, double* sum_ms, long long* launches);

/* The device a handle was created for (rr_create's `device`). */
int rr_get_device(rr_handle_t h, int* device);

/* Kernel tile-config overrides for this handle (tests and tuning tools; the
 * default 0 = the library's own pick, which the product path always uses).
 *   RR_TUNE_GEMM_CFG: exact-fp32 core tile, 22 (128x128), 41 (256x64), 88 (256x256)
 *   RR_TUNE_GEMM_BK:  exact-fp32 core k-tile depth, 16 or 32
 *   RR_TUNE_LP_CFG:   bf16/fp8 core (0, the default: for the bf16 stored-C GEMMs with
 *                     the ViT epilogues, N % 256 == 0 and K <= 1024, the persistent
 *                     256x256 k-stream; its one-tile form is 3), 1 (128x128), 2 (256x64),
 *                     3 (256x256), 6 (the persistent form with three A stages for the
 *                     epilogues without the LayerNorm fold, at any K; tests; this
 *                     value's meaning changed in ABI 5, see above),
 *                     4 (256x320 for bf16 filter / score sweeps, 256x256 otherwise),
 *                     5 (bf16 sweeps with K % 128 == 0, fp8 sweeps with K % 256 == 0:
 *                     256x256 8-phase pipeline; otherwise as 3, and like 3 the 128x128
 *                     tile where K is not a whole number of 128-byte k-tiles);
 *                     rr_gemm_route reports what a value selects
 *   RR_TUNE_S3_CFG:   f16x2 split core, 1..15 (the table of csrc/h2_route.hpp; rr_h2_route
 *                     reports what a value selects; 1, 2, 5 and 6 are accepted and mean the
 *                     library's pick among the one-tile configs 3, 4 and 7; 13 = the halo-staged stride-1 3x3 tile on
 *                     v_mfma_f32_32x32x16_f16, 14 = the same on v_mfma_f32_16x16x32_f16
 *                     (the default picks 14's form for cout % 256 == 0, 13's for cout 64);
 *                     15 = the 256x256 tile (12) as a persistent k-stream (the default
 *                     for dense A with cout % 256 == 0, K >= 256, its 256x128 form
 *                     for dense cout 128, K >= 256, its 256x64 form for dense cout 64,
 *                     K >= 64; forced, every other
 *                     GEMM runs the library's pick; 12 forces the one-tile-per-block form);
 *                     7 also selects the implicit-GEMM fused stem over the halo stem)
 *   RR_TUNE_S3_STAGGER: split core first-round stagger, 0..200 sleeps of
 *                     ~1 us for every other resident block (-1 = the library's pick)
 *   RR_TUNE_SWEEP_MF16: the 256x320 bf16 filter sweep on v_mfma_f32_16x16x32_bf16 (1)
 *                     or v_mfma_f32_32x32x16_bf16 (0); -1 = the library's pick (0)
 *   RR_TUNE_SWEEP_IL: the bf16 / fp8 filter sweeps: 1 = the next k-tile's LDS-DMA
 *                     issued chunk by chunk among the k-tile's first MFMAs, 0 = one
 *                     burst at the top of the k-tile; -1 = the library's pick (1 for the
 *                     256x320 bf16 and the fp8 sweeps, 0 for the 256x256 bf16 one)
 *   RR_TUNE_CONV_IL:  the f16x2 256x256 conv tile (RR_TUNE_S3_CFG 12): 1 = the next
 *                     k-tiles' B DMA and A loads issued one group at a time among the
 *                     MFMAs, 0 = one burst at the top of the k-tile; 1 also selects the
 *                     halo-staged 3x3 tile's 16x16x32 form with its B DMA spread the
 *                     same way; -1 = the library's pick (0)
 *   RR_TUNE_HALO_MF:  the f16x2 halo-staged 3x3 tiles on v_mfma_f32_16x16x32_f16 (1) or
 *                     v_mfma_f32_32x32x16_f16 (0); for cout 64: 2 = the 512-row
 *                     single-buffer tile (the pick where its 640-row halo holds the map,
 *                     round 6), 3 = the persistent 256-row stream (round 5's pick); for
 *                     cout 128: 4 = the two-buffer one-tap tile (the pick is the
 *                     single-buffer three-tap one, round 6);
 *                     -1 = the library's pick (RR_TUNE_S3_CFG 13 / 14 override it)
 *   RR_TUNE_S3_CFG_RES: as RR_TUNE_S3_CFG, for the split-core GEMMs with a residual
 *                     epilogue only (0 = RR_TUNE_S3_CFG's choice)
 *   RR_TUNE_SWEEP_FORM: the bf16 filter sweeps (the prefilter's pass 2, bf16
 *                     rr_cosine_topk_lp): 0 = the gemm core's tiles (RR_TUNE_LP_CFG
 *                     applies), 1 = the hand-scheduled 16x16x32 sweep (csrc/sweep16.hip)
 *                     on 128-B LDS rows (K % 64 == 0; else as 2), 2 = the same on
 *                     64-B rows; -1 = the library's pick
 *   RR_TUNE_HALO_2D:  the f16x2 stride-1 3x3 convs on 2-D block halo tiles (16 x 16 or,
 *                     for cout 64, 16 x 32 outputs of one image; no residual epilogue):
 *                     -1 = where no raster halo tile holds the map (the library's pick),
 *                     1 = wherever one serves, 0 = never (ABI 6, round 6)
 *   RR_TUNE_TRUNK_PARTS: the native trunk plan (rr_trunk_h2_forward_u8): 1 = the whole
 *                     batch on the caller's stream, 2 = two parts on the plan's two
 *                     streams, -1 = the library's pick (the rule stated at
 *                     rr_trunk_h2_parts)
 * Any other key or value: RR_EINVAL. */
#define RR_TUNE_GEMM_CFG 1
#define RR_TUNE_GEMM_BK 2
#define RR_TUNE_LP_CFG 3
#define RR_TUNE_S3_CFG 4
#define RR_TUNE_S3_STAGGER 5
/* 6, 7: retired (ABI 5) */
#define RR_TUNE_SWEEP_MF16 8
#define RR_TUNE_SWEEP_IL 9
#define RR_TUNE_CONV_IL 10
#define RR_TUNE_HALO_MF 11
/* 12: retired (ABI 5) */
#define RR_TUNE_S3_CFG_RES 13
#define RR_TUNE_SWEEP_FORM 14
#define RR_TUNE_HALO_2D 15
#define RR_TUNE_TRUNK_PARTS 16
int rr_set_tuning(rr_handle_t h, int key, int value);

/* ---- search (ranker) ----------------------------------------------------
 * Replaces iris_evaluate.py:383 `torch.mm(q, g.t())` + :386
 * `np.argsort(-similarity, axis=1)` (the only ranking driver), truncated to
 * the top k, with a STABLE order: score descending, then gallery index
 * ascending.  Scores are exact fp32 MFMA dot products (v_mfma_f32_32x32x2_f32,
 * a fixed k-ordered fmaf chain restated bit-for-bit by oracle/cosine_topk.c).
 *
 *   queries [nq][d], gallery [n][d]  (rows are expected L2-normalised by the
 *   caller, as iris_evaluate.py:379-380 does; the kernel does not renormalise)
 *   out_scores [nq][k] fp32, out_idx [nq][k] int64 = row + idx_offset.
 *   If n < k the tail is filled with (-inf, -1).
 *   1 <= k <= 16384, d % 4 == 0, 16-byte aligned rows.
 * Workspace: rr_cosine_topk_workspace_size(nq, n, d, k) bytes of device
 * memory, any alignment >= 256.  That size holds a worst-case candidate
 * buffer (every row of the gallery, per query: ~nq * n * 8 bytes), which can
 * never overflow.
 *
 * Bounded workspaces (all three rankers: rr_cosine_topk, rr_cosine_topk_lp,
 * rr_cosine_topk_prefilter with its _prefilter_ functions).  Any workspace of
 * at least rr_cosine_topk_workspace_size_cap(nq, n, d, k, k) bytes is
 * accepted; the ranker then keeps cap = rr_cosine_topk_cap_for(nq, n, d, k,
 * workspace_bytes) candidates per query (cap >= k; workspace_size_cap(...,
 * cap) gives the bytes for a chosen cap).  A query whose threshold filter
 * passes more than cap rows gets an incomplete candidate set: its output row
 * is NOT its exact top-k.  Every call zeroes and then sets the int32 at
 * rr_cosine_topk_overflow_offset (device, inside the workspace) to the number
 * of such queries; the int32 [nq] at rr_cosine_topk_counts_offset holds each
 * query's count (> cap = overflowed).  The caller re-runs those queries, e.g.
 * with a worst-case workspace for just them (ops.cosine_topk* with
 * max_workspace_bytes do this).  The status cannot be returned synchronously:
 * the counts exist only once the stream has run.  Offsets are valid for the
 * same (nq, n, d, k) until the workspace is reused.                         */
size_t rr_cosine_topk_workspace_size(int nq, long long n, int d, int k);
size_t rr_cosine_topk_workspace_size_cap(int nq, long long n, int d, int k, long long cap);
long long rr_cosine_topk_cap_for(int nq, long long n, int d, int k, size_t workspace_bytes);
size_t rr_cosine_topk_counts_offset(int nq, long long n, int d, int k);
size_t rr_cosine_topk_overflow_offset(int nq, long long n, int d, int k);
int rr_cosine_topk(rr_handle_t h, const float* queries, int nq,
                   const float* gallery, long long n, int d, int k,
                   long long idx_offset, float* out_scores, long long* out_idx,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Dense cosine scores, gallery-major: scores[j][i] = <gallery_j, query_i>,
 * i.e. the transpose of iris_evaluate.py:383's similarity matrix. [n][nq]. */
int rr_cosine_scores(rr_handle_t h, const float* queries, int nq,
                     const float* gallery, long long n, int d, float* scores,
                     void* stream);

/* Merge nparts partial top-k lists (the per-shard results gathered over RCCL)
 * into one top-k_out list per query, same stable order.  Layout
 * part_scores/part_idx [nparts][nq][k_in]; entries with idx < 0 are padding.
 * Indices must be < 2^32 - 1 (ShardedGallery refuses larger galleries).
 * No reference counterpart (the reference never
 * shards); it is the k-way merge of SURVEY.md §8(e).        */
int rr_topk_merge(rr_handle_t h, const float* part_scores,
                  const long long* part_idx, int nparts, int nq, int k_in,
                  int k_out, float* out_scores, long long* out_idx,
                  void* stream);

/* ---- low-precision search (configs C4 bf16, C5 fp8) ---------------------
 * dtype: 1 = bf16 (RNE), 2 = fp8 OCP e4m3 with one fp32 scale per row.
 * rr_quantize_rows: x [rows][d] fp32 -> y [rows][d] (2 or 1 bytes/elem);
 * fp8 writes row_scale[r] = amax(row)/448 (x ~= q * scale).
 * NaN: bf16 keeps it (a NaN element rounds to a bf16 NaN).  fp8: a row that
 * holds a NaN element gets row_scale[r] = NaN, so the whole row dequantises
 * to NaN and every score against it is NaN (rr_cosine_topk_lp multiplies
 * by the scales; such rows rank last, by index, as in rr_cosine_topk) --
 * the same as the exact ranker's score of a row with one NaN element.  The
 * row's amax, and the bytes of its finite elements, are those of its finite
 * elements; the byte written for a NaN element itself is unspecified.
 * Rows without a NaN are unaffected.                                        */
int rr_quantize_rows(rr_handle_t h, const float* x, long long rows, int d,
                     int dtype, void* y, float* row_scale, void* stream);

/* rr_cosine_topk on bf16 / fp8 rows (fp32 accumulate, scores dequantised
 * by q_scale[i] * g_scale[j] when given; required for fp8).  Same workspace
 * and output contract as rr_cosine_topk; scores are the low-precision
 * ones, so parity vs fp32 is recall@k, not index equality.  d*size % 16 == 0. */
int rr_cosine_topk_lp(rr_handle_t h, const void* queries, const float* q_scale,
                      int nq, const void* gallery, const float* g_scale,
                      long long n, int d, int dtype, int k, long long idx_offset,
                      float* out_scores, long long* out_idx, void* workspace,
                      size_t workspace_bytes, void* stream);

/* alpha-weighted query expansion (config C5; absent from the reference,
 * SURVEY.md §8f row 3 — defined as in Radenovic et al., TPAMI 2018, the GeM
 * paper models/gem_pooling.py:3 cites):
 *   out[i] = normalize(q[i] + sum_{r<n} max(s[i][r],0)^alpha * g[idx[i][r]-idx_offset])
 * top_idx / top_scores [nq][k] as returned by rr_cosine_topk (idx < 0 =
 * padding, skipped); gallery [n_rows][d] = the local rows, holding global
 * indices [idx_offset, idx_offset + n_rows): an index outside that range is
 * skipped, never read.  Re-rank by calling rr_cosine_topk with `out` as the
 * queries.                                                                 */
int rr_alpha_qe(rr_handle_t h, const float* queries, int nq,
                const float* gallery, long long n_rows, int d, const long long* top_idx,
                const float* top_scores, int k, int n, float alpha,
                long long idx_offset, float* out, void* stream);

/* Exact cosine top-k through a bf16 prefilter: the SAME scores and indices,
 * bit for bit, as rr_cosine_topk (iris_evaluate.py:383-386 ranker), with the
 * full gallery sweep on the bf16 MFMA and only rows that can still reach the
 * exact top-k rescored with the fp32 core's fmaf chain (proof and bound in
 * csrc/prefilter.hip).  gallery_bf16 = rr_quantize_rows(gallery, bf16);
 * bound3 (device, 3 doubles) = rr_prefilter_gallery_bound of the same pair,
 * computed once per gallery.  d % 8 == 0.                                   */
int rr_prefilter_gallery_bound(rr_handle_t h, const float* gallery,
                               const void* gallery_bf16, long long n, int d,
                               double* bound3, void* stream);
size_t rr_cosine_topk_prefilter_workspace_size(int nq, long long n, int d, int k);
/* Byte offset, inside that workspace, of the int32 [nq] count of rows each
 * query kept through the bf16 filter pass (the rows then bounded and, where
 * they can still reach the top-k, rescored exactly); valid after a call with
 * the same (nq, n, d, k) until the workspace is reused. */
size_t rr_cosine_topk_prefilter_counts_offset(int nq, long long n, int d, int k);
/* Bounded workspaces, as for rr_cosine_topk (the count above > cap marks an
 * overflowed query). */
size_t rr_cosine_topk_prefilter_overflow_offset(int nq, long long n, int d, int k);
size_t rr_cosine_topk_prefilter_workspace_size_cap(int nq, long long n, int d, int k, long long cap);
long long rr_cosine_topk_prefilter_cap_for(int nq, long long n, int d, int k, size_t workspace_bytes);
int rr_cosine_topk_prefilter(rr_handle_t h, const float* queries, int nq,
                             const float* gallery, const void* gallery_bf16,
                             const double* bound3, long long n, int d, int k,
                             long long idx_offset, float* out_scores,
                             long long* out_idx, void* workspace,
                             size_t workspace_bytes, void* stream);

/* PCA-whitening learning, GPU half (replaces the
 * m = X.mean(0), Xc = X - m, np.dot(Xc.T, Xc) lines of
 * networks/backbone.py:46-49, called from networks/spca.py:215-217):
 *   mean_out [d]   fp64 column means of X [n][d] (fp32, row-major, device)
 *   gram_out [d*d] fp64 sum_i (x_i - m)(x_i - m)^T, symmetric (device)
 * fp32 MFMA partials over <= 8192-row slices, summed in fp64.  The caller
 * symmetrises / scales by 1/(2n) and runs the eigendecomposition on the host
 * (backbone.py:50-57).  Workspace is bounded (<= 131072-row chunks).          */
size_t rr_pcaw_gram_workspace_size(long long n, int d);
int rr_pcaw_gram(rr_handle_t h, const float* x, long long n, int d,
                 void* workspace, size_t workspace_bytes, double* mean_out,
                 double* gram_out, void* stream);

/* ---- embed (extractor) ---------------------------------------------------
 * uint8 HWC pixels -> fp32 NHWC, (x/255 - mean[c]) / std[c].
 * Replaces transforms.ToTensor + Normalize(mean=[.485,.456,.406],
 * std=[.229,.224,.225]) (dataset/configdataset.py:417, :430-436).          */
int rr_preprocess_u8(rr_handle_t h, const uint8_t* img_nhwc, int b, int hgt,
                     int wid, const float* mean3, const float* std3,
                     float* out_nhwc, void* stream);

/* Same with out_c in {3, 4}: out_c == 4 writes NHWC4 pixels with a zero
 * 4th channel, the stem conv's 16-byte tap layout (see rr_conv2d).          */
int rr_preprocess_u8_ex(rr_handle_t h, const uint8_t* img_nhwc, int b, int hgt,
                        int wid, const float* mean3, const float* std3,
                        int out_c, float* out_nhwc, void* stream);

/* fp32 NCHW -> NHWC relayout (the reference's forward_test input is NCHW). */
int rr_nchw_to_nhwc(rr_handle_t h, const float* in, int b, int c, int hgt,
                    int wid, float* out, void* stream);
/* Same, zero-padding the channel dim to out_c >= c.                       */
int rr_nchw_to_nhwc_ex(rr_handle_t h, const float* in, int b, int c, int hgt,
                       int wid, int out_c, float* out, void* stream);

/* 2-D convolution, NHWC, implicit GEMM on fp32 MFMA with a fused epilogue:
 * y = relu?( conv(x, w) + bias[co] + residual? ).  Weights [cout][kh][kw][cin]
 * with eval-mode BatchNorm already folded into w/bias by the host.
 * Replaces the torchvision ResNet conv/BN/ReLU/residual ops behind
 * networks/backbone.py:103-109 and models/gem_pooling.py:44,61.
 * residual may be NULL; output is [b][oh][ow][cout].
 * A-operand paths: 1x1/s1 = dense rows; cin % 32 == 0 = im2col with one
 * filter tap per 32-deep k-tile; cin == 4 = one tap per float4 (the stem on
 * NHWC4 input, zero 4th channel and zero 4th weight channel); other cin =
 * per-element gather.                                                      */
int rr_conv2d(rr_handle_t h, const float* x, int b, int hgt, int wid, int cin,
              const float* w, const float* bias, int cout, int kh, int kw,
              int stride, int pad, const float* residual, int relu, float* y,
              void* stream);

/* Bilinear resize, NHWC, align_corners=False, PyTorch source-index rule:
 * src = max(scale * (dst + 0.5) - 0.5, 0) with scale = 1/scale_factor when a
 * scale factor was given (inv_scale_h/w > 0) else in/out.  Replaces the
 * F.interpolate(..., mode='bilinear', align_corners=False) calls of
 * extract_vectors (utils/helpfunc.py:26, :38).                             */
int rr_resize_bilinear(rr_handle_t h, const float* x, int b, int hgt, int wid,
                       int c, int out_h, int out_w, float inv_scale_h,
                       float inv_scale_w, float* y, void* stream);

/* fp32-accurate convolution on the fp16 matrix cores (h2_*.hip, the f16x2
 * split): the same operation, layouts and epilogue as rr_conv2d on the
 * 16-bit MFMA at three fp16 products per fp32 product.  Every fp32 operand is scaled by a power of two and split
 * into two fp16 pieces, x 2^e = x0 + x1 + r with |r| <= 2^-22 |x 2^e|; a.b
 * keeps a0b0 + (a0b1 + a1b0) (dropped terms <= 3 2^-22 |a||b|), three fp16
 * MFMAs with exact products and fp32 accumulation (a0b0 in its own
 * accumulator), and the accumulator is scaled back exactly.  Weights come
 * from rr_split2_f16: w2 = planes [2][cout][K] (fp16 bit patterns), w_iscale
 * [cout] the inverse row scales.  x_amax: the RR_AMAX_SLOTS-word max-|x|
 * record of x (from the producing call's y_amax, or rr_amax_f32); y_amax
 * (optional, zeroed by the caller): receives max |y| over the finite stored
 * values.  Needs cin % 32 == 0, or cin == 4 for the NHWC4 stem (w2 then holds
 * the flattened [kh][kw][4] filter zero-padded to K = kh*kw*4 rounded up to
 * 32).  y, bias and residual must be 16-byte aligned (RR_EINVAL otherwise).
 * The split scale of x is one per tensor: values more than 2^18 below its
 * max keep an absolute error <= 2^-40 max|x| instead of full relative
 * precision.  Replaces the same reference ops as rr_conv2d
 * (networks/backbone.py:103-109, :305-346; models/gem_pooling.py:44,61).    */
int rr_conv2d_h2(rr_handle_t h, const float* x, const unsigned* x_amax, int b,
                 int hgt, int wid, int cin, const void* w2,
                 const float* w_iscale, const float* bias, int cout, int kh,
                 int kw, int stride, int pad, const float* residual, int relu,
                 float* y, unsigned* y_amax, void* stream);

/* Which kernel instance rr_conv2d_h2 runs for a shape under given tuning
 * values, and how it is launched (ABI 8).  Host only, no handle, no GPU: the
 * same geometry and the same route function (csrc/h2_route.hpp) as the call
 * itself.  RR_EINVAL for a shape rr_conv2d_h2 rejects or a tuning value
 * rr_set_tuning rejects (b == 0, which launches nothing, reports the route
 * of its shape).
 * family: 0 one tile per block (h2_tile.hip), 1 the config-8 k-stream, 2 the
 * config-15 256-row k-stream, 3 the raster halo tile, 4 the 2-D halo tile.
 * cfg: the tile table's number (3, 4, 7 to 15; 13 / 14 = a halo tile on
 * 32x32x16 / 16x16x32).  wm .. t2: the kernel template's tuple, 0 where the
 * family has no such parameter: wm x wn waves of fm x fn 32x32 MFMA tiles,
 * k-tile depth bk, halo buffer rows hr, taps per barrier tpk, mf16 (1 =
 * v_mfma_f32_16x16x32_f16), LDS stages nstg, accumulator sets acc, il (loads
 * spread among the MFMAs), pers (1 = persistent stream; halo tiles 2 = one
 * halo buffer at 256 rows), t2 (2-D halo tile: output columns).  chunk_rows:
 * rows per launch where x or y has 4 GB or more, 0 = one launch.           */
typedef struct {
  int b, h, w, cin, cout, kh, kw, stride, pad;
  int residual, relu; /* 0 / 1 */
} rr_h2_shape_t;
typedef struct {
  int s3_cfg, s3_cfg_res, halo_mf, halo_2d, conv_il; /* as rr_set_tuning's keys */
} rr_h2_tune_t;
typedef struct {
  int family, cfg;
  int wm, wn, fm, fn, bk, hr, tpk, mf16, nstg, acc, il, pers, t2;
  long long chunk_rows;
} rr_h2_route_t;
int rr_h2_route(const rr_h2_shape_t* shape, const rr_h2_tune_t* tune, rr_h2_route_t* out);

/* Which kernel instance serves a GEMM of the exact-fp32, bf16 and fp8 kernels
 * (rr_conv2d, rr_linear*, rr_linear_bf16*, the rankers' seed and filter
 * sweeps) under given tuning values (ABI 9).  Host only, no handle, no GPU:
 * the same checks and the same route function (csrc/gemm_route.hpp) as the
 * launch itself.  RR_EINVAL for a shape the launch rejects or a tuning value
 * rr_set_tuning rejects (m == 0 or n == 0, which launches nothing, reports the
 * route of its shape).
 * shape: amode 0 dense A [m][lda], 1 implicit im2col (Cin % 32 == 0), 2 the
 * generic gather, 3 NHWC4; emode 0 stored C, 1 transposed scores (the
 * rankers' seed), 2 the filter sweep; dtype 0 fp32, 1 bf16, 2 fp8 (lda / ldb
 * in elements); bias .. sym: the epilogue facts, 0 / 1 but activation (0
 * none, 1 ReLU, 2 QuickGELU) and k_split (the k per split, 0 none); aligned16:
 * A and B are 16-byte aligned.
 * route: family -1 none (the launch fails), 0 the fp32 tile, 1 the bf16 / fp8
 * one-tile kernel, 2 the persistent bf16 k-stream, 3 its three-A-stage form,
 * 4 the 8-phase pipeline, 5 / 6 the hand-scheduled bf16 sweep on 128-B / 64-B
 * LDS rows.  cfg: 22 / 41 / 88 (RR_TUNE_GEMM_CFG) for fp32, 1 to 5
 * (RR_TUNE_LP_CFG) for bf16 / fp8 (the k-streams 3, the hand-scheduled sweep
 * 4: their tiles).  wm .. epi: the kernel template's tuple, 0 where the family
 * has no such parameter: wm x wn waves of fm x fn 32x32 MFMA tiles, fp32
 * k-tile depth bk, blocks per CU minb, gl (1 = LDS-DMA staging), mf16 (1 / 2 =
 * v_mfma_f32_16x16x32_bf16), il (the DMA spread among the MFMAs), epi (the
 * epilogue flag set compiled in: 1 bias, 2 residual, 8 QuickGELU, 16 bf16
 * output, 128 stats_out, 256 stats_in; -1 = flags read at run time).        */
typedef struct {
  int amode, emode, dtype, m, n, k;
  long long lda, ldb, ldc;
  int bias, residual, activation, out_bf16, stats_in, stats_out, row_scales, k_split, sym;
  int aligned16;
} rr_gemm_shape_t;
typedef struct {
  int gemm_cfg, gemm_bk, lp_cfg, sweep_form, sweep_mf16, sweep_il; /* as rr_set_tuning's keys */
} rr_gemm_tune_t;
typedef struct {
  int family, cfg;
  int wm, wn, fm, fn, bk, minb, gl, mf16, il, epi;
} rr_gemm_route_t;
int rr_gemm_route(const rr_gemm_shape_t* shape, const rr_gemm_tune_t* tune, rr_gemm_route_t* out);

/* The output of a stage-entry bottleneck block on the f16x2 core, its 1x1
 * conv3 and its 1x1 strided downsample projection as ONE GEMM over
 * K = planes + cin:
 *   out = ReLU(y . W3^T + x[:, ::stride, ::stride] . Wd^T + bias)
 * (torchvision Bottleneck / the reference's ResBlock sum,
 * networks/backbone.py:327-346), so the projected identity is never written
 * or read back.  y: conv2's output [b][oh][ow][planes] with its max-|x|
 * record y_amax; x: the block input [b][hx][wx][cin] with x_amax;
 * (oh - 1) * stride < hx, (ow - 1) * stride < wx.  w2 / w_iscale:
 * rr_split2_f16 of the concatenated rows [W3 | Wd] [cout][planes + cin];
 * bias = the two folded biases' sum.  planes % 32 == 0, cin % 32 == 0,
 * cout % 256 == 0.  out_amax as rr_conv2d_h2's y_amax.                      */
int rr_bottleneck_out_h2(rr_handle_t h, const float* y, const unsigned* y_amax,
                         int b, int oh, int ow, int planes, const float* x,
                         const unsigned* x_amax, int hx, int wx, int cin,
                         int stride, const void* w2, const float* w_iscale,
                         const float* bias, int cout, float* out,
                         unsigned* out_amax, void* stream);

/* The ResNet stem on the f16x2 core with its max-pool fused: NHWC4 conv
 * (cin == 4, as rr_conv2d_h2) + bias + ReLU, then the 3x3 stride-2 padding-1
 * max-pool, written only pooled: y_pool [b][ph][pw][64] with
 * ph = (oh - 1) / 2 + 1, pw likewise (oh, ow the conv's output size).  Each
 * tile computes a 17 x 15 patch of conv outputs and pools its 8 x 7 windows
 * from LDS: the stem's 112 x 112 x 64 map never reaches HBM.  The max is taken
 * over the raw accumulators and scaled once (scale > 0, bias add and ReLU are
 * monotone): the same bits as rr_conv2d_h2 followed by the max-pool, for
 * finite inputs.  y_amax (optional, zeroed): max |y_pool|, which equals the
 * conv output's (every conv output lies in some window).  cout == 64.
 * Replaces networks/backbone.py:103-109's conv1 / bn1 / relu / maxpool.     */
int rr_stem_pool_h2(rr_handle_t h, const float* x, const unsigned* x_amax,
                    int b, int hgt, int wid, const void* w2,
                    const float* w_iscale, const float* bias, int cout, int kh,
                    int kw, int stride, int pad, float* y_pool,
                    unsigned* y_amax, void* stream);

/* fp16 2-way split of the rows of w [rows][k] (done once per weight tensor):
 * row n is scaled by 2^e_n, its max |w| then in [2^14, 2^15), and split into
 * planes [2][rows][kpad] (fp16 bit patterns, zero past k; kpad >= k, a
 * multiple of 32 for rr_conv2d_h2); iscale[n] = 2^-e_n.                    */
int rr_split2_f16(rr_handle_t h, const float* w, int rows, int k, int kpad,
                  void* planes, float* iscale, void* stream);

/* max |x| over the finite values of x[n] into the RR_AMAX_SLOTS words at
 * amax (atomic max; zero them first): the x_amax record rr_conv2d_h2 needs
 * for an input no earlier call produced.                                   */
int rr_amax_f32(rr_handle_t h, const float* x, long long n, unsigned* amax,
                void* stream);

/* Max pool (torchvision ResNet stem maxpool 3x3/2 pad 1), NHWC. */
int rr_maxpool2d(rr_handle_t h, const float* x, int b, int hgt, int wid, int c,
                 int k, int stride, int pad, float* y, void* stream);

/* GeM pooling over the spatial axis of an NHWC map [b][hw][c] -> [b][c]:
 * (mean_hw clamp(x, eps)^p)^(1/p).  Replaces networks/RetrievalNet.py:324-325
 * (gem, python-float p) and models/gem_pooling.py:20-23 (GeMPooling).      */
int rr_gem_pool(rr_handle_t h, const float* x, int b, int hw, int c, float p,
                float eps, float* out, void* stream);

/* y[m][n] = x[m][:] . w[n][:] + bias[n]   (bias may be NULL).
 * Replaces GeM.whiten 1x1 conv (networks/RetrievalNet.py:332,342),
 * GeMModel.feature_proj Linear (models/gem_pooling.py:50,68) and the
 * PCA-whitening ConvDimReduction apply (networks/spca.py:205-227).
 * Any k and n: with k % 4 == 0 (x and w 16-byte aligned) the rows are staged
 * as 16-byte units; any other k (a classifier over feature_dim = 130) takes
 * the scalar gather of the generic convolution, same epilogue, no alignment
 * requirement.  m = 0 is a no-op.                                          */
int rr_linear(rr_handle_t h, const float* x, int m, int k, const float* w,
              const float* bias, int n, float* y, void* stream);

/* y = act(x . w^T + bias + residual); act 0 = none, 1 = ReLU, 2 = QuickGELU
 * (x * sigmoid(1.702 x)).  bias / residual ([m][n]) may be NULL.  Replaces the
 * ViT projections of networks/model.py:171-192 (MHA in/out_proj, c_fc +
 * QuickGELU, c_proj + residual) and `ln_post(x[:,0]) @ proj` (:239-241).
 * k % 4 == 0 and 16-byte aligned x and w (RR_EINVAL otherwise: the fused
 * projections have no scalar-gather form); any n, n % 4 != 0 stores per
 * element.  m = 0 is a no-op.                                              */
int rr_linear_ex(rr_handle_t h, const float* x, int m, int k, const float* w,
                 const float* bias, int n, const float* residual, int act,
                 float* y, void* stream);

/* bf16 x [m][k] . bf16 w [n][k]^T, fp32 accumulate, fp32 bias / residual,
 * act as rr_linear_ex; y fp32 or (out_bf16) bf16.  The C4 (ViT bf16) GEMMs. */
int rr_linear_bf16(rr_handle_t h, const void* x, int m, int k, const void* w,
                   const float* bias, int n, const float* residual, int act,
                   int out_bf16, void* y, void* stream);

/* rr_linear_bf16 with the ViT LayerNorms (networks/model.py:157-163, the ln_1
 * / ln_2 of :188-190) folded into the GEMMs, so no LayerNorm pass reads the
 * fp32 residual stream.  Exactly one of stats_in / stats_out is set:
 *  - stats_out (the out-proj / c_proj GEMMs: bias, residual, fp32 y, act 0,
 *    n % 256 == 0, k % 64 == 0): besides y, writes per row and 256-column tile
 *    t the LayerNorm partials of y, stats_out [m][n/256][2] = (mean_t, M2_t =
 *    sum (y - mean_t)^2 over the tile's 256 columns), and xb_out [m][n] =
 *    bf16(y - mean_t) (RNE), each tile centred on its own mean.
 *  - stats_in (the in-proj / c_fc GEMMs: bias, bf16 y, k % 64 == 0, k <= 768):
 *    x holds such centred bf16 rows (xb) with their partials
 *    [m][ceil(k/256)][2]; w = bf16(W o gamma) (columns scaled by the LayerNorm
 *    weight), colsum [ceil(k/256)][n] = sum over k-tile t of float(w[n][k]),
 *    bias = b + W beta:
 *      y = act(rstd_m (x.w^T + sum_t (mean_t - mean_m) colsum[t]) + bias),
 *    mean_m / rstd_m = 1 / sqrt(var + eps) from the partials (biased
 *    variance, combined as Chan et al.).  Equal to LayerNorm -> bf16 ->
 *    rr_linear_bf16 up to where bf16 rounding falls: the operand is
 *    bf16(y - mean_t) instead of bf16(LayerNorm(y)), an element rounding error
 *    of 2^-9 |y_k - mean_t| against the LayerNorm path's 2^-9 rstd |y_k -
 *    mean| -- the same scale, whatever the rows' |mean| / std (centring was
 *    added in ABI 5: with bf16(y) the error grew with |mean| / std;
 *    tests/test_gpu_vit.py::test_linear_bf16_ln_fold_large_mean).             */
int rr_linear_bf16_ln(rr_handle_t h, const void* x, int m, int k, const void* w,
                      const float* bias, int n, const float* residual, int act,
                      int out_bf16, void* y, const float* stats_in,
                      const float* colsum, float eps, float* stats_out,
                      void* xb_out, void* stream);

/* The producer side of rr_linear_bf16_ln for rows that no GEMM wrote (the
 * first block's ln_1 input): the partials stats [m][d/256][2] = (mean_t,
 * M2_t) of fp32 x [m][d] and xb [m][d] = bf16(x - mean_t); d % 256 == 0.   */
int rr_ln_partials_bf16(rr_handle_t h, const float* x, int m, int d, void* xb,
                        float* stats, void* stream);

/* ---- ViT-B/16 (networks/model.py:206-243) ------------------------------ */
/* LayerNorm over the last dim (fp32, biased variance), rows x + i*ldx ->
 * dense y [m][d].  Replaces LayerNorm (:157-163): ln_pre, ln_1, ln_2, and
 * ln_post on the CLS rows (ldx = seq*width).  d <= 4096.                   */
int rr_layernorm(rr_handle_t h, const float* x, long long ldx, int m, int d,
                 const float* gamma, const float* beta, float eps, float* y,
                 void* stream);

/* Same, output dtype 0 = fp32, 1 = bf16 (feeds rr_linear_bf16).           */
int rr_layernorm_ex(rr_handle_t h, const float* x, long long ldx, int m, int d,
                    const float* gamma, const float* beta, float eps,
                    int out_dtype, void* y, void* stream);

/* NHWC image -> non-overlapping patch rows [b*(H/p)*(W/p)][p*p*c], (kh,kw,c)
 * order: with weights [width][p][p][c] the patch conv (:223, stride = kernel
 * = p, no bias) becomes one dense GEMM (rr_linear).                        */
int rr_patchify(rr_handle_t h, const float* x, int b, int hgt, int wid, int c,
                int patch, float* y, void* stream);

/* Same, output dtype 0 = fp32, 1 = bf16 (RNE, the rows rr_linear_bf16 reads;
 * equal to rr_patchify followed by rr_quantize_rows bf16).                 */
int rr_patchify_ex(rr_handle_t h, const float* x, int b, int hgt, int wid,
                   int c, int patch, int out_dtype, void* y, void* stream);

/* tokens [b][1+np][width]: row 0 = cls + pos[0], row 1+i = patches[b][i] +
 * pos[1+i]  (class_embedding concat + positional_embedding, :226-227).     */
int rr_vit_tokens(rr_handle_t h, const float* patches, int b, int npatch,
                  int width, const float* cls, const float* pos, float* y,
                  void* stream);

/* Same with ln_pre (:229) fused when gamma and beta are given (both or
 * neither; width <= 4096): y = LayerNorm(tokens), bit-identical to
 * rr_vit_tokens followed by rr_layernorm, without the HBM round trip.      */
int rr_vit_tokens_ex(rr_handle_t h, const float* patches, int b, int npatch,
                     int width, const float* cls, const float* pos,
                     const float* gamma, const float* beta, float eps,
                     float* y, void* stream);

/* Multi-head self-attention core: qkv [b*seq][3*heads*64] (q | k | v, the
 * in_proj output) -> out [b*seq][heads*64] = softmax(q k^T / 8) v per head
 * (nn.MultiheadAttention, ResidualAttentionBlock.attention :184-186).
 * head_dim == 64, seq <= 256.  Fused on fp32 MFMA, scores never leave the
 * CU.                                                                      */
int rr_attention(rr_handle_t h, const float* qkv, int b, int seq, int heads,
                 int head_dim, float* out, void* stream);
/* Same, output dtype 0 = fp32, 1 = bf16.                                   */
/* (rr_attention_bf16 below: the C4 bf16 variant.)                          */
int rr_attention_ex(rr_handle_t h, const float* qkv, int b, int seq, int heads,
                    int head_dim, int out_dtype, void* out, void* stream);

/* The attention core on bf16 MFMA (config C4): q, k, v rounded to bf16 (RNE),
 * fp32 accumulation and fp32 softmax, P rounded to bf16 for P.V; output fp32
 * (out_dtype 0) or bf16 (1).  Same contract as rr_attention_ex.             */
int rr_attention_bf16(rr_handle_t h, const float* qkv, int b, int seq, int heads,
                      int head_dim, int out_dtype, void* out, void* stream);
/* Same, with the QKV rows already in bf16 (the QKV linear's bf16 output,
 * rr_linear_bf16 out_bf16 = 1: rounded RNE as rr_attention_bf16 rounds them,
 * so the result is bit-identical at half the bytes read).                  */
int rr_attention_bf16_qkv16(rr_handle_t h, const void* qkv_bf16, int b, int seq,
                            int heads, int head_dim, int out_dtype, void* out,
                            void* stream);

/* Row-wise L2 normalisation x / max(||x||_2, eps), in place allowed.
 * Replaces F.normalize (networks/RetrievalNet.py:343, models/gem_pooling.py:91,
 * utils/helpfunc.py:44, iris_evaluate.py:379-380).                        */
int rr_l2_normalize(rr_handle_t h, const float* x, int m, int d, float eps,
                    float* y, void* stream);

/* ---- DOLG head (networks/RetrievalNet.py:409-474, with_aspp=False) ------ */
/* The local branch's attention-weighted pooling in ONE read of the map.
 * y [b][hw][c] fp32 NHWC = bn(conv1(f3)) (pre-ReLU), w2 [c] and b2 = conv2's
 * weight and bias; out [b][c] =
 *   m = mean_p softplus(w2 . relu(y_p) + b2) * y_p / max(||y_p||_2, 1e-12)
 * (softplus: x for x > 20, else log1p(exp(x)); an all-zero pixel adds exactly
 * 0).  Replaces SpatialAttention2d.forward after the BN (:466-473: F.normalize
 * over channels, ReLU, conv2, softplus, expand, multiply) and, together with
 * rr_dolg_orth_fuse, DOLG.forward_test's two bmm, the division, the
 * subtraction and pool_l (:420-426): the projection is linear in the local
 * map, so only its mean m is needed and neither map is ever written.
 * c % 256 == 0, c <= 2048, hw > 0, y / w2 / out 16-B aligned (else RR_EINVAL);
 * b == 0 is RR_OK with no launch.  No float atomics: where few images leave
 * the chip short of work, an image's pixels are split over workgroups whose
 * partial sums go to the heads' scratch and are added in a fixed order; the
 * split depends on (b, hw) alone, so the result is the same bits on every run.
 * The heads' scratch: a per-stream buffer the handle owns (allocated on first
 * use, grown on demand), shared by rr_dolg_local_pool, rr_token_pool,
 * rr_how_vlad and rr_how_asmk and freed by rr_destroy.                      */
int rr_dolg_local_pool(rr_handle_t h, const float* y, int b, int hw, int c,
                       const float* w2, float b2, float* out, void* stream);

/* Orthogonal fusion: out [b][2c] = [fg | m - fg (fg . m) / (fg . fg)] for fg,
 * m [b][c].  Replaces DOLG.forward_test's torch.norm / bmm / bmm / divide /
 * subtract / pool_l / torch.cat (:418-428) given m from rr_dolg_local_pool.
 * No epsilon on fg . fg: a zero fg row gives NaN, as the reference's division
 * does.  c % 4 == 0, 16-B aligned rows.                                     */
int rr_dolg_orth_fuse(rr_handle_t h, const float* fg, const float* m, int b,
                      int c, float* out, void* stream);

/* ---- SOLAR head (networks/RetrievalNet.py:534-590) ---------------------- */
/* The second-order attention block's core: single-head self-attention over
 * the hw positions of a map, head width c.  fgh [b][hw][3c] fp32 NHWC is the
 * output of ONE 1x1 conv: columns [0,c) = f and [c,2c) = g, each with its BN
 * folded and BEFORE its ReLU (applied here on load), columns [2c,3c) = h.
 *   out[b][i][:] = sum_j softmax_j(float(c^-0.5) * relu(f_i) . relu(g_j)) h_j
 * out [b][hw][c].  Replaces SOABlock_GeM.forward's two bmm, the softmax and
 * the permutes (networks/RetrievalNet.py:558-565).  Both products run on the
 * exact-fp32 MFMA; key tiles stream past a 16-query tile with a running max
 * and sum, so the hw x hw scores are never written anywhere.  No workspace
 * and no float atomics: keys are visited in order, the result is the same
 * bits on every run and for an image alone or in a batch.  A query whose
 * relu(f) is all zero gets the plain mean of the h rows.
 * c % 256 == 0, 256 <= c <= 1024, 1 <= hw <= 65535, fgh / out 16-B aligned
 * (else RR_EINVAL); b == 0 is RR_OK with no launch.  Timing class 5.        */
int rr_soa_attention(rr_handle_t h, const float* fgh, int b, int hw, int c,
                     float* out, void* stream);

/* ---- Token head (networks/RetrievalNet.py:94-187, 263-305) -------------- */
/* Multi-head attention at head width 128 with separate query and key counts:
 * Attention.forward's reshape / permute / q @ k^T / softmax / attn @ v /
 * transpose (networks/RetrievalNet.py:120-124) given the projected rows.
 * q holds b * nq rows of ldq floats, head j in columns [128 j, 128 j + 128);
 * k and v hold b * nk rows of ldk / ldv floats likewise; out is dense
 * [b * nq][heads * 128].  Per image and head
 *   out[i] = sum_j softmax_j(float(128^-0.5) * q_i . k_j) v_j.
 * The strides let the caller stack projections in one GEMM and pass column
 * slices (q | k | v of one [rows][3 * heads * 128] buffer, or k1 | v1 | k2 | v2).
 * Both products run on the exact-fp32 MFMA; key tiles stream past a 16-query
 * tile with a running max and sum.  Only out is written: no workspace, no
 * atomics, keys visited in a fixed order, so the result is the same bits on
 * every run, for an image alone or in a batch, for a head alone (heads = 1 on
 * its column slice) or among others, and from dense or stacked buffers.  An
 * all-zero query gets the plain mean of the v rows.
 * head_dim is fixed at 128; 1 <= nq, nk <= 65535; heads >= 1; ldq, ldk, ldv
 * >= heads * 128 and % 4 == 0; q, k, v, out 16-B aligned (else RR_EINVAL);
 * b == 0 is RR_OK with no launch; offsets are 64-bit.  Timing class 5.      */
int rr_attention_hd128(rr_handle_t h, const float* q, long long ldq,
                       const float* k, long long ldk, const float* v,
                       long long ldv, int b, int nq, int nk, int heads,
                       float* out, void* stream);

/* Object-token pooling (Token_Refine.forward, networks/RetrievalNet.py:
 * 180-182: bmm, softmax(dim=1), bmm): x [b][hw][c], query [n_obj][c],
 *   out [b][n_obj][c] = sum_p softmax_o(query_o . x_p) x_p,
 * the softmax over the n_obj OBJECTS of each position (max subtracted), no
 * scale.  x is read once.  No float atomics: where few images leave the chip
 * short of work an image's positions are split over workgroups (a function of
 * b and hw only) and the partial sums, kept in the heads' scratch
 * (rr_dolg_local_pool), are added in a fixed order: the same bits on every
 * run, and for an image alone or in a batch wherever both choose the same
 * split (at least 16 positions per workgroup, about 1024 workgroups wanted:
 * any hw <= 16 * ceil(1024 / b)).
 * c % 256 == 0, 256 <= c <= 1024, 1 <= n_obj <= 8, hw >= 1, x / query / out
 * 16-B aligned (else RR_EINVAL); b == 0 is RR_OK.  Timing class 3.          */
int rr_token_pool(rr_handle_t h, const float* x, int b, int hw, int c,
                  const float* query, int n_obj, float* out, void* stream);

/* Exact GELU, y = 0.5 x (1 + erf(x / sqrt 2)) over n floats (F.gelu in Mlp,
 * networks/RetrievalNet.py:67-72, 87); y may be x.  NaN stays NaN, +inf gives
 * +inf, -inf gives -0 (the limit).  Timing class 3.                         */
int rr_gelu(rr_handle_t h, const float* x, long long n, float* y, void* stream);

/* ---- HOW head (models/how_vlad.py) --------------------------------------- */
/* VLAD pooling with a soft assignment, from the RAW local_proj rows: x
 * [b][n][d] fp32 (NHWC rows of the 1x1 conv), centroids [k][d]; per image
 *   x^_p = x_p / max(||x_p||_2, 1e-12)
 *   dist[p][c] = sqrt(max(||x^_p||^2 + ||c||^2 - 2 x^_p . c, 0))
 *   a[p][:] = softmax_c(-alpha dist[p][c])          (max subtracted)
 *   out[c][:] = sum_p a[p][c] (x^_p - centroid_c)
 * out [b][k * d].  Replaces HOWModel.extract_local_descriptors' F.normalize
 * (models/how_vlad.py:162) and VLADPooling.forward's cdist, softmax and loop
 * over the centroids (:36-55).  The final F.normalize over the k * d values
 * (:56) is NOT fused: launch rr_l2_normalize(out, b, k * d) afterwards.
 * x is read once; the normalised rows, the distances and the assignment never
 * reach global memory; x^ . C^T and A^T . x^ run on the exact-fp32 MFMA.  A
 * distance whose square rounds below zero is clamped to 0 (a descriptor equal
 * to a centroid never gives NaN); an all-zero row gives x^ = 0.  No float
 * atomics: where few images leave the chip short of work an image's positions
 * are split over workgroups (a function of b and n only: at least 64 positions
 * each, about 256 workgroups wanted) and the partial sums, kept in the heads'
 * scratch (rr_dolg_local_pool), are added in a fixed order: the same
 * bits on every run, and for an image alone or in a batch wherever both
 * choose the same split (any n <= 64 ceil(256 / b); never split at n <= 64).
 * 1 <= k <= 128, d % 32 == 0, 32 <= d <= 256, 1 <= n <= 65535, x / centroids /
 * out 16-B aligned (else RR_EINVAL, nothing written); b == 0 is RR_OK and
 * writes nothing; offsets are 64-bit.  Timing class 3.                      */
int rr_how_vlad(rr_handle_t h, const float* x, int b, int n, int d,
                const float* centroids, int k, float alpha, float* out,
                void* stream);

/* ASMK's thresholded nearest-centroid histogram from the same raw rows:
 * the normalisation and distances of rr_how_vlad, then per position the
 * nearest centroid (the lowest index among equal distances, as torch.argmin)
 * and its distance m_p; per image thr = mean_p m_p + std_p m_p (the unbiased
 * std, / (n - 1), both in double); out [b][k],
 *   out[c] = weights[c] * #{p : nearest(p) == c and m_p < thr}.
 * Replaces :162 and ASMKPooling.forward's cdist, argmin, gather, threshold
 * and double loop (:80-99); the F.normalize of :102 is the caller's
 * rr_l2_normalize.  n == 1 gives a zero row (the std of one value is NaN and
 * no comparison holds), and so do equal minima (std 0).  The count is an
 * integer and is multiplied by the weight once, so the result depends on
 * neither the order of the positions nor the split.  x is read once; the
 * minima and indices pass through the heads' scratch (rr_dolg_local_pool;
 * 8 bytes a position) to a second launch, one workgroup per image.
 * Limits, alignment (weights included), b == 0 and the timing class are
 * rr_how_vlad's.                                                            */
int rr_how_asmk(rr_handle_t h, const float* x, int b, int n, int d,
                const float* centroids, const float* weights, int k,
                float* out, void* stream);

/* ---- SoSNet head (models/sosnet.py) -------------------------------------- */
/* Attention-weighted, centred covariance pooling as its packed upper
 * triangle.  z [b][n][c] fp32: the RAW rows of the second-order projection
 * conv WITHOUT its bias (Wp x_p; the bias cancels under the centring); hid
 * [b][n][dh]: the ReLU'd output of the attention MLP's second layer, w3 [dh]
 * and b3 its last layer; per image
 *   a_p  = sigmoid(w3 . hid_p + b3)          (hid == NULL: a = 1, use_attention=False)
 *   y_p  = a_p z_p                           (= the projection of the attended row, minus bp)
 *   cov  = sum_p (y_p - mean_p y)(y_p - mean_p y)^T / (n - 1)
 *   out  = cov[i][j] for i <= j, row-major as torch.triu_indices(c, c):
 *          off(i, j) = i c - i (i - 1) / 2 + (j - i)
 *   inv_norm = 1 / max(||out row||_2, 1e-12)
 * out [b][c (c + 1) / 2] is NOT normalised: the L2 over it commutes with the
 * Linear that follows, whose reduce step takes inv_norm as its row scale
 * (rr_linear_splitk).  att_out [b][n] (may be NULL) receives the a_p.
 * Replaces SimilarityAttention.forward's last Linear, Sigmoid and multiply
 * (:84-90) and SecondOrderPooling.forward's mean, centring, bmm, gather and
 * F.normalize (:41-53).  The rows are centred BEFORE the product (a first
 * launch leaves a_p and the mean in the heads' scratch, rr_dolg_local_pool),
 * never as E[y y^T] - mu mu^T.  z is then read once per pair of 64-channel
 * tiles (upper-triangle pairs only); the weighted rows, the centred rows and
 * the square covariance never reach global memory; the Gram product runs on
 * the exact-fp32 MFMA.  No float atomics: where b < 64 an image's positions are
 * split over workgroups (a function of b and n only: at least 64 positions
 * each) and the partial tiles, kept in the scratch, are added in index order;
 * the sum of squares behind inv_norm is added in a fixed order as well: the
 * same bits on every run.
 * c % 32 == 0, 32 <= c <= 512; with hid: dh % 4 == 0, 4 <= dh <= 512;
 * 2 <= n <= 65535 (n == 1: the reference divides by N - 1 = 0 and returns
 * NaN); every pointer 16-B aligned (else RR_EINVAL, nothing written); b == 0
 * is RR_OK and launches nothing; offsets are 64-bit.  Timing class 3.       */
int rr_sos_cov(rr_handle_t h, const float* z, int b, int n, int c,
               const float* hid, int dh, const float* w3, float b3,
               float* att_out, float* out, float* inv_norm, void* stream);

/* Split-K form of the skinny linear:
 *   y[i][:] = act(row_scale[i] * (x_i . w^T) + bias),
 * x [m][k], w [n][k], y [m][n]; row_scale [m] and bias [n] may be NULL; act as
 * rr_linear_ex (0 none, 1 ReLU, 2 QuickGELU).  The k axis is cut into slices
 * that the fp32 MFMA core computes side by side (its split-K mode, partials
 * [m][slices][n] in the heads' scratch); a reduce kernel adds the slices in
 * index order and applies the scale, the bias and the activation.  The slice
 * count is a function of (m, k, n) and the device's compute-unit count only:
 * the same bits on every run.  For few rows and a long k, where rr_linear
 * leaves most of the chip idle (one workgroup per output tile walks all of k).
 * k % 4 == 0, x / w 16-B aligned (else RR_EINVAL); m == 0 is RR_OK.  Timing
 * class 1.                                                                   */
int rr_linear_splitk(rr_handle_t h, const float* x, int m, int k,
                     const float* w, int n, const float* row_scale,
                     const float* bias, int act, float* y, void* stream);

/* Same with a residual, as rr_linear_ex has one:
 *   y[i][:] = act(row_scale[i] * (x_i . w^T) + bias + residual[i][:]),
 * residual [m][n] dense, may be NULL (then the same bits as rr_linear_splitk:
 * both run the same kernels).  For the token aggregator's folded last layer,
 * whose B-row linears at K = 4096 and K = 2048 sit at rr_linear_ex's K-set
 * floor.                                                                     */
int rr_linear_splitk_ex(rr_handle_t h, const float* x, int m, int k,
                        const float* w, int n, const float* row_scale,
                        const float* bias, const float* residual, int act,
                        float* y, void* stream);

/* ---- token aggregator (models/token_based.py:60-86) ---------------------- */
/* The attention of the encoder's LAST layer for the global token alone
 * (TokenAggregator.forward keeps x[0], :81), with the K and V projections
 * folded away.  x [b][seq][d] dense: the layer's input rows; qt [b][heads][d]:
 * the folded, scaled query q~_h = Wk_h^T (Wq_h x0 + bq_h) / sqrt(d / heads)
 * (one rr_linear on b rows; the key bias shifts every score of a head alike and
 * cancels in the softmax); per image and head
 *   p_hj = softmax_j(qt_h . x_j)         (the maximum subtracted before exp)
 *   out_h = sum_j p_hj x_j               [b][heads][d]
 * and the caller applies M = [Wo[:,h] Wv_h]_h to out (rr_linear_splitk_ex with
 * the residual).  p (may be NULL) receives [b][heads][seq].
 * One workgroup per image takes all heads: x leaves HBM once, the second pass
 * reads it from cache; scores, p and the partial sums stay in LDS.  No float
 * atomics and no scratch: every sum runs in an order fixed by (seq, d, heads)
 * alone, so an image's result is the same bits alone or in a batch, on every
 * run and on every stream.
 * d % 64 == 0, 64 <= d <= 1024; 1 <= heads <= 16; 1 <= seq <= 256
 * (rr_attention's limit); x, qt, out and p 16-B aligned (else RR_EINVAL,
 * nothing written); b == 0 is RR_OK and launches nothing; offsets are 64-bit.
 * Timing class 5.                                                           */
int rr_cls_attn_pool(rr_handle_t h, const float* x, int b, int seq, int d,
                     const float* qt, int heads, float* p, float* out,
                     void* stream);

/* ---- SpoC head (models/spoc.py) ------------------------------------------ */
/* The spatial pyramid of max-pools in one launch.  x [b][hgt][wid][c] NHWC
 * fp32; levels [nlevels] is a HOST array read during the call.  Level L pools
 * kh x kw = (hgt / L) x (wid / L) windows (integer division) at a stride equal
 * to the window, no padding, floor mode: oh = hgt / kh, ow = wid / kw regions,
 * and trailing rows and columns that fill no window are dropped.  Regions are
 * row-major within a level and the levels follow one another, so out
 * [b][R][c] is the reference's pyramid_features [B,C,R] with the region axis
 * before the channels.  Replaces SpatialPyramidPooling.forward (:20-49,
 * pool_type 'max': one F.max_pool2d, view and cat per level).
 * The max starts from the window's first element (refined maps are signed);
 * it is defined for finite inputs, like rr_stem_pool_h2's.  One workgroup per
 * (image, region), 16-B loads along c.
 * 1 <= nlevels <= 8, 1 <= level <= min(hgt, wid), c % 4 == 0, x and out 16-B
 * aligned (else RR_EINVAL, nothing written); b == 0 is RR_OK and launches
 * nothing; offsets are 64-bit.  Timing class 3.
 * rr_spp_regions: R for (hgt, wid, levels), or -1 where rr_spp_max would
 * refuse them (a level above hgt or wid: the reference raises "stride should
 * not be zero").  Host only, no handle.                                     */
int rr_spp_regions(int hgt, int wid, const int* levels, int nlevels);
int rr_spp_max(rr_handle_t h, const float* x, int b, int hgt, int wid, int c,
               const int* levels, int nlevels, float* out, void* stream);

/* The gated refine conv.  With feature_refine's weight W = [Wx | Wc] split at
 * the input width, per position m
 *   a_m     = sigmoid(ctx_m . w_att + b_att)
 *   y[m][:] = a_m u[m][:] + ctx_m w_c^T + bias
 * u [m][c]: the RAW product Wx x_m from the conv core (no bias; the gate
 * commutes with it, as in rr_sos_cov's a_p (Wp x_p)); ctx [m][dc]: the context
 * encoder's output; w_att [dc], w_c [c][dc], bias [c]; att [m] (may be NULL)
 * receives the a_m.  y may alias u: each element is read and written by the
 * same thread.  Replaces ContextualAttention.forward's attention_conv +
 * sigmoid (:83), the multiply (:86), the cat (:89) and feature_refine's
 * context half and bias (:92): the attended map and the concatenation never
 * exist.  The product over dc runs on the exact-fp32 MFMA in 64 x 64 tiles;
 * the logit is computed inside the same kernel from the staged ctx rows, in
 * an order that depends on dc alone, so every column tile of a row applies
 * the same a_m bits; no scratch, the same bits on every run.
 * dc % 32 == 0, 32 <= dc <= 2048; c % 4 == 0; m >= 0; every pointer 16-B
 * aligned (else RR_EINVAL, nothing written); m == 0 is RR_OK and launches
 * nothing.  Timing class 1.                                                  */
int rr_spoc_refine(rr_handle_t h, const float* u, const float* ctx, int m,
                   int c, int dc, const float* w_att, float b_att,
                   const float* w_c, const float* bias, float* att, float* y,
                   void* stream);

/* A linear whose result is needed only as a per-image max over rows:
 *   out[i][j] = max_{q < r} act(x[i r + q] . w[j] + bias[j]),
 * x [b r][k], w [n][k], bias [n] (may be NULL), out [b][n]; act 0 none, 1 ReLU.
 * Replaces feature_aggregation (:131-136: Conv1d(1) + BatchNorm1d folded into
 * w and bias + ReLU + AdaptiveMaxPool1d(1)); the [b r][n] product never
 * reaches global memory.  One image's r rows are the rows of one 64-row tile
 * of the exact-fp32 MFMA; rows past r inside the tile are left out of the max
 * (as zero rows they would give act(bias[j])), and the max starts at -inf.
 * No split over k and no scratch: an image's result is the same bits alone
 * or in a batch, on every run.
 * 1 <= r <= 64; k % 4 == 0; n >= 1 (any n: stores are per element); b >= 0;
 * every pointer 16-B aligned (else RR_EINVAL, nothing written); b == 0 is
 * RR_OK and launches nothing.  Timing class 1.                               */
int rr_linear_groupmax(rr_handle_t h, const float* x, int b, int r, int k,
                       const float* w, const float* bias, int n, int act,
                       float* out, void* stream);

/* ---- Squeeze-and-Excitation block (models/senet_g2.py) ------------------- */
/* The squeeze: mean[i][ch] = (1 / hw) sum_p y[i][p][ch], y [b][hw][c] NHWC
 * fp32 (conv3 + bn3's output), mean [b][c].  Replaces SEBlock's
 * AdaptiveAvgPool2d(1) (:17, :27).  Values are signed and nothing is clamped
 * (rr_gem_pool clamps at eps, so it cannot serve).  One pass over y with 16-B
 * loads along c: a workgroup takes a chunk of an image's positions and one
 * 256-channel group; an image's positions are split over workgroups only
 * while whole images leave the chip short of work, by a rule of (b, hw)
 * alone, the chunks' partial sums pass through the heads' per-stream scratch
 * and are added in a fixed order, then divided by hw: no float atomics, the
 * same bits on every run and on every stream.
 * c % 256 == 0 (the fixed-order adder's row length; every bottleneck output
 * width is one), hw >= 1, b >= 0; y and mean 16-B aligned (else RR_EINVAL,
 * nothing written); b == 0 is RR_OK and launches nothing; offsets are 64-bit.
 * Timing class 3.                                                           */
int rr_se_squeeze(rr_handle_t h, const float* y, int b, int hw, int c,
                  float* mean, void* stream);

/* The excitation's second FC, the scale, the identity and the ReLU:
 *   g[i][ch]       = sigmoid(w2[ch][:] . hidden[i][:])
 *   out[i][p][ch]  = act(y[i][p][ch] * g[i][ch] + identity[i][p][ch])
 * w2 [c][cr] (fc.2.weight), hidden [b][cr] = relu(W1 mean) (from
 * rr_linear_splitk, act 1), y / identity / out [b][hw][c]; act is max(0, .)
 * when relu != 0.  Replaces SEBlock's fc[2], fc[3] and x * y.expand_as(x)
 * (:21-22, :28-29) and SEBottleneck's out += residual; relu (:69-70).
 * identity may be NULL (no add).  gate_out [b][c] (may be NULL) receives the
 * g.  out_amax (may be NULL; RR_AMAX_SLOTS words zeroed by the caller)
 * receives max |out| over the finite values, in the record format of
 * rr_conv2d_h2's y_amax: the next block's convs read it and need no extra
 * pass.  out may alias y or identity: each element is read and written by the
 * same thread.
 * A workgroup owns one (image, 64-channel slab, row chunk): it forms its 64
 * gates once from the w2 slab (64 x cr floats) in an order fixed by cr alone,
 * so every row chunk of an image applies the same gate bits and an image's
 * gates are the same bits alone or in a batch, then streams its rows with
 * 16-B loads and stores.  The sigmoid is 1 / (1 + exp(-z)): exactly 0 / 1 at
 * logits of -100 / +100, never NaN for a finite logit.
 * c % 64 == 0; cr % 4 == 0, 4 <= cr <= 512; hw >= 1; b >= 0; every pointer
 * 16-B aligned (else RR_EINVAL, nothing written); b == 0 is RR_OK and
 * launches nothing; offsets are 64-bit.  Timing class 3.                    */
int rr_se_apply(rr_handle_t h, const float* y, const float* hidden,
                const float* w2, const float* identity, int b, int hw, int c,
                int cr, int relu, float* gate_out, float* out,
                unsigned* out_amax, void* stream);

/* ---- native ResNet trunk plan (f16x2 core) -------------------------------
 * One call per forward for the whole bottleneck-ResNet trunk (torchvision
 * children[:-2], networks/backbone.py:60-109, or ResNet_DOLG :218-274) from
 * uint8 pixels: rr_preprocess_u8_ex (out_c 4), rr_amax_f32, the stem
 * (rr_stem_pool_h2, or rr_conv2d_h2 + rr_maxpool2d), then per bottleneck
 * conv1, conv2 and conv3 through rr_conv2d_h2 (a stage's first block: its
 * downsample projection first, or conv3 + projection as one
 * rr_bottleneck_out_h2), every conv reading its input's max-|x| record and
 * publishing its output's.  The plan adds no kernel: it issues exactly these
 * entry points, so the result is the same bits as calling them one by one.
 *
 * desc lists the convs in execution order: the stem, then per block
 * [downsample, only in a stage's first block when fuse_entry[stage] == 0,]
 * conv1, conv2, conv3.  With fuse_entry[stage] != 0 the first block's conv3
 * entry holds rr_split2_f16 of the concatenated rows [W3 | Wd] (cin = planes +
 * the block's input channels, bias = the two biases' sum, stride = the
 * block's stride), as rr_bottleneck_out_h2 takes them.  All pointers are
 * device pointers the caller keeps alive as long as the plan; the desc itself
 * is copied.  rr_trunk_h2_create checks the channel chain and the strides
 * against blocks[] and stride_on (RR_EINVAL otherwise).
 *
 * Parts.  A forward runs the batch in one part on the caller's stream, or cut
 * in two at B / 2 (part 0 = images [0, B / 2)) on the plan's two non-blocking
 * streams: both wait on an event recorded on the caller's stream, part 1
 * also on an event part 0 records after its lag-th conv (the stem is conv 0,
 * unfused downsample projections are not counted; a lag past the last conv
 * means no such wait), and the caller's stream waits on both at the end.  The
 * host issues the two parts' launches alternately.  The parts then run side by
 * side about one layer apart, and the last, partly filled round of one
 * part's kernel is filled with the other part's blocks.  Each part is exactly
 * the one-part forward of its images, its split scales taken from its own
 * max-|x| records, written straight into its rows of out_x4 / out_x3.
 * rr_trunk_h2_parts returns what a forward will choose: RR_TUNE_TRUNK_PARTS when
 * set to 1 or 2 (2 needs B >= 2), else the library's pick, which is 2 only when
 * each part still gives the last stage's output, [B / 2 * oh * ow rows] x cout
 * in 256 x 256 tiles, at least two tiles per compute unit:
 *   ceil((B / 2) oh ow / 256) * (cout / 256) >= 2 * CUs.
 * (The last stage has the smallest map, so the fewest row tiles; below two
 * tiles per CU a part's launch no longer fills the chip for two rounds, and
 * what the split costs -- every weight plane streamed twice, twice as many
 * partly filled last rounds -- outweighs the rounds it can fill.  R101, 224 x
 * 224, 256 CUs: two parts from B = 660.)  One part touches no plan stream.
 *
 * images: uint8 [B][H][W][3], H, W >= 1 (B < 0, H < 1 or W < 1: RR_EINVAL);
 * B == 0 is RR_OK with no launch.  out_x4 [B][oh][ow][cout]: each stride-2 step
 * (the stem, its pool, every stage but the first) maps n to (n - 1) / 2 + 1,
 * so a four-stage trunk gives ceil(H / 32) x ceil(W / 32) and x3 ceil(H / 16) x
 * ceil(W / 16).  out_x4_amax: x4's max-|x| record
 * (RR_AMAX_SLOTS words; zeroed by the call; with two parts both parts' last
 * conv publish into it, which gives the element-wise max of the records the
 * parts would have written alone).  out_x3 / out_x3_amax (both or neither,
 * NULL to skip; needs >= 4 stages): the third stage's output and its record;
 * with two parts that record is folded from the parts' records by rr_amax_f32
 * after the join: it holds the same maximum, not the same words.
 * workspace: rr_trunk_h2_workspace_size(plan, B, H, W, parts) bytes (parts 1
 * or 2; 0 for a bad argument), 256-B aligned, RR_EWORKSPACE when short.  The
 * plan's streams and events are shared by its forwards: calls on one plan are
 * serialised on the host (a mutex), and two-part forwards of one plan run one
 * after the other on the device.
 * rr_trunk_h2_counters: out[0] = forwards, out[1] = two-part forwards,
 * out[2] = launches, waits and records issued on the plan's own streams.    */
#define RR_TRUNK_MAX_STAGES 8
typedef struct rr_trunk_conv_s {
  const void* w2;        /* rr_split2_f16 planes [2][cout][K] */
  const float* w_iscale; /* [cout] */
  const float* bias;     /* [cout] or NULL */
  int cin, cout, kh, kw, stride, pad;
  int residual; /* 1: adds the block's identity (conv3 of a block) */
  int relu;
} rr_trunk_conv_t;
typedef struct rr_trunk_desc_s {
  int n_stages;
  int blocks[RR_TRUNK_MAX_STAGES];     /* bottlenecks per stage */
  int fuse_entry[RR_TRUNK_MAX_STAGES]; /* first block: conv3 + projection as one GEMM */
  int stride_on;                       /* 0: the 3x3 conv2 carries a block's stride, 1: the 1x1 conv1 */
  int fuse_stem_pool;                  /* the stem, its ReLU and the max-pool as one launch (stem cout 64) */
  int lag;                             /* part 1 starts after part 0's lag-th conv (>= 0; 1 is the measured default) */
  float mean[3], std[3];               /* rr_preprocess_u8's */
  int n_convs;
  const rr_trunk_conv_t* convs;
} rr_trunk_desc_t;
typedef struct rr_trunk_plan_s* rr_trunk_plan_t;
int rr_trunk_h2_create(rr_handle_t h, const rr_trunk_desc_t* desc, rr_trunk_plan_t* out);
int rr_trunk_h2_destroy(rr_handle_t h, rr_trunk_plan_t plan);
size_t rr_trunk_h2_workspace_size(rr_trunk_plan_t plan, int b, int hgt, int wid, int parts);
int rr_trunk_h2_parts(rr_handle_t h, rr_trunk_plan_t plan, int b, int hgt, int wid);
int rr_trunk_h2_counters(rr_trunk_plan_t plan, long long* out3);
int rr_trunk_h2_forward_u8(rr_handle_t h, rr_trunk_plan_t plan, const uint8_t* img_nhwc, int b, int hgt, int wid,
                           float* out_x4, unsigned* out_x4_amax, float* out_x3, unsigned* out_x3_amax,
                           void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RR_H_ */
