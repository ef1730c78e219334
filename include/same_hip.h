/*
 * same_hip.h -- C ABI of libsame_hip.so: the MI355X (gfx950) implementation of SAME's
 * pre-MIP data-parallel path.
 *
 * The reference (rohitsinghlab/SAME) is pure Python and has no FFI; its boundary for this
 * path is a set of Python functions and inline loops.  Each entry
 * point below names the reference code it replaces (file:line into the reference tree).
 * The Python host layer in same_amd/ keeps the reference's signatures and calls these
 * through ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - plain C: pointers + sizes only, no C++/torch types.
 *  - every function returns 0 on success or a negative SAME_E* code; on failure outputs are
 *    unspecified but never written out of bounds.  same_strerror() names the code and
 *    same_last_error() returns the HIP/RCCL detail recorded on the context.
 *  - "host" entry points take caller-owned, C-contiguous host buffers; the library copies
 *    in, runs on the context's own stream, copies out and is synchronous on return.  It
 *    never keeps a host pointer past the call.
 *  - "_dev" entry points take device pointers obtained from same_dev_alloc() and only
 *    enqueue work on the context's stream (call same_ctx_sync() to wait).  They exist so
 *    large operands (the dense cost matrix is 80 GB at 100k x 100k) stay resident in HBM.
 *  - indices are int32, sizes int64.  pairs are int32 [P][2] = (aligned i, ref j).
 *    triangles are int32 [Tr][3] of aligned-row indices.  xy arrays are double [n][2].
 *    type matrices are row-major double [n][T] (the commonCT columns, in commonCT order).
 *  - threading: a context is used by one caller at a time; any thread may make the call
 *    (every entry point selects the context's device itself).
 */
#ifndef SAME_HIP_H
#define SAME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAME_OK 0
#define SAME_EINVAL (-22)   /* bad shape / NULL / unsupported size */
#define SAME_ENOMEM (-12)   /* host or device allocation failed */
#define SAME_EIO (-5)       /* HIP or RCCL call failed; see same_last_error() */
#define SAME_ENODEV (-19)   /* no usable GPU */
#define SAME_ERANGE (-34)   /* an index in pairs/triangles/match is out of range */
#define SAME_EUNSURE (-11)  /* same_delaunay2d only: not an error -- the points are too close to degenerate to answer for Qhull */

#define SAME_ABI_VERSION 9
#define SAME_MAX_KNN 448     /* largest k supported by the prune kernel (k <= 64 runs the 8-rows-per-wave form) */
#define SAME_MAX_TYPES 4096  /* largest T (type columns) */

typedef struct same_ctx same_ctx;
typedef struct same_sweep same_sweep; /* resident state of one lazy-constraint sweep (same_sweep_bind) */

/* ---- index of this header ------------------------------------------------------------------------------------------------------
 * part 0  context, device memory                                     same_ctx_*, same_dev_*, same_h2d / d2h / d2d
 * part 1  HOST-BUFFER entry points (caller's arrays in and out; one   same_pair_cost_*, same_dense_cost_f64 / f32, same_knn_prune, same_tri_*, same_sweep_* /
 *         call = upload, kernels, download, wait)                     same_orient_sweep*, same_xyorder_sweep, same_area_flip, same_pair_rowmin,
 *                                                                     same_assign_matrix, same_greedy_*, same_tri_flip_stats, same_collapse_candidates,
 *                                                                     same_batched_assign, same_eager_signs, same_window_count, same_merge_dedup,
 *                                                                     same_check_alignment
 * part 2  DEVICE-RESIDENT forms (operands already in HBM; enqueue     same_dense_cost_*_dev, same_knn_prune_dev, same_knn_index_*,
 *         only unless noted)                                          same_knn_prune_indexed_dev, same_padded_cost_*_dev, same_tri_*_dev,
 *                                                                     same_area_flip_dev, same_xyorder_sweep_dev, same_orient_*_dev, same_first_candidate_dev
 * part 3  WINDOW path, sections resident (BASELINE cfg 5)             same_section_*, same_window_*, same_merge_acc_*, same_members_*, same_delaunay2d (host),
 *                                                                     same_delaunay_filtered, same_unpack_detail_*, same_unpack_map_*
 * part 4  COMM: RCCL collectives between the ranks' contexts          same_comm_*, same_allgather_dev*, same_allreduce_dev
 * Every declaration cites the reference lines it replaces (file:line into the reference tree).
 * Measurement hooks and opt-in controls that are NOT the path -- runtime-call counters, timers, the spread allocator, the fixed-point
 * dense build, the all-gather's device time -- are declared in same_hip_diag.h (same library). */

/* ======================================================================================================================
 * part 0 -- context, device memory
 * ====================================================================================================================== */
/* ---- context ------------------------------------------------------------------------- */
int same_abi_version(void);
int same_device_count(int *out_count);
int same_ctx_create(int device, same_ctx **out);
void same_ctx_destroy(same_ctx *ctx);
int same_ctx_sync(same_ctx *ctx);
const char *same_strerror(int code);
const char *same_last_error(same_ctx *ctx);
/* device name, CU count, HBM bytes (any pointer may be NULL) */
int same_ctx_info(same_ctx *ctx, char *name, size_t name_len, int *cu_count, int64_t *hbm_bytes);
/* ---- device memory (for resident operands) ------------------------------------------------ */
int same_dev_alloc(same_ctx *ctx, size_t bytes, void **out_dptr);
int same_dev_free(same_ctx *ctx, void *dptr);   /* either kind of buffer */
int same_h2d(same_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int same_d2h(same_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int same_dev_memset(same_ctx *ctx, void *dst_dev, int value, size_t bytes);
/* device-to-device copy, enqueued on the context's stream (no wait) */
int same_d2d(same_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);
/* The host-buffer entry points stage through per-context scratch blocks that grow on demand and are
 * reused across calls; this frees them all (same_sweep handles own their blocks and are not affected). */
int same_ctx_release_scratch(same_ctx *ctx);
/* ======================================================================================================================
 * part 1 -- HOST-BUFFER entry points: the caller's (NumPy) arrays in and out; synchronous
 * ====================================================================================================================== */
/* ---- a4: pair costs -------------------------------------------------------------------
 * Replaces the loop at src/same.py:1180-1189:
 *   c[p] = w * sum_t |A[i,t]-R[j,t]|  +  (w*0.001) * (|ax-rx| + |ay-ry|),  (i,j) = pairs[p]
 * with the type sum accumulated left to right in fp64 and no fused multiply-add. */
int same_pair_cost_f64(same_ctx *ctx, const double *A, const double *R, int64_t n_m, int64_t n_r,
                       int T, const double *axy, const double *rxy, const int32_t *pairs,
                       int64_t P, double w, double *out_c);
/* fp32 variant (BASELINE.json config 5: "fp32 cost"): the same expression evaluated in float, operands given as
 * float -- element (i, j) of same_dense_cost_f32.  The reference has no fp32 path; the check is bit-equality
 * with the test oracle's float twin plus a forward error bound against the fp64 costs. */
int same_pair_cost_f32(same_ctx *ctx, const float *A, const float *R, int64_t n_m, int64_t n_r,
                       int T, const float *axy, const float *rxy, const int32_t *pairs,
                       int64_t P, float w, float *out_c);

/* ---- dense cost tile builder ----------------------------------------------------------
 * The same expression for every (i, j), i in [row_begin,row_end), j in [0,n_r):
 *   out[(i-row_begin)*ld + j].  Generalises the only dense matrix of the reference
 * (src/init_helpers.py:151-155) to the metric of BASELINE.json (100k x 100k).
 * The device-resident forms (same_dense_cost_*_dev, part 2) are what large operands use: this form copies in, builds, copies out. */
int same_dense_cost_f64(same_ctx *ctx, const double *A, const double *R, int64_t n_m, int64_t n_r,
                        int T, const double *axy, const double *rxy, int64_t row_begin,
                        int64_t row_end, double w, double *out, int64_t ld);
int same_dense_cost_f32(same_ctx *ctx, const float *A, const float *R, int64_t n_m, int64_t n_r,
                        int T, const float *axy, const float *rxy, int64_t row_begin,
                        int64_t row_end, float w, float *out, int64_t ld);

/* ---- a2: KNN prune within a radius ----------------------------------------------------
 * Replaces the per-row body of utils.find_knn_within_radius (src/utils.py:720-728):
 * for aligned rows [row_begin,row_end): refs with dx*dx+dy*dy <= radius*radius (cKDTree
 * query_ball_point, p=2), ranked by (squared distance, ref index) ascending, first k kept.
 * out_idx[(i-row_begin)*k + q] (-1 padded), out_d2 likewise (+inf padded; may be NULL),
 * out_cnt[i-row_begin] = number kept.  The frame compaction of src/utils.py:734-742 stays
 * on the host (same_amd/knn.py). */
int same_knn_prune(same_ctx *ctx, const double *axy, int64_t n_m, const double *rxy, int64_t n_r,
                   int64_t row_begin, int64_t row_end, double radius, int k, int32_t *out_idx,
                   double *out_d2, int32_t *out_cnt);

/* ---- a7: triangle classes -------------------------------------------------------------
 * Replaces the per-triangle decisions of helpers.filter_triangles_by_radius
 * (src/helpers.py:303-341).  out_class: 0 kept, 1 max side >= radius, 2 min angle too
 * small, 3 passed both but all three type_id equal (type_id NULL = test off).
 * The angle rule degrees(arccos(c)) < min_angle_deg is passed as a cosine threshold
 * (angle_enabled, cos_thr): fails iff clipped cosine >= cos_thr; out_maxcos gets the
 * largest clipped corner cosine (2.0 if a side has zero length).  out_perim = s1+s2+s3.
 * The re-add pass (src/helpers.py:365-389) stays on the host (same_amd/triangles.py). */
int same_tri_classify(same_ctx *ctx, const double *xy, int64_t n_pts, const int32_t *tris,
                      int64_t Tr, double radius, int angle_enabled, double cos_thr,
                      const int32_t *type_id, uint8_t *out_class, double *out_perim,
                      double *out_maxcos);

/* ---- a8: triangle weights and source orientation signs --------------------------------
 * Replaces src/same.py:1128-1135 and :1139-1146.  size/out_weight may both be NULL. */
int same_tri_sign_weight(same_ctx *ctx, const double *xy, const double *size, int64_t n_pts,
                         const int32_t *tris, int64_t Tr, int8_t *out_sign, double *out_weight);

/* ---- a10: lazy-constraint orientation sweep -------------------------------------------
 * Replaces the body of _lazy_orientation_callback (src/same.py:631-669).
 * same_sweep_bind uploads triangles, source signs, reference XY and the pair list once (the model._*
 * state of src/same.py:1153-1158) into device blocks owned by the returned handle; pairs may be NULL
 * when only the match-vector form is used.  Several handles may live on one context (one per window /
 * per model); same_sweep_unbind frees one.  Every sweep call names the length of the array it passes and
 * fails with SAME_EINVAL if it is not the bound one, so a handle can never be run against another
 * model's shapes.  Calls on handles of one context must not overlap (the context has one stream), and
 * every handle must be unbound before its context is destroyed.
 * same_orient_sweep_x: x_vals[P] -> matching (last pair with x > 0.5 wins per aligned row,
 * src/same.py:634-639) -> sweep.  out_viol_idx needs room for Tr entries and comes out
 * ascending; out_flag (may be NULL): 0 skipped, 1 checked, 2 flipped;
 * out_match / out_pair_idx (may be NULL): the matching and its pair indices (for cbLazy). */
int same_sweep_bind(same_ctx *ctx, const int32_t *tris, int64_t Tr, const int8_t *src_sign,
                    const double *rxy, int64_t n_r, int64_t n_m, const int32_t *pairs, int64_t P,
                    same_sweep **out);
void same_sweep_unbind(same_sweep *sweep);
int same_orient_sweep(same_sweep *sweep, const int32_t *match, int64_t n_m, int64_t *out_checked,
                      int32_t *out_viol_idx, int64_t *out_nviol, uint8_t *out_flag);
int same_orient_sweep_x(same_sweep *sweep, const double *x_vals, int64_t P, int64_t *out_checked,
                        int32_t *out_viol_idx, int64_t *out_nviol, uint8_t *out_flag,
                        int32_t *out_match, int32_t *out_pair_idx);

/* ---- a11: XY-order preservation sweep -------------------------------------------------
 * Replaces the triangle loop of violationhelper.verify_spatial_preservation
 * (src/violationhelper.py:53-117).  edge_flags[t*3+e]: bit0 compared, bit1 X violated,
 * bit2 Y violated; e = (v0,v1),(v0,v2),(v1,v2).  counts = {comparisons, violations,
 * violated triangles}.  point_flag[n_m]. */
int same_xyorder_sweep(same_ctx *ctx, const double *axy, int64_t n_m, const double *rxy,
                       int64_t n_r, const int32_t *tris, int64_t Tr, const int32_t *match,
                       uint8_t *edge_flags, uint8_t *tri_flag, uint8_t *point_flag,
                       int64_t counts[3]);

/* ---- a12: signed areas before/after and flips -----------------------------------------
 * Replaces src/same.py:1362-1402 with helpers.calculate_signed_area (src/helpers.py:73-77).
 * after = NaN unless all three vertices are matched. */
int same_area_flip(same_ctx *ctx, const double *axy, int64_t n_m, const double *rxy, int64_t n_r,
                   const int32_t *tris, int64_t Tr, const int32_t *match, double *out_before,
                   double *out_after, uint8_t *out_matched3, uint8_t *out_flipped);

/* ---- a5: MIP-start helpers ------------------------------------------------------------
 * Per-row minimum pair cost (src/init_helpers.py:118-122; +inf for rows without pairs) and
 * the dense assignment matrix [n_m][n_r+n_m] (src/init_helpers.py:151-155). */
int same_pair_rowmin(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P,
                     int64_t n_m, double *out_min);
int same_assign_matrix(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P,
                       const double *unmatched, int64_t n_m, int64_t n_r, double big_m,
                       double *out);

/* ---- f1: greedy MIP start resolved on the device, node-local flip statistics ----------
 * same_greedy_match replaces the sort + sequential scan of src/init_helpers.py:109-133 with an
 * equivalent parallel rule (a pair is taken when it is the (cost, pair index)-minimum at both of
 * its endpoints among the pairs still alive).  prefer[i] = best_cost_i < unmatched_cost_i
 * (:118-122).  out_match_pair[i] = index of the pair chosen for aligned row i, or -1.
 * same_tri_flip_stats replaces the triangle loop of eval_utils.check_triangle_violations
 * (src/eval_utils.py:123-187) on node-indexed arrays: out_tri_flag bit0 all matched, bit1 same
 * type (type_id NULL = off), bit2 flipped; node counters over non-same-type triangles. */
int same_greedy_match(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P,
                      int64_t n_m, int64_t n_r, const uint8_t *prefer, int32_t *out_match_pair,
                      int *out_rounds);
int same_tri_flip_stats(same_ctx *ctx, const double *axy, const double *mapped_xy,
                        const uint8_t *matched, int64_t n, const int32_t *type_id,
                        const int32_t *tris, int64_t Tr, uint8_t *out_tri_flag,
                        uint32_t *out_node_tri, uint32_t *out_node_flip);

/* ---- f2: k-nearest-template label check of eval_utils.check_alignment (src/eval_utils.py:6-53) ----------------------------
 * For each query point: is its label code among the codes of its k nearest template points (cKDTree.query(k))?  Labels arrive
 * as int32 codes made by the caller (equal codes = equal labels; a code no template point carries never matches).  Exact against
 * scipy, whose order among (nearly) equidistant points follows its tree: with d_k the k-th smallest d2 = dx*dx + dy*dy (fp64,
 * no contraction), B = {d2 within d_k * 1e-12 + 1e-300 of d_k}, S = {d2 below B}, a row is decided on the device only when the
 * answer does not depend on which members of B scipy takes -- k > 1: label in S (match), in no member of B (no match),
 * |S| + |B| <= k (match); k == 1: |S| = 0 and |B| = 1.  out_flag[i] = SAME_ALIGN_DECIDED | SAME_ALIGN_MATCH bits; the caller
 * resolves the rows without SAME_ALIGN_DECIDED itself.  out_nearest (k == 1 only, else may be NULL) = the unique nearest
 * template row of a decided query, -1 otherwise; neighbour lists for k > 1 never leave the device.
 * 1 <= k <= SAME_ALIGN_MAX_KNN, k <= n_t when n_q > 0, n_q and n_t < 2^31, every coordinate finite (else SAME_EINVAL). */
#define SAME_ALIGN_MAX_KNN 64
#define SAME_ALIGN_MATCH 1
#define SAME_ALIGN_DECIDED 2
int same_check_alignment(same_ctx *ctx, const double *qxy, int64_t n_q, const int32_t *qcode,
                         const double *txy, int64_t n_t, const int32_t *tcode, int k,
                         uint8_t *out_flag, int32_t *out_nearest);

/* ---- f2: metacell collapse (metacell_utils.greedy_triangle_collapse) -----------------------
 * same_collapse_candidates replaces the per-triangle work of one collapse iteration
 * (src/metacell_utils.py:233-260 validity, :393-431 candidate test and priority):
 * out_flag bit0 = valid (no edge > r_max, no corner angle < min_angle, as a cosine threshold),
 * bit1 = collapsible (valid, one cell type, not size sum > max_size: a NaN sum or max_size
 * passes, as it does in the reference); out_perim = priority; out_total = size sum.  On NaN the
 * validity rule is the reference's Python max(edge1, edge2, edge3) and min(angle1, angle2,
 * angle3): the first operand stays unless a later one compares greater (less), so a leading NaN
 * wins (the test then passes) and later NaNs are skipped.  same_greedy_disjoint replaces the
 * sort + vertex-disjoint scan of :438-449 on items[M][3] with keys[M] (ties by item index; +0.0
 * and -0.0 are one key), out_selected[M], out_rounds (may be NULL) = rounds that took an item.
 * NaN keys are outside the contract: the reference's sort on them is not an order. */
int same_collapse_candidates(same_ctx *ctx, const double *xy, int64_t n, const int32_t *tris,
                             int64_t Tr, int rmax_enabled, double r_max, int angle_enabled,
                             double cos_thr, const int32_t *type_id, const double *size,
                             double max_size, uint8_t *out_flag, double *out_perim,
                             double *out_total);
int same_greedy_disjoint(same_ctx *ctx, const int32_t *items, const double *keys, int64_t M,
                         int64_t n_nodes, uint8_t *out_selected, int *out_rounds);

/* ---- f4: unpack_metacell_matches(strategy='nearest') --------------------------------------
 * Replaces the per-match cdist + np.tile + scipy linear_sum_assignment of
 * src/metacell_utils.py:711-761 with one batched launch.  Problem p assigns the aligned members
 * axy[a_off[p]..a_off[p+1]) to the ref members rxy[r_off[p]..r_off[p+1]) (CSR offsets, n_prob+1
 * entries, first 0); when there are more aligned than ref members every ref member may be used
 * ceil(n_a/n_r) times (tiled columns, :744-748).  out_ref[a_off[p]+i] = index within problem p's
 * ref members given to aligned member i; ties resolve as scipy's solver resolves them.
 * SAME_ERANGE if a problem has non-finite coordinates (scipy raises ValueError there);
 * SAME_EINVAL if a problem has aligned members but no ref member, or more than
 * SAME_ASSIGN_MAX_MEMBERS on either side (one lane solves one problem in O(n^3): metacells are
 * a handful of cells; the bound keeps a malformed input from occupying the GPU for minutes). */
#define SAME_ASSIGN_MAX_MEMBERS 512
int same_batched_assign(same_ctx *ctx, int64_t n_prob, const int64_t *a_off, const int64_t *r_off,
                        const double *axy, const double *rxy, int32_t *out_ref);

/* ---- a14: eager reference-orientation signs -------------------------------------------
 * Replaces calc_ref_area over all candidate combinations (src/helpers.py:425-441,455-510):
 * out[((t*k+x)*k+y)*k+z] = sign(round(cross, 3)) for cand[tris[t][0]][x], ..., 2 if any is -1. */
int same_eager_signs(same_ctx *ctx, const double *rxy, int64_t n_r, const int32_t *tris,
                     int64_t Tr, const int32_t *cand, int64_t n_m, int k, int8_t *out);

/* ---- a13: window membership -----------------------------------------------------------
 * subset_data (src/same.py:293-295) for a batch of boxes: boxes[b] = {x0,x1,y0,y1},
 * half-open.  out_count[b] = rows inside; out_mask (may be NULL) [n_boxes][n]. */
int same_window_count(same_ctx *ctx, const double *xy, int64_t n, const double *boxes,
                      int64_t n_boxes, int64_t *out_count, uint8_t *out_mask);

/* ---- f3: window merge, the de-duplication step ------------------------------------------
 * Replaces src/helpers.py:745-753 (merged_df.sort_values(['filtered_violation', 'window_id'], kind='mergesort') then
 * drop_duplicates([aligned, ref], keep='first')): rows i = 0..n-1 of the concatenated per-window match tables carry a
 * violation flag, a window id and integer codes of their aligned / ref ids (equal ids <=> equal codes; any
 * non-negative int32).  out_rows receives the indices of the rows that survive, in the order the reference's frame has
 * after those two calls (stable by violation, then window id; first row of every pair); *out_n their number.
 * The maximum-cardinality matching that follows (:755-815) is sequential and stays with the caller. */
int same_merge_dedup(same_ctx *ctx, const uint8_t *viol, const int32_t *window_id, const int32_t *aligned_code,
                     const int32_t *ref_code, int64_t n, int32_t *out_rows, int64_t *out_n);

/* ======================================================================================================================
 * part 2 -- DEVICE-RESIDENT forms: every pointer is a device pointer of the context's GPU; calls enqueue on the context's stream
 * ====================================================================================================================== */
/* ---- dense cost tile builder, operands resident (the roofline kernel of the bench; expression and indexing as
 * same_dense_cost_f64 in part 1): all pointers are device pointers; dA / dR / daxy / drxy hold the full arrays. */
int same_dense_cost_f64_dev(same_ctx *ctx, const double *dA, const double *dR, int T,
                            const double *daxy, const double *drxy, int64_t n_r,
                            int64_t row_begin, int64_t row_end, double w, double *dout, int64_t ld);
int same_dense_cost_f32_dev(same_ctx *ctx, const float *dA, const float *dR, int T,
                            const float *daxy, const float *drxy, int64_t n_r, int64_t row_begin,
                            int64_t row_end, float w, float *dout, int64_t ld);

/* ---- a2 on resident operands: the prune of same_knn_prune (part 1) with device pointers, the caller-held index, the costs of
 * the padded candidate lists */
int same_knn_prune_dev(same_ctx *ctx, const double *daxy, const double *drxy, int64_t n_r,
                       int64_t row_begin, int64_t row_end, double radius, int k,
                       int32_t *dout_idx, double *dout_d2, int32_t *dout_cnt);
/* Caller-held index of one reference set for one radius.  same_knn_prune_dev rebuilds the uniform grid
 * of the references (a counting sort) and reads their bounding box back on every call; when the same
 * references are pruned against repeatedly -- windows that share a reference section, the row blocks of
 * a sharded build, a benchmark step -- build the index once: same_knn_prune_indexed_dev then only
 * enqueues the query kernel (no rebuild, no host synchronisation) and returns bit-identical lists.
 * drxy is the caller's device array: it is not copied for the brute-force plan (small or degenerate
 * sets), so it must stay valid and unchanged until same_knn_index_destroy. */
typedef struct same_knn_index same_knn_index;
int same_knn_index_build(same_ctx *ctx, const double *drxy, int64_t n_r, double radius,
                         same_knn_index **out);
void same_knn_index_destroy(same_knn_index *index);
int same_knn_prune_indexed_dev(same_ctx *ctx, const same_knn_index *index, const double *daxy,
                               int64_t row_begin, int64_t row_end, int k, int32_t *dout_idx,
                               double *dout_d2, int32_t *dout_cnt);
/* costs of the padded candidate lists (a2 + a4 fused for the sharded path):
 * out_cost[(i-row_begin)*k + q] = pair cost of (i, idx[..]) or +inf where idx == -1. */
int same_padded_cost_f64_dev(same_ctx *ctx, const double *dA, const double *dR, int T,
                             const double *daxy, const double *drxy, int64_t row_begin,
                             int64_t row_end, int k, const int32_t *didx, double w,
                             double *dout_cost);
int same_padded_cost_f32_dev(same_ctx *ctx, const float *dA, const float *dR, int T,
                             const float *daxy, const float *drxy, int64_t row_begin,
                             int64_t row_end, int k, const int32_t *didx, float w,
                             float *dout_cost);

/* ---- device-resident forms of the triangle kernels and sweeps -------------------------
 * Same semantics as the host-buffer entry points above; every pointer is a device pointer
 * and the call only enqueues on the context's stream.  Index ranges are the caller's
 * responsibility here (the host-buffer forms validate them).  dcounts = 3 x uint64. */
int same_tri_classify_dev(same_ctx *ctx, const double *dxy, const int32_t *dtris, int64_t Tr,
                          double radius, int angle_enabled, double cos_thr, const int32_t *dtype_id,
                          uint8_t *dout_class, double *dout_perim, double *dout_maxcos);
int same_tri_sign_weight_dev(same_ctx *ctx, const double *dxy, const double *dsize,
                             const int32_t *dtris, int64_t Tr, int8_t *dout_sign, double *dout_weight);
int same_area_flip_dev(same_ctx *ctx, const double *daxy, const double *drxy, const int32_t *dtris,
                       int64_t Tr, const int32_t *dmatch, double *dout_before, double *dout_after,
                       uint8_t *dout_matched3, uint8_t *dout_flipped);
int same_xyorder_sweep_dev(same_ctx *ctx, const double *daxy, int64_t n_m, const double *drxy,
                           const int32_t *dtris, int64_t Tr, const int32_t *dmatch,
                           uint8_t *dedge_flags, uint8_t *dtri_flag, uint8_t *dpoint_flag,
                           uint64_t *dcounts);
int same_orient_sweep_dev(same_sweep *sweep, const int32_t *dmatch, int64_t *out_checked,
                          int32_t *out_viol_idx, int64_t *out_nviol);
/* Triangle-block forms for the sweep sharded over GPUs (the loops being sharded are
 * src/same.py:645-669 and src/violationhelper.py:53-117).  same_orient_flags_dev writes the flags of
 * triangles [t_begin, t_end) at their absolute positions dflag[t] (any block boundaries) and only
 * enqueues; after the blocks of all ranks have been all-gathered into one flag array,
 * same_orient_from_flags_dev produces what same_orient_sweep produces: checked count and the ascending
 * list of flipped triangles (src/same.py:687-703 relies on that order).  The XY-order and area sweeps
 * shard by calling their _dev forms on offset pointers (dtris + 3*t_begin, outputs + t_begin). */
int same_orient_flags_dev(same_sweep *sweep, const int32_t *dmatch, int64_t t_begin, int64_t t_end,
                          uint8_t *dflag);
int same_orient_from_flags_dev(same_sweep *sweep, const uint8_t *dflag, int64_t *out_checked,
                               int32_t *out_viol_idx, int64_t *out_nviol);
/* dmatch[i] = didx[i*k]: the nearest candidate of every row of a padded candidate list (-1 = none). */
int same_first_candidate_dev(same_ctx *ctx, const int32_t *didx, int64_t rows, int k, int32_t *dmatch);

/* ======================================================================================================================
 * part 3 -- WINDOW path: both sections resident on the device, a batch of windows = two calls
 * ====================================================================================================================== */
/* ---- a13 + the per-window pre-MIP path with the sections resident on the device -------------
 * The reference's window loop (src/same.py:507-593) subsets both frames per window (:293-295: one boolean mask over the
 * whole frame per window) and runs the whole pre-MIP path on the subset.  Here:
 *   same_section      one section's columns uploaded once (XY, the commonCT type columns, cell sizes; cost_f32 != 0 keeps the
 *                     cost operands as float, BASELINE cfg 5), its rows binned ONCE into a grid of cells (rows sorted by cell,
 *                     ascending inside a cell).  same_section_bin(section, x0, y0, cell_w, cell_h) re-bins it on the caller's
 *                     grid: with the window grid's origin (int(x_min), int(y_min)) and cell = gcd(window step, window size)
 *                     every window box of src/same.py:481-488 / :527-542 is a union of cells and its rows need no test at all;
 *                     other boxes test the rows of the cells they cut.  A box covering more than 64 cells falls back to one
 *                     mask over the section.  It waits for stage calls in flight on the section and for the device before it replaces the
 *                     grid (a lock per section); still, re-bin between passes, not between the two calls of a window.  Sections
 *                     may be shared by the windows of several contexts of one device.
 *   same_window       the device state of one window in flight (buffers grow on demand and are reused).  It reads the two sections it was
 *                     staged on until its finish call returns: destroy windows (or stage them elsewhere) before their sections.
 *   same_window_stage: for each of n_windows windows (window i takes boxes[4 i .. 4 i + 3] = {x0,x1,y0,y1}, half-open): the rows of both
 *     sections inside the box (ascending row order), radius / k prune (src/utils.py:709-728), candidate costs (src/same.py:1180-1189),
 *     compaction of the aligned cells that have candidates and of the pair list (src/utils.py:734-742).  out_counts[4 i ..] = {aligned
 *     rows in the box, reference rows in the box, aligned rows kept, pairs}.  Reference cells are not renumbered: pair[1] / match index
 *     the window's reference rows.  Every kernel takes up to EIGHT windows per launch (blockIdx.y = window, their arguments by value):
 *     per group of eight one zeroing launch, at most five kernels and one launch that writes what comes back into the windows' pinned
 *     blocks, reading O(rows of the covered cells); ONE wait for the whole batch.  The windows of a batch belong to one context and
 *     are distinct; n_windows <= SAME_WINDOW_BATCH_MAX.  If any window is refused nothing of the batch counts.
 *   same_window_filter_finish: for each window of the batch, the Delaunay simplices of its kept aligned cells, from `source`:
 *     SAME_TRIS_SIMPLICES the caller's host array (window i: simplices[3 simplex_offsets[i] .. 3 simplex_offsets[i+1]), offsets[0] = 0);
 *     SAME_TRIS_KEPT the same array holding the KEPT triangles in the reference's order (a caller's own triangulation; the knife-edge
 *     fallback below): no filter, the filter arguments are ignored; SAME_TRIS_DEVICE the candidates same_window_delaunay left on the
 *     device for each window (every window must have been answered by it since it was staged): no host array, no upload -- the classes,
 *     the keep list and the same-type re-add are decided by the filter's own kernels, with the reference's arithmetic, and out_counts'
 *     near and ORDER TIES mean what they mean there; SAME_TRIS_CALLER the triangles same_window_caller_tris left (below).  NULL simplices and simplex_offsets go with SAME_TRIS_DEVICE and only with it ->
 *     - filter_triangles_by_radius on the device (src/helpers.py:233-395: classes :300-330, the keep list, the same-type triangles
 *       added back so that every node keeps one :331-340 / :365-389, in the reference's order); the section's type_id codes play
 *       aligned_df["cell_type"].  Simplices must be distinct as vertex rows (Qhull's are): the re-add pass de-duplicates by triangle,
 *       the reference by vertex row;
 *     - source signs / weights (src/same.py:1128-1146); the incumbent: SAME_INCUMBENT_GREEDY the greedy MIP start with prefer = rowmin
 *       < no_match_penalty * size (src/init_helpers.py:104-133), SAME_INCUMBENT_ASSIGNMENT the optimal assignment (same_sparse_assign
 *       below; no_match cost = no_match_penalty * size, the fp64 product of the greedy rule);
 *     - refine_rounds_cap > 0: the local search on the lazy model's objective from the incumbent (same_refine_matching below), at most
 *       that many rounds, with delaunay_penalty (finite, >= 0); the matched rows, flags and sweeps then describe the search's result,
 *       the assignment's words keep describing the assignment.  0: no search;
 *     - lazy-constraint body (src/same.py:645-669), XY-order sweep (src/violationhelper.py:53-117), area flips (src/same.py:1362-1402).
 *     A bad source, mode, cap or penalty is SAME_EINVAL before any device work.
 *     Outputs are laid end to end in window order: out_match_row / out_point_flag hold kept[0] + kept[1] + ... entries (kept = the
 *     stage call's out_counts[4 i + 2]); out_match_row = SECTION row of the matched reference cell or -1; out_point_flag = per-cell
 *     flag byte: bit 0 the XY-order sweep flags the cell (src/violationhelper.py:100-104), bit 1 the cell is a vertex of a triangle
 *     whose signed area flips (src/same.py:1464-1469); out_stats[SAME_WINDOW_STATS i ..] = {orientation checked, flipped, XY
 *     comparisons, XY violations, triangles with a violation, area flips, greedy rounds (assignment: its searches), matched cells; the
 *     assignment's flags (!= 0: not certified, the matching must not be used) and objective; the search's productive rounds, moves
 *     applied, settled (1: a round found no improving move; 0: stopped at the cap), objective of its start and of its result}, the
 *     objectives as the bits of a double, the words of a mode that is off 0; out_counts[4 i ..] = {kept, added back, cosines within
 *     near_tol of cos_thr, order ties} (SAME_TRIS_KEPT: {n, 0, 0, order ties}).  When a window's third count is not zero
 *     nothing of that window counts (its slices of the outputs mean nothing, no triangles are left on the device): the caller
 *     re-decides its triangles with the reference's literal arccos (same_amd/triangles.py) and calls again for that window with
 *     SAME_TRIS_KEPT.  ORDER TIES (ABI 8) count the places where the reference's answer depends on the order in which the
 *     triangulation lists its triangles or their corners, beyond which triangles there are: an edge of the XY-order sweep whose
 *     ends share an x or a y (`<` is not symmetric, src/violationhelper.py:68-75), a signed area or orientation within rounding of
 *     zero (src/same.py:1401, :658), two same-type triangles of one node whose perimeters agree to the rounding of a three-term
 *     sum (src/helpers.py:334-340 keeps the first).  With Qhull's own simplices the count is of no consequence; a caller that
 *     triangulates otherwise (same_delaunay2d: same triangles, another order) asks Qhull for a window whose count is not zero.  The call's
 *     simplices go up in ONE copy; per group of eight windows one zeroing launch, 14 kernels (17 with fp64 costs) and one launch
 *     that writes the answers into the pinned blocks; ONE wait for the batch (more greedy rounds, in batches with a wait each, only
 *     for a window in which a pair could still be taken after the rounds enqueued up front; the search, when it still moves after its
 *     first rounds, in growing chunks with a wait each).
 *   same_window_refinish: a finished window's tail again (matched rows, the three sweeps, stats) under the caller's match_pair[n kept]
 *     (pair index per kept cell, -1 = none), the search from it when refine_rounds_cap > 0: how the caller replaces a flagged window's
 *     assignment.  It reads the window's staged arrays and kept triangles, no earlier call's options.  out_stats[SAME_WINDOW_STATS] as
 *     above (greedy rounds and the assignment's words 0).  One wait unless the search still moves.
 * same_window_fetch copies one array of the window's state to the host; bytes must be the array's exact size.
 * (Since ABI 6 same_window_stage / same_window_filter_finish take batches; same_window_filter and same_window_finish of ABI 5 are gone --
 * the former is the latter's first half, the latter is prefiltered = 1.  Since ABI 9 the finish call takes its source, incumbent and
 * search as arguments and answers with their records in the wider stats; gone with ABI 8, replaced by the source, the arguments and the
 * stats words: same_window_filter_finish_device, same_window_set_incumbent / _incumbent_result / _set_refine / _refine_result.) */
#define SAME_WINDOW_BATCH_MAX 64
typedef struct same_section same_section;
typedef struct same_window same_window;
enum {
    SAME_WINDOW_ALIGNED_XY = 0,   /* double[kept][2]: XY of the kept aligned cells (the Delaunay input)            */
    SAME_WINDOW_ALIGNED_ROWS = 1, /* int32[kept]: their section rows                                               */
    SAME_WINDOW_ROWS_M = 2,       /* int32[aligned rows in the box]                                                */
    SAME_WINDOW_ROWS_R = 3,       /* int32[reference rows in the box]                                              */
    SAME_WINDOW_PAIRS = 4,        /* int32[pairs][2]: (kept aligned index, reference index in the window)         */
    SAME_WINDOW_COSTS = 5,        /* double[pairs] (float costs widened)                                           */
    SAME_WINDOW_KEPT = 6,         /* int32[kept]: index of each kept aligned cell among the box's aligned rows     */
    SAME_WINDOW_SIGNS = 7,        /* int8[triangles]   (after same_window_filter_finish)                            */
    SAME_WINDOW_WEIGHTS = 8,      /* double[triangles] (after same_window_filter_finish)                            */
    SAME_WINDOW_MATCH = 9,        /* int32[kept]: matched reference index in the window or -1 (after finish)       */
    SAME_WINDOW_TRIANGLES = 10,   /* int32[triangles][3]: the kept triangles (after ..._filter_finish)           */
    SAME_WINDOW_CALLER_TRIANGLES = 11, /* int32[selected][3]: the caller's triangles of the window over its kept cells AS STAGED,
                                          in the caller's order (after same_window_caller_tris)                                  */
    SAME_WINDOW_STAGED_PAIRS = 12 /* int32[pairs as staged][2]: SAME_WINDOW_PAIRS before same_window_priority_pairs filtered the list
                                     and same_window_caller_tris removed cells                                                  */
};
int same_section_create(same_ctx *ctx, const double *xy, const double *types, int T, const double *size,
                        const int32_t *type_id /* may be NULL */, int64_t n, int cost_f32, same_section **out);
int same_section_bin(same_section *section, double x0, double y0, double cell_w, double cell_h);
void same_section_destroy(same_section *section);
int same_window_create(same_ctx *ctx, same_window **out);
void same_window_destroy(same_window *window);
int same_window_stage(same_window *const *windows, int n_windows, const same_section *moving, const same_section *ref,
                      const double *boxes, double radius, int k, double dist_ct_coeff, int64_t *out_counts);
int same_window_fetch(same_window *window, int what, void *out, int64_t bytes);
#define SAME_TRIS_SIMPLICES 0   /* host simplices, filtered on the device */
#define SAME_TRIS_KEPT 1        /* host kept triangles in the reference's order */
#define SAME_TRIS_DEVICE 2      /* the candidates same_window_delaunay left; simplices and simplex_offsets must be NULL */
#define SAME_TRIS_CALLER 3      /* the triangles same_window_caller_tris left (a caller's own triangulation); NULL arrays as above */
#define SAME_INCUMBENT_GREEDY 0
#define SAME_INCUMBENT_ASSIGNMENT 1
#define SAME_WINDOW_STATS 15    /* int64 words per window in out_stats */
int same_window_filter_finish(same_window *const *windows, int n_windows, int source, const int32_t *simplices,
                              const int64_t *simplex_offsets, double radius, int angle_enabled, double cos_thr, double near_tol,
                              int ignore_same_type, int ensure_min_triangle_per_node, double no_match_penalty,
                              int incumbent /* SAME_INCUMBENT_* */, int64_t refine_rounds_cap /* 0 = no search */, double delaunay_penalty,
                              int32_t *out_match_row, uint8_t *out_point_flag, int64_t *out_stats, int64_t *out_counts);
int same_window_refinish(same_window *window, const int32_t *match_pair, double no_match_penalty, int64_t refine_rounds_cap,
                         double delaunay_penalty, int32_t *out_match_row, uint8_t *out_point_flag, int64_t *out_stats);
/* The same two calls with the model's reference capacities in the search (csrc/refine.hip): reference j of a window may take up to
 * limit_j of its kept cells, each match after the first priced penalty_coeff (src/helpers.py:102-161, src/same.py:1191-1196).  limit_j
 * = max_matches * M when the window's frame of the references its pairs name holds a cell of size > 1 and j's size is > 1, else
 * max_matches; M = multiplier, or int(the frame's largest size) when multiplier is 0 (None); at most 1001 (p_j <= 1000).  The sizes are
 * the reference section's.  capacity NULL, or refine_rounds_cap 0: exactly the calls above.  out_stats holds SAME_WINDOW_STATS_CAP words
 * per window: the 15 above, then sum_j max(0, count_j - 1) of the search's result.  max_matches >= 1, multiplier >= 0, penalty_coeff
 * finite and >= 0, else SAME_EINVAL before any device work.  With every limit 1 the search is hip_refine="local" bit for bit. */
typedef struct same_window_capacity {
    int64_t max_matches;
    int64_t multiplier;       /* 0 = None */
    double penalty_coeff;
} same_window_capacity;
#define SAME_WINDOW_STATS_CAP 16
/* SAME_INCUMBENT_TRANSPORT (same_window_filter_finish_cap only; `capacity` must not be NULL, with or without a search): the incumbent is
 * the optimum of the model without its triangle term WITHIN those capacities (same_sparse_assign_cap below) -- the limits are worked
 * out on the device before the start, by the kernel the search uses.  out_stats then holds SAME_WINDOW_STATS_TRANSPORT words per window:
 * the 16 above (greedy rounds = the start's searches, the assignment's flags and objective = the transport's), then sum_j max(0,
 * count_j - 1) of the START.  A flagged window's matching is replaced through same_window_refinish_cap like an assignment's. */
#define SAME_INCUMBENT_TRANSPORT 2
#define SAME_WINDOW_STATS_TRANSPORT 17
int same_window_filter_finish_cap(same_window *const *windows, int n_windows, int source, const int32_t *simplices,
                                  const int64_t *simplex_offsets, double radius, int angle_enabled, double cos_thr, double near_tol,
                                  int ignore_same_type, int ensure_min_triangle_per_node, double no_match_penalty, int incumbent,
                                  int64_t refine_rounds_cap, double delaunay_penalty, const same_window_capacity *capacity,
                                  int32_t *out_match_row, uint8_t *out_point_flag, int64_t *out_stats, int64_t *out_counts);
int same_window_refinish_cap(same_window *window, const int32_t *match_pair, double no_match_penalty, int64_t refine_rounds_cap,
                             double delaunay_penalty, const same_window_capacity *capacity, int32_t *out_match_row,
                             uint8_t *out_point_flag, int64_t *out_stats);

/* ---- a caller's own triangulation on the window path (csrc/window_caller.hip): src/same.py:425-435, :1016-1085 with the frames
 * resident.  The reference remaps the caller's vertex ids to every window's rows, drops the triangles with a missing vertex, filters
 * with remove_unconstrained_nodes=True, deletes the unconstrained nodes (no triangle of theirs passes the side and angle tests,
 * src/helpers.py:323-325, :357-358) with their pairs and renumbers the rest.
 *   same_caller_tris_create: the triangulation of `moving` as section ROWS, int32[n_tris][3] in the caller's order, uploaded once and
 *     binned by the section's grid cell of each triangle's first corner (bin the section on the window grid first: the object is bound
 *     to the grid the section has now).  Every row must lie in [0, rows of the section) -> else SAME_ERANGE before any device work.
 *     Read-only afterwards: every context of the device may use it.  Destroy it before the section.
 *   same_window_caller_tris: for each staged window of the batch (ONE wait): the triangles whose three rows are among the window's kept
 *     aligned cells, as indices into them, in the caller's order and corner order (SAME_WINDOW_CALLER_TRIANGLES) -- only the triangles
 *     binned in the cells the window's box covers are looked at; the node mask of the filter (radius, angle_enabled, cos_thr, near_tol,
 *     ignore_same_type as for same_window_filter_finish); then the window WITHOUT its unconstrained nodes: kept rows, XY, sizes, kept
 *     index, pairs and costs compacted, pair rows and triangle corners renumbered, triangles that name a removed node dropped (none of
 *     them could be kept).  Every same_window_fetch array and count of the window is the smaller window's from then on
 *     (SAME_WINDOW_STAGED_PAIRS: the pair list as staged); the reference side is NOT compacted again, and the reference limits of the
 *     _cap calls are still read over the references the STAGED pair list names.  same_window_filter_finish follows with SAME_TRIS_CALLER.
 *     out_counts[6 i ..] = {triangles selected, nodes removed, cosines within near_tol of cos_thr, kept cells left, pairs left,
 *     triangles left}.  A window whose third count is not zero is left AS STAGED (kept cells and pairs: the staged numbers): the caller
 *     filters its selected triangles on the host and calls again with removed != NULL -- the PREFILTERED form: removed[removed_offsets[i]
 *     .. removed_offsets[i + 1]) holds one byte per kept cell as staged of window i, non-zero = unconstrained; no classification, the
 *     third count is 0 -- and finishes with SAME_TRIS_KEPT and its own kept list (renumbered).  removed NULL <=> removed_offsets NULL.
 *     A window without kept cells, or a triangulation without triangles, launches nothing over an empty grid.  SAME_EINVAL: a window
 *     not staged, not staged over the triangulation's section, or staged before the section was binned again; bad offsets.
 *   same_window_caller_pairs: the pair half of the second compaction again, for a sweep over knn.  Which rows a window keeps, which of the
 *     caller's triangles are its own, the node mask and the renumbering do not depend on k; only the pair list behind the mask does.
 *     After same_window_knn_prefix on a window same_window_caller_tris compacted (below: the window is as staged at the smaller k and
 *     HOLDS the selection) -- and same_window_priority_pairs where the job prunes -- this call, for each window of the batch that holds
 *     a selection (ONE wait; none when nothing is launched), pushes the window's current pair list through the held mask: pairs of
 *     removed rows go, pair rows are renumbered, reference numbers, reference section rows and costs are copied bit for bit; the aligned
 *     side and the triangles are NOT recomputed.  The window is from then on, array for array and count for count, the one
 *     same_window_stage at that k [+ same_window_priority_pairs] + same_window_caller_tris leaves: every same_window_fetch array, the
 *     frame of the _cap calls' reference limits (the list as staged at that k), SAME_WINDOW_CALLER_TRIANGLES; same_window_filter_finish
 *     follows with SAME_TRIS_CALLER, or -- a window whose mask the host made (the prefiltered form) -- with SAME_TRIS_KEPT and the host's
 *     kept list, as after same_window_caller_tris.  out_counts[6 i ..] as same_window_caller_tris reports them (the third is 0).  A
 *     window without kept cells holds nothing and is passed over (its counts are 0).  SAME_EINVAL before anything changes, and for the
 *     whole batch: a window with kept cells that holds no selection (never given same_window_caller_tris, left as staged by it, or not
 *     cut by same_window_knn_prefix since), a window not staged, a window filtered or finished since its last prefix.  A batch that
 *     fails later leaves its windows unstaged, as same_window_knn_prefix does. */
typedef struct same_caller_tris same_caller_tris;
int same_caller_tris_create(same_ctx *ctx, const same_section *moving, const int32_t *tris, int64_t n_tris, same_caller_tris **out);
void same_caller_tris_destroy(same_caller_tris *tris);
int same_window_caller_tris(same_window *const *windows, int n_windows, const same_caller_tris *tris, const uint8_t *removed,
                            const int64_t *removed_offsets, double radius, int angle_enabled, double cos_thr, double near_tol,
                            int ignore_same_type, int64_t *out_counts);
int same_window_caller_pairs(same_window *const *windows, int n_windows, int64_t *out_counts);

/* ---- the cell-type-priority prune on the window path (csrc/window_priority.hip): src/knn_utils.py:28-78, switched by
 * optim_params["ignore_knn_if_matched"] at src/same.py:974-976, with the frames resident.  The reference re-sorts every aligned row's
 * pruned list by distance (stable) and walks the rows in ascending order: a row whose nearest reference has its cell type and has not been
 * claimed by an earlier row keeps that one pair and claims the reference; every other row keeps all its pairs.  Closed form: among the
 * rows whose nearest reference j carries their label, the lowest row gets j.
 *   same_section_set_label_codes: codes[row] of the section's cell type LABELS, int32[rows], made JOINTLY over the two sections of a job so
 *     that equal non-negative codes <=> labels that compare equal (a label that equals nothing -- NaN -- gets a negative code).  A slot of
 *     its own: same_section_set_codes (the window merge's id codes) is not touched.  Set it before the first same_window_priority_pairs call
 *     over the section; setting it again waits for the device.  codes NULL only for a section without rows.
 *   same_window_priority_pairs: for each staged window of the batch (ONE wait): d = sqrt(dx*dx + dy*dy) of every pair in fp64, each
 *     operation rounded to nearest; the pair's stable rank in its row (#{q of the row: d_q < d_p, or d_q == d_p and q earlier}); rows whose
 *     rank-0 reference has their label code bid for it, the lowest row wins; a winner keeps its nearest pair, every other row all its
 *     pairs in rank order; pairs, their reference rows and costs are compacted into a second set of arrays.  SAME_WINDOW_PAIRS,
 *     SAME_WINDOW_COSTS and the pair count are the filtered list's from then on; the kept aligned cells do not change (every one keeps a
 *     pair), the reference side is NOT compacted again (src/knn_utils.py:78), SAME_WINDOW_STAGED_PAIRS stays the list as staged and the
 *     reference limits of the _cap calls are still read over the references IT names -- also after a same_window_caller_tris that follows.
 *     Call it right after same_window_stage, before same_window_delaunay / same_window_caller_tris / same_window_filter_finish.
 *     out_counts[4 i ..] = {pairs staged, pairs left, rows that kept one pair, rows that kept all}.  A window without pairs launches
 *     nothing over an empty grid (its counts are 0).  SAME_EINVAL before any device work: a window not staged, staged over sections
 *     without label codes, staged before a section was binned again, or already filtered (by this call, same_window_caller_tris or
 *     same_window_filter_finish). */
int same_section_set_label_codes(same_section *section, const int32_t *codes);
int same_window_priority_pairs(same_window *const *windows, int n_windows, int64_t *out_counts);

/* ---- a staged window at a smaller k (csrc/window_knn_prefix.hip): what a parameter sweep over `knn` needs instead of a stage call per
 * value.  The prune keeps an aligned row when any reference lies within the radius and orders a row's pairs by (squared distance,
 * reference row) ascending, so the list a stage call at k <= k_staged leaves is, row by row, the first min(k, count) pairs of the list
 * staged at k_staged: same kept aligned cells, same reference rows in the box, same costs.
 *   same_window_knn_prefix: for each staged window of the batch (ONE wait; none when nothing is launched): every kept aligned row keeps
 *     its first min(k, count) pairs, the pair offsets are rebuilt by an ordered scan, pairs, their reference rows and costs are COPIED
 *     (a fetched cost is the staged cost of the same pair, bit for bit) into a second set of arrays, and the window is from then on the
 *     one same_window_stage(..., k, ...) leaves: SAME_WINDOW_PAIRS, SAME_WINDOW_COSTS, SAME_WINDOW_STAGED_PAIRS, the pair count and the
 *     frame of the _cap calls' reference limits are the shorter list's.  The aligned side (SAME_WINDOW_ALIGNED_*, SAME_WINDOW_KEPT,
 *     SAME_WINDOW_ROWS_*) does not change, so what same_window_delaunay left for the window stays valid.  The list as staged stays where
 *     the stage call put it: every call derives from IT, so values of k may come in any order, and k == k_staged turns the window back
 *     to it without a launch.  same_window_priority_pairs and both finish calls run on the window as after a stage call; an earlier
 *     priority prune or finish of the window no longer holds.  out_counts[4 i ..] as same_window_stage reports them.  A window without
 *     pairs launches nothing.  A window same_window_caller_tris has compacted (either form of that call) is turned back to the arrays
 *     of its stage call first -- the aligned side as staged, the staged counts, XY and rows -- and cut like any other: it is the window
 *     a stage call at k leaves, and it HOLDS the caller's selection (node mask, renumbering, compacted aligned side, renumbered
 *     triangles) for same_window_caller_pairs (above); same_window_priority_pairs may come between the two.  A same_window_caller_tris
 *     call on such a window works from the cut list and replaces what is held; a stage call drops it.  SAME_EINVAL before anything
 *     changes: k < 1, k above the k a window was staged at, a window not staged. */
int same_window_knn_prefix(same_window *const *windows, int n_windows, int k, int64_t *out_counts);

/* ---- staged windows priced again from another type matrix of the moving section (csrc/window_recost.hip): what a study over VARIANTS
 * of the moving frame's type columns needs instead of a stage call (and a triangulation) per variant.  Rows, prune, compaction,
 * reference numbers, triangle filter and priority prune do not read the type columns; the pair costs do.
 *   same_types_layer: a resident copy of one (n, T) double matrix for the rows of an existing section -- and, in a float section, its
 *     float copy, made once as same_section_create makes the section's own.  Created from a host pointer (row-major, the section's n and
 *     T), destroyed on its own; it must not outlive its section.  Read-only: the contexts of its device share it.  Where a call takes a
 *     layer, NULL means the section's own types.
 *   same_window_recost: for each staged window of the batch (ONE wait; none when no window has pairs or was compacted): the costs of
 *     the pair list AS STAGED are written again -- moving rows from `layer`, reference rows from `ref`, the stage call's expression in
 *     the stage call's order, bit for bit what same_window_stage computes for a moving section created with the layer's matrix -- and
 *     the window is from then on what same_window_knn_prefix at the staged k leaves: the staged list current, an earlier prefix,
 *     priority prune or finish no longer holding, a caller's compaction turned back and HELD for same_window_caller_pairs.
 *     `moving` / `ref` are the sections the windows were staged from, dist_ct_coeff the weight of the stage call's cost.
 *     out_counts[4 i ..] as same_window_stage reports them.  SAME_EINVAL before anything changes: a window not staged or staged from
 *     other sections, a layer of another section. */
typedef struct same_types_layer same_types_layer;
int same_types_layer_create(same_ctx *ctx, const same_section *section, const double *types, same_types_layer **out);
void same_types_layer_destroy(same_types_layer *layer);
int same_window_recost(same_window *const *windows, int n_windows, const same_section *moving, const same_section *ref,
                       const same_types_layer *layer /* may be NULL */, double dist_ct_coeff, int64_t *out_counts);

/* ---- a6 on the window path without the library call --------------------------------------------------------------------------
 * The reference triangulates every window's kept aligned cells with scipy.spatial.Delaunay (Qhull; src/same.py:1023), on the host
 * -- three quarters of a cfg 5 pass.  same_delaunay2d is this library's own triangulator (HOST code, no device, no context, safe to
 * call from many threads at once): a sweep-hull construction with edge flips, every sign it relies on clear of its rounding bound by
 * three orders of magnitude.  It ANSWERS only when the answer is beyond doubt the set of triangles Qhull gives: after the
 * construction every interior edge and hull corner is measured the way Qhull sees it (distance of the fourth point from the lifted
 * triangle's plane in 'Qbb'-scaled paraboloid coordinates, against Qhull's round-off allowance for these coordinates), and when the
 * smallest of these ratios (*out_margin) is not above `guard`, or a sign was in doubt on the way (duplicate, collinear, cocircular
 * points), the return is SAME_EUNSURE and the caller asks Qhull as the reference does.  Measured against scipy 1.15.3 on 6 000 sets
 * (uniform, blobs, clusters, strips; offsets to 3e8): Qhull's triangles differ from the exact Delaunay triangulation only where the
 * margin is below 0.3 (tools/delaunay_margin.py, profiles/r06_delaunay_margin.md: 6 000 sets); same_amd uses guard = 16 (60 x that).
 * xy: n points (x, y) interleaved.  out_tris: room for `cap` triangles (2 n - 5 always suffices); *out_n_tris triangles are written,
 * counter-clockwise, in this function's own order (Qhull's order and corner order are its own: see the ORDER TIES of
 * same_window_filter_finish for what that touches).  SAME_OK | SAME_EUNSURE | SAME_EINVAL (NULL, n < 0 or above 3.5e8, cap too small) |
 * SAME_ENOMEM. */
int same_delaunay2d(const double *xy, int64_t n, int32_t *out_tris, int64_t cap, int64_t *out_n_tris, double guard,
                    double *out_margin /* may be NULL */);

/* ---- a6 on the DEVICE for the window path (csrc/delaunay_dev.hip): replaces the scipy.spatial.Delaunay call of src/same.py:1016-1031
 * where the filter of src/helpers.py:298-319 follows.  The filter drops every triangle with a side >= radius or an angle < min_angle and
 * nothing downstream sees a dropped triangle (:321-325, :331-340, :357, :365-389), so only Delaunay triangles that pass a slack screen of
 * it are needed: with points in general position those are exactly the screened triangles whose circumcircle is empty, and their
 * circumradius is at most radius / (2 sin min_angle) -- a map over points that reads a bounded neighbourhood.  Every in-circle sign is
 * measured as Qhull would see it (qhull_margin.h, the formula of same_delaunay2d); the answer is given only when every sign clears `guard`
 * x Qhull's allowance and the hull is clear of collinear runs, so an answer is the SET of kept-candidate triangles Qhull's triangulation
 * holds.  The candidates come counter-clockwise in this library's order (by owner = smallest vertex, then the other two ascending).
 *   same_window_delaunay: for each staged window of the batch (up to eight per launch, nine launches per group, ONE wait for the batch),
 *     the candidates over its kept aligned cells (SAME_WINDOW_ALIGNED_XY), left on the device.  out_status[i] = 0 (answered; out_n_tris[i]
 *     candidates) or a mask of SAME_DD_* reasons (refused: the caller asks Qhull, as the reference does).  A window's candidates stay valid
 *     until it is staged again; same_window_filter_finish takes them as SAME_TRIS_DEVICE (a caller re-finishes a window whose ORDER TIES
 *     count is not zero with Qhull's simplices).  cos_thr / angle_enabled as for same_window_filter_finish.
 *   same_delaunay_filtered: the same triangulation for a caller's host array of n points (xy interleaved): *out_status as above;
 *     answered: *out_n_tris triangles in out_tris (room for `cap`; 2 n always suffices).  SAME_EINVAL if cap is too small. */
#define SAME_DD_FEW_POINTS 1   /* fewer than 3 points */
#define SAME_DD_NO_ANGLE 2     /* no angle threshold (min_angle_deg None or ~0) or no finite radius: no circumradius bound */
#define SAME_DD_NONFINITE 4    /* a coordinate is not finite */
#define SAME_DD_IN_DOUBT 8     /* a sign within guard x Qhull's allowance: duplicates, cocircular quads, collinear runs, hull corners */
#define SAME_DD_OVERFLOW 16    /* a neighbour, candidate, hull or grid list longer than its buffer */
int same_window_delaunay(same_window *const *windows, int n_windows, double radius, int angle_enabled, double cos_thr, double guard,
                         int32_t *out_status, int64_t *out_n_tris);
int same_delaunay_filtered(same_ctx *ctx, const double *xy, int64_t n, double radius, int angle_enabled, double cos_thr, double guard,
                           int32_t *out_tris, int64_t cap, int64_t *out_n_tris, int32_t *out_status);

/* ---- the optimal-assignment incumbent (csrc/assign.hip): the reference's init_method="hungarian" MIP start (src/init_helpers.py:135-175)
 * on its SPARSE form, without the size cap of :136-142.  Rows are the aligned cells, columns the reference cells plus one private
 * no-match column per row; the edges are the pairs at their costs and each row's edge to its own no-match column; every row is
 * assigned at minimum total cost, and a row on its no-match column is unmatched (:163-175).  With every no-match cost below big_m / 2
 * this is the reference's dense big-M problem (same_assign_matrix); the caller checks that and max_matches == 1 (:97-98).  Solved by
 * successive shortest paths with Jonker-Volgenant potentials, one wave per problem, the searches in row order inside the kernel; a
 * certificate kernel checks every reduced cost (>= -delta, delta an fp64 rounding bound) and v = 0 on free reference columns.  The
 * answer depends on the input alone.  A problem the certificate refuses (or that needs more steps than a cap) is FLAGGED: its caller
 * solves it elsewhere.
 *   same_sparse_assign: host buffers.  pairs[P][2] = (row < n_m, column < n_r), each (row, column) at most once; unmatched[n_m] the
 *     no-match costs.  out_match_pair[i] = index of row i's pair, -1 = unmatched.  out_stats[4] = {searches, columns finalized, flags
 *     (!= 0: not certified, the matching must not be used), objective as the bits of a double}.  One wait.
 *   On the window path: same_window_filter_finish with SAME_INCUMBENT_ASSIGNMENT; same_window_refinish replaces a flagged window's. */
int same_sparse_assign(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched, int64_t n_m,
                       int64_t n_r, int32_t *out_match_pair, int64_t *out_stats);
/*   same_sparse_assign_cap: the TRANSPORT form -- the model without its triangle term (src/same.py:1191-1196 with delaunay_penalty 0):
 *     every row takes one of its pairs or its no-match column, reference j at most ref_limit[j] (1 .. 1001) rows, each after its first
 *     priced penalty_coeff (finite, >= 0): minimum of pair costs + no-match costs + penalty_coeff sum_j max(0, count_j - 1).  The
 *     surcharge is convex, so reference j splits exactly into a slot column (capacity 1, cost c_ij) and a shared column behind the
 *     no-match columns (capacity ref_limit[j] - 1, cost c_ij + penalty_coeff); the same searches, a column a sink while it has room, a
 *     full column relaxing each of its holders; the certificate also checks the holder lists, count <= capacity, v = 0 on columns with
 *     room and both tiers' reduced costs.  Its value is a lower bound on the full lazy model's optimum.  out_stats[5] = the four words
 *     above, then sum_j max(0, count_j - 1).  With every limit 1: same_sparse_assign's match, searches and objective bit for bit.  Bad
 *     limits or penalty_coeff: SAME_EINVAL before any device work.
 *   On the window path: same_window_filter_finish_cap with SAME_INCUMBENT_TRANSPORT. */
int same_sparse_assign_cap(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched, int64_t n_m,
                           int64_t n_r, const int32_t *ref_limit, double penalty_coeff, int32_t *out_match_pair, int64_t *out_stats);

/* ---- the local search on the lazy model's objective (csrc/refine.hip): from a window's one-to-one incumbent, moves that lower
 *   sum_p c_p x_p + no_match_penalty sum_i size_i n_i + delaunay_penalty sum_t w_t q_t        (src/same.py:1191-1196; p_j = 0;
 *   the _cap entry points below add penalty_coeff sum_j p_j with the model's reference capacities)
 * over the window's kept aligned cells, their pairs and the kept triangles; w_t = the corners' size sum (:1128-1134), q_t = 1 when the
 * lazy body (:645-669) sees t flip.  Moves: a matched cell to a free candidate reference, an unmatched cell to a free candidate, a cell to
 * unmatched, two matched cells swapping references (both crossed pairs candidates).  Rounds: every cell proposes its best improving
 * move (delta < -2^-40 scale); moves whose footprints (closed 1-rings of the moved cells + the references taken) do not meet apply
 * together, by a minimum key; a round without a move settles the search.  The result depends on the triangle SET only, not on its order.
 *   On the window path: same_window_filter_finish / same_window_refinish with refine_rounds_cap > 0.
 *   same_refine_matching: host buffers.  pairs[P][2] = (cell < n_m, reference < n_r), each once; unmatched[n_m] the no-match costs;
 *     tris[Tr][3] the kept triangles; axy[n_m][2], ref_xy[n_r][2], size[n_m]; match_pair_inout[n_m] = pair index per cell (-1 = none),
 *     one-to-one, replaced by the result.  out_stats[5] = {rounds, moves, settled, objective at the start, objective (both as the bits
 *     of a double)}.  One wait unless the search still moves after its first chunk of rounds. */
int same_refine_matching(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched, int64_t n_m,
                         int64_t n_r, const int32_t *tris, int64_t Tr, const double *axy, const double *ref_xy, const double *size,
                         double delaunay_penalty, int64_t rounds_cap, int32_t *match_pair_inout, int64_t *out_stats);
/*   same_refine_matching_cap: the same search with reference capacities: ref_limit[n_r] (1 .. 1001) matches per reference, each after
 *     the first priced penalty_coeff (finite, >= 0) -- the objective gains penalty_coeff sum_j max(0, count_j - 1).  Moves go to
 *     references with room (count < limit); a swap partner is a reference's only holder.  match_pair_inout may hold a reference up to
 *     its limit.  out_stats[6] = the five words above, then sum_j max(0, count_j - 1) of the result.  All limits 1 and penalty_coeff
 *     anything: same_refine_matching bit for bit. */
int same_refine_matching_cap(same_ctx *ctx, const int32_t *pairs, const double *costs, int64_t P, const double *unmatched, int64_t n_m,
                             int64_t n_r, const int32_t *tris, int64_t Tr, const double *axy, const double *ref_xy, const double *size,
                             double delaunay_penalty, const int32_t *ref_limit, double penalty_coeff, int64_t rounds_cap,
                             int32_t *match_pair_inout, int64_t *out_stats);

/* ---- f3 on the window path: the window merge where the windows' matches are ------------------------------------------------
 * The reference trims every window's match table to the window's central region (src/same.py:565-582), concatenates the tables and
 * merges them (helpers.merge_window_matches_unique_ref, src/helpers.py:692-815: one row per (aligned, ref) pair -- not violating
 * first, then the smaller window id, then the earlier row --, then one maximum matching of the pairs that are left, rows in the order
 * of the aligned ids).  In a tiled run nearly every pair stands alone (no other row names either of its cells) and is in the merged
 * table as it is.  On the device, per pass over a plan (ABI 7):
 *   same_section_set_codes   codes[row] = rank of the row's cell id among the section's ids, 0 .. n_codes-1 (equal id <=> equal code; the
 *                            merge compares and orders by them); NULL: a row's code is its number (ids ascending by row).
 *   same_merge_acc           the rows of one pass (one per context; grows on demand, reused from pass to pass).
 *   same_merge_acc_begin     a new pass.  expected_rows sizes the arrays up front (an upper bound saves a re-allocation, nothing more).
 *                            Seams, for a plan dealt over ranks (NULL near_start: one rank, no seams): window (plan position) p of this
 *                            rank lies near the central regions near_boxes[4 q .. 4 q + 3] = {x0, x1, y0, y1}, q in [near_start[p],
 *                            near_start[p+1]), of OTHER ranks' windows; a row of p whose aligned cell lies in one of them, or whose
 *                            reference cell lies within `reach` (the prune's radius) of one, may be named by another rank's table too
 *                            and is left to the host.  all_seam != 0: every row is (cell ids that name several rows of a frame).
 *   same_window_collect      after same_window_filter_finish, ENQUEUE ONLY: the matched kept cells of each window whose XY lies in
 *                            trims[4 i .. 4 i + 3] = {x0, x1, y0, y1} (half open) are appended to the accumulator of the windows'
 *                            context, windows in call order, cells ascending: (aligned section row, matched reference section row, flag
 *                            byte, window_ids[i], plan_pos[i], index among the window's kept cells).  Three launches per eight windows.
 *   same_merge_acc_resolve   the pass is over: the accumulators (accs[0] first -- the call runs on its context; the others are waited
 *                            for and laid behind it, in order: plan order when the contexts walked consecutive runs of the plan) ->
 *                            codes, the de-duplication of src/helpers.py:745-753 (merge.hip's kernels, on the device arrays), degrees,
 *                            classes.  out_counts = {rows, rows after the de-duplication, REST rows, rows final already}.  A surviving row
 *                            whose two cells are named by no other surviving row and that is not at a seam is final.  The REST --
 *                            contested or at a seam -- is for the host (same_amd/merge.py: connected components, Hopcroft-Karp, the
 *                            exchange between ranks): same_merge_acc_fetch(accs[0], SAME_MERGE_REST) = one record per row, in the order
 *                            the de-duplication left: int32 {row in the accumulator, aligned code, ref code, window id, plan position,
 *                            index among the window's kept cells}, uint32 flags (bit 0 XY-order flag, bit 1 area-flip flag, bit 2 seam).
 *   same_merge_acc_finish    winner_rows = the REST rows (accumulator row numbers) the host's matching kept -> the merged table's rows
 *                            in the order of the aligned codes (src/helpers.py:799-808), their number in *out_n_final; they stay on the
 *                            device (same_merge_acc_columns reads them there) unless fetched: same_merge_acc_fetch(.., SAME_MERGE_FINAL) =
 *                            int32 {aligned section row, reference section row, index among the window's kept cells, window id, plan
 *                            position}, uint32 flags (bits 0, 1 as above) per row.  The host gathers the columns of exactly these rows.
 *   same_merge_acc_load      rows from the HOST instead of from windows (the seam rows of every rank after their exchange: the common step
 *                            of a merge dealt over ranks, same_amd/merge.py): the accumulator holds exactly these n rows, their "section
 *                            rows" ARE codes (a_code < n_codes_a, r_code < n_codes_r), ties of the de-duplication go to the earlier row;
 *                            same_merge_acc_resolve then takes this one accumulator with NULL sections. */
typedef struct same_merge_acc same_merge_acc;
#define SAME_MERGE_REST 0
#define SAME_MERGE_FINAL 1
#define SAME_MERGE_REST_BYTES 28
#define SAME_MERGE_FINAL_BYTES 24
int same_section_set_codes(same_section *section, const int32_t *codes /* may be NULL */, int64_t n_codes);
int same_merge_acc_create(same_ctx *ctx, same_merge_acc **out);
void same_merge_acc_destroy(same_merge_acc *acc);
int same_merge_acc_begin(same_merge_acc *acc, int64_t expected_rows, int n_pos, const int32_t *near_start /* may be NULL */,
                         const double *near_boxes, double reach, int all_seam);
int same_window_collect(same_window *const *windows, int n_windows, same_merge_acc *acc, const double *trims,
                        const int32_t *window_ids, const int32_t *plan_pos);
int same_merge_acc_load(same_merge_acc *acc, const int32_t *a_code, const int32_t *r_code, const uint8_t *flags, const int32_t *window_ids,
                        const int32_t *pos, const int32_t *cidx, int64_t n, int64_t n_codes_a, int64_t n_codes_r);
int same_merge_acc_resolve(same_merge_acc *const *accs, int n_accs, const same_section *moving /* NULL after ..._load */,
                           const same_section *ref /* NULL after ..._load */, int64_t *out_counts /* [4] */);
int same_merge_acc_finish(same_merge_acc *acc, const int32_t *winner_rows, int64_t n_winners, int64_t *out_n_final);
/* Without the merge: every accumulated row is a final row, in the order the windows were collected (src/same.py:583-590: the window
 * tables concatenated) -- for the same fetch / same_merge_acc_columns calls.  accs as for same_merge_acc_resolve. */
int same_merge_acc_plain(same_merge_acc *const *accs, int n_accs, int64_t *out_n_rows);
int same_merge_acc_fetch(same_merge_acc *acc, int what, void *out, int64_t bytes);
/* The merged table's columns, written by the DEVICE (after same_merge_acc_finish; enqueue only -- same_ctx_sync waits) into out_host,
 * column after column, n_final entries each, in the order of the final rows:
 *   8-byte columns: the moving section's T type columns (src/same.py:1264-1278 copies them from aligned_df), its X and Y, the reference
 *   section's X and Y (ref_X, ref_Y); then n_extra_mov columns gathered by moving row and n_extra_ref columns gathered by reference row
 *   from the caller's DEVICE arrays of 8-byte values (cell ids, sizes: copied as bit patterns, whatever their type; at most 4 each); then
 *   aligned_idx (the cell's index among its window's kept cells), window_id and the window's plan position as int64;
 *   byte columns: triangle_violation (the area-flip flag, src/same.py:1464-1469) and the XY-order flag, 0 / 1.
 * out_host holds (T + 4 + n_extra_mov + n_extra_ref + 3) * 8 * n_final + 2 * n_final bytes and must be host memory the device can write:
 * same_host_alloc (page-locked, hipHostMalloc; same_host_free returns it).  The float columns are the bytes the caller uploaded with
 * same_section_create. */
int same_merge_acc_columns(same_merge_acc *acc, const same_section *moving, const same_section *ref, const void *const *extra_moving,
                           int n_extra_moving, const void *const *extra_ref, int n_extra_ref, void *out_host, int64_t n_final);
/* ... with the moving section's type columns read from a types layer of it (NULL: the section's own -- the call above) */
int same_merge_acc_columns_layer(same_merge_acc *acc, const same_section *moving, const same_types_layer *layer /* may be NULL */,
                                 const same_section *ref, const void *const *extra_moving, int n_extra_moving, const void *const *extra_ref,
                                 int n_extra_ref, void *out_host, int64_t n_final);
int same_host_alloc(same_ctx *ctx, size_t bytes, void **out_ptr);
int same_host_free(same_ctx *ctx, void *ptr);
/* A merged result reduced to the numbers it is read by (csrc/window_score.hip), without its table: after same_merge_acc_finish, on the
 * final rows where they are.  `moving`, `ref`: the sections the pass ran over, both with label codes (same_section_set_label_codes: the
 * joint codes of the frames' cell_type labels; a negative code equals nothing).  `tris`: the triangulation to score against as rows of
 * `moving` (same_caller_tris_create), or NULL: no triangle counts.  out_counts[8]:
 *   [0] final rows                      [1] rows whose moving cell's label code equals its matched reference cell's
 *   [2] triangles resident in `tris`    [3] of them: all three corners matched (src/eval_utils.py:66-223, check_triangle_violations)
 *   [4] of [3]: skipped, the three corners have one label (only with ignore_same_type)
 *   [5] of [3]: flipped -- the signs of _signed_area on the moving XY and on the matched reference cells' XY differ, neither is 0
 *   [6] of [5]: not skipped (the stats' triangles_flipped; percent_flipped is [6] of [3] - [4])
 *   [7] final rows whose moving cell is a corner of a flipped triangle that is not skipped; with node_local: of at least min_flips
 *       such triangles that are at least majority_threshold of the triangles not skipped it is a corner of
 * What the call asks of the runtime for n final rows on the accumulator's context: n == 0 nothing; else one launch, and two more where
 * `tris` holds a triangle; one copy (64 bytes back); ONE wait; no fill -- but the first call on an accumulator, and the first over a
 * moving section of more rows than any before, lay the accumulator's work buffer (three words per moving row) and fill it, two fills.
 * The call leaves that buffer as it found it, so the sets of a sweep follow each other without one.
 * SAME_EINVAL (out_counts untouched): before same_merge_acc_finish, after same_merge_acc_plain or same_merge_acc_load (their rows may
 * name a moving row twice), a section without label codes, `tris` made for another section.  SAME_ERANGE: a final row outside the
 * sections (the pass ran over others). */
int same_merge_acc_score(same_merge_acc *acc, const same_section *moving, const same_section *ref,
                         const same_caller_tris *tris /* may be NULL: no triangle counts */, int ignore_same_type, int node_local,
                         double majority_threshold, int64_t min_flips, int64_t *out_counts /* [8] */);
/* The same result broken down three ways (csrc/window_score_detail.hip): by label pair, by group of the moving rows, by the rank of the
 * moving cell's label among its matched reference cell's type columns -- binned where same_merge_acc_score totals.
 *   same_score_detail_create: what to bin by, uploaded once on `moving`'s context, resident on its device, read-only and shared by the
 *   worker contexts like same_caller_tris; destroy it before its section.  group_of[row] in [0, n_groups) is the moving row's group, a
 *   negative value: the row is in no group; NULL: every row in group 0.  col_of_label[code] is the type column (of the sections' T) the
 *   label with that joint code names, or -1; NULL: no label names a column (as n_labels entries of -1).  Checked on the host before
 *   anything is uploaded: SAME_EINVAL for n_labels < 0 or > SAME_SCORE_MAX_LABELS, n_groups < 1 or > SAME_SCORE_MAX_GROUPS; SAME_ERANGE
 *   for a group_of value >= n_groups or a col_of_label value outside [-1, T).
 *   same_merge_acc_score_detail: arguments as same_merge_acc_score's, and `detail`, made for `moving`.  With L = n_labels, G = n_groups,
 *   R = SAME_SCORE_RANKS, `out` holds out_words >= L*L + 1 + (G+1)*8 + 2*(R+1) + 1 words (SAME_SCORE_DETAIL_WORDS), in this order:
 *     confusion [L*L]   out[cm*L + cr]: final rows whose moving label code is cm and whose matched reference cell's is cr;
 *     unlabelled [1]    the final rows in no cell: a code that is negative or >= L on either side;
 *     groups [(G+1)*8]  bin g < G is group g, bin G is "cross".  A bin's eight words are out_counts[0 .. 7] of same_merge_acc_score
 *                       restricted to the bin: [0] final rows (a row is in its moving row's group; without one, in the cross bin)
 *                       [1] of them, the two label codes agree  [2] triangles resident (a triangle is in group g iff its three corners
 *                       carry g, else in the cross bin)  [3] all corners matched  [4] skipped, same type  [5] flipped  [6] flipped and
 *                       not skipped  [7] final rows whose moving cell is violating under the any-flip / node-local rule -- counted
 *                       over the triangles that are WITHIN a group and not skipped: a node is counted in its own group, the cross
 *                       bin's word stays 0.  Over all bins words [0 .. 6] sum to same_merge_acc_score's counts;
 *     ranks [2*(R+1)]   for final row (a, r): c = col_of_label[code of a], v = ref types[r][c] (the float64 matrix the section was made
 *                       from), strict = #{t != c: types[r][t] > v}, weak = #{t != c: types[r][t] >= v}; first the histogram of
 *                       min(strict, R), then that of min(weak, R);
 *     untyped [1]       the final rows in no rank bin: a moving code that is negative or >= L, c < 0, a NaN in the reference type row.
 * What the call asks of the runtime for n final rows on the accumulator's context: n == 0 and no triangle resident: nothing (out is zeros); else one launch, and two more where `tris` holds a triangle; one copy (the words of `out` and one more); ONE
 * wait; no fill -- but a call that lays the accumulator's score work buffer (same_merge_acc_score: the first, and the first over more
 * moving rows) fills it, two fills, and one that lays the bins' buffer (the first, and the first with more words than any before)
 * fills that, one fill.  The call leaves the score work buffer as it found it and the bins' buffer clear for the next call: score and
 * detail calls alternate on one accumulator without a fill.
 * SAME_EINVAL / SAME_ERANGE as same_merge_acc_score, `out` untouched; SAME_EINVAL also for a `detail` made for another section,
 * sections whose T differ where a label names a column, and out_words too small. */
#define SAME_SCORE_MAX_LABELS 64
#define SAME_SCORE_MAX_GROUPS 256
#define SAME_SCORE_RANKS 16
#define SAME_SCORE_DETAIL_WORDS(L, G) ((int64_t)(L) * (L) + 1 + ((int64_t)(G) + 1) * 8 + 2 * (SAME_SCORE_RANKS + 1) + 1)
typedef struct same_score_detail same_score_detail;
int  same_score_detail_create(const same_section *moving, const int32_t *group_of /* [rows] or NULL: every row in group 0 */, int n_groups,
                              int n_labels, const int32_t *col_of_label /* [n_labels] or NULL: no rank counts */,
                              same_score_detail **out);
void same_score_detail_destroy(same_score_detail *detail);
int  same_merge_acc_score_detail(same_merge_acc *acc, const same_section *moving, const same_section *ref,
                                 const same_caller_tris *tris /* may be NULL */, const same_score_detail *detail,
                                 int ignore_same_type, int node_local, double majority_threshold, int64_t min_flips,
                                 int64_t *out, int64_t out_words);
/* The same result per CELL (csrc/window_score_map.hip): same_merge_acc_score's counts and, per row of the moving section, one 16-byte
 * mark -- what the reference's notebooks plot per cell (in_violating_triangle, correct / incorrect, in the top k, on the ground truth).
 *   The mark of moving row i:
 *     ref_row      the reference section row the final rows put it on, -1: none (a final row outside the sections leaves its moving
 *                  row unmatched, as it leaves the counts);
 *     node_tri     the resident triangles not skipped the row is a corner of; node_flip: the flipped ones of them;
 *     flags        SAME_MARK_MATCHED 1; TYPE_MATCH 2: the two label codes agree (out_counts[1]'s rule); CONSIDERED 4: node_tri > 0;
 *                  VIOLATING 8: the any-flip / node-local rule of out_counts[7]; TRUTH_KNOWN 16: the map holds a truth row >= 0 for
 *                  the row; ON_TRUTH 32: matched and ref_row equals it; RANKED 64: the two rank bytes hold ranks;
 *     rank_strict, rank_weak   same_merge_acc_score_detail's strict and weak of (the row's label's column, the matched reference
 *                  row's type row), saturated at 254; 255 where the row is not ranked: unmatched, the label names no column, a NaN
 *                  in the type row, no `detail` or one without col_of_label.
 *   An unmatched row's mark is {-1, 0, 0, TRUTH_KNOWN or 0, 255, 255, 0}.
 *   same_score_map_create: what the marks are read against and folded into, made on `ctx` for the two sections, resident on its device
 *   and shared by the worker contexts of that device (at most 32 calling contexts); destroy it before its sections.  truth_row[i]
 *   (host, mov->n entries, may be NULL: every row unknown): the reference section row that is moving row i's true or baseline match,
 *   -1 unknown; SAME_EINVAL for a value < -1 or >= the reference section's rows, checked before anything is uploaded.  with_tally:
 *   the map holds tally[mov->n][4] (uint32, zero at first) -- per moving row in how many results folded in so far it was matched,
 *   type-matched, violating, on its truth row -- and every same_merge_acc_score_map call adds its result to it.
 *   same_score_map_tally: the tally copied out (out_tally: mov->n * 4 words, may be NULL; SAME_EINVAL when given for a map without a
 *   tally) and the number of results folded in since the creation or the last reset (out_results, may be NULL).  One copy, one wait.
 *   same_score_map_reset: tally and result count back to zero (one fill, one wait).
 *   same_merge_acc_score_map: arguments as same_merge_acc_score's; `detail` (may be NULL: no ranks) a same_score_detail of `moving`,
 *   of which only col_of_label and n_labels are read; `map` made for these two sections.  out_counts[10]: [0 .. 7] exactly
 *   same_merge_acc_score's for the same arguments, [8] matched rows whose truth is known, [9] of them: on it.  out_marks (may be NULL:
 *   counts and tally only): mov->n marks; any host memory, page-locked memory (same_host_alloc) takes them by DMA.
 * What the call asks of the runtime on the accumulator's context, whatever the number of final rows: the score call's rows launch, its
 * triangles launch where `tris` holds a triangle, one launch over the moving rows -- THREE launches, two without a triangle --; one
 * copy (80 bytes back) and with out_marks a second (the marks, from a device buffer of the map); ONE wait; no fill -- but the call that
 * lays the accumulator's score work buffer (same_merge_acc_score: the first, and the first over more moving rows) fills it, two fills.
 * The totals are counted in the map, two sets per calling context of which each call clears the other's, so the accumulator's score
 * work buffer is left as it was found and its own totals are not touched: map, score and detail calls alternate on one accumulator
 * without a fill.  Sections without a row and an accumulator without a final row: nothing.
 * SAME_EINVAL / SAME_ERANGE as same_merge_acc_score, out_counts untouched; SAME_EINVAL also for a `map` made for other sections or on
 * another device, a `detail` made for another section, sections whose T differ where a label names a column.  After SAME_ERANGE
 * out_marks is undefined and the tally holds the refused result's rows inside the sections: reset it. */
#define SAME_MARK_MATCHED     1
#define SAME_MARK_TYPE_MATCH  2
#define SAME_MARK_CONSIDERED  4
#define SAME_MARK_VIOLATING   8
#define SAME_MARK_TRUTH_KNOWN 16
#define SAME_MARK_ON_TRUTH    32
#define SAME_MARK_RANKED      64
typedef struct { int32_t ref_row; uint32_t node_tri, node_flip; uint8_t flags, rank_strict, rank_weak, reserved; } same_cell_mark;
typedef struct same_score_map same_score_map;
int  same_score_map_create(same_ctx *ctx, const same_section *moving, const same_section *ref,
                           const int32_t *truth_row /* host, [moving rows], -1 unknown; may be NULL */, int with_tally,
                           same_score_map **out);
void same_score_map_destroy(same_score_map *map);
int  same_score_map_tally(same_score_map *map, uint32_t *out_tally /* [moving rows][4], may be NULL */, int64_t *out_results);
int  same_score_map_reset(same_score_map *map);
int  same_merge_acc_score_map(same_merge_acc *acc, const same_section *moving, const same_section *ref,
                              const same_caller_tris *tris /* may be NULL */, const same_score_detail *detail /* may be NULL: no ranks */,
                              same_score_map *map, int ignore_same_type, int node_local, double majority_threshold, int64_t min_flips,
                              same_cell_mark *out_marks /* [moving rows], may be NULL */, int64_t *out_counts /* [10] */);
/* The same result read as FEATURE SUMS (csrc/window_score_feature.hip): the matched pairs put two feature matrices side by side, and the
 * reference's notebooks read them as means -- per group of the moving rows (examples/luad/reproduce_figures.ipynb cells 16-22, the
 * matrixplot by annotation) and per bin of the distance to the nearest pair of a marked zone (cdist(...).min(axis=1), pd.cut).
 *   FIXED-POINT COLUMNS.  A feature column c is quantised once on the host: with m = max |x| over the column and p = frexp(m)'s exponent,
 *   e_c = 30 - p (0 for an all-zero column) and q = rint(ldexp(x, e_c)) as int32, |q| <= 2^30.  The device sums the int32 values in int64:
 *   exact, the same from run to run and under every grid shape.  mean = ldexp((double)sum / n, -e_c); against the true mean it errs by
 *   at most 2^(-e_c-1) + 3 * 2^-53 * |mean|.  A column's step is 2^-e_c, which is 2^-30 of the power of two above its largest
 *   magnitude; a value is rounded by at most half of it, 2^-31 of that power of two.
 *   same_score_features_create: what to sum, uploaded once on `moving`'s context, resident on its device, read-only and shared by the
 *   worker contexts like same_caller_tris; destroy it before its sections.  mov_q[moving rows][F_m], ref_q[ref rows][F_r]: row-major
 *   int32, host memory (NULL where the side has no column or no row).  F = F_m + F_r.  group_of, n_groups: exactly
 *   same_score_detail_create's.  Checked on the host before anything is uploaded: SAME_EINVAL for F_m < 0, F_r < 0, F < 1,
 *   F > SAME_FEATURE_MAX_COLUMNS, a matrix missing where its side has columns and rows, n_groups < 1 or > SAME_SCORE_MAX_GROUPS;
 *   SAME_ERANGE for a |q| > 2^30 or a group_of value >= n_groups.
 *   same_feature_zone_create: the zone and the subset of a distance reading, made on `feats`' context for its sections and resident
 *   like it; destroy it before `feats`.  mov_flags[moving rows], ref_flags[ref rows]: uint8, bit 0 "zone side", bit 1 "subset side";
 *   NULL: every bit set.  A final row (a, r) is a ZONE pair iff mov_flags[a] & ref_flags[r] & 1, a SUBSET pair iff
 *   mov_flags[a] & ref_flags[r] & 2.  d2_edges[n_edges]: thresholds on the SQUARED distance, non-decreasing, +inf allowed; with
 *   B = n_edges - 1, bin b < B holds d2_edges[b] < d2 <= d2_edges[b+1] (pd.cut's right-closed rule).  SAME_EINVAL for n_edges < 2 or
 *   > SAME_FEATURE_MAX_EDGES, a NaN edge, a decreasing pair of edges.
 *   same_merge_acc_score_features: after same_merge_acc_finish, on the final rows where they are.  With G = n_groups, `out` holds
 *   out_words >= SAME_FEATURE_WORDS(G, F, B) int64 words (B = 0 without `zone`), in this order:
 *     counts [4]           final rows; those whose moving row has a group; zone pairs; subset pairs (both 0 without `zone`);
 *     rows [G+1]           final rows per group, bin G: the rows without a group;
 *     sums [(G+1)*F]       per bin, the sum over its final rows (a, r) of mov_q[a][0 .. F_m) and then of ref_q[r][0 .. F_r);
 *     with `zone` also
 *     bin_rows [B+1]       subset pairs per distance bin, bin B: the subset pairs in no bin;
 *     bin_sums [(B+1)*F]   as sums, over the subset pairs.
 *   A pair's position is its reference row's XY.  For a subset pair d2 = min over ALL zone pairs of dx*dx + dy*dy, in fp64 without
 *   contraction (a pair that is both: 0); with no zone pair every d2 is NaN and every subset pair is in bin B.  The minimum does not
 *   depend on the order of the zone pairs.  out_d2 (moving rows doubles, may be NULL): the d2 of the row's subset pair, NaN otherwise.
 * What the call asks of the runtime on the accumulator's context.  Without `zone`: no final row: nothing (out is zeros); else ONE
 * launch, one copy (the words of `out` and one more), ONE wait.  With `zone` and a final row: FOUR launches (the sums by group and
 * the flag kernel; after the first wait the walk and the sums by bin), two copies (32 bytes before the first wait, the words of
 * `out` and one more before the second) and with out_d2 a third, TWO waits; where there is a zone pair the grid of the zone pairs is
 * built between the two waits by knn.hip's build (grid.h: a bounding-box reduction with its 32-byte read-back and a wait, one fill
 * and three launches of its own, which the context's counters do not count).  No fill -- but the call that
 * lays the sums' buffer (the first, and the first with more words than any before) fills it, one fill, and with `zone` the call that
 * lays the zone work buffer (the first, and the first over more final rows or moving rows) fills it, one fill.  The call leaves
 * both clear for the next call and touches no other buffer of the accumulator: score, detail, map and feature calls alternate on
 * one accumulator without a fill.
 * SAME_EINVAL (`out`, out_d2 untouched): what same_merge_acc_score refuses -- before same_merge_acc_finish, after same_merge_acc_plain or
 * same_merge_acc_load, a section without label codes --, `feats` made for other sections or on another device, `zone` made for
 * another `feats`, out_words too small.  SAME_ERANGE (`out`, out_d2 untouched): a final row outside the
 * sections (the pass ran over others); with `zone`, a zone or subset pair whose reference XY is not finite (`out` untouched). */
#define SAME_FEATURE_MAX_COLUMNS 4096
#define SAME_FEATURE_MAX_EDGES 65
#define SAME_FEATURE_WORDS(G, F, B) (4 + ((int64_t)(G) + 1) * (1 + (int64_t)(F)) + ((B) > 0 ? ((int64_t)(B) + 1) * (1 + (int64_t)(F)) : 0))
typedef struct same_score_features same_score_features;
typedef struct same_feature_zone same_feature_zone;
int  same_score_features_create(const same_section *moving, const same_section *ref, const int32_t *mov_q /* host, [moving rows][F_m] */,
                                int F_m, const int32_t *ref_q /* host, [ref rows][F_r] */, int F_r,
                                const int32_t *group_of /* [moving rows] or NULL: every row in group 0 */, int n_groups,
                                same_score_features **out);
void same_score_features_destroy(same_score_features *feats);
int  same_feature_zone_create(const same_score_features *feats, const uint8_t *mov_flags /* [moving rows] or NULL */,
                              const uint8_t *ref_flags /* [ref rows] or NULL */, const double *d2_edges, int n_edges,
                              same_feature_zone **out);
void same_feature_zone_destroy(same_feature_zone *zone);
int  same_merge_acc_score_features(same_merge_acc *acc, const same_section *moving, const same_section *ref,
                                   const same_score_features *feats, const same_feature_zone *zone /* may be NULL */, int64_t *out,
                                   int64_t out_words, double *out_d2 /* [moving rows], may be NULL */);
/* A merged MetaCell result unpacked to cells (csrc/window_unpack.hip; src/metacell_utils.py:564-766, unpack_metacell_matches with
 * metacells on both sides), without its table: after same_merge_acc_finish, on the final rows where they are and in their order.
 *   same_members_create: the members of `section`'s rows as CSR -- row i owns members [off[i], off[i+1]); per member its XY (the
 *   ORIGINAL cell's, float64) and its label code (joint codes of the two original frames' labels; a negative code equals nothing).
 *   Uploaded once on the section's context, resident on its device, read-only and shared by the worker contexts like same_caller_tris;
 *   destroy it before its section.  SAME_EINVAL unless off[0] == 0, off is non-decreasing, off[n_rows] == m < 2^31 and no row has more
 *   than SAME_ASSIGN_MAX_MEMBERS members.
 *   same_merge_acc_unpack: a final row (a, r) with na moving and nr reference members yields na pairs, in the moving row's member order:
 *   member i with reference member i % nr (SAME_UNPACK_DISTRIBUTE; XY is not read), or with the one the optimal assignment of
 *   cdist(moving XY, reference XY) gives it, the reference columns tiled ceil(na / nr) times when na > nr and mapped back by % nr
 *   (SAME_UNPACK_NEAREST) -- solved by the very device function same_batched_assign's kernel runs (csrc/assign_solve.h), so ties
 *   resolve as scipy's linear_sum_assignment resolves them.  A moving row without members yields no pairs.  out_counts[4]:
 *     [0] final rows      [1] pairs (the sum of na)      [2] pairs whose two member codes are equal and non-negative
 *     [3] the largest member count met on either side of a final row
 *   out_ref_member (may be NULL: counts only), `capacity` entries: entry q = the flat index into `ref`'s CSR of the reference member
 *   pair q got; pair q's moving member is off[a] + i, pairs in the order of the final rows.  capacity < [1]: SAME_EINVAL with out_counts
 *   FILLED and out_ref_member untouched -- size the array and ask again.
 * What the call asks of the runtime for n final rows on the accumulator's context: n == 0 nothing; else one launch (sizes and their
 * scan), one copy (64 bytes back) and one wait -- and where there is a pair: one launch more per started budget (64 MiB) of the
 * rows' solver slices (DISTRIBUTE has no slices: one launch), a second copy (64 bytes) and a second wait; with out_ref_member a third
 * copy (the entries) and a third wait.  No fill -- but the first call on an accumulator, and the first over more final rows than any
 * before, lay the accumulator's work buffer (two words per final row and the scan's words) and fill its head, one fill.  The call
 * leaves that buffer as it found it, so the sets of a sweep follow each other without one.  The solver's slices live in a buffer of the
 * accumulator bounded by the budget plus one largest slice, whatever the section's size.
 * SAME_EINVAL (outputs untouched): before same_merge_acc_finish, after same_merge_acc_plain or same_merge_acc_load, an unknown
 * strategy, members made for a section other than the one the pass ran over, under NEAREST n final rows times the largest possible
 * slice (in 128-byte units) beyond 2^31.  SAME_ERANGE (outputs untouched): a final row pairs a non-empty moving list with an empty
 * reference list; under NEAREST a cost matrix is infeasible (non-finite member XY: same_batched_assign's rule). */
typedef struct same_members same_members;
int  same_members_create(const same_section *section, const int64_t *off /* n_rows + 1 */, const double *member_xy /* 2 * m */,
                         const int32_t *member_code /* m */, int64_t m, same_members **out);
void same_members_destroy(same_members *members);
#define SAME_UNPACK_DISTRIBUTE 0
#define SAME_UNPACK_NEAREST    1
int same_merge_acc_unpack(same_merge_acc *acc, const same_members *moving, const same_members *ref, int strategy,
                          int64_t *out_counts /* [4] */, int64_t *out_ref_member /* may be NULL */, int64_t capacity);
/* The unpacked pairs broken down three ways (csrc/window_unpack_detail.hip): by label pair, by group of the moving row, by the rank of
 * the moving CELL's label among the type columns of the reference CELL it was put on (examples/luad/reproduce_figures.ipynb cell 13) --
 * binned on the device behind same_merge_acc_unpack's own phases; no pair comes to the host.
 *   same_unpack_detail_create: what cell pairs are binned by, uploaded once on `ref_members`' context, resident on its device, read-only
 *   and shared by the worker contexts like same_members; destroy it before its members.  n_labels: the number of CELL-level joint label
 *   codes, the codes the members were uploaded with.  col_of_label[code] is the type column (of T) the label names, or -1; NULL: no
 *   label names a column.  ref_member_types: one float64 type row of T columns per reference member, in CSR order; NULL: no type rows.
 *   Checked on the host before anything is uploaded: SAME_EINVAL for n_labels < 0 or > SAME_SCORE_MAX_LABELS, T < 0, col_of_label given
 *   without ref_member_types or with T == 0; SAME_ERANGE for a col_of_label value outside [-1, T).  A failure after these checks (an
 *   allocation, a copy) can leave *out set: destroy a non-null *out whatever the call returned.
 *   same_merge_acc_unpack_detail: `moving`, `ref`, `strategy` as same_merge_acc_unpack's; `detail` made for `ref`; `groups` (may be NULL:
 *   one group, 0) a same_score_detail of the moving members' section, of which only group_of and n_groups are read.  With L = n_labels,
 *   G = groups' n_groups (1 without groups) and R = SAME_SCORE_RANKS, `out` holds out_words >= 4 + L*L + 1 + (G+1)*2 + 2*(R+1) + 1 words
 *   (SAME_UNPACK_DETAIL_WORDS), in this order:
 *     counts [4]        exactly same_merge_acc_unpack's out_counts for the same arguments;
 *     confusion [L*L]   out[4 + cm*L + cr]: the pairs whose moving member's code is cm and whose reference member's code is cr;
 *     unlabelled [1]    the pairs in no cell: a code that is negative or >= L on either side;
 *     groups [(G+1)*2]  per bin (pairs, pairs whose two codes are equal and non-negative).  A pair is in the group of its final row's
 *                       moving section row (group_of[a_row]); bin G takes the pairs whose moving row has no group;
 *     ranks [2*(R+1)]   for the pair (moving member i, reference member j): c = col_of_label[code of i], v = ref_member_types[j][c],
 *                       strict = #{t != c: types[j][t] > v}, weak = #{t != c: types[j][t] >= v}, float64 comparisons (the rule of
 *                       same_merge_acc_score_detail's ranks); first the histogram of min(strict, R), then that of min(weak, R);
 *     untyped [1]       the pairs in no rank bin: a moving code that is negative or >= L, c < 0, no type rows, a NaN anywhere in the
 *                       reference member's type row.
 *   confusion + unlabelled, the groups' pairs, and weak + untyped each sum to counts[1]; the groups' agreeing pairs sum to counts[2].
 * What the call asks of the runtime for n final rows on the accumulator's context: n == 0 nothing (out is zeros); without a pair what
 * same_merge_acc_unpack asks (one launch, one copy, one wait); else exactly ONE launch more than same_merge_acc_unpack for the same
 * rows -- the sizes' launch, one launch per started budget of solver slices, the bins' launch --, THREE copies (64 bytes after the sizes;
 * 64 bytes and the words of `out` behind its counts after the bins) and TWO waits, the sizes' and the last.  No fill -- but a call that
 * lays the accumulator's unpack work buffer (same_merge_acc_unpack: the first, and the first over more final rows) fills its head, one
 * fill, and one that lays the bins' buffer (the first, and the first with more words than any before) fills that, one fill.  Both
 * buffers are left clear for the next call: both unpack calls, same_merge_acc_score and same_merge_acc_score_detail alternate on one
 * accumulator without a fill.
 * SAME_EINVAL / SAME_ERANGE as same_merge_acc_unpack, `out` untouched -- under NEAREST an infeasible row's pairs are never read, its
 * entries are marked on the device; SAME_EINVAL also for a `detail` made for other reference members, `groups` made for another section
 * than the moving members', and out_words too small. */
#define SAME_UNPACK_DETAIL_WORDS(L, G) (4 + (int64_t)(L) * (L) + 1 + ((int64_t)(G) + 1) * 2 + 2 * (SAME_SCORE_RANKS + 1) + 1)
typedef struct same_unpack_detail same_unpack_detail;
int  same_unpack_detail_create(const same_members *ref_members, int n_labels, const int32_t *col_of_label /* [n_labels] or NULL */,
                               const double *ref_member_types /* [m][T] or NULL */, int T, same_unpack_detail **out);
void same_unpack_detail_destroy(same_unpack_detail *detail);
int  same_merge_acc_unpack_detail(same_merge_acc *acc, const same_members *moving, const same_members *ref, int strategy,
                                  const same_unpack_detail *detail, const same_score_detail *groups /* may be NULL: one group */,
                                  int64_t *out, int64_t out_words);
/* The unpacked pairs read as FEATURE SUMS (csrc/window_unpack_feature.hip): same_merge_acc_score_features' reading at cell level -- what
 * examples/luad/reproduce_figures.ipynb cells 16-22 compute, which gather the two modalities' rows of every CELL pair of cell 12's
 * unpacked matches.  The pairs stay on the device behind same_merge_acc_unpack's own phases; the kernels are the section call's
 * (csrc/feature_kernels.h), reading a cell pair where that call reads a final row.
 *   same_unpack_features_create: one int32 fixed-point row per MEMBER, in CSR order -- mov_q[moving members][F_m], ref_q[reference
 *   members][F_r]; the quantisation is same_score_features_create's, word for word.  member_group[moving members]: the group of the
 *   moving CELL, negative: the cell has no group; NULL: every cell in group 0.  Uploaded once on `moving`'s context, resident on its
 *   device, read-only and shared by the worker contexts like same_members; destroy it before the members.  Checked on the host before
 *   anything is uploaded: SAME_EINVAL for the shapes same_score_features_create refuses (over member counts) and for members on
 *   different devices; SAME_ERANGE for a |q| > 2^30 or a group >= n_groups.  Caps: SAME_FEATURE_MAX_COLUMNS, SAME_SCORE_MAX_GROUPS.
 *   same_unpack_zone_create: exactly same_feature_zone_create's rules, per member: mov_flags[moving members], ref_flags[reference
 *   members], bit 0 "zone side", bit 1 "subset side", NULL: every bit set; a pair (i, j) is a ZONE pair iff mov_flags[i] & ref_flags[j]
 *   & 1, a SUBSET pair iff ... & 2; d2_edges cut the SQUARED distance right-closed; 2 to SAME_FEATURE_MAX_EDGES edges.  Destroy it
 *   before `feats`.
 *   same_merge_acc_unpack_features: `moving`, `ref`, `strategy` as same_merge_acc_unpack's.  With G = n_groups, F = F_m + F_r and
 *   B = n_edges - 1 (0 without `zone`), `out` holds out_words >= SAME_UNPACK_FEATURE_WORDS(G, F, B) = 4 + SAME_FEATURE_WORDS(G, F, B)
 *   int64 words:
 *     [0 .. 4)   exactly same_merge_acc_unpack's out_counts for the same arguments;
 *     [4 ..)     same_merge_acc_score_features' `out`, with "final row" read as "cell pair": counts [4] (pairs; those whose moving cell
 *                has a group; zone pairs; subset pairs), rows [G+1], sums [(G+1)*F], and with `zone` bin_rows [B+1], bin_sums [(B+1)*F].
 *   A pair's bin is its moving member's group, its position its REFERENCE MEMBER's XY (same_members').  d2: the fp64 minimum over all
 *   zone pairs of dx*dx + dy*dy, without contraction (a pair that is both: 0); with no zone pair every d2 is NaN and every subset pair
 *   is in bin B.  out_d2 (may be NULL) and out_ref_member (may be NULL), `capacity` entries each, are indexed by PAIR, in
 *   same_merge_acc_unpack's pair order -- which keeps the call defined where hostile final rows name a moving row twice: the d2 of a
 *   subset pair, NaN otherwise (all NaN without `zone`); the flat reference member.  capacity < out[1] with either array given:
 *   SAME_EINVAL with out[0 .. 4) FILLED, the rest of `out` and the arrays untouched.
 * What the call asks of the runtime for n final rows on the accumulator's context: n == 0 nothing (out is zeros); without a pair what
 * same_merge_acc_unpack asks.  Else, without `zone`: exactly ONE launch more than same_merge_acc_unpack for the same rows (the sums by
 * group), THREE copies (64 bytes after the sizes; 64 bytes and the words of `out` and one more before the last wait) and with
 * out_ref_member a fourth, TWO waits -- the sizes' and the last: no wait of its own.  With `zone`: FOUR launches more (the sums by group,
 * the flag kernel; after the reader's wait the walk and the sums by bin), one copy more (32 bytes) and ONE wait more, taken INSIDE the
 * reader between the flag kernel and the grid build -- the host must know the zone pairs' count and box first --, with out_d2 one copy
 * more; where there is a zone pair grid.h's build runs behind that wait as in same_merge_acc_score_features (its own read-back, wait,
 * fill and three launches, which the context's counters do not count).  No fill -- but a call that lays the unpack work buffer fills
 * its head, one that lays the sums' buffer (the first, and the first with more words) fills it, and with `zone` one that lays the
 * zone work buffer (the first, and the first over more pairs) fills its head: one fill each.  Every buffer is left as it was found:
 * score, detail, map, feature, both unpack calls and this call alternate on one accumulator without a fill, and a call that failed
 * between an enqueue and its wait leaves the buffers it worked in marked not laid, so the next call lays them again.
 * SAME_EINVAL / SAME_ERANGE as same_merge_acc_unpack, outputs untouched; SAME_EINVAL also for `feats` made for other members or on
 * another device, `zone` made for other `feats`, out_words too small, an array given with capacity < 0; SAME_ERANGE (outputs
 * untouched) with `zone` for a zone or subset pair whose reference member XY is not finite -- found by the flag kernel, before
 * anything is binned by it. */
#define SAME_UNPACK_FEATURE_WORDS(G, F, B) (4 + SAME_FEATURE_WORDS(G, F, B))
typedef struct same_unpack_features same_unpack_features;
typedef struct same_unpack_zone same_unpack_zone;
int  same_unpack_features_create(const same_members *moving, const same_members *ref, const int32_t *mov_q /* host, [moving members][F_m] */,
                                 int F_m, const int32_t *ref_q /* host, [ref members][F_r] */, int F_r,
                                 const int32_t *member_group /* [moving members] or NULL: every cell in group 0 */, int n_groups,
                                 same_unpack_features **out);
void same_unpack_features_destroy(same_unpack_features *feats);
int  same_unpack_zone_create(const same_unpack_features *feats, const uint8_t *mov_member_flags /* [moving members] or NULL */,
                             const uint8_t *ref_member_flags /* [ref members] or NULL */, const double *d2_edges, int n_edges,
                             same_unpack_zone **out);
void same_unpack_zone_destroy(same_unpack_zone *zone);
int  same_merge_acc_unpack_features(same_merge_acc *acc, const same_members *moving, const same_members *ref, int strategy,
                                    const same_unpack_features *feats, const same_unpack_zone *zone /* may be NULL */, int64_t *out,
                                    int64_t out_words, double *out_d2 /* [capacity], may be NULL */,
                                    int64_t *out_ref_member /* [capacity], may be NULL */, int64_t capacity);
/* The unpacked pairs per moving CELL (csrc/window_unpack_map.hip): same_merge_acc_score_map's reading at cell level -- what
 * examples/tongue/reproduce_figures.ipynb cells 15-16 and examples/luad cells 12-13 plot, every cell coloured by what the reference CELL
 * it was put on says of it.  The pairs stay on the device behind same_merge_acc_unpack's own phases; one 16-byte mark per moving member.
 *   The mark of moving member i (a flat index into `moving`'s CSR):
 *     ref_member   the flat index into `ref`'s CSR of the reference member the unpack gave it: exactly entry out_ref_member[pair] of
 *                  same_merge_acc_unpack for the same arguments;
 *     ref_row      the reference section row that owns that member;
 *     pair         the pair's index in same_merge_acc_unpack's pair order;
 *     flags        the SAME_MARK_* bits: MATCHED 1; TYPE_MATCH 2: the two member codes are equal and non-negative (out_counts[2]'s
 *                  rule); TRUTH_KNOWN 16: the map holds a truth member >= 0 for i; ON_TRUTH 32: matched and ref_member equals it;
 *                  RANKED 64: the two rank bytes hold ranks.  CONSIDERED and VIOLATING are never set: triangles are a metacell-level
 *                  reading;
 *     rank_strict, rank_weak   same_merge_acc_unpack_detail's strict and weak of (col_of_label[code of i], the reference MEMBER's type
 *                  row), saturated at 254 as same_cell_mark's; 255 with RANKED clear where the member is not ranked: unmatched, no
 *                  `detail` or one without col_of_label or type rows, a code that is negative or >= n_labels, a label that names no
 *                  column, a NaN anywhere in the type row.
 *   An unmatched member's mark is {-1, -1, -1, TRUTH_KNOWN or 0, 255, 255, 0}: no final row names its moving row (or the row has no
 *   pair, which a non-empty list on a named row cannot).  A merge's final rows name a moving row at most once, so a member has at most
 *   one pair; the call relies on that, as same_merge_acc_score_map does.
 *   out_counts[6]: [0 .. 3] exactly same_merge_acc_unpack's for the same arguments; [4] the matched members whose truth is known, [5]
 *   those of them that are on it.  The marks with MATCHED number [1], those with TYPE_MATCH [2].
 *   same_unpack_map_create: what the marks are read against and folded into, made on `moving`'s context for these two member objects,
 *   resident on its device and shared by the worker contexts of that device like same_score_map (at most 32 calling contexts); destroy
 *   it before the members.  truth_member[i] (host, one per moving member, may be NULL: every member unknown): the flat reference member
 *   that is member i's true or baseline partner, -1 unknown; SAME_EINVAL for a value < -1 or >= the reference members' count, checked on
 *   the host before anything is uploaded.  with_tally: the map holds tally[moving members][3] (uint32, zero at first) -- per member in
 *   how many results folded in so far it was matched, type-matched, on its truth -- added to by 32-bit atomics, results of one study may
 *   be folded in from several worker contexts.
 *   same_unpack_map_tally, same_unpack_map_reset: same_score_map_tally's and same_score_map_reset's rules (out_tally: members * 3
 *   words, may be NULL, SAME_EINVAL when given for a map without a tally; one copy and one wait -- one fill and one wait).
 *   same_merge_acc_unpack_map: `moving`, `ref`, `strategy` as same_merge_acc_unpack's; `detail` (may be NULL: no ranks) made for `ref`;
 *   `map` made for these members.  out_marks (may be NULL: counts and tally only): one mark per moving member, any host memory, written
 *   by the host from a page-locked block of the map and only by a call that succeeds.
 * What the call asks of the runtime on the accumulator's context: without a pair -- no final row, or none whose moving row has a member
 * -- what same_merge_acc_unpack asks and nothing more: out_counts[4], [5] are zero, out_marks is written on the host as the unmatched
 * marks (the map keeps the truth members for the TRUTH_KNOWN bit), the result count goes up by one.  Else same_merge_acc_unpack's own
 * budget for the same rows and beyond it: TWO launches (pair_of by pair, the marks by member), one copy of the totals (16 bytes) and with
 * out_marks one copy of the marks, from a device buffer of the map; no wait beyond same_merge_acc_unpack's second, the call's last -- so
 * THREE copies (four with out_marks) and TWO waits.  No fill -- but a call that lays the accumulator's unpack work buffer fills its
 * head, one fill, and a calling context's first call on a map (and the first after a call that failed half way) lays its slot: two
 * fills (pair_of to -1, the slot's totals to zero).  The totals are counted in the map, two sets per calling context of which each
 * call clears the other's (work_sets.h), and pair_of is returned to -1 member by member: every buffer is left as it was found, so the
 * unpack, unpack-detail, unpack-feature, score, detail, map, feature calls and this call alternate on one accumulator without a fill.
 * SAME_EINVAL / SAME_ERANGE as same_merge_acc_unpack, out_counts and out_marks untouched; SAME_EINVAL also for a `map` made for other
 * members or on another device and a `detail` made for other reference members.  After SAME_ERANGE the tally may hold part of the
 * refused result: reset it. */
typedef struct { int32_t ref_member, ref_row, pair; uint8_t flags, rank_strict, rank_weak, reserved; } same_member_mark;   /* 16 bytes */
typedef struct same_unpack_map same_unpack_map;
int  same_unpack_map_create(const same_members *moving, const same_members *ref,
                            const int32_t *truth_member /* host, [moving members], -1 unknown; may be NULL */, int with_tally,
                            same_unpack_map **out);
void same_unpack_map_destroy(same_unpack_map *map);
int  same_unpack_map_tally(same_unpack_map *map, uint32_t *out_tally /* [moving members][3], may be NULL */, int64_t *out_results);
int  same_unpack_map_reset(same_unpack_map *map);
int  same_merge_acc_unpack_map(same_merge_acc *acc, const same_members *moving, const same_members *ref, int strategy,
                               const same_unpack_detail *detail /* may be NULL: no ranks */, same_unpack_map *map,
                               same_member_mark *out_marks /* [moving members], may be NULL */, int64_t *out_counts /* [6] */);

/* ======================================================================================================================
 * part 4 -- COMM: one communicator per context, RCCL over xGMI
 * ====================================================================================================================== */
/* ---- multi-GPU: RCCL all-gather of the pruned candidate lists -------------
 * One process per GPU.  Rank 0 calls same_comm_unique_id and hands the 128 bytes to the
 * other ranks by any host channel; all ranks then call same_comm_init.  same_allgather_dev
 * gathers equal-sized device blocks (send_bytes each) into recv (nranks*send_bytes) on the
 * context's stream. */
#define SAME_UNIQUE_ID_BYTES 128
int same_comm_unique_id(char out_id[SAME_UNIQUE_ID_BYTES]);
int same_comm_init(same_ctx *ctx, int nranks, int rank, const char id[SAME_UNIQUE_ID_BYTES]);
int same_comm_destroy(same_ctx *ctx);
int same_allgather_dev(same_ctx *ctx, const void *dsend, void *drecv, size_t send_bytes);
/* Overlapped form: the gather runs on a second stream of the context, ordered after all compute queued
 * so far, and does not block later compute (e.g. the next row block's dense build).  same_comm_wait
 * orders the compute stream after every gather issued so far; call it before overwriting the send
 * buffers or reading the gathered ones.  same_ctx_sync waits for both streams. */
int same_allgather_dev_async(same_ctx *ctx, const void *dsend, void *drecv, size_t send_bytes);
int same_comm_wait(same_ctx *ctx);
/* In-place all-reduce of count elements on the context's stream (sweep counters: U64 SUM; point flags:
 * U8 MAX = logical OR; timings: F64 MAX). */
#define SAME_DT_U8 0
#define SAME_DT_I32 1
#define SAME_DT_U64 2
#define SAME_DT_F64 3
#define SAME_OP_SUM 0
#define SAME_OP_MAX 1
#define SAME_OP_MIN 2
int same_allreduce_dev(same_ctx *ctx, void *dbuf, size_t count, int dtype, int op);
/* collectives issued between these two calls go to RCCL as one group (ncclGroupStart / ncclGroupEnd): one fused launch */
int same_comm_group_start(same_ctx *ctx);
int same_comm_group_end(same_ctx *ctx);
/* What the communicator itself reports -- ncclCommCount (0 = no communicator) and ncclCommUserRank, not the arguments
 * same_comm_init was given -- and the RCCL version the library is running against.  Any pointer may be NULL. */
int same_comm_info(same_ctx *ctx, int *out_nranks, int *out_rank, int *out_rccl_version);
/* ncclCommCuDevice of the communicator (-1 = none) */
int same_comm_device(same_ctx *ctx, int *out_device);
#ifdef __cplusplus
}
#endif
#endif /* SAME_HIP_H */
