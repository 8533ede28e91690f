/*
 * pointops2_hip.h — C ABI of libpointops2_hip.so, the MI355X (gfx950) implementation of the
 * Stratified Transformer's pointops2 hot path.
 *
 * PART 1 are the reference's own raw-pointer launchers (the "true C ABI" of lib/pointops2,
 * SURVEY.md §8b seam B2): same names, same argument order and meaning.  Every pointer is a
 * DEVICE pointer to a contiguous fp32 / int32 array.  Ownership follows the reference: the caller
 * allocates every output (and zero-fills it where the reference does, see each entry); the library
 * borrows the pointers for the duration of the launch, allocates nothing and returns void.
 *
 * Differences from the reference, all "stricter is compatible":
 *   - launches go to the stream set with pointops2_set_stream() (thread-local; default: the NULL
 *     stream, which is what the reference's <<<grid, block, 0>>> launches use);
 *   - instead of `throw "d != 16 and d != 32"` (attention_cuda_kernel_v2.cu:116) an unsupported
 *     argument records an error readable with pointops2_last_error(); the call is then a no-op;
 *   - outputs are fully written by the kernels (the caller's zero-fill is harmless, not required),
 *     except where noted "accumulates".
 *
 * PART 2 are the launch options (pointops2_launch_opts) and the additional native entry points this
 * build adds on the same path (segment softmax = the torch_scatter.scatter_softmax call of the model,
 * CSC transposition used by the backward kernels, the index build, ...).
 */
#ifndef POINTOPS2_HIP_H
#define POINTOPS2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* runtime plumbing                                                                           */
/* ------------------------------------------------------------------------------------------ */
/* hipStream_t as void*.  Thread-local.  NULL = legacy default stream. */
void pointops2_set_stream(void *hip_stream);
void *pointops2_get_stream(void);
/* NULL when the last call on this thread succeeded; otherwise a static message.  Reading clears. */
const char *pointops2_last_error(void);
/* library/ABI version, bumped when a signature changes (3: pointops2_launch_opts replaces the per-fact setters; 5: the packed
 * cell_attention_qkv_*_launcher pair).  Entry points that are only ADDED leave it: the kpconv_aggregate_*_launcher pair came in at
 * version 5, the grouped_max_*_launcher pair, the five pointops2_dbscan_*_launcher, the pointops2_evaltile_* entry points, the two
 * pointops2_contacts_*_launcher, pointops2_label_boxes_launcher / pointops2_reach_rows_launcher and the three
 * pointops2_supports_*_launcher, the two pointops2_augment_*_launcher optim_adamw_step_launcher, optim_step_launcher and the gather_add_*_launcher pair after them - a caller that needs them looks the symbols up. */
int pointops2_abi_version(void);
/* Diagnostic: how long (ticks of the 100 MHz clock, default 2 s) a workgroup of the round sampler waits at its grid barrier before
 * the sampler gives up and pointops2_last_error() reports the call's indices invalid (tests force the path with a tiny value). */
void pointops2_diag_set_fps_patience(unsigned long long ticks_100mhz);

/* ------------------------------------------------------------------------------------------ */
/* PART 1 — the reference's launcher set                                                      */
/* ------------------------------------------------------------------------------------------ */

/* sampling/sampling_cuda_kernel.h:14  — furthest point sampling per batch element.
 * n = largest batch element (selects the reference's block size, which fixes its tie rule);
 * xyz [N,3]; offset/new_offset [b] cumulative ends; tmp [N] scratch PRE-FILLED with 1e10;
 * idx [new_offset[b-1]] out. */
void furthestsampling_cuda_launcher(int b, int n, const float *xyz, const int *offset,
                                    const int *new_offset, float *tmp, int *idx);

/* knnquery/knnquery_cuda_kernel.h:14 — exact kNN, ascending; dist2 = SQUARED distances. nsample <= 100. */
void knnquery_cuda_launcher(int m, int nsample, const float *xyz, const float *new_xyz,
                            const int *offset, const int *new_offset, int *idx, float *dist2);

/* grouping/grouping_cuda_kernel.h:14-15 — gather rows / scatter-add (grad_input accumulates). */
void grouping_forward_cuda_launcher(int m, int nsample, int c, const float *input, const int *idx, float *output);
void grouping_backward_cuda_launcher(int m, int nsample, int c, const float *grad_output, const int *idx, float *grad_input);

/* interpolation/interpolation_cuda_kernel.h:34-35 — k-NN weighted sum (output / grad_input accumulate). */
void interpolation_forward_cuda_launcher(int n, int c, int k, const float *input, const int *idx, const float *weight, float *output);
void interpolation_backward_cuda_launcher(int n, int c, int k, const float *grad_output, const int *idx, const float *weight, float *grad_input);

/* attention/attention_cuda_kernel.h:17-21 — pair-indexed (v1) forms; outputs ACCUMULATE (atomics in
 * the reference), so the caller's zero-fill is required. */
void attention_step1_forward_cuda_launcher(int N, int M, int h, int C, const float *q, const float *k,
                                           const int *index0, const int *index1, float *attn);
void attention_step1_backward_cuda_launcher(int N, int M, int h, int C, const float *grad_out,
                                            const int *index0, const int *index1, const float *q,
                                            const float *k, float *grad_q, float *grad_k);
void attention_step2_forward_cuda_launcher(int N, int M, int h, int C, const float *attn, const float *v,
                                           const int *index0, const int *index1, float *output);
void attention_step2_backward_cuda_launcher(int N, int M, int h, int C, const float *grad_out,
                                            const int *index0, const int *index1, const float *attn,
                                            const float *v, float *grad_attn, float *grad_v);

/* attention_v2/attention_cuda_kernel_v2.h:19-23 — CSR forms.  index0_offsets [N+1]; index1 [M];
 * n_max = longest segment (<= 1024, pointops.py:150).  C/h must be 16 or 32.
 * backward: grad_q fully written; grad_k ACCUMULATES (pre-zeroed by the caller). */
void attention_step1_forward_cuda_launcher_v2(int N, int M, int h, int C, const unsigned int n_max,
                                              const float *q, const float *k, const int *index0_offsets,
                                              const int *index1, float *attn);
void attention_step1_backward_cuda_launcher_v2(int N, int M, int h, int C, const unsigned int n_max,
                                               const float *grad_out, const int *index0_offsets,
                                               const int *index1, const float *q, const float *k,
                                               float *grad_q, float *grad_k);
void attention_step2_forward_cuda_launcher_v2(int N, int M, int h, int C, const float *attn, const float *v,
                                              const int *index0, const int *index1, float *output);
void attention_step2_backward_cuda_launcher_v2(int N, int M, int h, int C, const float *grad_out,
                                               const int *index0, const int *index1, const float *attn,
                                               const float *v, float *grad_attn, float *grad_v);

/* rpe/relative_pos_encoding_cuda_kernel.h:17-21 — v1 single-table forms (outputs accumulate). */
void dot_prod_with_idx_forward_cuda_launcher(int N, int M, int h, int hdim, const float *q, const int *index,
                                             const float *table, const int *rel_idx, float *output);
void dot_prod_with_idx_backward_cuda_launcher(int N, int M, int h, int hdim, const float *grad_out,
                                              const float *q, const int *index, const float *table,
                                              const int *rel_idx, float *grad_q, float *grad_table);
void attention_step2_with_rel_pos_value_forward_cuda_launcher(int N, int M, int h, int hdim, const float *attn,
                                                              const float *v, const int *index0, const int *index1,
                                                              const float *table, const int *rel_idx, float *output);
void attention_step2_with_rel_pos_value_backward_cuda_launcher(int N, int M, int h, int hdim, const float *grad_out,
                                                               const int *index0, const int *index1, const float *attn,
                                                               const float *v, const float *table, const int *rel_idx,
                                                               float *grad_attn, float *grad_v, float *grad_table);

/* rpe_v2/relative_pos_encoding_cuda_kernel_v2.h:22-29 — CSR forms.  table [L,h,hdim,3]; rel_idx [M,3].
 * hdim must be 16 or 32.  backward: grad_q / grad_attn fully written; grad_k / grad_v / table grads
 * ACCUMULATE (pre-zeroed by the caller).  The table length L is not part of the reference signature
 * but the fast kernels stage the tables in LDS: pass it as launch_opts.table_rows (PART 2) for any
 * *_v3 bias or *_v2 rel-pos-value launcher (forward and backward).  Without it the launchers are still
 * callable with the reference's arguments alone: generic kernels then read the tables from global
 * memory and accumulate with atomics as the reference does (same results, several times slower). */
void dot_prod_with_idx_forward_cuda_launcher_v2(int N, int M, int h, int hdim, int n_max, int T, const float *q,
                                                const int *index_q, const float *k, const int *index_k,
                                                const float *table_q, const float *table_k, const int *rel_idx,
                                                const int *rel_idx_offsets, const int *sort_indices, float *output);
void dot_prod_with_idx_backward_cuda_launcher_v2(int N, int M, int h, int hdim, int n_max, int T, const float *grad_out,
                                                 const float *q, const int *index_q, const float *k, const int *index_k,
                                                 const float *table_q, const float *table_k, const int *rel_idx,
                                                 const int *rel_idx_offsets, const int *sort_indices, float *grad_q,
                                                 float *grad_k, float *grad_table_q, float *grad_table_k);
void dot_prod_with_idx_forward_cuda_launcher_v3(int N, int M, int h, int hdim, int n_max, const float *q,
                                                const int *index_q_offsets, const float *k, const int *index_k,
                                                const float *table_q, const float *table_k, const int *rel_idx,
                                                float *output);
void dot_prod_with_idx_backward_cuda_launcher_v3(int N, int M, int h, int hdim, int n_max, const float *grad_out,
                                                 const float *q, const int *index_q_offsets, const float *k,
                                                 const int *index_k, const float *table_q, const float *table_k,
                                                 const int *rel_idx, float *grad_q, float *grad_k,
                                                 float *grad_table_q, float *grad_table_k);
void attention_step2_with_rel_pos_value_forward_cuda_launcher_v2(int N, int M, int h, int hdim, int n_max,
                                                                 const float *attn, const float *v,
                                                                 const int *index0_offsets, const int *index1,
                                                                 const float *table, const int *rel_idx, float *output);
void attention_step2_with_rel_pos_value_backward_cuda_launcher_v2(int N, int M, int h, int hdim, int n_max,
                                                                  const float *grad_out, const int *index0_offsets,
                                                                  const int *index1, const float *attn, const float *v,
                                                                  const float *table, const int *rel_idx,
                                                                  float *grad_attn, float *grad_v, float *grad_table);

/* subtraction/subtraction_cuda_kernel.h:14-15, aggregation/aggregation_cuda_kernel.h:14-15 — Point-Transformer
 * vector-attention ops bound by pointops_api.cpp:23-26 and called by no model of the reference (out of scope):
 * exported so that the reference's shim sources link; a call records an error and does nothing. */
void subtraction_forward_cuda_launcher(int n, int nsample, int c, const float *input1, const float *input2, const int *idx, float *output);
void subtraction_backward_cuda_launcher(int n, int nsample, int c, const int *idx, const float *grad_output, float *grad_input1,
                                        float *grad_input2);
void aggregation_forward_cuda_launcher(int n, int nsample, int c, int w_c, const float *input, const float *position, const float *weight,
                                       const int *idx, float *output);
void aggregation_backward_cuda_launcher(int n, int nsample, int c, int w_c, const float *input, const float *position, const float *weight,
                                        const int *idx, const float *grad_output, float *grad_input, float *grad_position,
                                        float *grad_weight);

/* ------------------------------------------------------------------------------------------ */
/* PART 2 — additional entry points of this build                                             */
/* ------------------------------------------------------------------------------------------ */

/* ---- launch options: the facts the fast kernels need that the PART-1 signatures do not carry ------------------
 * ONE RULE: the options set with pointops2_set_launch_opts() apply to the next library launch on this thread, and that
 * launch resets them, whether or not it used them (the stream is not an option: it stays until set again).  0 / NULL = not
 * given; all-zero = the reference's arguments alone (same results, in places slower generic kernels).  The *_workspace_bytes
 * queries, pointops2_cell_forward_variant, pointops2_last_error, pointops2_get_stream and pointops2_abi_version are no launches:
 * they leave the options. */
typedef struct pointops2_launch_opts {
    /* L of the [L,h,hdim,3] tables of a *_v3 bias, *_v2 rel-pos-value or window_* call: the fast kernels stage them in LDS.
     * Without it the rel-pos launchers read the tables from global memory (several times slower), window_* record an error. */
    int table_rows;
    /* rows of k / v when they outnumber the CSR's query rows N (a rank of a sharded scene); 0 = N */
    int key_rows;
    /* key-major view of the call's pair list (pointops2_csc_build): the *_backward_* launchers gather the key-side gradients
     * by key; without it they accumulate them with global float atomics, as the reference does */
    const int *csc_offsets;
    const int *csc_pair;
    const int *csc_query;
    /* rows in window order (pointops2_row_order_launcher) and their count: the A1 / A2 / A4 pair walkers take their rows in
     * that order when a launch walks exactly row_order_rows >= 2048 rows (same results, partner gathers hit L2) */
    const int *row_order;
    int row_order_rows;
    /* scratch lent to furthestsampling_cuda_launcher (>= pointops2_fps_workspace_bytes(b, N)) or knnquery_cuda_launcher
     * (>= pointops2_knn_workspace_bytes(n, m, b)) with the counts the signatures lack: point_count = N = offset[b-1] (FPS) or
     * n (kNN), batch_count = b (kNN).  FPS: bucketed exact sampler in rounds when n >= 2048; kNN: exact grid search; without
     * them the reference's scans.  Same indices either way. */
    void *workspace;
    size_t workspace_bytes;
    int point_count;
    int batch_count;
    /* FPS resume: idx / new_offset of the previous call on the SAME xyz/offset whose state the workspace still holds - the
     * sampler continues that chain instead of starting over (the model asks for n/8+1, then n/4+1 samples, :289,103) */
    const int *fps_prev_idx;
    const int *fps_prev_new_offset;
    /* != 0: the FPS cloud is a raw scene, not an earlier FPS output in selection order - skips the identity-prefix probe
     * (~60 us); same result with a wrong flag */
    int fps_unordered;
} pointops2_launch_opts;
/* copies *opts into this thread's launch options (NULL clears them) */
void pointops2_set_launch_opts(const pointops2_launch_opts *opts);
size_t pointops2_fps_workspace_bytes(int b, int N);
size_t pointops2_knn_workspace_bytes(int n, int m, int b);
/* key-major ("CSC") transposition of a CSR pair list: csc_offsets [keys+1] (keys = launch_opts.key_rows, 0: N), csc_pair [M]
 * (pair ids, ascending per key), csc_query [M] (query of each pair) */
size_t pointops2_csc_workspace_bytes(int N, int M);
void pointops2_csc_build(int N, int M, const int *index0_offsets, const int *index1,
                         int *csc_offsets, int *csc_pair, int *csc_query,
                         void *workspace, size_t workspace_bytes);

/* torch_scatter.scatter_softmax(src [M,h], index_0, dim=0) over CSR segments
 * (model/stratified_transformer.py:205) and its backward. */
void segment_softmax_forward_launcher(int N, int M, int h, const float *src, const int *offsets, float *out);
void segment_softmax_backward_launcher(int N, int M, int h, const float *out, const float *grad_out,
                                       const int *offsets, float *grad_src);
/* ---- on-device index build of one stage (model/stratified_transformer.py:10-65, 186-190, 312-317) ----
 * All arrays are caller-allocated device memory; ws is scratch of pointops2_index_workspace_bytes(N) bytes.
 *   bbox:       out6 = {min x,y,z, max x,y,z} of xyz [N,3]
 *   partition:  one grid_sample(): cluster [N] dense window id (torch.unique rank of the voxel id), order [N] point
 *               ids sorted by (window, id), starts [N+2] bucket boundaries into order, n_windows [1].
 *               size = window edge, shift = value added to xyz before binning (0, or size/2 for the shifted
 *               partitions); key_bits = significant bits of the voxel ids (0 = all 64)
 *   window_coord: wc [N,3] = ((xyz [+ window/2]) - xyz_min) // window  (fp32 floor division), the mask operand of :28-34
 *   sampled_buckets: the FPS subset (sample_idx [m]) bucketed by a large-window partition: ls [m] point ids in
 *               (window, id) order, ls_starts [N+1]; `sampled` [N] must be zero-filled by the caller
 *   pairs_count: offsets [N+1] = exclusive scan of keys per query (offsets[N] = M)
 *   pairs_fill:  index_0 / index_1 [M], rel_idx [M,3] in the canonical order (dense keys ascending, then
 *               stratified keys ascending) */
void pointops2_bbox_launcher(int N, const float *xyz, float *out6);
size_t pointops2_index_workspace_bytes(int N);
void pointops2_window_partition_launcher(int N, int b, const float *xyz, const int *offset, const float *bbox6, float size,
                                         float shift, int key_bits, int *cluster, int *order, int *starts, int *n_windows,
                                         void *ws, size_t ws_bytes);
/* the four partitions of a stage in one sort (variant 0 small, 1 small shifted by window/2, 2 large = 2 window, 3 large shifted by
 * window): cluster / order [4][N], starts [4][N+2], n_windows [4], same contents as four partition calls.  The key is of fixed width
 * (ten bits per voxel coordinate: no bounding-box read-back); *overflow = 1 when a coordinate does not fit - the outputs are then
 * meaningless (but in range) and the caller builds the partitions one by one. */
/* Rows in window order: order [N] = the rows of a CSR pair list sorted by their first partner (rows of one window become neighbours),
 * for launch_opts.row_order. */
size_t pointops2_row_order_workspace_bytes(int N);
void pointops2_row_order_launcher(int N, int M, const int *offsets, const int *index1, int *order, void *ws, size_t ws_bytes);
size_t pointops2_partitions4_workspace_bytes(int N);
void pointops2_window_partitions4_launcher(int N, int b, const float *xyz, const int *offset, const float *bbox6, float window,
                                           int *cluster, int *order, int *starts, int *n_windows, int *overflow, void *ws,
                                           size_t ws_bytes);
void pointops2_window_coord_launcher(int N, const float *xyz, const float *bbox6, float window, int shifted, float *wc);
void pointops2_sampled_buckets_launcher(int N, int m, const int *sample_idx, const int *l_order, const int *l_starts,
                                        const int *l_n_windows, int *sampled, int *ls, int *ls_starts, void *ws, size_t ws_bytes);
void pointops2_pairs_count_launcher(int N, const int *s_cluster, const int *s_starts, const int *l_cluster, const int *ls,
                                    const int *ls_starts, const float *wc, int *offsets, void *ws, size_t ws_bytes);
void pointops2_pairs_fill_launcher(int N, const float *xyz, float window, float quant, const int *s_cluster, const int *s_order,
                                   const int *s_starts, const int *l_cluster, const int *ls, const int *ls_starts, const float *wc,
                                   const int *offsets, int *index_0, int *index_1, int *rel_idx);

/* expands CSR offsets to the per-pair query id (index_0); segment bounds are clamped into [0, M], so offsets that do not
 * describe an M-pair list leave entries unwritten but never write outside index0[0, M) */
void csr_expand_launcher(int N, int M, const int *offsets, int *index0);

/* *bad (device int) = 0 iff offsets [N+1] describes the per-pair query ids index [M] exactly (offsets[0] = 0,
 * offsets[N] = M, ordered segments, every pair of segment i carries the id i), non-zero otherwise.  Reads nothing
 * outside offsets[0..N] and index[0..M) whatever the offsets hold.  index: int32 or int64 (index_is_int64); the model's
 * scatter_softmax call site (model/stratified_transformer.py:205) passes int64. */
void pointops2_csr_matches_launcher(int N, int M, const int *offsets, const void *index, int index_is_int64, int *bad);

/* ---- optional fused path (no counterpart in the reference's launcher set) -----------------------
 * attn[m,hh] = softmax over the query's pairs of (<q,k[j]> + <q,Tq(m)> + <k[j],Tk(m)>): A1 + A2 + add + A3 of
 * WindowAttention.forward (model/stratified_transformer.py:183-205) in one kernel.  d = 16 only; needs
 * launch_opts.table_rows.  attn [M,h] is fully written (no zero-fill needed). */
void window_logits_softmax_forward_launcher(int N, int M, int h, int hdim, const float *q, const int *index_q_offsets,
                                             const float *k, const int *index_k, const float *table_q,
                                             const float *table_k, const int *rel_idx, float *attn);

/* Backward of the whole sequence for that module: grad_logit [M,h] (scratch/output, fully written), grad_q [N,h,16],
 * grad_k / grad_v [rows of k, h, 16] fully written; the three table gradients [L,h,16,3] are ACCUMULATED (zero-fill them).
 * attn = the forward's softmax output.  Needs launch_opts.table_rows, launch_opts.csc_* and, when k / v have other rows
 * than q, launch_opts.key_rows. */
void window_attention_backward_launcher(int N, int M, int h, int hdim, const float *grad_out, const float *q, const float *k,
                                        const float *v, const float *attn, const int *index0_offsets, const int *index1,
                                        const float *table_q, const float *table_k, const float *table_v,
                                        const int *rel_idx, float *grad_logit, float *grad_q, float *grad_k, float *grad_v,
                                        float *grad_table_q, float *grad_table_k, float *grad_table_v);

/* ---- window-centric ("cell") attention: SURVEY 8f-1, second step ------------------------------------------------
 * A cell = the queries of one (small window, large window) intersection of a block pattern; they share one candidate key
 * list (the small window's points, then the sampled points of the large window), so a cell is a dense n_q x n_k tile of
 * pairs (model/stratified_transformer.py:15-18, :20-38).  The plan of a pattern is built from the arrays the index build
 * already has (window partitions, bucketed samples, window coordinates):
 *   pass 1  pointops2_cell_plan_count_launcher  cells, their order, sizes and scans; counts[8] = {cells, tile entries P,
 *           key slots K, largest key count, parents (cells before the cut)} (device; the caller reads P and K to allocate the arrays of pass 2);
 *           max_queries > 0 cuts every cell into pieces of at most that many queries (a piece = one wave's unit of work)
 *   pass 2  pointops2_cell_plan_fill_launcher   key list per cell, owner cell per key slot, and per tile entry the packed
 *           rel-pos index r0 | r1 << 8 | r2 << 16 (model :186-190, clamped to [0, L)) with bit 31 set where the candidate is
 *           NOT a key of that query (same window coordinate, :34)
 * All arrays are caller-allocated device memory: cell_order, qcell, cell_perm [N]; cell_desc [4N]; cell_qstart, cell_kbase,
 * cell_pbase, parent_first [N+2]; counts [8]; cell_keys, kcell [K]; relp [P]. */
typedef struct pointops2_cell_plan {
    int n_points;            /* N */
    int n_cells;             /* host copy of counts[0] */
    int n_parents;           /* host copy of counts[4]: cells before the cut into pieces of max_queries */
    int n_pairs;             /* P = sum over cells of n_q * n_k (host copy of counts[1]) */
    int n_keyslots;          /* K = sum over cells of n_k       (host copy of counts[2]) */
    const int *counts;       /* device [8] */
    const int *parent_first; /* [N+2] first piece (cell id) of a parent; pieces of a parent are consecutive, their tiles contiguous */
    const int *cell_perm;    /* [N]   cell ids, largest tile first (first counts[0] entries) */
    const int *cell_qstart;  /* [N+2] first sorted query position of a cell */
    const int *cell_kbase;   /* [N+2] first key slot of a cell */
    const int *cell_pbase;   /* [N+2] first tile entry of a cell; entry (il, jl) is at pbase + il * n_k + jl */
    const int *cell_order;   /* [N]   query (point) ids grouped by cell, ascending inside a cell */
    const int *qcell;        /* [N]   cell of a sorted query position */
    const int *cell_keys;    /* [K]   key (point) ids per cell: dense keys ascending, then stratified candidates ascending */
    const int *kcell;        /* [K]   cell of a key slot */
    const unsigned int *relp;/* [P]   packed rel-pos index + "not a key" flag */
    int task_first;          /* the launch works on the cells cell_perm[task_first + i * task_step] only (one scene over several */
    int task_step;           /* ranks: rank r of w takes r, r + w, ... - cells are sorted by size, so the shares are balanced); */
                             /* 0 / 0 (or step 1): all cells.  A partial forward writes only its cells' rows of `out`, a partial */
                             /* backward only its queries' rows of grad_q: zero-fill them and sum over the ranks. */
    int table_rows;          /* L the packed rel-pos indices of relp were clamped to (pass 2): the attention launchers */
                             /* reject tables with any other row count (ABI version 2) */
    int max_queries;         /* the max_queries the plan was cut with in pass 1 (0 = uncut): sizes the kernels' query tiles */
    const int *task_list;    /* optional (NULL: all cells / the task_first, task_step share): the cell ids this launch works on, */
    const int *task_count;   /* device [1]: how many of them.  One scene over several ranks with cells assigned by OWNER of */
                             /* their first query (sharding.py, halo exchange): same zero-fill rules as a task_step share. */
} pointops2_cell_plan;
size_t pointops2_cell_plan_workspace_bytes(int N);
void pointops2_cell_plan_count_launcher(int N, int max_queries, const int *s_cluster, const int *s_starts, const int *l_cluster,
                                        const int *ls_starts, int *cell_order, int *qcell, int *cell_desc, int *cell_qstart,
                                        int *cell_kbase, int *cell_pbase, int *cell_perm, int *parent_first, int *counts, void *ws,
                                        size_t ws_bytes);
/* pass 1 in two halves, for a caller that builds beside the stage's sampler: `prepare` needs the two partitions only (cells = points
 * sorted by (small, large) window, their cut into pieces, the parents) and leaves its intermediate arrays in ws, which must stay untouched
 * until `sizes` - which needs the sampled points too (ls_starts) - has run on the same ws. */
void pointops2_cell_plan_prepare_launcher(int N, int max_queries, const int *s_cluster, const int *l_cluster, int *cell_order,
                                          int *parent_first, int *counts, void *ws, size_t ws_bytes);
void pointops2_cell_plan_sizes_launcher(int N, const int *s_cluster, const int *s_starts, const int *l_cluster, const int *ls_starts,
                                        const int *cell_order, int *qcell, int *cell_desc, int *cell_qstart, int *cell_kbase,
                                        int *cell_pbase, int *cell_perm, int *counts, void *ws, size_t ws_bytes);
void pointops2_cell_plan_fill_launcher(int N, const float *xyz, float window, float quant, int L, const int *s_order, const int *ls,
                                       const float *wc, const int *cell_order, const int *qcell, const int *cell_qstart,
                                       const int *cell_desc, const int *cell_kbase, const int *cell_pbase, int *cell_keys, int *kcell,
                                       unsigned int *relp);
/* Swin3D variant (model/swin3d_transformer.py:149-154: vanilla windows, no sampled keys, tables of L = 2 * qgl - 1 rows with
 * qgl = int(window / quant)).  The rel-pos index of a pair is q[index_0] - q[index_1] + qgl - 1 with q the per-point quantised in-window
 * coordinate ((xyz - min + shift) % window) // quant in torch's fp32 arithmetic: `quant` writes q [N,3] for the plain (shifted = 0) or
 * the shifted pattern (bbox6: pointops2_bbox_launcher), `pairs_rel` the rel_idx [M,3] of a pair list, `cell_fill` is pass 2 of a cell
 * plan (pointops2_cell_plan_fill_launcher: same arrays, same layout and flag rule) with the indices clamped to [0, L). */
void pointops2_swin_quant_launcher(int N, const float *xyz, const float *bbox6, float window, float quant, int shifted, int *q);
void pointops2_swin_pairs_rel_launcher(int N, int M, const int *index_0, const int *index_1, const int *q, int qgl, int *rel_idx);
void pointops2_swin_cell_fill_launcher(int N, int L, int qgl, const int *q, const int *s_order, const int *ls, const float *wc,
                                       const int *cell_order, const int *qcell, const int *cell_qstart, const int *cell_desc,
                                       const int *cell_kbase, const int *cell_pbase, int *cell_keys, int *kcell, unsigned int *relp);
/* The whole operator sequence of WindowAttention.forward (:183-208) on a cell plan, d = 16.  q, k, v [N,h,16]; tables [L,h,16,3];
 * out [N,h,16] fully written; pbuf [h, P] receives the softmax weights in tile order (kept for the backward); ml [N,h,2] is
 * scratch (running max / sum of rows longer than one register chunk). */
void cell_attention_forward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *q, const float *k,
                                     const float *v, const float *table_q, const float *table_k, const float *table_v, float *out,
                                     float *ml, float *pbuf);
/* Its backward.  out / pbuf = the forward's; gsbuf [h, P] scratch (receives the logit gradients in tile order); grad_q fully
 * written; grad_k, grad_v and the three table gradients are ACCUMULATED (zero-fill them).  L <= 80.
 * Both launchers record an error (pointops2_last_error) unless L == plan->table_rows. */
void cell_attention_backward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const float *q,
                                      const float *k, const float *v, const float *out, const float *table_q, const float *table_k,
                                      const float *table_v, const float *pbuf, float *gsbuf, float *grad_q, float *grad_k,
                                      float *grad_v, float *grad_table_q, float *grad_table_k, float *grad_table_v);
/* Which forward kernel cell_attention_forward_launcher (bf16 = 0) or cell_attention_forward_bf16_launcher (bf16 != 0) runs for these
 * arguments: the launchers take their decision from this function.  Reads the plan's host fields only (n_points, n_pairs,
 * n_keyslots, table_rows); not a launch.  fp32 with L <= 80 runs on the matrix cores unless n_points * h >= 96000 and the cells
 * average fewer than 15 queries (n_pairs / n_keyslots < 15); bf16 storage always takes the VALU kernels. */
#define POINTOPS2_CELL_FWD_ERROR   (-1) /* the launcher records an error (d != 16, L < 1, L != plan->table_rows, L > 160) */
#define POINTOPS2_CELL_FWD_NONE    0    /* no plan or no points: the launcher does nothing */
#define POINTOPS2_CELL_FWD_MFMA64  1    /* matrix-core forward, table image of 64 rows (fp32, L <= 64) */
#define POINTOPS2_CELL_FWD_MFMA80  2    /* matrix-core forward, table image of 80 rows (fp32, 64 < L <= 80) */
#define POINTOPS2_CELL_FWD_VALU80  3    /* VALU forward, table image of 80 rows (L <= 80) */
#define POINTOPS2_CELL_FWD_VALU160 4    /* VALU forward, table image of 160 rows (80 < L <= 160, forward only) */
int pointops2_cell_forward_variant(const pointops2_cell_plan *plan, int h, int hdim, int L, int bf16);

/* ---- the data-side step in front of the path ----
 * voxel keys of util/voxelize.py:46-59,79-84 (floor(coord / voxel), the FNV-style 64-bit hash of the three cells) and the
 * crop distances of util/data_util.py:188-191 (squared distance to the seed point), in the coordinates' own precision
 * (is_f64: coord / dist are double arrays, else float). */
void pointops2_voxel_keys_launcher(int N, int is_f64, const void *coord, double voxel, unsigned long long *keys);
void pointops2_crop_dist_launcher(int N, int is_f64, const void *coord, int seed, void *dist);

/* The same two entry points with q / k / v / tables STORED as bf16 (raw 16-bit patterns; BASELINE config 3's second leg).
 * Arithmetic, outputs (out, pbuf) and all gradients stay fp32: the reference's operators are fp32-only
 * (model/stratified_transformer.py:183,194,208 cast every operand with .float()), so this is an extension whose parity
 * target is "the fp32 path on the bf16-rounded operands" (identical up to summation order). */
void cell_attention_forward_bf16_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const uint16_t *q, const uint16_t *k,
                                          const uint16_t *v, const uint16_t *table_q, const uint16_t *table_k, const uint16_t *table_v,
                                          float *out, float *ml, float *pbuf);
void cell_attention_backward_bf16_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const uint16_t *q,
                                           const uint16_t *k, const uint16_t *v, const float *out, const uint16_t *table_q,
                                           const uint16_t *table_k, const uint16_t *table_v, const float *pbuf, float *gsbuf, float *grad_q,
                                           float *grad_k, float *grad_v, float *grad_table_q, float *grad_table_k, float *grad_table_v);
/* The same on the PACKED projection (ABI version 5): qkv [N, 3, h, 16] contiguous as the model's qkv Linear returns it (:180), read in
 * place - point i's q, k, v rows of head t start at element i * 3 * h * 16 + {0, 1, 2} * h * 16 + t * 16.  row_type is the storage
 * type of qkv: fp32, IEEE half or bf16 (raw 16-bit patterns; what the Linear yields under autocast); the tables are fp32 and so are
 * the arithmetic (on exactly widened operands), out, ml, pbuf and every gradient.  q is scaled as it is loaded:
 * q' = round_to_row_type(float(q) * scale), which is `query * self.scale` (:181) bit for bit.  The forward kernel is the one
 * pointops2_cell_forward_variant(plan, h, hdim, L, 0) names.  Backward: grad_qkv [N, 3, h, 16] fp32 receives scale * dL/dq' (written
 * for every query of the launch's cells) and dL/dk, dL/dv (ACCUMULATED); zero-fill it and the three table gradients.
 * Errors as the unpacked launchers record them, and for a row_type that is none of the three. */
#define POINTOPS2_ROWS_F32  0
#define POINTOPS2_ROWS_F16  1
#define POINTOPS2_ROWS_BF16 2
void cell_attention_qkv_forward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const void *qkv, int row_type, float scale,
                                         const float *table_q, const float *table_k, const float *table_v, float *out, float *ml, float *pbuf);
void cell_attention_qkv_backward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const void *qkv, int row_type,
                                          float scale, const float *out, const float *table_q, const float *table_k, const float *table_v,
                                          const float *pbuf, float *gsbuf, float *grad_qkv, float *grad_table_q, float *grad_table_k,
                                          float *grad_table_v);

/* ---- deterministic backward of the cell attention: no float atomics, the same bits from run to run ----
 * The three backward launchers above add dK, dV and the table gradients across workgroups with float atomics, in the order the
 * workgroups arrive.  The three below take the same arguments, compute the same sums and fix their order: a store pass, then a sum
 * pass per destination, as separate launches (no tickets or flags between workgroups).
 *   1  the sweeps store a chunk's key-side rows to key_partials [2, K, h, 16] fp32 (K = plan->n_keyslots; plane 0: dK, plane 1: dV) at
 *      slot cell_kbase[cell] + (position of the key in the cell's list): every slot of every cell is written exactly once
 *   2  the table bodies run on a grid of R = pointops2_cell_table_partial_rows(plan, h) workgroups per body and head; each stores its
 *      whole image of L * 48 sums, zeros included, to table_partials [3 = q, k, v][R][h][L * 48] fp32
 *   3  cell_key_grads_reduce_launcher:   grad[i, :] = ((0 + partials[order[a]]) + partials[order[a + 1]]) + ... over
 *      a .. b - 1 = slot_offsets[i] .. slot_offsets[i + 1] - 1 IN THAT ORDER, fp32; a point without a slot gets 0.  grad: n rows of h * 16
 *      floats, row_stride floats apart (h * 16, or 3 * h * 16 for the k / v third of a packed [N, 3, h, 16] gradient: pass the third's
 *      first row); partials [K, h, 16]; every row of grad is written
 *   4  cell_table_grads_reduce_launcher: grad_table[x] = ((0 + p[0][x]) + p[1][x]) + ... over the partial_rows images IN ASCENDING
 *      ORDER, fp32, for the three tables [L, h, 16, 3] in one launch; every element is written
 * slot_offsets [N + 1], slot_order [K]: the key-major view of plan->cell_keys - per point its key slots, ascending (pointops2_csc_build
 * on index0_offsets = 0 .. K, index1 = cell_keys).  grad_q as in the launchers above; grad_k, grad_v (the k and v thirds of grad_qkv)
 * and the table gradients are fully WRITTEN, not accumulated: no zero-fill, and none of the partial buffers (sizes in floats; the
 * composites check them).  Errors, nothing enqueued: those of the launchers above; a plan that is a share of the cells (task_step > 1
 * or a task_list: the ranks' sums would meet in an all-reduce of no fixed order); a NULL operand; a partial buffer that is too small.
 * Reproducible for one build of the library on one device model: R follows the device's CU count (not the CUs free at the moment of
 * the launch, as the grids of the launchers above), so another device groups the table sums differently. */
int pointops2_cell_table_partial_rows(const pointops2_cell_plan *plan, int h);
void cell_key_grads_reduce_launcher(int n, int h, const int *slot_offsets, const int *slot_order, const float *partials, float *grad, int row_stride);
void cell_table_grads_reduce_launcher(int partial_rows, int h, int L, const float *table_partials, float *grad_table_q, float *grad_table_k,
                                      float *grad_table_v);
void cell_attention_det_backward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const float *q, const float *k,
                                          const float *v, const float *out, const float *table_q, const float *table_k, const float *table_v,
                                          const float *pbuf, float *gsbuf, float *grad_q, float *grad_k, float *grad_v, float *grad_table_q,
                                          float *grad_table_k, float *grad_table_v, const int *slot_offsets, const int *slot_order, float *key_partials,
                                          size_t key_partial_floats, float *table_partials, size_t table_partial_floats);
void cell_attention_det_backward_bf16_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const uint16_t *q,
                                               const uint16_t *k, const uint16_t *v, const float *out, const uint16_t *table_q, const uint16_t *table_k,
                                               const uint16_t *table_v, const float *pbuf, float *gsbuf, float *grad_q, float *grad_k, float *grad_v,
                                               float *grad_table_q, float *grad_table_k, float *grad_table_v, const int *slot_offsets,
                                               const int *slot_order, float *key_partials, size_t key_partial_floats, float *table_partials,
                                               size_t table_partial_floats);
void cell_attention_qkv_det_backward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const void *qkv, int row_type,
                                              float scale, const float *out, const float *table_q, const float *table_k, const float *table_v,
                                              const float *pbuf, float *gsbuf, float *grad_qkv, float *grad_table_q, float *grad_table_k,
                                              float *grad_table_v, const int *slot_offsets, const int *slot_order, float *key_partials,
                                              size_t key_partial_floats, float *table_partials, size_t table_partial_floats);

/* ---- KPConv stem (model/stratified_transformer.py:344-392: KPConvLayer of torch_points3d 1.3.0, rigid kernel points, linear
 * influence, sum aggregation; third party, not under the reference: PARITY UNPINNED) ----
 * With j = neighbors[i, n] (a j outside [0, n_s) - the -1 padding of a ball query, or n_s, the original's shadow point - is skipped):
 *   w[i,k,n]  = max(0, 1 - |(support_xyz[j] - query_xyz[i]) - k_points[k]| / extent)
 *   forward:  wf[i,k,:]      = sum_n w[i,k,n] * feat[j,:]              wf [n_q, n_kp, c] fully written, no atomics (bitwise reproducible)
 *   backward: grad_feat[j,:] += sum_k w[i,k,n] * grad_wf[i,k,:]        grad_feat [n_s, c] ACCUMULATES (zero-fill it); w is recomputed
 * query_xyz [n_q,3], support_xyz [n_s,3], neighbors [n_q,n_nb] int32, feat [n_s,c], k_points [n_kp,3].  The layer's output is
 * wf [n_q, n_kp*c] @ weight [n_kp*c, out]: a matrix product the caller does.  1 <= c <= 64, 1 <= n_nb <= 64, 1 <= n_kp <= 32 and
 * extent > 0, otherwise an error is recorded and nothing is launched. */
void kpconv_aggregate_forward_launcher(int n_q, int n_s, int n_nb, int c, int n_kp, const float *query_xyz, const float *support_xyz,
                                       const int *neighbors, const float *feat, const float *k_points, float extent, float *wf);
void kpconv_aggregate_backward_launcher(int n_q, int n_s, int n_nb, int c, int n_kp, const float *query_xyz, const float *support_xyz,
                                        const int *neighbors, const float *k_points, float extent, const float *grad_wf,
                                        float *grad_feat);

/* ---- grouped max pooling: the tail of TransitionDown (model/stratified_transformer.py:106-109).  LayerNorm and the bias-free Linear
 * act on one row at a time, so pooling linear(norm(feats[knn])) over the k gathered copies is pooling y = linear(norm(feats)) ----
 *   forward:  out[i,ch] = max_n feat[idx[i,n], ch]; arg[i,ch] = the smallest n that attains it (nn.MaxPool1d's rule: first maximum,
 *             a NaN among the k values gives NaN, arg then the n of the first NaN).  An idx entry outside [0, n_s) is skipped and never
 *             read; a row with no valid entry gives 0 and arg = 255, which carries no gradient.  The maximum is a selection: exact in
 *             every row type.  out [m,c] (row_type) and arg [m,c] are fully written; arg may be NULL (no backward wanted).
 *   backward: grad_feat[j,ch] = sum over the pairs (i,n) with idx[i,n] == j and arg[i,ch] == n of grad_out[i,ch], gathered by source
 *             row through the key-major view of idx: src_offsets [n_s+1] / src_pair [m*k] are what pointops2_csc_build yields for the
 *             CSR offsets = {0, k, 2k, ...}, index1 = idx with launch_opts.key_rows = n_s (pair id = i * k + n, ascending per source
 *             row; idx entries outside [0, n_s) must be kept out of that build - key them to an extra row n_s).  fp32 accumulation in
 *             pair order, one rounding to the row type; grad_feat [n_s,c] (row_type) is FULLY WRITTEN: no float atomics, no zero-fill,
 *             bitwise reproducible.  Offsets and pair ids are clamped / skipped, never followed outside the arrays.
 * feat [n_s,c], grad_out [m,c]: row_type = POINTOPS2_ROWS_F32, _F16 or _BF16 (the Linear in front yields half under autocast); idx
 * [m,k] int32.  1 <= k <= 64, 1 <= c <= 1024 and m * k < 2^31, otherwise an error is recorded and nothing is launched; m = 0 or
 * n_s = 0 is a no-op.  Rows of whole 16-byte chunks (c % 4 == 0 for fp32, c % 8 == 0 for the halves) of 16-byte aligned operands take
 * the chunked kernels, anything else one thread per element: same results. */
void grouped_max_forward_launcher(int m, int n_s, int k, int c, int row_type, const void *feat, const int *idx, void *out,
                                  unsigned char *arg);
void grouped_max_backward_launcher(int m, int n_s, int k, int c, int row_type, const void *grad_out, const unsigned char *arg,
                                   const int *src_offsets, const int *src_pair, void *grad_feat);

/* ---- gather-add: the decoder's Upsample behind its kNN search (model/stratified_transformer.py:341): the weighted sum of k source rows
 * (lib/pointops2/functions/pointops.py:767-769) and the add of the support row, in one pass (csrc/upsample.hip) ----
 *   forward:  t = 0; for i = 0 .. k-1: t = t + (float(feat[idx[n,i], ch]) * weight[n,i]);  out[n,ch] = float(base[n,ch]) + t (base
 *             NULL: out = t).  Each product is rounded, then each add; nothing is contracted to an FMA: the reference's loop and its
 *             `+`, operation for operation.  An idx entry outside [0, m) is skipped and never read.  out [n,c] fp32 is FULLY WRITTEN:
 *             no zero-fill.
 *   backward: grad_feat[j,ch] = sum over the pairs (n,i) with idx[n,i] == j of (grad_out[n,ch] * weight[n,i]), gathered by source row
 *             through the key-major view of idx: src_offsets [m+1] / src_pair [n*k] are what pointops2_csc_build yields for the CSR
 *             offsets = {0, k, 2k, ...}, index1 = idx with launch_opts.key_rows = m (pair id = n * k + i, ascending per source row;
 *             idx entries outside [0, m) must be kept out of that build - key them to an extra row m).  fp32 accumulation from 0 in
 *             pair order, each product rounded before its add, one rounding to feat's row type; grad_feat [m,c] (feat_type) is FULLY
 *             WRITTEN, a source row nobody references gets exact zeros: no float atomics, no zero-fill, bitwise reproducible.
 *             Offsets and pair ids are clamped / skipped, never followed outside the arrays.  base's gradient is grad_out itself.
 * feat [m,c]: feat_type, base [n,c]: base_type, each POINTOPS2_ROWS_F32, _F16 or _BF16 independently of the other (the two Linears
 * in front yield half under autocast), widened exactly; base_type is not read when base is NULL.  idx [n,k] int32; weight [n,k],
 * out and grad_out [n,c] fp32.  1 <= k <= 64, 1 <= c <= 1024 and n * k < 2^31, otherwise an error is recorded and nothing is
 * launched.  n = 0 is a no-op of the forward, m = 0 of the backward; with m = 0 the forward writes base (or zeros), with n = 0 the
 * backward writes zeros.  Rows of whole 16-byte chunks of feat (c % 4 == 0 for fp32, c % 8 == 0 for the halves) on aligned operands
 * (feat, out, grad_out, grad_feat and an fp32 base to 16 bytes, a half base to 8) take the chunked kernels, anything else one thread
 * per element: same bits. */
void gather_add_forward_launcher(int n, int m, int k, int c, int feat_type, int base_type, const void *feat, const int *idx,
                                 const float *weight, const void *base, float *out);
void gather_add_backward_launcher(int n, int m, int k, int c, int feat_type, const float *grad_out, const float *weight,
                                  const int *src_offsets, const int *src_pair, void *grad_feat);

/* ---- residual add + DropPath row scale + LayerNorm in one pass over the rows: the glue of a pre-norm block
 * (model/stratified_transformer.py:245-246 and the next block's :241; model/swin3d_transformer.py:206-210) ----
 *   forward:  z[n,ch] = x[n,ch] + s[n] * y[n,ch] (s NULL: x + y; y NULL: x), s * y rounded before the add;
 *             o[n,ch] = ((z - mean_n) * rstd_n) * gamma[ch] + beta[ch], mean_n and the biased var_n by two passes over the row,
 *             rstd_n = 1 / sqrt(var_n + eps); stat[n] = (mean_n, rstd_n).  z may be NULL (not wanted: with y NULL it is x).
 *   backward: xhat = (z - mean) * rstd, g = grad_o * gamma, dz = rstd * ((g - mean_ch(g)) - xhat * mean_ch(g * xhat)) + grad_z;
 *             grad_x = dz, grad_y = s[n] * dz (NULL: not wanted), grad_gamma[ch] = sum_n grad_o * xhat, grad_beta[ch] = sum_n grad_o.
 *             grad_o or grad_z may be NULL (a zero gradient).  grad_x [n,c] and grad_y [n,c] are FULLY WRITTEN.  The two parameter
 *             gradients take no float atomics: workgroup b writes its rows' sums to partials[b] (partials: fp32 [partial_rows, 2, c],
 *             a workspace, no zero-fill; the grid is at most partial_rows workgroups) and a second kernel adds them in a fixed order:
 *             bitwise reproducible on one device.  partials NULL: grad_gamma / grad_beta are not computed.
 * x, z, grad_x, grad_z [n,c], gamma, beta [c], s [n], stat [n,2]: fp32.  y / grad_y have y_type and o / grad_o have o_type, each
 * POINTOPS2_ROWS_F32, _F16 or _BF16, widened exactly, arithmetic in fp32 without fused operations, one rounding to the row type.
 * 1 <= c <= 1024 and the row types are checked: otherwise an error is recorded and nothing is launched; n = 0 is a no-op; offsets
 * are 64-bit, so n * c is bounded by n alone.  c % 4 == 0 with operands aligned for 16-byte (fp32) / 8-byte (half) accesses takes
 * four channels per lane, anything else one channel per lane: same results.  A NaN or Inf stays in its row. */
void residual_norm_forward_launcher(int n, int c, int y_type, int o_type, const float *x, const void *y, const float *s, const float *gamma,
                                    const float *beta, float eps, float *z, void *o, float *stat);
void residual_norm_backward_launcher(int n, int c, int y_type, int o_type, const void *grad_o, const float *grad_z, const float *z,
                                     const float *stat, const float *s, const float *gamma, float *grad_x, void *grad_y, float *partials,
                                     int partial_rows, float *grad_gamma, float *grad_beta);

/* ---- BatchNorm1d over the rows + activation (+ residual add): the per-row glue of the stem and the heads
 * (model/stratified_transformer.py:358, :367-368 with :391, :426-443) ----
 *   stats:    per channel over the n rows, mean = sum x / n and M2 = sum (x - mean)^2, by shifted sums per lane and Chan's merge of
 *             (count, mean, M2) in a fixed tree - never E[x^2] - mean^2; stat [2,c] = (mean, rstd = 1 / sqrt(M2 / n + eps)).  Workgroup b
 *             writes its rows' moments to partials[b] (fp32 [partial_rows, 3, c], a workspace, no zero-fill; the grid is at most
 *             partial_rows workgroups); the kernel that merges them also updates the running statistics where they are not NULL:
 *             running_mean = (1 - momentum) * running_mean + momentum * mean, running_var likewise with M2 / (n - 1) (torch's rule).
 *   forward:  pre = ((x - mean[ch]) * rstd[ch]) * gamma[ch] + beta[ch], o = act(pre) (+ residual, NULL: none).  mean / scale [c]: the two
 *             rows of stat, or with scale_is_var != 0 a mean and a variance (eval mode: the running statistics; rstd = 1 / sqrt(scale +
 *             eps) is taken per lane); stat_out [2,c] (NULL: not wanted) receives (mean, rstd) as used.  o [n,c] is FULLY WRITTEN.
 *             act: POINTOPS2_ACT_NONE, _RELU (pre <= 0 ? 0 : pre), _LEAKY_RELU (pre > 0 ? pre : pre * slope) or _TANH.
 *   backward: xhat = (x - mean) * rstd and pre are recomputed from x and stat; g = grad_o * act'(pre) (tanh: 1 - tanh(pre)^2);
 *             grad_gamma[ch] = sum_n g * xhat, grad_beta[ch] = sum_n g: computed when partials is not NULL (fp32 [partial_rows, 2, c], as
 *             above), without float atomics; grad_x (NULL: not wanted; FULLY WRITTEN) = (gamma * rstd) * ((g - grad_beta / n) - xhat *
 *             (grad_gamma / n)) with training != 0 - it reads grad_gamma / grad_beta, which this call or an earlier one computed -
 *             and (g * gamma) * rstd with training == 0 (the statistics did not depend on x).
 * x, o, grad_o, grad_x [n,c] have x_type and residual [n,c] has r_type, each POINTOPS2_ROWS_F32, _F16 or _BF16, widened exactly,
 * arithmetic in fp32 without fused operations, one rounding to the row type.  gamma, beta, mean, scale, the running statistics and the
 * parameter gradients [c], stat [2,c]: fp32.  1 <= c <= 1024, the row types, act and partial_rows in [1, 1024] are checked: otherwise
 * an error is recorded and nothing is launched; n = 0 is a no-op; offsets are 64-bit.  c % 4 == 0 with operands aligned for 16-byte
 * (fp32) / 8-byte (half) accesses takes four channels per lane, anything else one channel per lane: same results.  Bitwise
 * reproducible on one device.  A NaN or Inf stays in its channel. */
#define POINTOPS2_ACT_NONE       0
#define POINTOPS2_ACT_RELU       1
#define POINTOPS2_ACT_LEAKY_RELU 2
#define POINTOPS2_ACT_TANH       3
void batch_norm_act_stats_launcher(int n, int c, int x_type, const void *x, float *partials, int partial_rows, float eps, float momentum,
                                   float *running_mean, float *running_var, float *stat);
void batch_norm_act_forward_launcher(int n, int c, int x_type, int r_type, int act, float slope, const void *x, const float *mean,
                                     const float *scale, int scale_is_var, float eps, const float *gamma, const float *beta,
                                     const void *residual, void *o, float *stat_out);
void batch_norm_act_backward_launcher(int n, int c, int x_type, int act, float slope, int training, const void *x, const void *grad_o,
                                      const float *stat, const float *gamma, const float *beta, float *partials, int partial_rows,
                                      float *grad_gamma, float *grad_beta, void *grad_x);
/* The same norm with the statistics of SEVERAL RANKS' rows (training under SyncBatchNorm).  The caller moves two small arrays between the
 * ranks by an exact gather; everything else stays on the device, nothing is read back.
 *   moments:        row [3,c] = this rank's (count, mean, M2): the pass of `stats` above, its partials merged in the same order.  n = 0
 *                   writes a row of zeros and runs no row pass (x and partials may then be NULL).
 *   merge:          rows [world,3,c], rank r's row at r, are merged by Chan's formula strictly in rank order 0 .. world-1 (a row of count 0
 *                   is skipped); stat [2,c] = (mean, rstd = 1 / sqrt(M2 / N + eps)), total [1] = N, the summed count; the running
 *                   statistics (both or neither) take the update of `stats` with the merged mean and M2 / (N - 1), unless N = 0.  The same
 *                   rows give the same bits on every rank; with world = 1 they are the bits of `stats`.
 *   forward:        batch_norm_act_forward_launcher with the two rows of stat.
 *   local sums:     batch_norm_act_backward_launcher with grad_x = NULL: this rank's (sum g * xhat, sum g) - its parameter gradients.
 *   sync backward:  sums [world,2,c], rank r's (sum g * xhat, sum g) at r, are added in rank order to (S_gx, S_g);
 *                   grad_x (FULLY WRITTEN) = (gamma * rstd) * ((g - S_g / N) - xhat * (S_gx / N)) with N = total[0] read on the device.
 *                   n = 0 is a no-op.
 * 1 <= world <= 1024.  Counts are fp32 values: exact while N < 2^24 rows. */
void batch_norm_act_moments_launcher(int n, int c, int x_type, const void *x, float *partials, int partial_rows, float *row);
void batch_norm_act_merge_launcher(int world, int c, const float *rows, float eps, float momentum, float *running_mean, float *running_var,
                                   float *stat, float *total);
void batch_norm_act_sync_backward_launcher(int n, int c, int x_type, int act, float slope, const void *x, const void *grad_o, const float *stat,
                                           const float *gamma, const float *beta, int world, const float *sums, const float *total,
                                           void *grad_x);

/* ---- the loss tail of a segmentation training step in one pass: cross-entropy on the class logits, L1 on the shift head, their
 * weighted sum and the per-class IoU counts (tool/train.py:336-362, train_backup.py:403, util/common_util.py:180-185) ----
 * Row n is VALID when 0 <= target[n] < c and target[n] != ignore_index; any other label is never used as an index.
 *   forward:  m_n = max_ch x[n,ch], ls_n = log(sum_ch exp(x[n,ch] - m_n)), stat[n] = (m_n, ls_n) (the row's log-sum-exp is m_n + ls_n:
 *             kept apart, a softmax rebuilt from their fp32 sum would lose digits on rows of large logits);
 *             logp[n,ch] = (x[n,ch] - m_n) - ls_n; loss_n = -logp[n,t] with t = target[n], or for smooth_eps > 0
 *             -((1 - eps) * logp[n,t] + eps / (c - 1) * sum_{ch != t} logp[n,ch]); ce = sum over the valid rows of loss_n / their number
 *             (none: NaN, as torch); l1 = sum |shift_pred - shift| / (3 n) over ALL rows (shift_pred and shift both NULL: 0);
 *             total = ce + offset_weight * l1 (no shift pair: ce); losses = (ce, l1, total), fully written (n = 0: ce and total NaN).
 *             With pred_n = the smallest ch at which x[n,:] is largest (the first NaN if there is one), over the valid rows:
 *             counts[0,k] += #(pred == t == k), counts[1,k] += #(pred == k) + #(t == k) - #(pred == t == k), counts[2,k] += #(t == k);
 *             rows[0] += valid rows, rows[1] += rows whose label is neither valid nor ignore_index.  counts [3,c] and rows [2] ACCUMULATE
 *             by integer atomics (exact, order-free): zero-fill them.
 *   backward: a = g[0] + g[2], b = g[1] + offset_weight * g[2] with g = grad_losses [3] and n_valid = rows[0], both read on the device;
 *             grad_logits[n,ch] = (a / n_valid) * (exp((x[n,ch] - m_n) - ls_n) - w[n,ch]) on valid rows (w: 1 at t; smoothed: 1 - eps at
 *             t, eps / (c - 1) elsewhere) and 0 on every other row; grad_shift_pred[n,j] = (b / (3 n)) * sign(shift_pred - shift),
 *             sign(0) = 0.  Both are FULLY WRITTEN; either may be NULL (not wanted).
 * logits / grad_logits [n,c] have logits_type and shift_pred / grad_shift_pred [n,3] have shift_type, each POINTOPS2_ROWS_F32, _F16 or
 * _BF16, widened exactly, arithmetic in fp32 without fused operations, one rounding to the row type (a loss scale in grad_losses is
 * applied before it).  target [n] int64, shift [n,3] and stat [n,2] fp32.  The two float sums take no float atomics: workgroup b
 * writes its sums as doubles to partials[b] (partials: double [partial_rows, 2], a workspace, no zero-fill; the forward's grid is at
 * most partial_rows workgroups of 256 rows - 128 for c > 32) and a second kernel adds them in a fixed order: bitwise reproducible on
 * one device.  1 <= c <= 64, 0 <= smooth_eps < 1 (> 0 needs c >= 2), the row types, and shift_pred and shift given together are
 * checked: otherwise an error is recorded and nothing is launched.  n = 0 launches no row kernel; offsets are 64-bit.  A 16-byte aligned
 * logits (and grad_logits) is read 16 bytes a lane, anything else one element a lane: same results.  A NaN or Inf in a row stays in
 * that row's stat and gradient and reaches only the scalar sums. */
void seg_loss_forward_launcher(int n, int c, int logits_type, int shift_type, const void *logits, const long long *target, const void *shift_pred,
                               const float *shift, long long ignore_index, float smooth_eps, float offset_weight, float *stat, double *partials,
                               int partial_rows, long long *counts, long long *rows, float *losses);
void seg_loss_backward_launcher(int n, int c, int logits_type, int shift_type, const void *logits, const long long *target, const float *stat,
                                const void *shift_pred, const float *shift, const float *grad_losses, const long long *rows,
                                long long ignore_index, float smooth_eps, float offset_weight, void *grad_logits, void *grad_shift_pred);

/* ---- DBSCAN: the clustering behind the model (util/train_utils.py:549-566 runs sklearn.cluster.DBSCAN per predicted class) ----
 * Neighbours: same group and d2 <= eps2[group], in fp32 with d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = xi - xj, no fused operation; a
 * point is its own neighbour.  Core: at least min_samples[group] neighbours.  Clusters: the connected components of the core points,
 * numbered per group by ascending smallest core index; a non-core point takes the smallest cluster number among its core neighbours
 * or -1.  The five steps, in order (stratified_transformer_amd/cluster.py drives them and owns every buffer):
 *   keys:    keys[i] = ((group * nz + cz) * ny + cy) * nx + cx with c? = clamp(floor((x - o?) / cell), 0, n? - 1) taken in double; a
 *            point whose group is outside [0, n_groups) gets INT64_MAX.  cell must exceed every eps by enough that two points the
 *            fp32 test accepts are at most one cell apart (cluster.py: max eps * (1 + 2^-7)); n_groups * nx * ny * nz < 4e18.
 *   prepare: from the caller's ascending sort of the keys (sorted_keys, order: int64 [n]; n_valid = points inside a group, which sort
 *            first): pts [n_valid] = {x, y, z, original index as bits} (16-byte aligned), sorted_group [n_valid], ranges [18, n_valid]
 *            = begin / end in sorted positions of the nine (dy, dz) rows of three x-adjacent cells around every point.
 *   core:    sorted_core [n_valid] and, by original index, core [n] (1 / 0) and parent [n] = own index for a core point, else -1.
 *            Entries of points outside every group are not written: the caller presets core = 0 and parent = -1.
 *   round:   one hook (atomicMin of the smaller label onto parent[larger label], over every core-core neighbour pair whose labels
 *            differ) and one full pointer jump; *changed (device int) = 1 when a hook happened, else 0.  The caller repeats rounds
 *            until it reads 0 and bounds their number; at that point parent[i] is the smallest core index of i's component.
 *   label:   labels[i] for the n_valid points from cluster_of_root [n] (the cluster number of every root index, -1 elsewhere, which
 *            the caller ranks from parent); entries of points outside every group are not written (preset -1).
 * No kernel waits on another thread; ranges and indices are clamped / skipped, never followed outside the arrays.  n = 0 or
 * n_valid = 0 launches nothing. */
void pointops2_dbscan_keys_launcher(int n, int n_groups, const float *xyz, const int *group, double ox, double oy, double oz, double cell,
                                    int nx, int ny, int nz, long long *keys);
void pointops2_dbscan_prepare_launcher(int n, int n_valid, int nx, int ny, int nz, const float *xyz, const long long *sorted_keys,
                                       const long long *order, float *pts, int *sorted_group, int *ranges);
void pointops2_dbscan_core_launcher(int n, int n_valid, const float *pts, const int *sorted_group, const int *ranges, const float *eps2,
                                    const int *min_samples, unsigned char *sorted_core, unsigned char *core, int *parent);
void pointops2_dbscan_round_launcher(int n, int n_valid, const float *pts, const int *sorted_group, const int *ranges, const float *eps2,
                                     const unsigned char *sorted_core, int *parent, int *changed);
void pointops2_dbscan_label_launcher(int n, int n_valid, const float *pts, const int *sorted_group, const int *ranges, const float *eps2,
                                     const unsigned char *sorted_core, const int *parent, const int *cluster_of_root, int *labels);

/* ---- Contacts between labelled point sets: the distance primitive of the grouping behind the clustering (util/train_utils.py:595-714
 * runs one dense cdist per (edge instance, face instance) pair; :251-261 and test.py:311 ask the same with other thresholds) ----
 * Over the points with a label in [0, n_labels), in fp32 with d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = xp - xq, no fused operation:
 *   count [n_labels, n_labels] (int): count[a, b] = points p of label a for which some q of label b has d2(p, q) < r2 (strict; once per
 *            b however many q are near; p is its own partner, so the diagonal holds the sizes).  The caller zeroes it.
 *   min_d2 [n_labels, n_labels] (float): min over p in a, q in b of d2(p, q).  The caller presets +inf, which an empty label keeps.
 * The two steps are independent (stratified_transformer_amd/cluster.py drives them and owns every buffer):
 *   count: behind pointops2_dbscan_keys_launcher / _prepare_launcher run with ONE group (group 0 = labelled, -1 = not) and a cell of
 *          at least r * (1 + 2^-7): pts and ranges as prepare wrote them, sorted_label [n_valid] = the labels in the same sorted order.
 *          One thread per point walks its nine runs and marks the labels in reach in its own row of bitmap [n_valid, ceil(n_labels / 32)]
 *          (unsigned, zeroed by the caller; not read or written, and may be NULL, for n_labels <= 64: the row stays in registers), then
 *          adds its marks to count with integer atomics.
 *   min:   label_pts [n_valid] = {x, y, z, label as bits} (16-byte aligned) in ASCENDING label order; a tiled sweep over all pairs,
 *          atomicMin on the bit pattern of the non-negative float.  Quadratic in n_valid: callers that need count alone skip it.
 * Both tables are independent of the order in which threads run.  No kernel waits on another workgroup; ranges are clamped and labels
 * outside [0, n_labels) skipped, never followed outside the tables.  n_valid = 0 or n_labels = 0 launches nothing;
 * n_labels * n_labels >= 2^31 records an error. */
void pointops2_contacts_count_launcher(int n_valid, int n_labels, const float *pts, const int *sorted_label, const int *ranges, float r2,
                                       unsigned *bitmap, int *count);
void pointops2_contacts_min_launcher(int n_valid, int n_labels, const float *label_pts, float *min_d2);

/* ---- Boxes and reach rows of labelled point sets: what the OBB merging behind the grouping (test.py:294-326, test_iou.py:373-406: one
 * trimesh box per set and one dense cdist per pair of sets, every rotation) needs of the points ----
 * Over the points with a label in [0, n_labels); the two steps are independent (stratified_transformer_amd/cluster.py drives them and
 * owns every buffer; the merge loop itself runs on the host from one read-back of their results):
 *   label_boxes: xyz [n, 3] float and label [n] in any order.  lo / hi [n_labels, 3] (float) = componentwise minimum / maximum of the
 *          points of every label, size [n_labels] (int) = their number.  The caller presets lo = +inf, hi = -inf, size = 0; a label
 *          without a point keeps them, and a further call on the same arrays accumulates.  Minimum and maximum are signed integer atomics
 *          on an order-preserving image of the fp32 value (the bit pattern, its 31 low bits inverted for a negative value); -0.0 is taken
 *          as +0.0, so results are to be compared by value.  Coordinates must not be NaN.  Up to 1024 labels every workgroup keeps a
 *          private table in LDS and flushes the entries it touched; above that the atomics go to global memory.  Same result either way.
 *   reach_rows: behind pointops2_dbscan_keys_launcher / _prepare_launcher run with ONE group (group 0 = labelled, -1 = not) and a cell of
 *          at least r * (1 + 2^-7): pts and ranges as prepare wrote them, sorted_label [n_valid] = the labels in the same sorted order.
 *          rows [n_valid, ceil(n_labels / 32)] (unsigned), in that sorted order: bit b of row p is set when some point q of label b
 *          has d2(p, q) < r2 (strict), in fp32 with d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = xp - xq, no fused operation - the test of
 *          pointops2_contacts_count_launcher - and the bit of p's OWN label is cleared.  For n_labels <= 64 the row is built in registers
 *          and every row is written (a point whose label is outside the range gets zeros); above that the caller zeroes rows and a
 *          thread builds its row in place - no other thread touches it.  Plain stores, no atomics.
 * Both results are independent of the order in which threads run.  No kernel waits on another workgroup; ranges are clamped and labels
 * outside [0, n_labels) skipped, never followed outside the arrays.  n = 0, n_valid = 0 or n_labels = 0 launches nothing; a NULL array
 * records an error. */
void pointops2_label_boxes_launcher(int n, int n_labels, const float *xyz, const int *label, float *lo, float *hi, int *size);
void pointops2_reach_rows_launcher(int n_valid, int n_labels, const float *pts, const int *sorted_label, const int *ranges, float r2,
                                   unsigned *rows);

/* ---- The clean-up of every box support (util/train_utils.py:716-723: Open3D's voxel_down_sample(0.04), then
 * remove_radius_outlier(nb_points = 3, radius = 0.1), per support) ----
 * Per object, independent of every other object (stratified_transformer_amd/cluster.py: clean_supports drives the steps and owns every
 * buffer; the sort between keys and means is the caller's, and it must be STABLE):
 *   keys:  xyz [n, 3] float, object [n] in any order, lo [n_objects, 3] (float) = the componentwise minimum of every object's points, as
 *          pointops2_label_boxes_launcher writes it.  keys [n] (long long) = ((o * nz + vz) * ny + vy) * nx + vx with
 *          v = floor((double(p) - (double(lo[o]) - voxel * 0.5)) / voxel) per axis, in float64 with a true division, clamped to the
 *          axis; a point whose object is outside [0, n_objects) gets the largest key.  The caller chooses nx, ny, nz so that no object
 *          spans more voxels (floor(extent of the scene / voxel) + 2) and n_objects * nx * ny * nz < 2^61.
 *   means: sorted_keys [n] and order [n] (long long) = the keys in ascending order and the stable sort's permutation, the n_valid points of
 *          the objects first; slot [n_valid] (long long) = the number of voxel heads before every sorted position (a position is a head
 *          when its key differs from its predecessor's), n_voxels their total.  The head's thread walks its run: mean [n_voxels, 3]
 *          (float) = the float64 sum of the voxel's points in ascending original index, from 0.0, divided by their number as a double and
 *          rounded once to float; mean_object / mean_size [n_voxels] (int) = the voxel's object and its number of points.  No atomics: the
 *          result does not depend on the order in which threads run.  A run is walked by one thread however long it is.
 *   count: behind pointops2_dbscan_keys_launcher / _prepare_launcher run on the means with group = object and a cell of at least
 *          r * (1 + 2^-7): pts and ranges as prepare wrote them.  keep [n_means] (unsigned char), by ORIGINAL index of the mean: 1 when
 *          the number of means q of the same object with d2(p, q) < r2 (strict; p itself counts) is greater than nb_points, in fp32 with
 *          d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = xp - xq, no fused operation - the test of pointops2_reach_rows_launcher.
 * No kernel waits on another workgroup; ranges are clamped, indices and slots checked, never followed outside the arrays.  n = 0,
 * n_valid = 0, n_voxels = 0 or n_means = 0 launches nothing; a NULL array records an error. */
void pointops2_supports_keys_launcher(int n, int n_objects, const float *xyz, const int *object, const float *lo, double voxel, int nx, int ny,
                                      int nz, long long *keys);
void pointops2_supports_means_launcher(int n, int n_valid, int n_voxels, const float *xyz, const int *object, const long long *sorted_keys,
                                       const long long *order, const long long *slot, float *mean, int *mean_object, int *mean_size);
void pointops2_supports_count_launcher(int n_means, const float *pts, const int *ranges, float r2, int nb_points, unsigned char *keep);

/* ---- Whole-scene evaluation: the crop cover and the vote of the reference's test loop (test_backup.py:238-251, :278-281) ----
 * One crop of a part of n points (stratified_transformer_amd/evaluate.py drives the loop and owns every buffer):
 *   seed_dist: seed = argmin(priority) (float64 [n], non-negative; the LOWEST index among equal values; 0 when every value is a NaN),
 *              found on the device - per-workgroup (value, index) pairs in part_value / part_index (pointops2_evaltile_max_parts()
 *              entries each), reduced again by every workgroup of the distance kernel - and written to *seed (device int64); then
 *              dist[i] = sum over the three axes, left to right, of (coord[i] - coord[seed])^2 in the coordinates' own precision
 *              (is_f64: coord / dist are double arrays, else float), exactly as pointops2_crop_dist_launcher evaluates it.
 *   update:    for crop [voxel_max] int64 (the caller's first voxel_max entries of the stable ascending sort of dist; distinct):
 *              dmax = dist[crop[voxel_max-1]]; priority[crop[j]] += (double)((1 - dist[crop[j]] / dmax)^2), the three operations rounded
 *              one by one in the coordinates' precision; covered[crop[j]] = 1; report[0] += the points newly covered.  When dmax is
 *              not positive (voxel_max points coincide with the seed: the reference divides 0 / 0 and never ends) report[1] = 1 and
 *              NOTHING else is written; an entry of crop outside [0, n) sets report[1] = 2 and is skipped.  report: two device ints the
 *              caller zeroes before the first crop and reads after every crop.
 * Vote: pred[idx[r], :] += softmax(logits[r, :]) for the m rows of one call (logits [m, classes] of row_type POINTOPS2_ROWS_F32, _F16
 * or _BF16, arithmetic fp32, max-subtracted; idx int64 [m]; pred fp32 [n_points, classes]).  When an index repeats inside the call only
 * the row at the LAST position writes (the reference's indexed assignment, as CPU torch evaluates it): stamp (int32 [n_points], preset
 * -1 by the caller) takes the largest row number per point and is back at -1 when the call has run.  An index outside [0, n_points)
 * sets status[0] = 2 (device int) and its row is skipped.  Bitwise reproducible; no [m, classes] temporary.  m = 0 is a no-op.
 * n < 1, voxel_max outside [1, n], n_points < 1, classes outside [1, 64], an unknown row_type or a NULL array record an error and
 * launch nothing.  No kernel waits on another workgroup; no index is followed outside its array.
 * Vote with shifts (the fork's test_iou.py:284-285): pointops2_evaltile_vote_shift_launcher is the vote above with a second accumulator -
 * the row that writes pred[idx[r], :] also does pred_shift[idx[r], 0:3] += float(shift[r, 0:3]) (shift [m, 3] of shift_row_type
 * POINTOPS2_ROWS_F32, _F16 or _BF16, chosen independently of row_type; converted exactly, one fp32 add; pred_shift fp32 [n_points, 3]).
 * One winner per point serves both tensors (the last position, as above); a losing row or a bad index writes to neither.  Every
 * classes in [1, 64] writes all three components.  Same validation, errors, status and stamp contract as the vote; no float atomics. */
int pointops2_evaltile_max_parts(void);
void pointops2_evaltile_seed_dist_launcher(int n, int is_f64, const void *coord, const double *priority, double *part_value, int *part_index,
                                           long long *seed, void *dist);
void pointops2_evaltile_update_launcher(int n, int voxel_max, int is_f64, const void *dist, const long long *crop, double *priority,
                                        unsigned char *covered, int *report);
void pointops2_evaltile_vote_launcher(int m, int classes, int n_points, int row_type, const void *logits, const long long *idx, int *stamp,
                                      float *pred, int *status);
void pointops2_evaltile_vote_shift_launcher(int m, int classes, int n_points, int row_type, const void *logits, int shift_row_type, const void *shift,
                                            const long long *idx, int *stamp, float *pred, float *pred_shift, int *status);

/* ---- Train-time augmentations: the transform chain of util/transform.py on device rows (stratified_transformer_amd/augment.py compiles a
 * Compose into op tapes, makes every random draw and owns every buffer) ----
 * pass: one thread per point of coord [n, 3] (and feat [n, 3] with POINTOPS2_AUGMENT_HAS_FEAT) - float rows, or double rows when in_f64.
 *       The row is widened to double, the thread finds its scene in offset [n_scenes] (cumulative ends, int) and runs the n_ops ops of the
 *       tape - opcodes [n_ops] (int, POINTOPS2_AUGMENT_OP_*), op_ptrs [n_ops][2] (long long: device addresses an op reads, 0 = none),
 *       params [n_scenes][n_ops][POINTOPS2_AUGMENT_PARAMS] (double; [0] = the op's gate for that scene) - in float64, in the reference's
 *       expression order, nothing fused.  With POINTOPS2_AUGMENT_STORE the rows are stored to coord_out / feat_out, rounded once to float,
 *       or as doubles when out_f64 (a workspace; in == out is allowed).  With POINTOPS2_AUGMENT_STATS the pass accumulates, per scene, the
 *       minimum and the maximum of the six columns of its RESULT into stats_out [n_scenes][POINTOPS2_AUGMENT_STAT_WORDS] (long long: six
 *       minima, six maxima, one word of "column held a NaN" bits; preset by the caller to LLONG_MAX, LLONG_MIN, 0): signed integer atomics
 *       on an order-preserving image of the double (the bit pattern, its 63 low bits inverted for a negative value; -0.0 counts as +0.0),
 *       one per wave and column where a wave lies in one scene.  NaNs are left out of the extrema and set the column's bit.  stats_in is
 *       the table the pass in front of this one wrote: FLIP, AUTOCONTRAST read it on the device, a set NaN bit reads as NaN.
 *       Parameters per op, after the gate: ROTATE [1..9] the matrix R row by row (out_j = (p0 R0j + p1 R1j) + p2 R2j), [10] / [11] rotate
 *       coord / feat; SCALE [1]; SHIFT [1..3]; JITTER [1] sigma, [2] clip, ptr 0 = noise [n, 3] double; FEAT_MUL [1]; FLIP [1..3] one flag
 *       per axis; AUTOCONTRAST [1] the blend factor; CHROMA_TRANSLATE [1..3]; CHROMA_JITTER [1] std * 255, ptr 0 = noise [n, 3] double;
 *       HUE_SATURATION [1] hue_val, [2] sat_ratio; ELASTIC [1] magnitude, [2] the scene's first grid value, [3..5] nx, ny, nz, [6] the
 *       scene's first axis value, ptr 0 = the blurred grids (float), ptr 1 = the axes (double: nx, ny, nz ascending node positions).
 *       The three chromatic ops convert feat to 0..255 and back even when their gate is shut, as the reference does.
 * blur: one 3-tap box filter (scipy.ndimage.convolve, mode 'constant', cval 0) along `axis` of the [nx, ny, nz, 3] float grids laid end to
 *       end in `in`: out = float((a[i-1] * w + a[i] * w) + a[i+1] * w) in double, w = double(float(1) / float(3)); desc [n_grids][4]
 *       (long long) = first value, nx, ny, nz of every grid, ascending; total = all values.  in != out.
 * No float atomics: equal inputs give bitwise equal results.  n = 0 / total = 0 launches nothing.  n_scenes outside
 * [1, POINTOPS2_AUGMENT_MAX_SCENES], n_ops above POINTOPS2_AUGMENT_MAX_OPS or a missing array record an error and launch nothing.  No kernel
 * waits on another workgroup; scene, interval and node indices are clamped into their arrays. */
#define POINTOPS2_AUGMENT_PARAMS 16
#define POINTOPS2_AUGMENT_MAX_SCENES 1024
#define POINTOPS2_AUGMENT_MAX_OPS 32
#define POINTOPS2_AUGMENT_STAT_WORDS 13
#define POINTOPS2_AUGMENT_HAS_FEAT 1
#define POINTOPS2_AUGMENT_STORE 2
#define POINTOPS2_AUGMENT_STATS 4
#define POINTOPS2_AUGMENT_OP_NOP 0
#define POINTOPS2_AUGMENT_OP_ROTATE 1
#define POINTOPS2_AUGMENT_OP_SCALE 2
#define POINTOPS2_AUGMENT_OP_SHIFT 3
#define POINTOPS2_AUGMENT_OP_JITTER 4
#define POINTOPS2_AUGMENT_OP_FEAT_MUL 5
#define POINTOPS2_AUGMENT_OP_FLIP 6
#define POINTOPS2_AUGMENT_OP_AUTOCONTRAST 7
#define POINTOPS2_AUGMENT_OP_CHROMA_TRANSLATE 8
#define POINTOPS2_AUGMENT_OP_CHROMA_JITTER 9
#define POINTOPS2_AUGMENT_OP_HUE_SATURATION 10
#define POINTOPS2_AUGMENT_OP_ELASTIC 11
void pointops2_augment_pass_launcher(int n, int n_scenes, int n_ops, int in_f64, int out_f64, int flags, const void *coord_in,
                                     const void *feat_in, void *coord_out, void *feat_out, const int *offset, const int *opcodes,
                                     const long long *op_ptrs, const double *params, const long long *stats_in, long long *stats_out);
void pointops2_augment_blur_launcher(long long total, int n_grids, int axis, const long long *desc, const float *in, float *out);

/* ---- The optimizer step: the loss scaler's finite check and torch.optim.AdamW's update (amsgrad = False, maximize = False) of every
 * parameter tensor in one call (stratified_transformer_amd/optim.py; csrc/optim.hip states the arithmetic and its order) ----
 * host_table: HOST memory, n_tensors pointops2_optim_tensor followed at once by n_groups pointops2_optim_group.  The launcher checks it,
 *       fills every first_chunk (the prefix sum of ceil(numel / POINTOPS2_OPTIM_CHUNK)) and copies it to `workspace` on the stream.  In
 *       page-locked memory the copy is asynchronous: the caller leaves the table alone until the stream has passed this call (from pageable
 *       memory the runtime stages the copy before it returns, and may wait for the stream to do so).
 * workspace: device memory, at least pointops2_optim_workspace_bytes(n_tensors, n_groups) bytes, 16-byte aligned, the caller's until the
 *       stream has passed this call: the table's copy and one record of bias corrections per tensor.
 * scale: device, 1 float, the loss scale the gradients carry (they are multiplied by float(1.0 / (double)*scale)), or NULL: 1.
 * found_inf: device, 1 float.  run_check != 0: cleared on the stream, then set to 1.0f when any element of any gradient is an infinity
 *       or a NaN.  run_check == 0: the caller's own verdict, only read.  When it is not 0 the call changes nothing else: parameters, moments
 *       and step counts keep their bits.  Otherwise every tensor's *step (1 float, device) advances by one.
 * All pointers inside the table are device pointers of fp32 arrays of numel elements, at any 4-byte alignment; the tensors must not overlap.
 * At most 4 launches and one copy whatever n_tensors is; no device-to-host copy and no synchronisation.  Recorded as errors, nothing
 * enqueued: a negative n_tensors or n_groups, a numel outside [0, 2^31), a group outside [0, n_groups), a NULL pointer, a short workspace. */
#define POINTOPS2_OPTIM_CHUNK 4096
typedef struct pointops2_optim_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    float *step;
    long long numel;
    int group;
    int first_chunk; /* written by the launcher */
} pointops2_optim_tensor;
typedef struct pointops2_optim_group {
    double lr, beta1, beta2, eps, weight_decay;
} pointops2_optim_group;
size_t pointops2_optim_workspace_bytes(int n_tensors, int n_groups);
void optim_adamw_step_launcher(int n_tensors, int n_groups, void *host_table, void *workspace, size_t workspace_bytes, const float *scale,
                               float *found_inf, int run_check);
/* The general step: optim_adamw_step_launcher is optim_step_launcher(POINTOPS2_OPTIM_ADAMW, ..., 0.0, NULL).
 * kind: POINTOPS2_OPTIM_ADAMW, or POINTOPS2_OPTIM_SGD: torch.optim.SGD's update (dampening = 0, maximize = False) over the same two structs:
 *       exp_avg is the momentum buffer (zeros before the first step; may be NULL when the group's momentum is 0), exp_avg_sq and step are
 *       NULL and unused; in the group beta1 is the momentum, beta2 is 1.0 for Nesterov and 0.0 otherwise, eps is unused.
 * max_norm, grad_norm: max_norm > 0 with a grad_norm (device, 1 float) clips by the global 2-norm as torch.nn.utils.clip_grad_norm_ does:
 *       *grad_norm = the norm of all the table's gradients after the unscale, summed in float64 in a fixed order (csrc/optim.hip) inside the
 *       finite check's read, and every gradient enters its update multiplied by float(min(1.0, max_norm / (norm + 1e-6))).  The gradients
 *       themselves are not written.  max_norm <= 0 or grad_norm == NULL: no clipping, *grad_norm is not touched.
 * workspace: with clipping at least pointops2_optim_step_workspace_bytes(n_tensors, n_groups, n_chunks) bytes, n_chunks = the sum of
 *       ceil(numel / POINTOPS2_OPTIM_CHUNK) over the table (one float64 partial per chunk); without it the size above is enough.
 * At most 4 launches and one copy without clipping and 5 with it; no device-to-host copy and no synchronisation.  Recorded as errors,
 * nothing enqueued: what optim_adamw_step_launcher refuses (for SGD the NULL rule above), an unknown kind, a NaN max_norm, max_norm > 0 with
 * a workspace short of the size with n_chunks. */
#define POINTOPS2_OPTIM_ADAMW 0
#define POINTOPS2_OPTIM_SGD 1
size_t pointops2_optim_step_workspace_bytes(int n_tensors, int n_groups, long long n_chunks);
void optim_step_launcher(int kind, int n_tensors, int n_groups, void *host_table, void *workspace, size_t workspace_bytes, const float *scale,
                         float *found_inf, int run_check, double max_norm, float *grad_norm);

/* ---- residual add + DropPath row scale + LayerNorm on a residual stream of any row type: residual_norm_*_launcher above with the stream
 * operands x, z, grad_x and grad_z of x_type (POINTOPS2_ROWS_F32, _F16 or _BF16) - under autocast every stage behind a TransitionDown
 * carries a half stream.  residual_norm_*_launcher is this pair with x_type = POINTOPS2_ROWS_F32: the same bits.  For a 16-bit x_type:
 *   forward:  x and y are widened exactly, p = fp32(s[n] * y) (s NULL: y), z32 = fp32(x + p), z = z32 rounded ONCE to x_type.  mean_n,
 *             var_n, stat and o are computed from the STORED z widened back, not from z32: o is the LayerNorm of the tensor the caller
 *             holds, which the backward reads again.  y NULL: z is x; nothing is rounded, and z (if not NULL) receives a copy of x.
 *   backward: dz as above, in fp32, from the widened stored z, stat, grad_o and the exactly widened grad_z; grad_x = dz rounded to
 *             x_type and grad_y = s[n] * dz rounded to y_type, both from the unrounded dz; grad_gamma and grad_beta stay fp32.
 * Validation, NULL rules, partials, the 64-bit offsets and the n = 0 no-op are those of the fp32 pair, with x_type checked like the other
 * two row types.  Four channels per lane need c % 4 == 0 and every [n,c] operand aligned for its own type (16 bytes fp32, 8 bytes
 * half); anything else takes one channel per lane: same results. */
void residual_norm_stream_forward_launcher(int n, int c, int x_type, int y_type, int o_type, const void *x, const void *y, const float *s,
                                           const float *gamma, const float *beta, float eps, void *z, void *o, float *stat);
void residual_norm_stream_backward_launcher(int n, int c, int x_type, int y_type, int o_type, const void *grad_o, const void *grad_z,
                                            const void *z, const float *stat, const float *s, const float *gamma, void *grad_x, void *grad_y,
                                            float *partials, int partial_rows, float *grad_gamma, float *grad_beta);

/* ---- the parameter gradients of a Linear layer over point rows (csrc/linear_grads.hip): with x [n, in] the layer's input and
 * g [n, out] the gradient of its output, both row-contiguous and each of its own row type (POINTOPS2_ROWS_F32, _F16 or _BF16, widened
 * exactly),
 *   grad_weight[o, i] = sum_n g[n, o] * x[n, i]        grad_bias[o] = sum_n g[n, o]
 * in fp32 on the matrix cores (v_mfma_f32_16x16x4_f32: per element a chain of fp32 fused multiply-adds in ascending row order), from
 * ONE read of x and g.  The rows are cut into G = pointops2_linear_grads_partial_rows(n, in, out) chunks of POINTOPS2_LINEAR_GRADS_ROWS
 * rows - a function of n alone (1 for n == 0; 0 for arguments out of range) - and the work is two launches:
 *   linear_grads_partial_launcher: chunk c writes its sums to block c of partials [G][out][in + 1] (caller-allocated fp32; column `in`
 *       of a row is the bias partial).  Every element of every block is written; rows behind n and columns behind in / out enter the
 *       products as zeros.  partial_rows must be G.
 *   linear_grads_reduce_launcher: grad_weight [out, in] and, with has_bias != 0, grad_bias [out] = the sum of the partial_rows blocks in
 *       ascending chunk order.  Both are fully written (n == 0: zeros); has_bias == 0: grad_bias is not touched and may be NULL.
 * No float atomics: the same operands give the same bits on every run, wherever they lie.  1 <= in, out <= 1536, n >= 0.  Recorded as
 * errors, nothing enqueued: a shape or row type out of range, a partial_rows other than G (partial) or < 1 (reduce), a NULL operand. */
#define POINTOPS2_LINEAR_GRADS_ROWS 512
int pointops2_linear_grads_partial_rows(int n, int in, int out);
void linear_grads_partial_launcher(int n, int in, int out, int x_type, int g_type, const void *x, const void *g, float *partials,
                                   int partial_rows);
void linear_grads_reduce_launcher(int in, int out, int has_bias, const float *partials, int partial_rows, float *grad_weight,
                                  float *grad_bias);

#ifdef __cplusplus
}
#endif
#endif /* POINTOPS2_HIP_H */
