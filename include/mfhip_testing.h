/*
 * mfhip_testing.h -- test hooks of libmfhip.so.  NOT part of the product surface (mfhip.h):
 * the test suite and tools/ use these to check the device schedules' invariants on a CPU
 * machine and to name the kernels in profiles.  The Scala/JNI drop-in never binds them.
 */
#ifndef MFHIP_TESTING_H
#define MFHIP_TESTING_H

#include "mfhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Testing hooks (host only, no GPU): expose the device schedules so their invariants can be
   checked on a CPU machine.
   mf_debug_levels: dependency level of each update of a sequence visited in `order`
   (order may be NULL = identity); rows are caller indices.
   mf_debug_fast_schedule: for every input rating, the rating block (ub*n+ib), rotation
   sub-step, item group and position inside its cell of the fast-mode plan with `groups`
   groups per rating block (groups < 0: the systolic sweep's per-block choice for a budget of
   -groups waves per superstep, as mf_dsgd_prepare makes it with MFHIP_TEST=sys_waves=-groups for
   rank k: the group model's constants depend on the row width, plan.hpp sys_cell_ns /
   sys_run_pair_ns), MF_BLOCKING_* `blocking` and hazard window `window` (0: 8). */
int mf_debug_levels(const uint32_t* urow, const uint32_t* irow, const int32_t* order, int64_t n,
                    int32_t* level_out);
int mf_debug_fast_schedule(const int32_t* users, const int32_t* items, int64_t n, int32_t n_blocks,
                           int64_t seed, int32_t groups, int32_t blocking, int32_t window, int32_t k,
                           int32_t* block_out, int32_t* substep_out, int32_t* group_out, int64_t* pos_out);
/* mf_debug_fast_split: mf_debug_fast_schedule with hot-item replicas (the MFHIP_ITEM_SPLIT
   experiment, item_split ratings per chain); replica_out[j] = 0 when rating j updates its item's own row, r >= 1 when it
   updates replica r (merged when the superstep ends). */
int mf_debug_fast_split(const int32_t* users, const int32_t* items, int64_t n, int32_t n_blocks,
                        int64_t seed, int32_t groups, int32_t blocking, int32_t window, int32_t k, int32_t item_split,
                        int32_t* block_out, int32_t* substep_out, int32_t* group_out, int64_t* pos_out,
                        int32_t* replica_out);
/* mf_debug_ring_schedule: the item-block ring step ring_shift runs after superstep `superstep`
   (1-based) on rank `rank` of `world` with n blocks (n = c * world): the item block it sends
   (*out_blk) to rank *dst and the one it receives (*in_blk) from rank *src -- nextRatingBlock
   (DSGDforMF.scala:611-619) over ranks. */
int mf_debug_ring_schedule(int32_t rank, int32_t world, int32_t n_blocks, int64_t superstep, int32_t* out_blk,
                           int32_t* in_blk, int32_t* dst, int32_t* src);
/* mf_debug_det_slot_table: the split deterministic sweep's slot table (det_slot_table) for nw waves
   {begin, count, flags} (flags bit 0: every entry of the wave updates one item), at most max_blocks
   co-resident blocks of two slots, `alone` != 0: the longest single-item chains on CUs of their own,
   blocks b and b + period sharing a CU.  The *_out arrays have room for 4 * nw + 4 slots;
   *nslots_out = the slots written.  MF_ERR_INVALID when the work needs more than max_blocks blocks. */
int mf_debug_det_slot_table(const int64_t* begin, const int32_t* count, const int32_t* flags, int64_t nw,
                            int64_t max_blocks, int32_t alone, int64_t period, int64_t* begin_out, int32_t* count_out,
                            int32_t* flags_out, int64_t* nslots_out);
/* mf_debug_sys_placement: the block -> wave map of one systolic fast-sweep launch of nw waves with
   modelled times load[0 .. nw), when `cap` blocks can be resident at once and the `iso` (0..8)
   heaviest waves of every XCD are to be alone on their CUs: *pad_out = the empty blocks per XCD
   (sys_iso_pad; 0 for iso = 0), place_out[b] = the wave of block b or -1 for an empty block, nw +
   8 * *pad_out entries (room for nw + 24 * iso), checked to hold every wave exactly once. */
int mf_debug_sys_placement(const double* load, int64_t nw, int64_t cap, int32_t iso, int32_t* pad_out,
                           int32_t* place_out);
/* mf_debug_plan_digest: after mf_dsgd_prepare of a fast-mode fit on one shard, an FNV-1a digest
   of the device schedule -- the pair records, the wave table and (systolic) the per-wave cell
   tables -- and the pair-record count: out[0] = digest, out[1] = records.  Compares the device-
   built plan (kernels_plan.hip) with the host-built one (MFHIP_TEST=device_plan=0). */
int mf_debug_plan_digest(mf_ctx* ctx, uint64_t out[2]);
/* The plan window (records between two uses of a row inside a cell unless adjacent) the fast
   sweep uses at rank k: the prefetch distance of the kernel selected for k. */
int mf_fast_plan_window(int32_t k, int32_t* window_out);
/* Name of the fast-mode sweep kernel used at rank k (for profiles and bench reports). */
const char* mf_fast_kernel_name(int32_t k);
/* Build flags: bit 0 = built with -DMFHIP_EXPERIMENTS (hot-item replicas, wave traces and the
   other experiment switches exist; the default build has none of them). */
int32_t mf_debug_build_flags(void);
/* Device memory this process holds through the library: out[0] = live bytes, out[1] = the
   high-water mark since the library was loaded (rank rehearsals report it per rank). */
int mf_debug_device_bytes(int64_t out[2]);
/* mf_debug_als_normal_eq: after mf_als_prepare, the system an ALS half-sweep would solve for `id` of
   `side` from the current factors: A_out[k * k] = sum q q^T + lambda' I (full symmetric, row-major)
   and b_out[k] = sum r q, as the device accumulates them -- through the sweep's own kernels, the
   chunked path of a long row included -- widened to f64.  The factors are not changed.
   MF_ERR_INVALID for an id that is unknown or has no rating in the prepared data. */
int mf_debug_als_normal_eq(mf_ctx* ctx, int side, int32_t id, double lambda, int32_t reg, double* A_out,
                           double* b_out);
/* mf_debug_als_gram: after mf_als_prepare, G_out[k * k] = sum of y y^T over the rows of `side` that
   have a rating in the prepared data, from the current factors, through the implicit half-sweep's
   own two launches (k_als_gram and its reduction), widened to f64.
   mf_debug_als_normal_eq_implicit: as mf_debug_als_normal_eq for the system mf_als_run_implicit
   would solve: A_out = G + sum w q q^T + lambda' I, b_out = sum_{r > 0} (1 + w) q.  A row with no
   positive rating reports its system (b_out zero); the half-sweep sets that row to zero unsolved. */
int mf_debug_als_gram(mf_ctx* ctx, int side, double* G_out);
int mf_debug_als_normal_eq_implicit(mf_ctx* ctx, int side, int32_t id, double lambda, int32_t reg, double alpha,
                                    double* A_out, double* b_out);
/* mf_debug_als_cg_matvec: after mf_als_prepare, for `id` of `side` and a vector v[k]: Av_out[k] = A v and
   b_out[k] = b of the system mf_als_run_cg (alpha < 0) or mf_als_run_implicit_cg (alpha >= 0) iterates
   on, from the current factors, through the half-sweep's own kernels -- the row's vectors staged in
   LDS, gathered again in every pass (MFHIP_TEST als_cg_stage=0, or a row past the LDS budget) or the
   chunked path of a long row -- in the order mfhip.h documents, widened to f64.  Fast contexts round v
   to f32.  The factors are not changed.  MF_ERR_INVALID as for mf_debug_als_normal_eq.
   mf_debug_als_cg_capacity: the most ratings of a row whose vectors are staged at this context's rank
   and precision. */
int mf_debug_als_cg_matvec(mf_ctx* ctx, int side, int32_t id, double lambda, int32_t reg, double alpha,
                           const double* v, double* Av_out, double* b_out);
int mf_debug_als_cg_capacity(mf_ctx* ctx, int32_t* ratings_out);
/* mf_debug_als_nnls_row: after mf_als_prepare, the row mf_als_run_nonneg (alpha < 0) or
   mf_als_run_implicit_nonneg (alpha >= 0) would store for `id` of `side` from the current factors, solved
   through the half-sweep's own kernels -- the chunked path of a long row included -- and widened to f64:
   x_out[k], *iters_out = the row's iteration count, *reason_out = its reason code (mfhip.h).  An implicit
   row with no positive rating is solved here (b = 0: x = +0, 0 iterations, reason 0), which is what the
   half-sweep stores for it unsolved.  Neither the factors nor mf_als_nonneg_stats change.
   MF_ERR_INVALID as for mf_debug_als_normal_eq. */
int mf_debug_als_nnls_row(mf_ctx* ctx, int side, int32_t id, double lambda, int32_t reg, double alpha,
                          double* x_out, int32_t* iters_out, int32_t* reason_out);
/* mf_debug_rank_csr: the pair table mf_rank_eval builds on the device for one pair list, copied back.
   The evaluated queries are the distinct ids of query[] the model holds on query_side, in ascending
   factor-row order: q_ids_out[*nq_out].  off_out[*nq_out + 1] and entries_out[*ne_out] are the table:
   per query its distinct entries, ascending.  ground_truth = 0, the exclusion table: an entry is the
   candidate's factor row (what the selection kernels read), pairs with an unknown candidate are
   dropped.  ground_truth = 1: an entry is the candidate id, unknown candidates kept.  *nq_out and
   *ne_out are always set; MF_ERR_CAPACITY when cap_q < *nq_out or cap_e < *ne_out (nothing else is
   written then). */
int mf_debug_rank_csr(mf_ctx* ctx, int query_side, int ground_truth, const int32_t* query, const int32_t* cand,
                      int64_t n, int32_t* q_ids_out, int64_t* off_out, int32_t* entries_out, int64_t cap_q,
                      int64_t cap_e, int64_t* nq_out, int64_t* ne_out);
/* mf_debug_als_csr: after mf_als_prepare, the resident CSR of `side` copied back in row order.  *rows_out =
   the rows it covers (those the side had at the last mf_als_prepare / mf_als_append), *nnz_out = its entries;
   off_out[*rows_out + 1], cols_out[*nnz_out] = the counterpart's factor rows, vals_out[*nnz_out] = the ratings
   widened to f64, npos_out[*rows_out] = per row its ratings > 0 (the n+ of its work items).  *rows_out and
   *nnz_out are always set; MF_ERR_CAPACITY when cap_rows < *rows_out or cap_nnz < *nnz_out (nothing else is
   written then). */
int mf_debug_als_csr(mf_ctx* ctx, int side, int64_t* off_out, int32_t* cols_out, double* vals_out,
                     int32_t* npos_out, int64_t cap_rows, int64_t cap_nnz, int64_t* rows_out, int64_t* nnz_out);
/* mf_debug_als_append_placement: the rule mf_als_append's kernels follow, on the host (no GPU needed).  For
   a side with offsets old_off[old_rows + 1] and a batch whose entry j belongs to row batch_row[j] < new_rows
   (new_rows >= old_rows): new_off_out[new_rows + 1], and batch_pos_out[j] = where entry j lands in the new
   arrays.  An old entry p of row x lands at p + new_off_out[x] - old_off[x].  mf_als_append itself uses only
   the new_off half of this routine; its kernels place the batch entries from the sorted batch, and that is
   checked through mf_debug_als_csr on the device. */
int mf_debug_als_append_placement(const int64_t* old_off, int64_t old_rows, const int32_t* batch_row, int64_t n,
                                  int64_t new_rows, int64_t* new_off_out, int64_t* batch_pos_out);
/* mf_debug_als_remove_select: the rule mf_als_remove's kernels follow, on the host in plain C++ (no GPU
   needed).  For one side's CSR off[rows + 1] / cols[off[rows]] and a batch whose entry j names the pair
   (batch_row[j] < rows, batch_col[j]): in ascending j, entry j takes the oldest remaining instance of its pair,
   the first position of the row that holds batch_col[j] and that no earlier entry took.  pos_out[j] = that
   position in cols[], or -1 for a miss.  MF_ERR_INVALID: off[0] != 0, descending offsets, a batch row outside
   [0, rows), a negative count or a NULL array that would be read. */
int mf_debug_als_remove_select(const int64_t* off, int64_t rows, const int32_t* cols, const int32_t* batch_row,
                               const int32_t* batch_col, int64_t n, int64_t* pos_out);
/* mf_debug_seen_csr: the resident seen set's table of `side` copied back (MF_SIDE_ITEM: the item-major table,
   built here if it is not there, as an item query would).  *rows_out = the rows `side` holds now, *nnz_out =
   the distinct pairs held; row_ids_out[*rows_out] = the id of every factor row, off_out[*rows_out + 1] and
   entries_out[*nnz_out] = the table as the readers see it, padded to the present rows: per factor row its
   distinct counterpart factor rows, ascending; entry_ids_out (may be NULL) = the ids of those counterpart
   rows.  No set reads as an empty one.  *rows_out and *nnz_out are always set; MF_ERR_CAPACITY when cap_rows <
   *rows_out or cap_nnz < *nnz_out (nothing else is written then). */
int mf_debug_seen_csr(mf_ctx* ctx, int side, int32_t* row_ids_out, int64_t* off_out, int32_t* entries_out,
                      int32_t* entry_ids_out, int64_t cap_rows, int64_t cap_nnz, int64_t* rows_out, int64_t* nnz_out);
/* mf_debug_seen_merge_placement: the rule mf_seen_add's kernels follow, on the host (no GPU needed).  Keys are
   (row << 32) | counterpart row.  old_keys[n_old]: the table's keys, distinct and ascending; batch_keys[n_batch]:
   a batch in any order, duplicates allowed.  With `novel` the distinct batch keys the table does not hold, in
   ascending order (*n_novel_out of them): old_pos_out[p] = p + #(novel keys < old_keys[p]) and novel_pos_out[i]
   = i + #(old keys < novel[i]), the positions in the merged arrays; novel_pos_out has room for n_batch. */
int mf_debug_seen_merge_placement(const uint64_t* old_keys, int64_t n_old, const uint64_t* batch_keys, int64_t n_batch,
                                  int64_t* old_pos_out, int64_t* novel_pos_out, int64_t* n_novel_out);
/* mf_debug_bpr_triples: the triples of the last step mf_bpr_run or mf_bpr_step_triples ran on the device, as
   factor rows, copied back: *n_out = its slots, users_out / pos_out / neg_out [*n_out] = the slot's rows, -1 in
   all three for a void slot.  A call with steps == 0 changes nothing here: an earlier step's triples stay.  A call
   on an empty set or with pool == 1 runs no kernel and leaves none.  MF_ERR_STATE when there are none;
   MF_ERR_CAPACITY when cap < *n_out (only *n_out is written). */
int mf_debug_bpr_triples(mf_ctx* ctx, int32_t* users_out, int32_t* pos_out, int32_t* neg_out, int64_t cap,
                         int64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* MFHIP_TESTING_H */
