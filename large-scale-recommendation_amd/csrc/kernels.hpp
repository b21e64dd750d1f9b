// kernels.hpp -- host-side launch wrappers of the HIP kernels, grouped by the kernel file that
// defines them (kernels_*.hip).  All launches are asynchronous on the given stream.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <type_traits>

#include "plan.hpp"

namespace mfhip {

// ---- kernels_det.hip: level replay, ticket sweep, evaluation, initial rows ----------------------
// Update arithmetic of one replayed rating.
enum class Arith : int {
  kDsgd = 0,     // DSGDforMF.updateLocalFactors body (:405-413), regularised
  kSgdNext = 1,  // SGDUpdater.nextFactors (core/FactorUpdater.scala:37-45)
};

// Deterministic replay of one dependency level: one wave per entry, sequential dot.
// T = double (bit-exact) or float (fast-mode online).  eta = learning rate of the superstep
// (kDsgd) or SGDUpdater's learningRate (kSgdNext).
void launch_level(hipStream_t st, const DetEntry* entries, int64_t n, void* U, void* I,
                  const void* regU, const void* regI, int k, double eta, Arith arith, bool f64);
// Online micro-batch as one persistent launch (k_online_sweep, kernels_det.hip): wave w applies
// entries [wbeg[w], wbeg[w+1]) (the updates of its items, in sequence order), each after its
// user's ticket reaches useq; tickets (one int32 per user row) start at 0.  Every wave must be
// resident: nw <= online_sweep_capacity(k, f64).
int online_sweep_capacity(int k, bool f64);
void launch_online_sweep(hipStream_t st, int nw, const int64_t* wbeg, const DetEntry* ent, const uint32_t* useq,
                         void* U, void* I, int k, double eta, bool f64, int32_t* ticket, int32_t* err);
// Per-rating records of the online operators (mf_online_update_out), f64 rows of k at
// [src[entry] * k]: kOutNext = (user', item') (FlinkOnlineMF.scala:131-135), kOutDelta =
// (user + deltaItem, deltaItem) with user before the update (PSOfflineOnlineMF.scala:174-176).
enum class OnlineOut : int { kNone = 0, kOutNext = 1, kOutDelta = 2 };
void launch_level_out(hipStream_t st, const DetEntry* entries, int64_t n, void* U, void* I, int k, double eta, bool f64,
                      OnlineOut mode, const int32_t* src, double* uout, double* iout);
// Gather-dot over resolved pairs (row -1 = unknown id).  out[j] = p.q summed left to right in
// f64 (predictRating's ddot).  When r != nullptr every workgroup writes partials[3*wg + c]:
//   c=0: sum (r - p.q)^2, c=1: matched count, c=2: sum mult*((r-p.q)^2 + lambda*(p.p + q.q)).
// The grid has predict_grid(n) workgroups; the host adds the partials in a fixed order.
int predict_grid(int64_t n);
void launch_predict(hipStream_t st, const int32_t* urow, const int32_t* irow, int64_t n,
                    const void* U, const void* I, int k, bool f64, double* out, const double* r,
                    const int32_t* mult, double lambda, double* partials);
// Initial factor rows on the device (DSGDforMF.scala:548-549, MatrixFactorization.scala:278-280):
// row x, factor f = the f-th nextDouble of new Random(ids[x] ^ seed) (xor_seed) or of
// new Random(ids[x]).  One thread per element: the JVM LCG state after m steps is
// jump[2(m-1)] * s0 + jump[2(m-1)+1] mod 2^48 (host table, m = 1..2k), so every element is
// computed independently and written coalesced; bit-exact with JavaRandom::nextDouble.
// out: rows x k, double (f64) or float (rounded from the same double).
void launch_jvm_init_rows(hipStream_t st, const int32_t* ids, int64_t rows, int k, bool xor_seed, int64_t seed,
                          const uint64_t* jump, void* out, bool f64);

// ---- kernels_detsweep.hip: the deterministic f64 sweep, one launch per superstep ----------------
// Deterministic persistent sweep (kernels_detsweep.hip): one launch per superstep, nw waves of
// 64 lanes, all of which must be resident at once (nw <= det_sweep_capacity(k)).  Entries are
// build_det_step's SoA arrays; ticket: one int32 per user row, zero before the launch; err[0]
// set when a wave gave up waiting.  ev0 / ev1 (may be null): dispatch-recorded timing events.
int det_sweep_capacity(int k);
// Entry arrays are read in 64-entry chunks up to 192 entries past a wave's end (kDetPad slack).
// u_bytes / i_bytes: slab sizes (< 4 GiB, 32-bit row offsets); dummy_ticket: 16 scratch words
// per wave (nw * 16 int32).
constexpr int64_t kDetPad = 256;
void launch_det_sweep(hipStream_t st, const DetWave* waves, int nw, const uint32_t* eu, const uint32_t* ei,
                      const uint32_t* eq, const double* er, double* U, double* I, uint64_t u_bytes, uint64_t i_bytes,
                      const double* regU, const double* regI, int k, double eta, int32_t* ticket,
                      int32_t* dummy_ticket, int32_t* err, hipEvent_t ev0, hipEvent_t ev1);

// Split single-item chains (k = 64, 128, 256; kernels_detsweep.hip k_det_sweep_split): blocks of
// two wave slots, slots[2b + w] for wave w (nslots even, nslots / 2 blocks, all resident at once:
// nslots <= det_split_capacity(k), counted in wave slots; 0 = k not supported).  A block whose
// slot 0 is a single-item wave runs it as a chain wave plus a helper wave (slot 1 ignored, by
// convention kDetWaveHelper); any other slot is an ordinary k_det_sweep2 wave (count 0: none).
int det_split_capacity(int k);
// The same split sweep with SGDUpdater.nextFactors' update (the online f64 batch, no lambda /
// omega); k = 64, 128, 256 (capacity 0 otherwise).
int online_det_capacity(int k);
void launch_online_det(hipStream_t st, const DetWave* slots, int nslots, const uint32_t* eu, const uint32_t* ei,
                       const uint32_t* eq, const double* er, double* U, double* I, uint64_t u_bytes, uint64_t i_bytes,
                       int k, double eta, int32_t* ticket, int32_t* err, hipEvent_t ev0, hipEvent_t ev1);
void launch_det_sweep_split(hipStream_t st, const DetWave* slots, int nslots, const uint32_t* eu, const uint32_t* ei,
                            const uint32_t* eq, const double* er, double* U, double* I, uint64_t u_bytes,
                            uint64_t i_bytes, const double* regU, const double* regI, int k, double eta,
                            int32_t* ticket, int32_t* err, hipEvent_t ev0, hipEvent_t ev1);

// ---- kernels_online_sweep.hip: the f32 online batch, one launch ---------------------------------
// The f32 batch at k <= 256 (k_online_f32, kernels_online_sweep.hip): the same plan and tickets,
// rows and tickets pipelined two updates deep, the dot product of online_f32.hpp (the f32 level
// replay's).  dummy_ticket: 16 int32 per wave of scratch.  skip (may be null): the launch does
// nothing when *skip != 0 (read on the device).  ev0 / ev1 (may be null) time the launch.
bool online_f32_supports(int k);
int online_f32_capacity(int k);
void launch_online_f32(hipStream_t st, int nw, const int64_t* wbeg, const DetEntry* ent, const uint32_t* useq, float* U,
                       float* I, uint64_t u_bytes, uint64_t i_bytes, int k, double eta, int32_t* ticket,
                       int32_t* dummy_ticket, int32_t* err, int nsingle, const int32_t* skip, hipEvent_t ev0,
                       hipEvent_t ev1);

// ---- kernels_online.hip: the sweeps' inputs built on the device ---------------------------------
// k_online_sweep's inputs from one batch in sequence order (eu / ei / er: user row, item row,
// rating of update x; device arrays), on the device (kernels_online.hip): ent / useq (n each,
// grouped by wave = item row mod W, sequence order inside a wave, useq = the update's rank among
// its user's updates) and wbeg (W + 1); touched[0..1] = distinct user / item rows of the batch.
// user_rows / item_rows bound eu / ei.  erf non-null: the ratings are floats there (the f32
// sweep's upload) and er is not read.
struct OnlineSweepScratch;
// Returns H: waves [0, H) hold one item each (the heavy items), the others any number.
uint32_t online_sweep_plan(hipStream_t st, OnlineSweepScratch& sc, const uint32_t* eu, const uint32_t* ei,
                           const double* er, int64_t n, uint32_t W, uint32_t user_rows, uint32_t item_rows,
                           DetEntry* ent, uint32_t* useq, int64_t* wbeg, int32_t* touched,
                           const float* erf = nullptr);
// The online batch's id -> row lookup on the device, over a mirror of the host IdIndex (same
// hash, same slots; id_index.hpp): in[0, n) user ids and in[n, 2n) item ids (the batch as
// uploaded) are replaced by their rows, kRowMiss where the table has no such id; *misses counts
// those (the host then gives the unseen ids rows in first-touch order).  A null table: all misses.
void launch_id_lookup(hipStream_t st, uint32_t* in, int64_t n, const void* uslots, uint64_t umask, const void* islots,
                      uint64_t imask, int32_t* misses);
// The same lookup for one array of ids against one table, n of any size (launch_id_lookup's grid reaches 2^24
// entries: an online batch; mf_recommend_among sends whole candidate lists): in[0, n) replaced by rows or kRowMiss.
void launch_id_lookup_one(hipStream_t st, uint32_t* in, int64_t n, const void* slots, uint64_t mask);
// slots[pos[j]] = vals[j] (8-B slots): the mirror takes the host table's writes since its last sync
void launch_id_scatter(hipStream_t st, void* slots, const uint32_t* pos, const void* vals, int64_t m);

// ---- kernels_negsample.hip: the sampled online batch ---------------------------------------------
// mf_online_update_sampled's expansion (kernels_negsample.hip): pos holds the n_in events as
// launch_id_lookup leaves them (user rows, item rows, ratings -- floats when rf32); out receives the
// N = n_in * (1 + negatives) updates in the same layout, event j's own record followed by its negatives
// (the event's user row, neg_row(seed, first_event + j, s, pool, its item row) of neg_sample.hpp,
// neg_rating), the batch online_sweep_plan takes.  pool: the item rows of the model.  skip (may be
// null): nothing is written when *skip != 0 (the lookup's miss count, read on the device).
void launch_neg_expand(hipStream_t st, const uint32_t* pos, int64_t n_in, int32_t negatives, uint32_t pool,
                       int64_t seed, int64_t first_event, double neg_rating, bool rf32, uint32_t* out,
                       const int32_t* skip);
// The f64 online batch on the deterministic sweep (kernels_detsweep.hip): the plan's entries as
// SoA arrays in sc.soa (eu / ei / eq / er, padded by kDetPad) and one DetWave per wave (single-item
// flag from the entries) into waves[0 .. W).  Call after online_sweep_plan on the same scratch.
void online_det_entries(hipStream_t st, OnlineSweepScratch& sc, const DetEntry* ent, const uint32_t* useq,
                        const int64_t* wbeg, int64_t n, uint32_t W, uint32_t*& eu, uint32_t*& ei, uint32_t*& eq,
                        double*& er, struct DetWave* waves);
// The deterministic sweep's superstep input built on the device (MFHIP_TEST det_build=host: on the
// host, plan.cpp build_det_step -- the same arrays, bit for bit).  One block of the superstep:
struct DetBuildBlock {
  int64_t e0;     // its first entry in the superstep's arrays
  int64_t st;     // its first rating in the device copy of RatingBlocks::det_aos
  int64_t iwoff;  // its item -> wave map in the concatenated maps
  uint32_t i0;    // first global item row of its item block
  uint32_t w0;    // its first wave in the superstep's wave order
};
static_assert(sizeof(DetBuildBlock) == 32, "DetBuildBlock is two 16-B words");
struct DetBuildScratch;
// ord[e0 + j] = the block's j-th rating in shuffle order (position inside the block, from the
// host's JVM shuffle); out = the entries in wave order (a wave's entries in shuffle order) with
// useq = the user's count of earlier ratings in shuffle order: exactly build_det_step's SoA.
// Reserve scratch for up to n_max entries first (det_device_build_reserve; no allocation after).
void det_device_build_reserve(DetBuildScratch& sc, int64_t n_max, uint32_t wave_bound, uint32_t user_rows);
void det_device_build(hipStream_t st, DetBuildScratch& sc, const int32_t* ord, int64_t n, const DetBuildBlock* blocks,
                      int nblk, const DetEntry* aos, const int32_t* item_wave, uint32_t wave_bound,
                      uint32_t user_rows, uint32_t* ou, uint32_t* oi, uint32_t* oq, double* orr);

// ---- kernels_fast.hip: fast-mode sweep, one update per step (every rank) ------------------------
// Fast-mode sweep, one rotation sub-step t for nblk rating blocks of one superstep.
struct FastBlk {
  int64_t rec_base;   // first record of the rating block
  int64_t cell_base;  // its G*G+1 cell offsets in the cell table
};
// Factor slabs are addressed through 32-bit buffer offsets (u_bytes/i_bytes < 4 GiB each).
// dummy_u_off / dummy_i_off: byte offsets of rows that are never written (idle prefetches of
// rows forwarded in registers).
// Cells of at least prio_len records run at raised wave priority (s_setprio 3).
void launch_fast_substep(hipStream_t st, const FastBlk* blks, int nblk, int G, int t, const FastRec* recs,
                         const int32_t* cell_off, float* U, float* I, int k, float eta, uint64_t u_bytes,
                         uint64_t i_bytes, uint32_t dummy_u_off, uint32_t dummy_i_off, int prio_len);

// Fast-mode sweep, one persistent launch per superstep: wave g of a block sweeps its G cells in
// order and waits on wave g+1's progress word before each cell (progress: nblk*G*kProgStride
// int32, zeroed before every launch; err[0] != 0 after a bounded wait timed out).
constexpr int kProgStride = 32;  // one 128-B line per progress word
void launch_fast_superstep(hipStream_t st, const FastBlk* blks, int nblk, int G, const FastRec* recs,
                           const int32_t* cell_off, float* U, float* I, int k, float eta, uint64_t u_bytes,
                           uint64_t i_bytes, uint32_t dummy_u_off, uint32_t dummy_i_off, int32_t* progress,
                           int32_t* err);

// ---- kernels_pair.hip: fast-mode sweep, pair schedule (k = 64, 128, 256) ------------------------
// Fast-mode sweep, pair schedule (kernels_pair.hip): one launch per sub-step, one wave per
// cell, two updates of one item per step (build_pair_plan).  k in {64, 128, 256}; the plan
// window must be >= 2 * pair_ring(pair_kpl(k)) (plan.hpp pair_window).
bool pair_kernel_supports(int k);
// ev0 / ev1 (may be null): start / stop events recorded by the dispatch itself.
void launch_sweep_pair(hipStream_t st, const WaveDesc* waves, int nwaves, const PairRec* recs, float* U, float* I,
                       uint64_t u_bytes, uint64_t i_bytes, int k, float eta, uint64_t* trace, hipEvent_t ev0,
                       hipEvent_t ev1);
// Systolic variant, one launch per superstep: sw = this superstep's PairPlan::sys_waves (nw of
// them, all of which must be resident at once: nw <= sweep_pair_sys_capacity(k)), sys =
// PairPlan::sys.  prog: nw*kProgStride int32 progress words, monotonic across launches (this
// launch writes base+1 .. base+G_j and must advance base by more than the largest G_j);
// err[0] is set when a wave gave up waiting.  trace (may be null): per cell {start, end} at
// [2*(cell index in sys)].
int sweep_pair_sys_capacity(int k);
// lbase: index of sw[0] among the superstep's waves (a superstep may be split over two launches,
// see dsgd_fast.cpp ring overlap); prog and SysWave::nbr count from the superstep's first wave.
// place (may be null): block b of the launch sweeps wave sw[place[b]] (sys_placement, placement.cpp);
// null: the XCD-contiguous map.
void launch_sweep_pair_sys(hipStream_t st, const SysWave* sw, const WaveDesc* sys, int nw, int lbase,
                           const PairRec* recs, float* U, float* I, uint64_t u_bytes, uint64_t i_bytes, int k, float eta,
                           int32_t* prog, uint32_t base, int32_t* err, uint64_t* trace, hipEvent_t ev0, hipEvent_t ev1,
                           const int32_t* place = nullptr);
// Hot-item replicas around a fast superstep (plan.hpp SplitItem): fork before the sweep, join
// after it, on the sweep's stream; n split items, f32 rows of k.
void launch_split_fork(hipStream_t st, const SplitItem* sp, int n, float* I, int k);
void launch_split_join(hipStream_t st, const SplitItem* sp, int n, float* I, int k);

// ---- kernels_block.hip: DSGD blocking -----------------------------------------------------------
// DSGD blocking on the device (kernels_block.hip): both SideLayouts (initFactorBlockAndIndices,
// DSGDforMF.scala:513-588, the reference's seeded blocking) and the rating blocks of user blocks
// [ub_lo, ub_hi) (:301-327; sort_ui: (user, item) order inside a block), bitwise what
// build_side + build_rating_blocks (plan.cpp) produce.  Host arrays in, host structures out.
class DevBuf;
// keep (optional): the rating blocks' device arrays (urow u32, irow u32, r f64, rb order, the
// first rb.start[n*n] entries valid) are handed over instead of freed.
struct DevRatingBlocks;
// host_arrays = false (with keep): rb gets only its block starts; fetch_rating_blocks copies the
// arrays later if a host-side plan needs them.
void device_blocking(hipStream_t st, const int32_t* u, const int32_t* i, const double* r, int64_t n, int32_t nb,
                     int64_t seed, int32_t ub_lo, int32_t ub_hi, bool sort_ui, SideLayout& U, SideLayout& I,
                     RatingBlocks& rb, DevRatingBlocks* keep = nullptr, bool host_arrays = true);

// ---- kernels_plan.hip: the fast schedule --------------------------------------------------------
void fetch_rating_blocks(hipStream_t st, const DevRatingBlocks& dr, RatingBlocks& rb);
// Per rating block (n*n): the rating count of its most rated item, from the device arrays.
std::vector<int64_t> device_block_tops(hipStream_t st, const DevRatingBlocks& dr, const RatingBlocks& rb,
                                       const SideLayout& I);

// The fast pair schedule's per-cell work on the device (kernels_plan.hip): the greedy emission of
// every cell of `work` (build_fast_plan's phase-1 output, blocks in ascending order) and the pair
// records of every wave, bitwise the host build_fast_plan + build_pair_plan.  Fills fp's cell /
// record offsets and pads, pp's tables and stats (pp.recs stays empty) and d_pairs (device).
void device_pair_schedule(hipStream_t st, std::vector<FastBlockWork>& work, FastPlan& fp, int32_t nb, int32_t c,
                          int32_t shard, int32_t k, uint32_t dummy_row, int32_t window, bool substep_waves,
                          PairPlan& pp, DevBuf& d_pairs);
// The whole fast schedule from the device rating blocks (kernels_plan.hip): phase 1 as device
// sorts (cell-major order, spreading) around host LPT groups from device histograms, then the
// emission and pair records as above.  Gb: the rotation groups of every rating block.
void device_fast_schedule(hipStream_t st, const DevRatingBlocks& dr, const RatingBlocks& rb, const SideLayout& U,
                          const SideLayout& I, const std::vector<int32_t>& Gb, double lambda, uint64_t order_seed,
                          FastPlan& fp, int32_t c, int32_t shard, int32_t k, uint32_t dummy_row, int32_t window,
                          PairPlan& pp, DevBuf& d_pairs);

// ---- kernels_recommend.hip: top-N recommendation ------------------------------------------------
// Top-N recommendation (kernels_recommend.hip): for each of the nq query rows qrows[] of slab Q (all
// valid rows) the top_n best of candidate rows [0, C) of slab Cf by p.q, as ids / scores / counts
// ([nq][top_n], [nq]; device).  What one launch takes; a caller sets per batch only what varies per batch.
struct RecLaunch {
  hipStream_t st = nullptr;
  // the query slab and the candidate slab, in the context's precision.  f64: the sequential pq = pq + a*b
  // chain (k_predict's value); f32: the fmaf chain over f = 0..k-1 on the f32-input MFMA.
  const void *Q = nullptr, *Cf = nullptr;
  int k = 0, top_n = 0;
  bool f64 = false;
  const int32_t* cand_id = nullptr;  // row -> id of the candidate side
  // the candidate rows [0, C) are walked in S <= 64 splits; part: nq * S * top_n keys of
  // recommend_key_bytes(f64) scratch.  recommend_query_tile: the queries one workgroup owns (the host sizes S
  // by it).
  int32_t C = 0;
  int S = 1;
  void* part = nullptr;
  // excl_beg / excl_end (nq each) / excl_rows: per query the sorted candidate rows never returned,
  // excl_rows[excl_beg[q], excl_end[q]).  A call's own CSR passes (off, off + 1); the resident seen set passes
  // two arrays gathered from its offsets through qrows (launch_seen_gather).
  const int64_t *excl_beg = nullptr, *excl_end = nullptr;
  const int32_t* excl_rows = nullptr;
  int32_t* ids = nullptr;
  double* scores = nullptr;  // may be null (mf_rank_eval reads only ids and counts)
  int32_t* counts = nullptr;
  // Cosine (mf_similar, mf_recommend_vectors): c_inv given -- one inverse norm per candidate row, q_inv one per
  // row of Q (indexed through qrows like Q), both in the context's precision, as launch_row_inv_norm writes
  // them; a score is then dot * (q_inv * c_inv), scaled before it is selected.  Null: the dot kernels.
  const void *q_inv = nullptr, *c_inv = nullptr;
  // pos_row (mf_recommend_among's shared list; dot metric only): Cf is a slab gathered from the factor rows,
  // cand_id its ids by slab position, and excl_rows still name factor rows -- position p is row pos_row[p].
  // Null: the candidates are factor rows.
  const int32_t* pos_row = nullptr;
};
size_t recommend_key_bytes(bool f64);
int recommend_query_tile(int top_n, bool f64);
void launch_recommend(const RecLaunch& L, const int32_t* qrows, int nq);
// launch_row_inv_norm: inv[r] = 1 / sqrt(sum over ascending f of X[r][f]^2) for rows [0, rows) of X.
void launch_row_inv_norm(hipStream_t st, const void* X, int64_t rows, int k, bool f64, void* inv);

// ---- kernels_among.hip: top N within caller-given candidate lists (mf_recommend_among) ------------
// The shared list as launch_id_lookup_one resolved it (rows[0, n): candidate rows, kRowMiss for an id the side does
// not hold; 0 < n < 2^31) -> its distinct held rows, ascending, into out (room for n); returns their count (one
// small read-back, the stream is drained).  A radix sort, a flag per first occurrence, a scan and a compaction;
// the scratch is sc's, grown by temp_storage's rule.
struct RankScratch;
int64_t among_distinct_rows(hipStream_t st, RankScratch& sc, const uint32_t* rows, int64_t n, int32_t* out);
// dst row p = row rows[p] of slab src (n rows of k elements in the context's precision),
// ids[p] = row_id[rows[p]] -- the compact slab, its ids and (rows itself) the position -> row map that
// launch_recommend takes.
void launch_among_gather(hipStream_t st, const void* src, const int32_t* rows, int64_t n, int k, bool f64,
                         const int32_t* row_id, void* dst, int32_t* ids);
// Per-query lists, one batch of nq positions.  crows: the batch's lists one after the other as launch_id_lookup
// leaves them (candidate rows, kRowMiss for an id the side does not hold).  A task is one part of one position's
// list: entries [beg, beg + len) of crows; the tasks of a position are consecutive, pbeg[q] .. pbeg[q + 1]
// (nq + 1 offsets into tasks, at most 64 per position; none: count 0).  Per position: its query row qrow (a
// valid row of Q for every position that has tasks) and the range excl_beg / excl_end of excl_rows (sorted
// candidate rows) never returned.  Scores, keys, order and the outputs ids / scores (may be null) / counts are
// launch_recommend's; an id named several times in a list counts once.  part: ntasks * top_n keys of
// recommend_key_bytes(f64) scratch.
struct AmongTask {
  int64_t beg;
  int32_t len;
  int32_t pos;  // the position of the batch the part belongs to
};
static_assert(sizeof(AmongTask) == 16, "AmongTask is one 16-B word");
void launch_among(hipStream_t st, const void* Q, const void* Cf, const AmongTask* tasks, int64_t ntasks,
                  const int64_t* pbeg, int nq, const uint32_t* crows, const int32_t* qrow, const int32_t* cand_id,
                  const int64_t* excl_beg, const int64_t* excl_end, const int32_t* excl_rows, int k, int top_n, bool f64,
                  void* part, int32_t* ids, double* scores, int32_t* counts);

// ---- table kernels: what they share (kernels_table.hip, csr_search.hpp, csr_device.hpp) --------
// The table kernels build, merge, search or compact a packed CSR on the device: kernels_rank.hip,
// kernels_seen.hip, kernels_als_append.hip, kernels_als_remove.hip, kernels_foldin.hip, with readers in
// kernels_recommend.hip and kernels_pairrank.hip.  A new one includes csr_search.hpp for its searches (row_of,
// lower, upper, contains), csr_device.hpp when it walks a CSR's entries in tiles (csr_tile, kCsrThreads,
// kCsrTile), takes kRowMiss (id_index.hpp) for "no row", and sizes, fills, sorts and scans with the functions
// below -- it defines none of these again.
//
// grid_for: workgroups of kGridThreads threads for a grid-stride loop over n elements, at least 1, at most cap.
constexpr int kGridThreads = 256;
inline unsigned grid_for(int64_t n, int64_t cap = 1 << 16) {
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n + kGridThreads - 1) / kGridThreads, cap)));
}
// The radix bits that hold every key < v (1 .. 32): the end bit of a sort over rows or waves.
inline int radix_bits_for(uint64_t v) {
  int b = 1;
  while (b < 32 && (uint64_t{1} << b) < v) ++b;
  return b;
}
// out[x] = x, x in [0, n): a sort's payload, and the identity the pair-rank kernels take as qpos with a
// table keyed by row.
void launch_iota(hipStream_t st, int32_t* out, int64_t n);
// The temp storage of a rocprim / hipcub call of `bytes` bytes, kept in buf.  THE RULE: a block that work
// queued on st may still use is never freed under it -- buf grows only after st has drained.  This adds no
// wait to any path: hipFree waits for the device before it frees, and where a caller drains the stream
// between two launches that share a scratch the wait finds nothing queued.  The size query / get storage /
// run pairs of the table kernels take their storage here.
void* temp_storage(hipStream_t st, DevBuf& buf, size_t bytes);
// kout = kin[0, n) sorted over key bits [0, end_bit), stable (rocprim radix sort, SortCfg of
// radix_sort_cfg.hpp), pos[s] = the position in kin of the key at sorted place s; 0 < n < 2^31.  tmp and
// iota (the identity payload) are scratch, grown by the rule above.  K: uint32_t or uint64_t.
template <typename K>
void sort_positions(hipStream_t st, DevBuf& tmp, DevBuf& iota, const K* kin, K* kout, int32_t* pos, int64_t n,
                    int end_bit);
// out[x] = in[0] + .. + in[x - 1], x in [0, n) (rocprim); tmp as above.  T: int32_t or int64_t.
template <typename T>
void scan_exclusive(hipStream_t st, DevBuf& tmp, const T* in, T* out, int64_t n);

// ---- kernels_rank.hip: ranking metrics ----------------------------------------------------------
// The pair tables of mf_rank_eval on the device.  qrow[n]: the query-side row of every pair
// (kRowMiss: unknown id), rows: the rows of that side.
// rank_query_set: the distinct known rows, ascending, into qrows (the list launch_recommend takes);
// returns their count nq (one small read-back) and leaves every row's flag / position in sc.
// rank_pair_csr (after rank_query_set on the same scratch; the pairs may be another list): per
// evaluated query its distinct entries, sorted: off (int64, nq + 1) and ent (room for n).  gt = false:
// cand[] holds candidate rows, pairs with kRowMiss are dropped, ent = rows ascending (launch_recommend's
// excl_off / excl_rows).  gt = true: cand[] holds candidate ids, all kept, ent = ids ascending.
// Pairs whose query is unknown or not in the query set are dropped.
struct RankScratch;
int64_t rank_query_set(hipStream_t st, RankScratch& sc, const uint32_t* qrow, int64_t n, uint32_t rows, DevBuf& qrows);
void rank_pair_csr(hipStream_t st, RankScratch& sc, const uint32_t* qrow, const uint32_t* cand, int64_t n, uint32_t rows,
                   int64_t nq, bool gt, DevBuf& off, DevBuf& ent);
// rank_pair_csr's three steps after its keys, for a caller that forms the keys itself (the resident seen
// set, kernels_seen.hip).  A key is (position << 32) | low with position in [0, nq), or nq << 32 for a
// pair that is dropped.  rank_keys_reserve sizes sc.key / key2 / head / wp for n keys (n < 2^31 - 1); the
// caller writes sc.key[0, n).  rank_keys_sort: sc.key2 = the keys sorted over the bits in use, sc.head[p]
// = 1 where a kept key differs from its predecessor (n + 1 entries, the last 0); a caller may clear
// heads before the next step.  rank_keys_csr: ent = the low part of every head in order, off[q] = the
// heads before position q's first key, q = 0 .. nq; sc.wp is left as the exclusive scan of the heads.
void rank_keys_reserve(RankScratch& sc, int64_t n);
void rank_keys_sort(hipStream_t st, RankScratch& sc, int64_t n, int64_t nq);
void rank_keys_csr(hipStream_t st, RankScratch& sc, int64_t n, int64_t nq, bool gt, int64_t* off, int32_t* ent);
// Per-query metrics of a batch of nb lists (ids [nb][top_n] / counts [nb] as launch_recommend wrote
// them) against the ground-truth rows gt_off[0 .. nb] / gt_ent: met[q][MF_RANK_NMETRICS] and cnt[q][2] =
// (hits, g).  gt_off / met / cnt point at the batch's first query.  tab: 128 gains 1 / log(i + 2), then
// their 129 prefix sums (host libm).
void launch_rank_metrics(hipStream_t st, const int32_t* ids, const int32_t* counts, int nb, int top_n,
                         const int64_t* gt_off, const int32_t* gt_ent, const double* tab, double* met, int64_t* cnt);
// Sums over all nq queries in a fixed order: slices of 1024 queries (a fixed tree inside a slice) into
// part [slices][MF_RANK_NMETRICS] / ipart [slices][2], then the slices in ascending order into sums[6] /
// isums[2].
int64_t rank_reduce_slices(int64_t nq);
void launch_rank_reduce(hipStream_t st, const double* met, const int64_t* cnt, int64_t nq, double* part, int64_t* ipart,
                        double* sums, int64_t* isums);

// ---- kernels_seen.hip: the resident seen set ----------------------------------------------------
// The set's tables are CSRs over a side's factor rows: off (int64, rows + 1) and ent (int32, the distinct
// counterpart rows of a row, ascending) -- per row the shape launch_recommend's excl_rows and the pair-rank
// kernels' exclusion table have.  Keys are (row << 32) | counterpart row; a dropped pair takes rows << 32
// (rank_keys_sort's convention).  All of it is integer work: sort, scan, search and move.
// launch_seen_pair_keys: key[j] of the pair (qrow[j], crow[j]); dropped when qrow[j] >= rows or crow[j] is
// kRowMiss (an unknown id).
void launch_seen_pair_keys(hipStream_t st, const uint32_t* qrow, const uint32_t* crow, int64_t n, uint32_t rows,
                           uint64_t* key);
// launch_seen_csr_keys: key[e] of every entry e of a CSR (off[rows + 1], cols[nnz]), by the tile walk of
// csr_device.hpp.  swap: the key of the other orientation, (col << 32) | row.
void launch_seen_csr_keys(hipStream_t st, const int64_t* off, int64_t rows, int64_t nnz, const int32_t* cols,
                          bool swap, uint64_t* key);
// The merge of a sorted batch into a table (mf_seen_add; the rule mf_debug_seen_merge_placement states).
// launch_seen_novel, after rank_keys_sort of the batch: clears head[p] where the table (old_off[old_rows + 1],
// old_ent) already holds key2[p], and lb[p] = the table's keys below key2[p] for every remaining head.
// launch_seen_merge, after rank_keys_csr of those heads gave the novel keys as a CSR (nov_off[new_rows + 1],
// nov_ent) and wp: new_off[r] = old_off[min(r, old_rows)] + nov_off[r]; an old entry e with key K moves to
// e + #(novel keys < K) (the tile walk over the old entries; the novel range of a tile's first and last key
// found once per workgroup); the novel key at sorted position p lands at wp[p] + lb[p].  No atomics: every
// position follows from the sorted keys alone.
void launch_seen_novel(hipStream_t st, const uint64_t* key2, int32_t* head, int64_t n, const int64_t* old_off,
                       int64_t old_rows, const int32_t* old_ent, int64_t* lb);
void launch_seen_merge(hipStream_t st, const int64_t* old_off, int64_t old_rows, int64_t old_nnz, const int32_t* old_ent,
                       const int64_t* nov_off, const int32_t* nov_ent, int64_t new_rows, const uint64_t* key2,
                       const int32_t* head, const int32_t* wp, const int64_t* lb, int64_t n, int64_t* new_off,
                       int32_t* new_ent);
// off[r] = off[have] for r in (have, want]: rows gained since the table was built hold nothing.
void launch_seen_pad(hipStream_t st, int64_t* off, int64_t have, int64_t want);
// beg[q] = off[qrows[q]], end[q] = off[qrows[q] + 1]: a batch's exclusion ranges for launch_recommend.
void launch_seen_gather(hipStream_t st, const int64_t* off, const int32_t* qrows, int n, int64_t* beg, int64_t* end);

// ---- kernels_pairrank.hip: ranks of given pairs -------------------------------------------------
// The position of pairs (query row, candidate row) in the query's complete ranked list (mf_pair_ranks,
// mf_online_prequential): rank = the candidates whose key (mf_recommend's order) beats the pair's.
// qrow / crow: the factor rows of the n pairs (kRowMiss: unknown id).  qpos: per query-side row its
// position in the exclusion CSR excl_off / excl_rows (rank_query_set's positions, rank_pair_csr's
// table).  Per pair: tord (pair_rank_ord_bytes(f64) each; 0 = not ranked) and tid, the two parts of its
// key; rank (the count, or MF_PAIR_RANK_COLD / MF_PAIR_RANK_EXCLUDED), valid (the list's length) and
// score (the value mf_recommend reports for the pair; 0.0 where not ranked).
// launch_pair_targets fills all five for every pair; launch_pair_count then adds, for pairs [0, n) of
// one batch (the pointers at the batch's first pair), every candidate row of [0, C) that beats the
// target (S splits of the rows, combined with integer atomics) and, with have_excl, takes the query's
// excluded rows that beat it off again.  nw (1, 2, 4): waves per workgroup of the f32 walk;
// pair_rank_tile: the pairs one workgroup owns.
size_t pair_rank_ord_bytes(bool f64);
int pair_rank_tile(bool f64, int nw);
void launch_pair_targets(hipStream_t st, const void* Q, const void* Cf, const uint32_t* qrow, const uint32_t* crow,
                         int64_t n, int32_t C, int k, bool f64, const int32_t* cand_id, const int32_t* qpos,
                         const int64_t* excl_off, const int32_t* excl_rows, void* tord, uint32_t* tid, int32_t* rank,
                         int32_t* valid, double* score);
void launch_pair_count(hipStream_t st, const void* Q, const void* Cf, const uint32_t* qrow, int n, int32_t C, int S,
                       int k, bool f64, int nw, const int32_t* cand_id, const int32_t* qpos, const int64_t* excl_off,
                       const int32_t* excl_rows, bool have_excl, const void* tord, const uint32_t* tid, int32_t* rank);
// Per pair ndcg / rr / pr (columns 0 .. 2 of a met row of MF_RANK_NMETRICS, the rest 0) and cnt[j][2] =
// (hit, evaluated), the rows launch_rank_reduce sums; tab as launch_rank_metrics takes it.
void launch_pair_metrics(hipStream_t st, const int32_t* rank, const int32_t* valid, int64_t n, int top_n,
                         const double* tab, double* met, int64_t* cnt);

// ---- kernels_als.hip: ALS half-sweeps -----------------------------------------------------------
// ALS half-sweep (kernels_als.hip).  A work item is a whole row of the side being solved (slot < 0:
// its system is solved in the kernel and x stored to X[row]) or one chunk of a long row (slot >= 0:
// its partial matrix and right-hand side go to partial[slot], als_partial_elems(k) elements each);
// an AlsSplit names a long row's partials [slot0, slot0 + chunks), added in that order and solved.
constexpr int kAlsMaxRank = 256;
struct AlsItem {
  int64_t begin;  // first rating of the item in cols / vals
  int32_t row;
  int32_t count;  // ratings of the item (of the whole row when slot < 0)
  int32_t slot;
  int32_t npos;   // ratings r > 0 of the whole row (the implicit half-sweep's n+)
};
struct AlsSplit {
  int32_t row, slot0, chunks;
  int32_t count;  // ratings of the whole row (lambda' = lambda * count when weighted)
  int32_t npos;   // of them r > 0
};
struct AlsCgWork {
  int32_t item;   // index into items[]
  int32_t split;  // index into splits[]
};
// What one ALS launch takes (launch_als, launch_als_wide, launch_als_cg).
struct AlsLaunch {
  hipStream_t st = nullptr;
  const AlsItem* items = nullptr;
  int n_items = 0;
  const AlsSplit* splits = nullptr;
  int n_splits = 0;
  // the side's CSR (counterpart rows of Q, ratings in the context's precision)
  const int32_t* cols = nullptr;
  const void* vals = nullptr;
  const void* Q = nullptr;
  void* X = nullptr;
  int k = 0;
  double lambda = 0.0;
  bool weighted = false;  // lambda' = lambda * count (npos in the implicit half-sweep)
  bool f64 = false;
  void* partial = nullptr;
  // dump != null (the testing hook, one row).  Cholesky: the row's k x k matrix and right-hand side are
  // stored there instead of being solved.  Conjugate gradients: dump[0 .. k) = A v and dump[k .. 2k) = b
  // for v = hook_v (device, k elements); X is not written.
  void* dump = nullptr;
  // gram != null: the implicit-feedback half-sweep (mf_als_run_implicit), (G + sum w q q^T + lambda' I) x
  // = sum_{r > 0} (1 + w) q with w = alpha |r|; gram is G, als_gram_elems(k) elements (launch_als_gram),
  // lambda' = lambda * npos when weighted, and a row with npos == 0 is set to zero.
  const void* gram = nullptr;
  double alpha = 0.0;
  // Cholesky at ranks 129..256 (kernels_als_wide.hip).  The normal matrix of a row lives in global
  // memory: slab holds `slabs` matrices of als_gram_elems(k) elements, one per workgroup of the grid,
  // which strides over the work items; als_wide_slabs is the count for a device of `cus` CUs (0 at a
  // rank the narrow kernels take).
  void* slab = nullptr;
  int slabs = 0;
  // nnls (mf_als_run_nonneg, mf_als_run_implicit_nonneg): the same launches with the non-negative solve
  // (als_nnls_device.hpp) in the Cholesky solve's place; nnls_stats are the six 64-bit device counters of
  // mf_als_nonneg_stats.  With dump != null (the testing hook, one row) dump[0 .. k) = x, dump[k] = the
  // iterations, dump[k + 1] = the reason code; X and the counters are not touched.
  bool nnls = false;
  void* nnls_stats = nullptr;
  // Conjugate gradients (kernels_als_cg.hip).  Whole rows (slot < 0) take `steps` CG steps from X[row]
  // in one launch; a row of at most als_cg_capacity(k, f64) ratings keeps its counterpart vectors in LDS
  // for all of them when `stage` is set, a longer one gathers them again in every pass (the same
  // arithmetic).  Long rows: work[0 .. n_work) names the launch's chunk items and, for each, the index of
  // its row in splits[]; their state (als_cg_state_elems(k) elements per row of splits[]) lives in
  // `state`, and every pass is two launches (a k-vector per chunk into partial[slot], then the row's
  // update): 2 * (steps + 1) launches.
  const AlsCgWork* work = nullptr;
  int n_work = 0;
  int steps = 0;
  bool stage = false;
  void* state = nullptr;
  const void* hook_v = nullptr;
};
// The runtime (f64, implicit) of a launch as compile-time (T, W): f(T(), std::bool_constant<W>()).
template <typename F>
void als_dispatch(bool f64, bool implicit, F&& f) {
  auto w = [&](auto t) { implicit ? f(t, std::true_type()) : f(t, std::false_type()); };
  f64 ? w(double()) : w(float());
}
// ... and the rank bucket (k + 31) / 32 in NB0 .. NB0 + 3 as NB: f(T(), std::bool_constant<W>(),
// std::integral_constant<int, NB>()).  Any other bucket is refused.
[[noreturn]] void als_refuse_rank();
template <int NB0, typename F>
void als_dispatch(bool f64, bool implicit, int k, F&& f) {
  als_dispatch(f64, implicit, [&](auto t, auto w) {
    switch ((k + 31) / 32 - NB0) {
      case 0: return f(t, w, std::integral_constant<int, NB0>());
      case 1: return f(t, w, std::integral_constant<int, NB0 + 1>());
      case 2: return f(t, w, std::integral_constant<int, NB0 + 2>());
      case 3: return f(t, w, std::integral_constant<int, NB0 + 3>());
      default: als_refuse_rank();
    }
  });
}
size_t als_partial_elems(int k);
// Ranks above 128 go on to launch_als_wide.
void launch_als(const AlsLaunch& L);
// G = sum of y y^T over rows rated[0 .. m) of Y, KP x KP (KP = k rounded up to 32, full symmetric,
// zero past k): workgroup b sums rows [b * slice, (b + 1) * slice) into part[b] (als_gram_slices(m,
// slice) partials of als_gram_elems(k) elements), then one launch adds them in ascending order.
struct AlsGramLaunch {
  hipStream_t st;
  const int32_t* rated;
  int m, slice;
  const void* Y;
  int k;
  bool f64;
  void* part;
  void* G;
};
size_t als_gram_elems(int k);
int als_gram_slices(int m, int slice);
void launch_als_gram(const AlsGramLaunch& L);

// ---- kernels_als_wide.hip: the same at ranks 129..256 ------------------------------------------
// launch_als and launch_als_gram hand these ranks on.  launch_als_gram_wide stores the slice partials only.
int als_wide_slabs(int k, bool f64, int cus);
void launch_als_wide(const AlsLaunch& L);
void launch_als_gram_wide(const AlsGramLaunch& L);

// ---- kernels_als_cg.hip: ALS half-sweeps by conjugate gradients ---------------------------------
// The work lists, CSR, partial slots and G of launch_als, every rank 1..kAlsMaxRank in one code path
// (mf_als_run_cg; gram != null: mf_als_run_implicit_cg).
size_t als_cg_state_elems(int k);
int als_cg_capacity(int k, bool f64);
void launch_als_cg(const AlsLaunch& L);

// ---- kernels_als_objective.hip: mf_als_objective --------------------------------------------------
// The fit pass over one side's work list (the user side's: its gathers hit the smaller table): item_sums[x] =
// sum64 of the terms of work item x in CSR order, one wave per item, X the side's own slab and Q the
// counterpart's.  kAlsObjFlight: the counterpart rows a wave gathers before it uses the first.
constexpr int kAlsObjFlight = 4;
struct AlsObjectiveLaunch {
  hipStream_t st;
  const AlsItem* items;
  int64_t n_items;
  const int32_t* cols;
  const void* vals;
  const void* X;
  const void* Q;
  int k;
  bool f64, implicit;
  double alpha;
  double* item_sums;
};
void launch_als_objective_fit(const AlsObjectiveLaunch& L);
// out[a] = dot64(x, x) of row rated[a] of X, widened, times the row's weight in f64: weight 0 = 1, 1 = its
// ratings off[row + 1] - off[row], 2 = those of them whose stored value is > 0.
void launch_als_objective_norms(hipStream_t st, const int32_t* rated, int64_t m, const int64_t* off, const void* vals,
                                const void* X, int k, bool f64, int weight, double* out);
// *out = sum64 over e = f * k + g of GU[f][g] * GI[f][g] (launch_als_gram's layout), the product in T.
void launch_als_objective_trace(hipStream_t st, const void* GU, const void* GI, int k, bool f64, double* out);
// *out = sum64(v[0 .. n)): lane l of one wave chains v[l], v[l + 64], ... from 0.0, then v[l] += v[l ^ 32], 16,
// 8, 4, 2, 1.  n == 0 gives 0.0.
void launch_sum64(hipStream_t st, const double* v, int64_t n, double* out);

// ---- kernels_als_append.hip: mf_als_append ------------------------------------------------------
// One side's packed CSR (counterpart rows, rating bits of 4 or 8 bytes) with a batch appended, into fresh
// arrays: row x keeps its old entries in their order, then takes the batch's in batch order.  Integer
// moves only.  old_off[old_rows + 1] and new_off[new_rows + 1] are device arrays, new_rows >= old_rows;
// brow / bcol / bval are the batch in the caller's order (every brow < new_rows), n < 2^31; new_off must be
// old_off's counts plus the batch's (als_append_placement).  The batch alone is sorted (stable radix sort
// by row, rocprim); every old entry is read once and written once, a workgroup per 2048 consecutive old
// entries, whatever rows they belong to.  The launch may reallocate `sc`: drain the stream between two
// launches that share it.
struct AlsAppendScratch;
struct AlsAppendLaunch {
  hipStream_t st;
  const int64_t* old_off;
  int64_t old_rows, old_nnz;
  const int64_t* new_off;
  int64_t new_rows;
  const int32_t* old_cols;
  const void* old_vals;
  int32_t* new_cols;
  void* new_vals;
  int elem_bytes;  // 4 or 8
  const uint32_t* brow;
  const uint32_t* bcol;
  const void* bval;
  int64_t n;
};
void launch_als_append(const AlsAppendLaunch& L, AlsAppendScratch& sc);

// ---- kernels_als_remove.hip: mf_als_remove, mf_als_remove_rows, mf_seen_remove -------------------
// Entries taken out of a packed CSR (off[rows + 1], cols, values of elem_bytes = 4 or 8, or 0 for a CSR
// without values: the seen set's table), the survivors keeping their order.  Integer work only, but for the
// `> 0` on the stored value behind rempos.  Two ways to name what goes:
//   bkey != null: nb keys (row << 32) | col in the caller's order, every row < rows.  Key j takes the OLDEST
//     entry of its pair that no earlier key of the batch took (the first in the row's order): m keys of one
//     pair take its m oldest entries.  found[j] (device, nb bytes; may be null) = 1 where there was one.
//   bkey == null: every entry whose row is marked in rowmark[rows] or whose column in colmark[] (either
//     may be null).
// launch_als_remove_select finds them and returns how many go (it drains the stream); rempos (device, rows
// int32; may be null; needs values) receives per row the removed entries whose value is > 0.  Nothing has
// moved yet.  When it returned > 0, launch_als_remove_move with the same L and scratch writes new_off[rows +
// 1] and the surviving entries into fresh arrays of nnz - gone entries: every survivor is read once and
// written once, a workgroup per 2048 consecutive entries whatever rows they belong to.  A select may
// reallocate `sc`: drain the stream between a move and the next select.
struct AlsRemoveScratch;
struct AlsRemoveLaunch {
  hipStream_t st;
  const int64_t* off;
  int64_t rows, nnz;
  const int32_t* cols;
  const void* vals;
  int elem_bytes;  // 4, 8, or 0: no values
  const uint64_t* bkey;
  int64_t nb;
  const uint8_t* rowmark;
  const uint8_t* colmark;
};
int64_t launch_als_remove_select(const AlsRemoveLaunch& L, AlsRemoveScratch& sc, uint8_t* found, int32_t* rempos);
void launch_als_remove_move(const AlsRemoveLaunch& L, const AlsRemoveScratch& sc, int64_t* new_off, int32_t* new_cols,
                            void* new_vals);

// ---- kernels_foldin.hip: mf_als_foldin, mf_recommend_foldin ---------------------------------------
// One batch of fold-in lists as uploaded -> the transient CSR the ALS launches read.  off[nq + 1] (device, off[0]
// = 0, off[nq] = n) cuts the n entries into the batch's nq lists; ids holds 2n words, the lists' ids in the
// first n (replaced by their rows of the counterpart side, kRowMiss for an id it does not hold -- slots / mask:
// that side's id mirror as launch_id_lookup takes it) and scratch behind them; ratings are the callers' f64.
// The kept entries (known ids) are compacted stably: cols / vals (room for n; vals in the context's
// precision, converted by one rounding) hold query 0's kept entries in list order, then query 1's, ...;
// cnt[q] = (kept entries, of them rating > 0 after the conversion), two int32 per query -- all the host reads
// back.  keys (may be null; room for n): per kept entry, beside it, (query position << 32) | row, the keys
// rank_keys_sort takes.  Entry-tiled (csr_device.hpp): the cost follows the entries, not the longest list.
struct FoldinScratch;
struct FoldinLaunch {
  hipStream_t st;
  const int64_t* off;
  int64_t nq, n;
  uint32_t* ids;
  const double* ratings;
  const void* slots;
  uint64_t mask;
  bool f64;
  int32_t* cols;
  void* vals;
  int32_t* cnt;
  uint64_t* keys;
};
void launch_foldin_compact(const FoldinLaunch& L, FoldinScratch& sc);

// ---- kernels_bpr.hip: BPR minibatch steps (mf_bpr_run, mf_bpr_step_triples) ------------------------
// One step over the `batch` triples in sc.trip, as include/mfhip.h defines it: weights from the model as the step
// found it, every touched row written once.  P / Q: the user / item slabs in the context's precision.  bpr_reserve
// sizes the scratch for steps of `batch` slots (it drains the stream; the steps after it allocate nothing);
// launch_bpr_draw fills sc.trip from the seen set's user-major table (off[table_rows + 1], ent, pairs > 0 entries;
// item_rows >= 2), launch_bpr_resolve from caller-given triples as launch_id_lookup_one left them in sc.trip.
// launch_bpr_step adds the step's counts to sc.stats (void slots, user rows, item rows at [1], [2], [3]); lap (may
// be empty) is called with a phase's name after the phase's launches: the caller's phase clock (bpr.cpp).
struct BprScratch;
struct BprStep {
  hipStream_t st;
  int64_t batch;
  void* P;
  void* Q;
  uint32_t user_rows, item_rows;
  int k;
  bool f64;
  double lr, lambda;
  bool mean;
  int64_t chunk;
};
void bpr_reserve(hipStream_t st, BprScratch& sc, int64_t batch, int64_t user_rows, int k, size_t es, int64_t chunk);
void launch_bpr_draw(const BprStep& L, BprScratch& sc, const int64_t* off, const int32_t* ent, int64_t table_rows,
                     int64_t pairs, int64_t seed, int64_t step, int32_t redraws);
void launch_bpr_resolve(const BprStep& L, BprScratch& sc);
using BprLap = std::function<void(const char*)>;
void launch_bpr_step(const BprStep& L, BprScratch& sc, const BprLap& lap = BprLap());

}  // namespace mfhip
