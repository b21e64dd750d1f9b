// context.hpp -- the context (mf_ctx), its shards, and the helpers more than one host translation
// unit uses.  Private to the host side: included by the .cpp files only (mfhip.cpp, dsgd_det.cpp,
// dsgd_fast.cpp, ring.cpp, abi.cpp, online.cpp, eval.cpp, recommend.cpp, rank_eval.cpp, pair_rank.cpp, als.cpp,
// seen.cpp),
// never by a .hip file or by kernels.hpp / plan.hpp; placement.cpp, which knows no context, does without it.
#pragma once

#include <array>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <future>
#include <string>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mfhip {

struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    MF_HIP(hipSetDevice(dev));
  }
  ~DeviceGuard() { (void)hipSetDevice(prev); }
};

#define MF_NCCL(call)                                                                     \
  do {                                                                                    \
    ncclResult_t _r = (call);                                                             \
    if (_r != ncclSuccess) ::mfhip::fail(MF_ERR_COMM, std::string(#call) + ": " + ncclGetErrorString(_r)); \
  } while (0)

// Deterministic persistent sweep: one superstep's entries, staged in pinned memory by a host
// thread while earlier supersteps run, then copied to the device (fixed SoA offsets).  A ring of
// kDetSlots buffers: the host builds supersteps s+1 and s+2 (two builders at once) while the device
// runs s.  On the GPU box (16 host threads) one NFLX build takes ~28 ms alone and about as long
// with another beside it, i.e. ~14 ms per superstep -- the split sweep's ~14.4 ms launch; a third
// builder does not raise that rate (three at once: ~44 ms each, the host threads are saturated).
constexpr int kDetSlots = 3;
struct DetBuf {
  PinnedBuf pin;
  DevBuf dev;
  hipEvent_t copied = nullptr;  // the H2D from `pin` finished (pin may be rewritten)
  hipEvent_t swept = nullptr;   // the sweep that read `dev` finished (dev may be rewritten)
  bool pending = false;         // `copied` was recorded and not yet waited for
  bool dev_built = false;       // det_build left only the shuffle here: the device builds the entries
  int64_t n = 0, nw = 0;
  DetStepScratch scratch;  // build_det_step's gathers for this slot (kept: no page faults per superstep)
};

// A device mirror of one side's IdIndex (same slots), for the online batch's id lookup.
struct DevIndex {
  DevBuf slots, upd_pos, upd_val;
  uint64_t gen = 0, cap = 0;
  size_t applied = 0;  // entries of the table's write log already in the mirror
};

struct Shard {
  int device = 0;
  int index = 0;  // global shard index (== rank in rank mode)
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;  // host-to-device staging beside the sweeps (deterministic mode)
  // ring overlap (c >= 2 user blocks per shard, systolic fast sweep): the shard's last local block
  // runs on `aux` behind the arriving item block; the leaving block moves on `comm` as soon as
  // the launch holding the other blocks has finished
  hipStream_t aux = nullptr, comm = nullptr;
  hipEvent_t ev_front = nullptr;  // launch A (local blocks 0..c-2) of the latest superstep done
  hipEvent_t ev_last = nullptr;   // launch B (local block c-1) of the latest superstep done
  hipEvent_t ev_moved = nullptr;  // the item block this shard sent / received in the latest ring step
  std::vector<int64_t> st_sys_block_off;  // PairPlan::sys_block_off
  hipEvent_t done = nullptr;  // ring hand-off ordering between in-process shards
  DevBuf uf, itf, regu, regi;
  int64_t cap_u = 0, cap_i = 0;
  // deterministic mode staging
  DevBuf det_dev;
  PinnedBuf det_pin;
  OnlineSweepScratch online_sc;  // online micro-batches (k_online_sweep)
  DevIndex didx[2];              // device mirrors of the user [0] / item [1] IdIndex (online id lookup)
  PinnedBuf small_pin;           // online batch: {lookup misses, sweep error, touched users, items}, read back async
  PinnedBuf slots_pin;           // online f64 batch: the wave table read back for det_slot_table
  DevBuf blk_u, blk_i, blk_ru, blk_ri;  // mf_block_update: the block's factor rows and lambda / omega
  // fast mode
  DevBuf fast_recs, fast_cells, fast_blks;
  DevBuf fast_prog, fast_err;  // persistent sweep: progress words + timeout flag
  DevBuf st_recs, st_waves;    // pair schedule: records and per-cell wave table
  int64_t st_nrecs = 0;        // pair records in st_recs
  std::vector<int64_t> st_sub_off;
  std::vector<WaveDesc> st_waves_host;  // kept only when tracing
  DevBuf st_sys, st_sysw;               // systolic pair tables (PairPlan::sys, sys_waves)
  DevBuf st_place;                      // per systolic wave slot: block -> wave of its launch (sys_placement)
  std::vector<int64_t> st_place_off;     // per superstep: its first slot in st_place (nb + 1)
  std::vector<int32_t> st_place_pad;     // per superstep: empty blocks per XCD in its launch (sys_placement)
  std::vector<int64_t> st_sys_off;      // PairPlan::sys_off
  std::vector<WaveDesc> st_sys_host;    // kept only when tracing
  std::vector<SysWave> st_sysw_host;    // kept only when tracing
  uint32_t sys_base = 0;                // progress-word base of the next systolic launch
  uint32_t sys_step = 1;                // base advance per launch (> the largest G_j)
  DevBuf st_trace;                      // MFHIP_WAVE_TRACE: {start, end} per wave
  DevBuf st_split;                      // hot-item replicas (SplitItem), superstep-major
  std::vector<int64_t> st_split_off;    // per superstep (n + 1)
  std::vector<double> sm_bytes;         // per superstep index (s-1) mod n: bytes the sweep requests
  // deterministic persistent sweep (kernels_detsweep.hip)
  DetSweepLayout det_layout;
  DetBuf det_buf[kDetSlots];
  DevBuf det_ticket, det_err, det_scratch;
  int64_t det_n_max = 0, det_nw_max = 0;
  // the superstep's input built on the device (det_device_build; MFHIP_TEST det_build=host: on the
  // host): the rating blocks' 16-B records, the blocks' item -> wave maps, per superstep index
  // (s-1) mod n its block table and its wave / slot table (both fixed: a wave's count is the sum
  // of its items' counts), the uploaded shuffle permutation, and the build's scratch
  DevBuf det_aos_dev, det_iw, det_bt, det_ord;
  DetBuildScratch det_bs;
  std::vector<std::vector<DetWave>> det_sm_slots;
  std::vector<int64_t> det_sm_n;
  std::vector<int32_t> det_sm_nblk;
  uint32_t det_wave_bound = 1;
  // evaluation scratch
  DevBuf ev_u, ev_i, ev_r, ev_mult, ev_out, ev_part;
  // recommendation (mf_recommend): the row -> id table of each side (valid while rec_id_gen matches
  // the context's layout_gen), the query rows and exclusion CSR of a call, and a batch's partial
  // lists and results
  DevBuf rec_id[2];
  uint64_t rec_id_gen[2] = {0, 0};
  DevBuf rec_q, rec_eoff, rec_erows, rec_part, rec_ids, rec_scores, rec_counts;
  // ... the cosine metric (mf_similar, mf_recommend_vectors): one call's inverse norms of the candidate rows
  // and of the staged queries, and one batch of the caller's vectors in the context's precision with its
  // pinned host stage (mf_recommend_vectors)
  DevBuf rec_cinv, rec_qinv, rec_qvec;
  PinnedBuf rec_pin;
  // ... mf_recommend_among (which also uses the rec_* buffers and rank_sc).  Shared list: its distinct rows (the
  // position -> row map), the gathered slab and its ids.  Per-query lists, one batch: the lists as uploaded and resolved, the tasks,
  // and per position its first task, query row and exclusion range
  DevBuf am_rows, am_slab, am_id, am_in, am_tasks, am_pbeg, am_qrow, am_ebeg, am_eend;
  // ranking metrics (mf_rank_eval, which also uses the rec_* buffers): the table build's scratch, a pair
  // list as uploaded (query rows, then candidate rows or ids), the ground-truth CSR, the per-query
  // metrics and (hits, g), the slice sums, the gain table and the call's totals
  RankScratch rank_sc;
  DevBuf rk_in, rk_goff, rk_gent, rk_met, rk_cnt, rk_part, rk_tab, rk_res;
  // pair ranks (mf_pair_ranks / mf_online_prequential, which also use the rec_* exclusion table and the
  // rk_* sums): the pairs' factor rows (query rows, then candidate rows), the two parts of their keys,
  // and the per-pair rank / list length / score
  DevBuf pr_in, pr_ord, pr_tid, pr_rank, pr_valid, pr_score;
  // the resident seen set (mf_seen_*; on the context's first shard, like the evaluation it serves)
  SeenTable seen;
  // ALS (mf_als_prepare): per solved side [user, item] the CSR (counterpart rows, ratings) and the
  // work lists; the long rows' partial systems of one launch; the testing hook's output
  DevBuf als_cols[2], als_vals[2], als_items[2], als_splits[2], als_part, als_dump;
  // ... at a rank above 128 the normal matrices of the resident workgroups (kernels_als_wide.hip)
  DevBuf als_slab;
  // ... the implicit half-sweep: per side its rated rows, the Gram partials of one side and G itself
  DevBuf als_rated[2], als_gram_part, als_gram;
  // ... the conjugate-gradient half-sweeps: per side the chunk items of its long rows, the state of one
  // launch's long rows, the testing hook's vector and chunk list
  DevBuf als_cg_work[2], als_cg_state, als_cg_v, als_cg_hook_work;
  // ... the non-negative half-sweeps: the six 64-bit counters of mf_als_nonneg_stats (zeroed in mf_als_prepare)
  DevBuf als_nnls_stats;
  // ... mf_als_append: per side the CSR's 64-bit row offsets, the batch and its sort (kernels_als_append.hip)
  DevBuf als_off[2];
  AlsAppendScratch als_app;
  // ... mf_als_remove / mf_als_remove_rows / mf_seen_remove: the batch, the selection and what comes back
  AlsRemoveScratch als_rem;
  // ... mf_als_run_rows: the item, split and chunk lists of one call
  DevBuf als_sub_items, als_sub_splits, als_sub_work;
  // ... mf_als_objective: the per-item / per-row f64 partials of one pass, the user side's G beside als_gram,
  // and the four sums that come back
  DevBuf als_obj_part, als_obj_gram, als_obj_out;
  // ... mf_als_foldin / mf_recommend_foldin (which also use als_sub_*, the rec_* buffers and rank_sc)
  FoldinScratch fold;
  // BPR training (mf_bpr_run, mf_bpr_step_triples)
  BprScratch bpr;
  // profiling
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  int64_t ev_launches = 0;
};

}  // namespace mfhip

struct mf_ctx {
  mfhip::Reaper reaper;  // host plan buffers being released in the background (first member: joined last)
  mf_params P{};
  std::vector<uint32_t> on_ur, on_ir;  // online batches: factor rows per rating (kept: no page faults per batch)
  bool f64 = true;
  size_t es = 8;  // bytes per factor element
  int G = 1;      // global shard count
  bool rank_mode = false;
  ncclComm_t comm = nullptr;
  std::vector<mfhip::Shard> shards;  // local shards
  mfhip::SideLayout U, I;
  bool have_model = false;
  bool prepared = false;
  int32_t nb = 1;
  int32_t c = 1;  // user blocks per shard
  int64_t superstep_done = 0;
  std::vector<int> item_loc;  // item block -> shard holding it
  mfhip::RatingBlocks rb;     // deterministic mode keeps the rating blocks on the host
  int32_t G_fast = 0;
  uint32_t fast_dummy_u = 0, fast_dummy_i = 0;  // zeroed rows past the real ones (padding / idle prefetch)
  int32_t fast_prio_len = 1 << 30;  // cells at least this long run at raised priority
  bool fast_persistent = false;  // MFHIP_TEST fast_kernel=persistent selects the systolic single launch
  bool fast_pair = false;         // two updates per step (kernels_pair.hip), k in {64, 128, 256}
  bool fast_sys = false;          // pair cells as one systolic launch per superstep (k_sweep_pair_sys)
  bool det_sweep = false;         // deterministic mode: one persistent k_det_sweep launch per superstep
  bool det_split = false;         // ... with single-item chains split over two waves (k_det_sweep_split)
  bool det_dev_build = false;     // ... its input built on the device from the host's shuffle (det_device_build)
  bool det_dev_ready = false;     // ... the device build prepared (the switch below may turn it on)
  bool det_mixed = false;         // ... MFHIP_TEST det_build=mixed: switch from the third superstep on
  std::atomic<bool> det_switch{false};  // ... the host builds fell behind the device: device builds from now on
  int det_idle = 0;               // ... consecutive supersteps whose build the device had to wait for
  bool det_alone = true;          // ... the longest chains on CUs of their own (det_slot_table)
  int64_t det_split_blocks = 0;   // resident blocks of k_det_sweep_split (per device share)
  int64_t det_cu_period = 256;    // CUs of the device: blocks b and b + period share a CU
  bool ring_overlap = false;      // fast systolic sweep, >1 shard, c >= 2: the ring step overlaps the sweep
  // fast-mode hot-item replicas (plan.hpp SplitItem), an experiment outside the product surface:
  // MFHIP_ITEM_SPLIT=m sweeps an item with more than m ratings in one rating block as ceil(r / m)
  // chains averaged when the superstep ends (read at prepare; 0 / unset = off)
  int32_t item_split = 0;
  std::vector<int64_t> fast_rb_size;  // per rating block (fast mode)
  mf_stats stats{};
  bool profiling = false;
  std::vector<int32_t> rows_by_id_u, rows_by_id_i;  // ascending-id row permutations
  bool order_dirty = true;
  uint64_t layout_gen = 1;  // bumped wherever a side's rows change (with order_dirty): device row -> id tables
  int64_t init_seed = 0;      // seed of the initial factors (P.seed, or a random one when unseeded)
  std::string failed;         // non-empty: a device-side bound tripped; the fit must be prepared again
  // deterministic sweep: the next run's first supersteps, built on worker threads when a run ends
  // (a superstep's schedule depends only on its number and the training data): det_spec_s[slot] =
  // the superstep built into det_buf[slot], -1 = none (det_run takes them over; det_spec_wait
  // joins them where the data, layouts or superstep change)
  // ALS (mf_als_prepare / mf_als_run): per solved side the work lists (host copies of the device
  // arrays) cut into launches; the CSR itself lives on the device only
  struct AlsBatch { int64_t item0, items, split0, splits; };
  struct AlsSide {
    std::vector<mfhip::AlsItem> items;
    std::vector<mfhip::AlsSplit> splits;
    std::vector<AlsBatch> batches;
    int64_t max_slots = 0;
    int64_t rated = 0;  // rows with at least one rating (the length of Shard::als_rated)
    // the CSR's shape as of the last mf_als_prepare / mf_als_append (the entries live on the device only):
    // off[rows + 1], and per row its ratings > 0; rows the model gained since have no entry here
    std::vector<int64_t> off;
    std::vector<int32_t> npos;
    // the conjugate-gradient half-sweeps (built on first use): the chunk items of every batch, batch b's
    // at [cg_work0[b], cg_work0[b + 1]), and the most long rows of one batch
    std::vector<mfhip::AlsCgWork> cg_work;
    std::vector<int64_t> cg_work0;
    int64_t cg_max_splits = 0;
    bool cg_ready = false;
  } als[2];
  // ratings per work item of a long row and rows per launch, as mf_als_prepare read them (mf_als_append
  // rebuilds the work lists with the same values)
  int64_t als_chunk = 0, als_batch = 0;
  int64_t als_gram_slice = 0;  // rated rows per workgroup of k_als_gram (fixed in mf_als_prepare)
  // k > 128: normal-matrix slabs = workgroups per launch of the wide kernels (fixed in mf_als_prepare
  // from the device's CU count; MFHIP_TEST als_slabs=N caps it, results do not depend on it)
  int64_t als_slabs = 0;
  bool als_prepared = false;
  int64_t als_half_sweeps = 0;  // half-sweeps run since mf_als_prepare (even: the item side is next)
  std::future<void> det_spec[mfhip::kDetSlots];
  int64_t det_spec_s[mfhip::kDetSlots] = {-1, -1, -1};
};

namespace mfhip {

constexpr int kSideU = MF_SIDE_USER;

enum class FastKernel { kPair, kCell, kPersistent };

inline SideLayout& side_of(mf_ctx* ctx, int side) { return side == kSideU ? ctx->U : ctx->I; }

// The rating block that user block j of a shard runs in the supersteps with (s - 1) mod n == sm:
// (p, (p + sm) mod n) as a rating block id (toRatingBlockId, DSGDforMF.scala:597-601).
inline int64_t rating_block_of(const mf_ctx* ctx, int shard_index, int64_t sm, int32_t j) {
  const int32_t p = shard_index * ctx->c + j;
  return static_cast<int64_t>(p) * ctx->nb + (p + sm) % ctx->nb;
}

// ---------------------------------------------------------------------------------------
// profiling: a pair of HIP events around every sweep-kernel launch on the shard's stream.
// ext = true: the launch records the pair itself (hipExtLaunchKernel start/stop events, part
// of the dispatch packet, so timing adds no commands between kernels); start() / stop() give
// the events, or null when profiling is off.
struct LaunchTimer {
  Shard& s;
  bool on, ext;
  size_t slot = 0;
  LaunchTimer(Shard& sh, bool enabled, bool ext_events = false) : s(sh), on(enabled), ext(ext_events) {
    if (!on) return;
    if (s.ev_used + 2 > s.ev.size()) {
      for (int x = 0; x < 512; ++x) {
        hipEvent_t e;
        MF_HIP(hipEventCreate(&e));
        s.ev.push_back(e);
      }
    }
    slot = s.ev_used;
    s.ev_used += 2;
    if (!ext) MF_HIP(hipEventRecord(s.ev[slot], s.stream));
  }
  hipEvent_t start() const { return on ? s.ev[slot] : nullptr; }
  hipEvent_t stop() const { return on ? s.ev[slot + 1] : nullptr; }
  ~LaunchTimer() {
    if (on) {
      if (!ext) (void)hipEventRecord(s.ev[slot + 1], s.stream);
      s.ev_launches++;
    }
  }
};

// MFHIP_TIMING=1: host phases of prepare on stderr.
struct PhaseClock {
  bool on = std::getenv("MFHIP_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[mfhip] %-28s %10.3f ms\n", what, 1e3 * std::chrono::duration<double>(now - t).count());
    t = now;
  }
};

struct RingStep {
  int32_t out_blk, in_blk, dst, src;
};

// Evaluation: resolve ids on the host, gather-dot on the device.
struct EvalOut {
  double sse = 0, cnt = 0, risk = 0;
};

// mfhip.cpp: context lifetime, slabs, health, model construction, the top of the DSGD driver
mf_ctx* create_ctx(const mf_params* p, const int* device_ids, int n_devices);
mf_ctx* create_rank_ctx(const mf_params* p, int device_id, int nranks, int rank, const uint8_t* uid);
void destroy_ctx(mf_ctx* ctx);
double bytes_per_update(const mf_ctx* ctx);
void ensure_rows(mf_ctx* ctx, Shard& s, int side, int64_t rows);
void upload_rows(mf_ctx* ctx, Shard& s, int side, int64_t row0, const double* src, int64_t n);
void upload_regs(mf_ctx* ctx, Shard& s, int side, int64_t row0, const double* src, int64_t n);
void download_rows(mf_ctx* ctx, Shard& s, int side, int64_t row0, int64_t n, double* out);
void init_vectors(const int32_t* ids, int64_t n, int k, bool xor_seed, int64_t seed, std::vector<double>& out);
void init_factors(mf_ctx* ctx);
void sync_all(mf_ctx* ctx);
void require_healthy(const mf_ctx* ctx);
void ensure_order(mf_ctx* ctx);
int32_t online_row(mf_ctx* ctx, SideLayout& S, int32_t id, std::vector<int32_t>& fresh);
void prepare(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n);
void run_supersteps(mf_ctx* ctx, int64_t count);
void debug_levels(const uint32_t* urow, const uint32_t* irow, const int32_t* order, int64_t n, int32_t* level_out);

// dsgd_det.cpp: deterministic supersteps (level launches; the persistent sweep and its builds)
void prepare_det_sweep(mf_ctx* ctx);
void det_superstep(mf_ctx* ctx, Shard& s, int64_t superstep, double eta);
void det_run(mf_ctx* ctx, int64_t count);
void det_spec_wait(mf_ctx* ctx, bool invalidate);
int64_t device_cu_count(int dev);

// dsgd_fast.cpp: fast supersteps (the four launch shapes, their schedules and device tables)
bool want_pair_sys();
FastKernel choose_fast_kernel(int k);
int32_t plan_window(int32_t k);
void prepare_fast(mf_ctx* ctx, DevRatingBlocks& dev_rb, PhaseClock& clk, int32_t lo, int32_t hi);
void fast_superstep(mf_ctx* ctx, Shard& s, int64_t superstep, double eta);
void dump_wave_trace(mf_ctx* ctx);
int debug_fast_plan(const int32_t* u, const int32_t* i, int64_t n, int32_t n_blocks, int64_t seed, int32_t groups,
                    int32_t blocking, int32_t window, int32_t k, int32_t item_split, int32_t* block_out, int32_t* substep_out, int32_t* group_out, int64_t* pos_out,
                    int32_t* replica_out);
void plan_digest(mf_ctx* ctx, uint64_t out[2]);

// ring.cpp: the item-block ring between shards
RingStep ring_step(int32_t g, int32_t G, int32_t c, int32_t n, int64_t superstep);
void ring_shift(mf_ctx* ctx, int64_t superstep);
void reset_item_loc(mf_ctx* ctx);
void consolidate(mf_ctx* ctx, Shard& dst);

// online.cpp
// Brings the device mirror d up to the host table ix (the whole table after a rehash, else the slots written
// since the last sync); under the caller's DeviceGuard.
void sync_dev_index(Shard& s, const IdIndex& ix, DevIndex& d);
void online_update(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                   int num_partitions, int64_t* tu, int64_t* ti, double* uout = nullptr, double* iout = nullptr);
// mf_online_update_sampled: the batch with `negatives` drawn updates (neg_sample.hpp) behind every event
struct NegSampling {
  int32_t negatives = 0;
  double rating = 0.0;
  int64_t seed = 0, first_event = 0;
};
void check_negative_sampling(const NegSampling& neg);
void online_update_sampled(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                           const NegSampling& neg, int32_t* sampled_out, int64_t* tu, int64_t* ti);
void block_update(mf_ctx* ctx, const double* r, const int32_t* uidx, const int32_t* iidx, int64_t len, double* users,
                  const int32_t* uomega, int64_t nu, double* items, const int32_t* iomega, int64_t ni, int k,
                  int iteration, int rating_block_id, int64_t seed, double lr, int lr_method, double lr_arg,
                  double lambda);
void set_factors(mf_ctx* ctx, int side, const int32_t* ids, const double* vecs, int64_t n);

// eval.cpp
void allgather_items(mf_ctx* ctx);
EvalOut evaluate(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                 const int32_t* mult, double lambda, double* pred_out, uint8_t* found_out);
void get_factors(mf_ctx* ctx, int side, int32_t* ids, double* vecs, int64_t cap, int64_t* written);
void lookup_factors(mf_ctx* ctx, int side, const int32_t* ids, int64_t n, double* vecs_out, uint8_t* found);

// seen.cpp: what a reader of the resident seen set takes (below)
struct SeenView {
  const int64_t* off = nullptr;
  const int32_t* ent = nullptr;
  const int32_t* iota = nullptr;
  bool any = false;
};

// recommend.cpp: the top-N lists
void recommend(mf_ctx* ctx, int qside, const int32_t* queries, int64_t nq, int32_t top_n, const int32_t* eq,
               const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out, int32_t* counts_out,
               bool seen = false);
// mf_recommend_among: off null = one shared list cand[0 .. n_cand), else position j owns cand[off[j] .. off[j + 1]).
void recommend_among(mf_ctx* ctx, int qside, const int32_t* queries, int64_t nq, int32_t top_n, const int64_t* off,
                     const int32_t* cand, int64_t n_cand, bool seen, const int32_t* eq, const int32_t* ec, int64_t ne,
                     int32_t* ids_out, double* scores_out, int32_t* counts_out);
void similar(mf_ctx* ctx, int side, const int32_t* queries, int64_t nq, int32_t top_n, int metric, bool include_self,
             const int32_t* eq, const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out,
             int32_t* counts_out);
void recommend_vectors(mf_ctx* ctx, int cside, const double* vecs, int64_t nq, int32_t top_n, int metric,
                       const int64_t* eqi, const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out,
                       int32_t* counts_out);
// The row -> id table of a side on the device (s.rec_id[side]), current with the layout.
void sync_row_ids(mf_ctx* ctx, Shard& s, int side);
// How n queries (or pairs) are walked against C candidate rows: `batch` of them a launch, the candidate rows in
// S splits -- enough workgroups for two per CU (qtile: the queries one workgroup owns), each split at least one
// candidate tile of 128 rows, at most 64 splits, and 1 where there is no candidate.  MFHIP_TEST <batch_knob>=B /
// <split_knob>=S override both.
struct TopNShape { int64_t batch, S; };
TopNShape topn_shape(int64_t n, int64_t C, int qtile, int64_t default_batch, const char* batch_knob,
                     const char* split_knob);
// The exclusions of a call, per batch as launch_recommend's (beg, end, rows).  Either the call's CSR on the device
// (query j of the call: rows[off[j] .. off[j + 1]), sorted distinct candidate rows), or the resident seen set,
// whose ranges are gathered through the batch's query rows into two buffers that batch() sizes.
struct ExclSource {
  struct Range { const int64_t *beg, *end; const int32_t* rows; };
  static ExclSource csr(const int64_t* off, const int32_t* rows) { return {off, rows, SeenView{}, nullptr, nullptr}; }
  static ExclSource seen(const SeenView& v, DevBuf& qbeg, DevBuf& qend) { return {nullptr, nullptr, v, &qbeg, &qend}; }
  // the batch of nb queries from the call's b0-th on, whose rows are qrows[0 .. nb) on the device
  Range batch(hipStream_t st, int64_t b0, int64_t nb, const int32_t* qrows) const;

  const int64_t* off;
  const int32_t* rows;
  SeenView sv;
  DevBuf *qbeg, *qend;  // (the gather buffers)
};
// The queries of a call.  rows (device): query j is row rows[j] of the resident slab Q (q_rows rows of k
// elements in the context's precision; side: the model side it is, -1 a slab of the caller's that kernels queued
// on the stream may still be writing).  staged: the queries are the host's n x k f64 vectors instead; they are
// converted as upload_rows converts factor rows and staged one batch ahead, so the conversion of batch b + 1 runs
// on the host while the device scores batch b, and rows is the identity 0 .. n-1.
struct TopNQueries {
  int64_t n = 0;
  const int32_t* rows = nullptr;
  const void* Q = nullptr;
  int64_t q_rows = 0;
  int side = -1;
  bool staged = false;
  const double* vecs = nullptr;
  // the rows s.rec_q[0 .. n) of a side; every row of the caller's slab Q (the identity list is made on the
  // device); host vectors (s.rec_q holds the identity)
  static TopNQueries of_side(mf_ctx* ctx, Shard& s, int side, int64_t n) {
    return {n, s.rec_q.as<int32_t>(), side == kSideU ? s.uf.get() : s.itf.get(), side_of(ctx, side).rows(), side};
  }
  static TopNQueries of_slab(Shard& s, const void* Q, int64_t n);
  static TopNQueries of_vectors(Shard& s, const double* vecs, int64_t n) {
    return {n, s.rec_q.as<int32_t>(), nullptr, 0, -1, true, vecs};
  }
};
// The candidates: every row of a side, or (gathered; mf_recommend_among's shared list, MF_METRIC_DOT) only the
// rows s.am_rows[0 .. n) of it, distinct and ascending on the device.  Those are gathered into a compact slab
// with their ids, the kernels walk that slab, and the row list itself maps a slab position back to the factor
// row the exclusion tables name.
struct TopNCandidates {
  int side; bool gathered; int64_t n;
  static TopNCandidates of_side(mf_ctx* ctx, int side) { return {side, false, side_of(ctx, side).rows()}; }
  static TopNCandidates of_rows(int side, int64_t n) { return {side, true, n}; }
};
// Where a finished batch goes: to the host after a wait for it (ids [n][top_n], scores or null, counts [n]), or to
// on_batch(b0, nb) -- the lists stay in s.rec_ids / s.rec_counts (no scores), no copy and no wait in the driver.
struct TopNSink {
  int32_t* ids = nullptr;
  double* scores = nullptr;
  int32_t* counts = nullptr;
  std::function<void(int64_t, int64_t)> on_batch;
};
// The one driver, on the shard's stream under the caller's DeviceGuard: the queries against the candidates minus
// each query's exclusions, in batches that bound the scratch at batch x S x top_n keys (topn_shape; rec_batch, rec_split).
void recommend_scored(mf_ctx* ctx, Shard& s, const TopNQueries& q, const TopNCandidates& c, int32_t top_n, int metric,
                      const ExclSource& ex, const TopNSink& sink);

// rank_eval.cpp
const std::vector<double>& gain_table();  // 128 gains 1 / log(i + 2), then their 129 prefix sums
void rank_eval(mf_ctx* ctx, int qside, const int32_t* gq, const int32_t* gc, int64_t ng, int32_t top_n,
               const int32_t* eq, const int32_t* ec, int64_t ne, mf_rank_metrics* out, int32_t* q_ids_out,
               int32_t* q_counts_out, double* q_metrics_out, int64_t cap, bool seen = false);
void debug_rank_csr(mf_ctx* ctx, int qside, bool gt, const int32_t* q, const int32_t* c, int64_t n, int32_t* q_ids_out,
                    int64_t* off_out, int32_t* entries_out, int64_t cap_q, int64_t cap_e, int64_t* nq_out,
                    int64_t* ne_out);

// pair_rank.cpp
// The ranks of n pairs, left on the device in the shard's pr_rank / pr_valid / pr_score and copied to the
// non-null outputs; returns the number of cold pairs.
int64_t pair_ranks(mf_ctx* ctx, int qside, const int32_t* q, const int32_t* c, int64_t n, const int32_t* eq,
                   const int32_t* ec, int64_t ne, int32_t* rank_out, int32_t* valid_out, double* score_out,
                   bool seen = false);
void online_prequential(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                        int num_partitions, int32_t top_n, const int32_t* eu, const int32_t* ei, int64_t ne,
                        mf_prequential* out, int32_t* rank_out, int64_t* tu, int64_t* ti);
// ... with online_update_sampled as step 2
void online_prequential_sampled(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                                int flavour, int32_t top_n, const int32_t* eu, const int32_t* ei, int64_t ne,
                                const NegSampling& neg, int32_t* sampled_out, mf_prequential* out, int32_t* rank_out,
                                int64_t* tu, int64_t* ti);
// mf_online_prequential_seen: ... with the resident seen set as the exclusions, and (add_events) the batch
// added to the set after the update
void online_prequential_seen(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                             int32_t top_n, const NegSampling& neg, int32_t* sampled_out, mf_prequential* out,
                             int32_t* rank_out, int64_t* tu, int64_t* ti, bool add_events);

// seen.cpp: the resident seen set (mf_seen_*), on the context's first shard.  In each of the four readers
// above `seen` = true takes the set for the exclusions (eq / ec / ne are not read).
// seen_put: mf_seen_set (add = false) / mf_seen_add; *ignored (may be null) = pairs naming an unknown id.
void seen_put(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, bool add, int64_t* ignored);
// seen_remove: mf_seen_remove; *removed = the distinct held pairs that went, *ignored as seen_put's (either may be null).
void seen_remove(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, int64_t* removed, int64_t* ignored);
void seen_from_als(mf_ctx* ctx);
void seen_clear(mf_ctx* ctx);  // no set (mf_seen_clear; mf_dsgd_prepare, which rebuilds the rows)
int64_t seen_count(const mf_ctx* ctx);
// What a reader takes: the table of query side qside, its offsets padded to the side's present rows (a row
// gained since holds nothing), and the identity as qpos.  any = false: no pair is held (n_excl == 0).  Made
// on the shard's stream, under the caller's DeviceGuard; the item-major table is built here on first use.
SeenView seen_view(mf_ctx* ctx, Shard& s, int qside);
void seen_debug_csr(mf_ctx* ctx, int side, int32_t* row_ids_out, int64_t* off_out, int32_t* ent_out, int32_t* ent_ids_out,
                    int64_t cap_rows, int64_t cap_nnz, int64_t* rows_out, int64_t* nnz_out);
// Where the keys land when a batch is merged into a sorted table of distinct keys (the rule the merge kernels
// follow): with `novel` the distinct batch keys the table does not hold, ascending, old key p moves to
// p + #(novel < it) and novel key i to i + #(old < it).
void seen_merge_placement(const uint64_t* old_keys, int64_t n_old, const uint64_t* batch_keys, int64_t n_batch,
                          int64_t* old_pos, int64_t* novel_pos, int64_t* n_novel);

// als.cpp
// How a half-sweep solves its rows.
struct AlsParams {
  double lambda;
  int32_t reg;            // MF_ALS_REG_*
  bool implicit = false;  // the implicit-feedback system (mf_als_run_implicit), with confidence scale alpha
  double alpha = 0.0;
  int32_t cg_steps = 0;   // 0: Cholesky; 1 .. MF_ALS_CG_MAX_STEPS: that many conjugate-gradient steps
  bool nnls = false;      // (with cg_steps == 0) the non-negative solve in the Cholesky solve's place
};
void als_check(const mf_ctx* ctx);
void als_check_alpha(double alpha);
void als_check_run(const AlsParams& P);  // lambda, reg, cg_steps
void als_prepare(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n);
void als_run(mf_ctx* ctx, int64_t half_sweeps, const AlsParams& P);
void als_normal_eq(mf_ctx* ctx, int side, int32_t id, const AlsParams& P, double* A_out, double* b_out);
void als_gram(mf_ctx* ctx, int side, double* G_out);
void als_cg_matvec(mf_ctx* ctx, int side, int32_t id, const AlsParams& P, const double* v, double* Av_out,
                   double* b_out);
void als_nnls_row(mf_ctx* ctx, int side, int32_t id, const AlsParams& P, double* x_out, int32_t* iters_out,
                  int32_t* reason_out);
void als_nonneg_stats(mf_ctx* ctx, struct mf_als_nonneg_stats* out);
// mf_als_append / mf_als_run_rows / mf_als_update (which checks everything mf_als_run_rows would refuse
// before it appends)
void als_append(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n);
int64_t als_run_rows(mf_ctx* ctx, int side, const int32_t* ids, int64_t n_ids, const AlsParams& P);
void als_update(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, const AlsParams& P,
                int32_t rounds, int64_t* solved_users, int64_t* solved_items);
// mf_als_objective / mf_als_run_until.  als_check_objective: lambda (0 is valid here), reg and, when implicit,
// alpha; solver and cg_steps are not read.  als_run_until checks als_check_run's too before anything runs;
// history may be null.  Returns the iterations taken.
void als_check_objective(const AlsParams& P);
void als_objective(mf_ctx* ctx, const AlsParams& P, struct mf_als_loss* out);
int32_t als_run_until(mf_ctx* ctx, const AlsParams& P, int32_t max_iterations, double rel_tol, double* history);
// mf_als_foldin / mf_recommend_foldin (rec != null: the fused call; vecs_out may then be null).  The argument
// checks that read nothing of the context are abi.cpp's.
struct FoldinRecommend {
  int32_t top_n;
  bool exclude_rated;
  int32_t* ids_out;
  double* scores_out;  // may be null
  int32_t* counts_out;
};
void als_foldin(mf_ctx* ctx, int side, const int64_t* off, const int32_t* ids, const double* r, int64_t nq,
                const AlsParams& P, const FoldinRecommend* rec, double* vecs_out, int32_t* used_out);
// mf_als_remove / mf_als_remove_rows / mf_als_retract (which checks everything mf_als_run_rows would refuse
// before it removes); each returns the ratings removed.  found: n bytes or null.
int64_t als_remove(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, uint8_t* found);
int64_t als_remove_rows(mf_ctx* ctx, int side, const int32_t* ids, int64_t n_ids);
int64_t als_retract(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, const AlsParams& P, int32_t rounds,
                    uint8_t* found, int64_t* solved_users, int64_t* solved_items);
// Which stored entry each batch entry removes (the rule the removal kernels follow, mf_debug_als_remove_select):
// in ascending j, entry j takes the first position of row batch_row[j] that holds batch_col[j] and that no
// earlier entry took; pos_out[j] = that position in cols[], or -1.
void als_remove_select(const int64_t* off, int64_t rows, const int32_t* cols, const int32_t* batch_row,
                       const int32_t* batch_col, int64_t n, int64_t* pos_out);
void als_debug_csr(mf_ctx* ctx, int side, int64_t* off_out, int32_t* cols_out, double* vals_out, int32_t* npos_out,
                   int64_t cap_rows, int64_t cap_nnz, int64_t* rows_out, int64_t* nnz_out);
// Where the entries of a side land when a batch is appended (the rule the append kernels follow): new_off
// [new_rows + 1] from old_off[old_rows + 1] and the batch's rows (each < new_rows), and per batch entry j its
// position in the new arrays; an old entry p of row x moves to p + new_off[x] - old_off[x].  mf_als_append
// itself takes only new_off from here (batch_pos == null): k_als_place derives a batch entry's position from
// the sorted keys; batch_pos states the same rule for mf_debug_als_append_placement.
void als_append_placement(const int64_t* old_off, int64_t old_rows, const uint32_t* batch_row, int64_t n,
                          int64_t new_rows, int64_t* new_off, int64_t* batch_pos);
// The factor rows of a rating list for mf_als_prepare, mf_als_append and mf_bpr_fit.  ur / ir hold the rows of
// the ids the model has (lookup_rows); ids it does not have take new rows in order of appearance, the user
// looked at before the item within one rating, with the initial values a DSGD fit gives them times init_scale
// (in f64, before the rounding to the context's precision).
void als_insert_rows(mf_ctx* ctx, Shard& s, const int32_t* u, const int32_t* i, int64_t n, std::vector<uint32_t>& ur,
                     std::vector<uint32_t>& ir, double init_scale = 1.0);

// bpr.cpp: BPR training on the resident seen set.  The argument checks that read nothing of the context are
// bpr_check_params'; every entry validates before it changes anything.
void bpr_check_params(const mf_bpr_params& p, bool sampled);
void bpr_check_steps(int64_t first_step, int64_t steps);
void bpr_run(mf_ctx* ctx, const mf_bpr_params& p, int64_t first_step, int64_t steps, mf_bpr_stats* out);
void bpr_step_triples(mf_ctx* ctx, const mf_bpr_params& p, const int32_t* u, const int32_t* pos, const int32_t* neg,
                      int64_t n, mf_bpr_stats* out);
void bpr_fit(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, double init_scale, const mf_bpr_params& p,
             int64_t steps, mf_bpr_stats* out);
void bpr_debug_triples(mf_ctx* ctx, int32_t* u, int32_t* pos, int32_t* neg, int64_t cap, int64_t* n_out);

// nnls.cpp: mf_nnls_solve
void nnls_solve_host(int32_t k, const double* A, const double* b, bool f64, double* x_out, int32_t* iters_out,
                     int32_t* reason_out);

}  // namespace mfhip
