// als.cpp -- ALS training (mf_als_prepare / mf_als_run / mf_als_fit, their _implicit, _cg, _implicit_cg,
// _nonneg and _implicit_nonneg variants), incremental ALS (mf_als_append / mf_als_run_rows / mf_als_update),
// removal (mf_als_remove / mf_als_remove_rows / mf_als_retract), the objective (mf_als_objective /
// mf_als_run_until) and their testing hooks.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <functional>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "common.hpp"
#include "context.hpp"
#include "jvm_random.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mfhip {

// ---------------------------------------------------------------------------------------
// ALS (mf_als_prepare / mf_als_run; kernels_als.hip), single shard.  prepare resolves the ids
// (unseen ones get rows as in an online batch, initialised like a DSGD fit's), builds each side's
// CSR on the host with a stable counting sort (ratings of a row in the caller's order) and uploads
// it with the work lists; a half-sweep is then launches only.
constexpr int64_t kAlsChunk = 16384;     // ratings per work item of a long row (MFHIP_TEST als_chunk=N)
constexpr int64_t kAlsBatch = 16384;     // rows per launch (MFHIP_TEST als_batch=B)
constexpr int64_t kAlsBatchSlots = 2048; // partial systems per launch: a new launch starts past this
// Rated rows per workgroup of k_als_gram (MFHIP_TEST als_gram_slice=N): 32 tiles.  A constant of the
// data, never of the device, so G's summation order is the same everywhere; at 480,189 rows it gives
// 469 workgroups and 30 MB of f32 partials at k = 128.
constexpr int64_t kAlsGramSlice = 1024;

void als_check(const mf_ctx* ctx) {
  if (ctx->rank_mode || ctx->shards.size() != 1)
    fail(MF_ERR_STATE, "ALS runs on a single-process context on one device");
  MF_REQUIRE(ctx->P.num_factors <= kAlsMaxRank,
             "ALS supports a rank of at most " + std::to_string(kAlsMaxRank) +
                 " (the widest instance of the half-sweep kernels); this context has k = " +
                 std::to_string(ctx->P.num_factors));
}

void als_check_alpha(double alpha) {
  MF_REQUIRE(alpha >= 0.0 && std::isfinite(alpha), "implicit ALS needs a finite alpha >= 0");
}

void als_check_run(const AlsParams& P) {
  MF_REQUIRE(P.lambda > 0.0 && std::isfinite(P.lambda), "ALS needs lambda > 0");
  MF_REQUIRE(P.reg == MF_ALS_REG_WEIGHTED || P.reg == MF_ALS_REG_PLAIN, "unknown ALS regularisation (reg)");
  MF_REQUIRE(P.cg_steps >= 0 && P.cg_steps <= MF_ALS_CG_MAX_STEPS,
             "cg_steps must lie in 1 .. " + std::to_string(MF_ALS_CG_MAX_STEPS));
}

namespace {

// The chunk, batch, Gram-slice and slab values mf_als_prepare reads now (the constants above, the MFHIP_TEST
// knobs, the device's CU count): what a prepare keeps in the context, and what a fold-in on a context without
// prepared data cuts its work by.
struct AlsCuts {
  int64_t chunk, batch, gram_slice, slabs;
};
AlsCuts als_cuts_now(const mf_ctx* ctx, const Shard& s) {
  AlsCuts c{kAlsChunk, kAlsBatch, kAlsGramSlice, 0};
  if (const std::string v = test_knob("als_chunk"); !v.empty()) c.chunk = std::max<int64_t>(1, std::atoll(v.c_str()));
  if (const std::string v = test_knob("als_batch"); !v.empty()) c.batch = std::max<int64_t>(1, std::atoll(v.c_str()));
  if (const std::string v = test_knob("als_gram_slice"); !v.empty())
    c.gram_slice = std::min<int64_t>(std::max<int64_t>(1, std::atoll(v.c_str())), 1 << 30);
  c.slabs = als_wide_slabs(ctx->P.num_factors, ctx->f64, static_cast<int>(device_cu_count(s.device)));
  if (const std::string v = test_knob("als_slabs"); !v.empty())
    c.slabs = std::min<int64_t>(c.slabs, std::max<int64_t>(1, std::atoll(v.c_str())));
  return c;
}

// Cuts rows into work items, long-row splits and launches: what mf_als_prepare and mf_als_append do for
// every rated row of a side and mf_als_run_rows for the rows of one call.  Rows are added in ascending order.
struct AlsCutter {
  std::vector<AlsItem>& items;
  std::vector<AlsSplit>& splits;
  std::vector<mf_ctx::AlsBatch>& batches;
  int64_t& max_slots;
  int64_t chunk, batch;
  mf_ctx::AlsBatch cur{0, 0, 0, 0};
  int64_t cur_rows = 0, cur_slots = 0;
  void close() {
    if (cur.items > 0) batches.push_back(cur);
    max_slots = std::max(max_slots, cur_slots);
    cur = {static_cast<int64_t>(items.size()), 0, static_cast<int64_t>(splits.size()), 0};
    cur_rows = cur_slots = 0;
  }
  // row's c >= 1 ratings at [begin, begin + c) of the CSR, npos of them > 0
  void add(int64_t row, int64_t begin, int64_t c, int32_t npos) {
    MF_REQUIRE(c <= INT32_MAX, "ALS: a row has more than 2^31 - 1 ratings");
    const int64_t nch = c <= chunk ? 1 : (c + chunk - 1) / chunk;
    if (cur_rows >= batch || (nch > 1 && cur_slots > 0 && cur_slots + nch > kAlsBatchSlots)) close();
    if (nch == 1) {
      items.push_back({begin, static_cast<int32_t>(row), static_cast<int32_t>(c), -1, npos});
      cur.items += 1;
    } else {
      for (int64_t ch = 0; ch < nch; ++ch)
        items.push_back({begin + ch * chunk, static_cast<int32_t>(row),
                         static_cast<int32_t>(std::min(chunk, c - ch * chunk)), static_cast<int32_t>(cur_slots + ch), npos});
      splits.push_back({static_cast<int32_t>(row), static_cast<int32_t>(cur_slots), static_cast<int32_t>(nch),
                        static_cast<int32_t>(c), npos});
      cur.items += nch;
      cur.splits += 1;
      cur_slots += nch;
    }
    ++cur_rows;
  }
};

void als_upload(DevBuf& d, const void* src, size_t bytes) {
  d.alloc(std::max<size_t>(bytes, 16));
  if (bytes) MF_HIP(hipMemcpy(d.get(), src, bytes, hipMemcpyHostToDevice));
}

// A side's work lists from the shape of its CSR -- off[rows + 1] and per row its ratings > 0 -- with the
// chunk and batch lengths mf_als_prepare read: the long-row chunking, the launch batches and the rated-row
// list that G is summed over, on the host and on the device.  The one routine behind mf_als_prepare and
// mf_als_append; the conjugate-gradient work lists are rebuilt on their next use.
void als_work_lists(mf_ctx* ctx, Shard& s, int side, std::vector<int64_t> off, std::vector<int32_t> npos) {
  mf_ctx::AlsSide& A = ctx->als[side];
  A = mf_ctx::AlsSide();
  const int64_t rows = static_cast<int64_t>(off.size()) - 1;
  AlsCutter cut{A.items, A.splits, A.batches, A.max_slots, ctx->als_chunk, ctx->als_batch};
  std::vector<int32_t> rated;
  for (int64_t row = 0; row < rows; ++row) {
    const int64_t c = off[row + 1] - off[row];
    if (c == 0) continue;
    rated.push_back(static_cast<int32_t>(row));
    cut.add(row, off[row], c, npos[row]);
  }
  cut.close();
  A.rated = static_cast<int64_t>(rated.size());
  A.off = std::move(off);
  A.npos = std::move(npos);
  DeviceGuard g(s.device);
  als_upload(s.als_items[side], A.items.data(), A.items.size() * sizeof(AlsItem));
  als_upload(s.als_splits[side], A.splits.data(), A.splits.size() * sizeof(AlsSplit));
  als_upload(s.als_rated[side], rated.data(), rated.size() * 4);
}

// The end of an append or a removal: the side takes the fresh arrays its entries were moved into and its work
// lists are rebuilt from the new shape.  d_off / d_cols / d_vals come back holding the OLD arrays, which
// queued moves may still read: the caller frees them only once the stream is done.  (The lists this uploads
// are read by no queued kernel: the moves do not touch them and als_enter drained the half-sweeps.)
void als_adopt_arrays(mf_ctx* ctx, Shard& s, int side, DevBuf& d_off, DevBuf& d_cols, DevBuf& d_vals,
                      std::vector<int64_t> off, std::vector<int32_t> npos) {
  std::swap(s.als_off[side], d_off);
  std::swap(s.als_cols[side], d_cols);
  std::swap(s.als_vals[side], d_vals);
  als_work_lists(ctx, s, side, std::move(off), std::move(npos));
}

template <typename T>
void als_build_side(mf_ctx* ctx, Shard& s, int side, const std::vector<uint32_t>& xr, const std::vector<uint32_t>& yr,
                    const double* r, int64_t n, int64_t rows) {
  std::vector<int64_t> off(static_cast<size_t>(rows) + 1, 0);
  for (int64_t j = 0; j < n; ++j) ++off[xr[j] + 1];
  for (int64_t x = 0; x < rows; ++x) off[x + 1] += off[x];
  std::vector<int32_t> cols(static_cast<size_t>(n));
  std::vector<T> vals(static_cast<size_t>(n));
  {
    std::vector<int64_t> pos(off.begin(), off.end() - 1);
    for (int64_t j = 0; j < n; ++j) {
      const int64_t p = pos[xr[j]]++;
      cols[p] = static_cast<int32_t>(yr[j]);
      vals[p] = static_cast<T>(r[j]);
    }
  }
  std::vector<int32_t> npos(static_cast<size_t>(rows), 0);  // MLlib's numExplicits: the implicit half-sweep's n+
  for (int64_t row = 0; row < rows; ++row) {
    int32_t np = 0;
    for (int64_t p = off[row]; p < off[row + 1]; ++p) np += vals[p] > T(0);
    npos[row] = np;
  }
  {
    DeviceGuard g(s.device);
    als_upload(s.als_cols[side], cols.data(), cols.size() * 4);
    als_upload(s.als_vals[side], vals.data(), vals.size() * sizeof(T));
    als_upload(s.als_off[side], off.data(), off.size() * 8);
  }
  als_work_lists(ctx, s, side, std::move(off), std::move(npos));
}

}  // namespace

// (context.hpp)
void als_insert_rows(mf_ctx* ctx, Shard& s, const int32_t* u, const int32_t* i, int64_t n, std::vector<uint32_t>& ur,
                     std::vector<uint32_t>& ir, double init_scale) {
  const int k = ctx->P.num_factors;
  const int64_t u0 = ctx->U.rows(), i0 = ctx->I.rows();
  std::vector<int32_t> fu, fi;
  for (int64_t j = 0; j < n; ++j) {  // unseen ids take new rows in order of appearance
    if (ur[j] == kRowMiss) ur[j] = static_cast<uint32_t>(online_row(ctx, ctx->U, u[j], fu));
    if (ir[j] == kRowMiss) ir[j] = static_cast<uint32_t>(online_row(ctx, ctx->I, i[j], fi));
  }
  // as in an online batch: new rows take the slab rows a fast DSGD schedule keeps zeroed
  if (ctx->prepared && !ctx->f64 && (!fu.empty() || !fi.empty())) ctx->prepared = false;
  // the initial factors a DSGD fit gives these ids: new Random(id ^ seed) (DSGDforMF.scala:548-549)
  if (ctx->P.has_seed) {
    ctx->init_seed = ctx->P.seed;
  } else if (ctx->init_seed == 0) {
    std::random_device rd;
    ctx->init_seed = (static_cast<int64_t>(rd()) << 32) ^ rd();
  }
  for (int side = 0; side < 2; ++side) {
    const std::vector<int32_t>& fresh = side == kSideU ? fu : fi;
    ensure_rows(ctx, s, side, std::max<int64_t>(side_of(ctx, side).rows(), 1));
    if (fresh.empty()) continue;
    std::vector<double> vec;
    init_vectors(fresh.data(), static_cast<int64_t>(fresh.size()), k, true, ctx->init_seed, vec);
    if (init_scale != 1.0)
      for (double& v : vec) v *= init_scale;
    upload_rows(ctx, s, side, side == kSideU ? u0 : i0, vec.data(), static_cast<int64_t>(fresh.size()));
  }
}

void als_prepare(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n) {
  MF_REQUIRE(n >= 0, "negative rating count");
  MF_REQUIRE(n == 0 || (u && i && r), "null rating arrays");
  als_check(ctx);
  require_healthy(ctx);
  det_spec_wait(ctx, true);  // new ids change the layouts the builds read
  sync_all(ctx);
  Shard& s = ctx->shards[0];
  ctx->als_prepared = false;
  if (!ctx->have_model) {
    ctx->U = SideLayout();
    ctx->I = SideLayout();
    ctx->have_model = true;
    ++ctx->layout_gen;
  }
  std::vector<uint32_t> ur, ir;
  lookup_rows(ctx->U, u, n, ur);
  lookup_rows(ctx->I, i, n, ir);
  als_insert_rows(ctx, s, u, i, n, ur, ir);
  const AlsCuts cuts = als_cuts_now(ctx, s);
  ctx->als_chunk = cuts.chunk;
  ctx->als_batch = cuts.batch;
  ctx->als_gram_slice = cuts.gram_slice;
  ctx->als_slabs = cuts.slabs;
  if (ctx->f64) {
    als_build_side<double>(ctx, s, kSideU, ur, ir, r, n, ctx->U.rows());
    als_build_side<double>(ctx, s, MF_SIDE_ITEM, ir, ur, r, n, ctx->I.rows());
  } else {
    als_build_side<float>(ctx, s, kSideU, ur, ir, r, n, ctx->U.rows());
    als_build_side<float>(ctx, s, MF_SIDE_ITEM, ir, ur, r, n, ctx->I.rows());
  }
  {
    DeviceGuard g(s.device);
    s.als_nnls_stats.alloc(sizeof(struct mf_als_nonneg_stats));
    MF_HIP(hipMemset(s.als_nnls_stats.get(), 0, sizeof(struct mf_als_nonneg_stats)));
  }
  ctx->als_prepared = true;
  ctx->als_half_sweeps = 0;
}

namespace {

// What every entry past mf_als_prepare starts with; `api` is the name in the MF_ERR_STATE text.
Shard& als_enter(mf_ctx* ctx, const std::string& api) {
  als_check(ctx);
  if (!ctx->als_prepared) fail(MF_ERR_STATE, api + " before mf_als_prepare");
  require_healthy(ctx);
  sync_all(ctx);
  return ctx->shards[0];
}

// n elements of a device buffer in the context's precision as host doubles, and the way back.
std::vector<double> read_as_f64(const mf_ctx* ctx, const DevBuf& d, size_t n) {
  std::vector<double> h(n);
  if (ctx->f64) {
    MF_HIP(hipMemcpy(h.data(), d.get(), n * 8, hipMemcpyDeviceToHost));
  } else {
    std::vector<float> f(n);
    MF_HIP(hipMemcpy(f.data(), d.get(), n * 4, hipMemcpyDeviceToHost));
    for (size_t x = 0; x < n; ++x) h[x] = static_cast<double>(f[x]);
  }
  return h;
}

void write_from_f64(const mf_ctx* ctx, DevBuf& d, const double* src, size_t n) {
  d.alloc(std::max<size_t>(n * ctx->es, 16));
  if (ctx->f64) {
    MF_HIP(hipMemcpy(d.get(), src, n * 8, hipMemcpyHostToDevice));
  } else {
    std::vector<float> f(n);
    for (size_t x = 0; x < n; ++x) f[x] = static_cast<float>(src[x]);
    MF_HIP(hipMemcpy(d.get(), f.data(), n * 4, hipMemcpyHostToDevice));
  }
}

// G of rows rated[0 .. m) of `side` into s.als_gram, in slices of `slice` rows, on the shard's stream: two
// launches.
void als_gram_launch(mf_ctx* ctx, Shard& s, int side, const int32_t* rated, int64_t m64, int64_t slice64) {
  const int k = ctx->P.num_factors;
  const int m = static_cast<int>(m64), slice = static_cast<int>(slice64);
  const size_t ge = als_gram_elems(k) * ctx->es;
  s.als_gram_part.alloc(std::max<size_t>(static_cast<size_t>(als_gram_slices(m, slice)) * ge, 16));
  s.als_gram.alloc(ge);
  launch_als_gram({s.stream, rated, m, slice, side == kSideU ? s.uf.get() : s.itf.get(), k, ctx->f64,
                   s.als_gram_part.get(), s.als_gram.get()});
  MF_HIP(hipGetLastError());
}
// ... of `side`'s rated rows as the prepared data lists them
void als_gram_launch(mf_ctx* ctx, Shard& s, int side) {
  als_gram_launch(ctx, s, side, s.als_rated[side].as<int32_t>(), ctx->als[side].rated, ctx->als_gram_slice);
}

// The chunk items of `side`'s long rows, per batch, with the index of each one's row among the batch's splits.
void als_cg_work(const std::vector<AlsItem>& items, const std::vector<AlsSplit>& splits,
                 const std::vector<mf_ctx::AlsBatch>& batches, std::vector<AlsCgWork>& work, std::vector<int64_t>& work0,
                 int64_t& max_splits) {
  work.clear();
  work0.assign(1, 0);
  max_splits = 0;
  for (const mf_ctx::AlsBatch& b : batches) {
    int64_t sp = b.split0;
    for (int64_t x = b.item0; x < b.item0 + b.items; ++x) {
      const AlsItem& it = items[static_cast<size_t>(x)];
      if (it.slot < 0) continue;
      while (splits[static_cast<size_t>(sp)].row != it.row) ++sp;  // both lists are in row order
      work.push_back({static_cast<int32_t>(x - b.item0), static_cast<int32_t>(sp - b.split0)});
    }
    work0.push_back(static_cast<int64_t>(work.size()));
    max_splits = std::max(max_splits, b.splits);
  }
}

void als_cg_lists(mf_ctx* ctx, Shard& s, int side) {
  mf_ctx::AlsSide& A = ctx->als[side];
  if (A.cg_ready) return;
  als_cg_work(A.items, A.splits, A.batches, A.cg_work, A.cg_work0, A.cg_max_splits);
  als_upload(s.als_cg_work[side], A.cg_work.data(), A.cg_work.size() * sizeof(AlsCgWork));
  A.cg_ready = true;
}

// The work of one row (the testing hooks) in the form of a batch: its items and, if it is a long row,
// its split; items == 0 if the row has no rating.
mf_ctx::AlsBatch als_row_span(const mf_ctx::AlsSide& A, int64_t row) {
  auto lo = std::lower_bound(A.items.begin(), A.items.end(), row,
                             [](const AlsItem& a, int64_t r) { return a.row < r; });
  auto hi = lo;
  while (hi != A.items.end() && hi->row == row) ++hi;
  auto sp = std::lower_bound(A.splits.begin(), A.splits.end(), row,
                             [](const AlsSplit& a, int64_t r) { return a.row < r; });
  return {lo - A.items.begin(), hi - lo, sp - A.splits.begin(), sp != A.splits.end() && sp->row == row ? 1 : 0};
}

// The device copies of a call's work lists: the side's own, or those of one mf_als_run_rows / fold-in batch.
struct AlsWork {
  const AlsItem* items;
  const AlsSplit* splits;
  const AlsCgWork* work;
};

// What the launches of one call share beyond the CSR, the slabs Q and X and the NNLS counters (the caller's):
// the regularisation and the solver's switches, and the scratch sized by the call's work W -- the long rows'
// partial slots, the conjugate-gradient state of a launch's long rows or (k > 128) the normal-matrix slabs.
void als_launch_setup(mf_ctx* ctx, Shard& s, AlsLaunch& L, const AlsParams& P, const mf_ctx::AlsSide& W, int64_t slabs) {
  const int k = ctx->P.num_factors;
  s.als_part.alloc(std::max<size_t>(static_cast<size_t>(W.max_slots) * als_partial_elems(k) * ctx->es, 16));
  L.k = k;
  L.lambda = P.lambda;
  L.weighted = P.reg == MF_ALS_REG_WEIGHTED;
  L.f64 = ctx->f64;
  L.partial = s.als_part.get();
  L.alpha = P.alpha;
  if (P.cg_steps > 0) {
    s.als_cg_state.alloc(std::max<size_t>(static_cast<size_t>(std::max<int64_t>(W.cg_max_splits, 1)) *
                                              als_cg_state_elems(k) * ctx->es, 16));
    L.steps = P.cg_steps;
    L.stage = test_knob("als_cg_stage") != "0";
    L.state = s.als_cg_state.get();
  } else {
    // k > 128: one normal matrix in global memory per workgroup of the grid, however many rows there are
    L.slabs = static_cast<int>(std::min<int64_t>(slabs, static_cast<int64_t>(W.items.size())));
    if (L.slabs > 0) s.als_slab.alloc(static_cast<size_t>(L.slabs) * als_gram_elems(k) * ctx->es);
    L.slab = s.als_slab.get();
    L.nnls = P.nnls;
  }
}

void als_launch_one(AlsLaunch& L, bool cg, const AlsWork& D, const mf_ctx::AlsBatch& b) {
  L.items = D.items + b.item0;
  L.n_items = static_cast<int>(b.items);
  L.splits = D.splits + b.split0;
  L.n_splits = static_cast<int>(b.splits);
  cg ? launch_als_cg(L) : launch_als(L);
  MF_HIP(hipGetLastError());
}

// The launch loop of a half-sweep, of mf_als_run_rows and of a fold-in batch: W's batches in order, after G
// (gram != null: the implicit system, G made by *gram before the first launch; a caller that made G itself
// sets L.gram and passes null).
void als_launch_batches(mf_ctx* ctx, Shard& s, AlsLaunch& L, const AlsParams& P, const mf_ctx::AlsSide& W,
                        const AlsWork& D, const std::function<void()>* gram) {
  const bool cg = P.cg_steps > 0;
  LaunchTimer t(s, ctx->profiling);
  if (gram && !W.batches.empty()) {
    (*gram)();
    ctx->stats.kernel_launches += 2;
  }
  for (size_t b = 0; b < W.batches.size(); ++b) {
    const mf_ctx::AlsBatch& B = W.batches[b];
    if (cg) {
      L.work = D.work + W.cg_work0[b];
      L.n_work = static_cast<int>(W.cg_work0[b + 1] - W.cg_work0[b]);
    }
    als_launch_one(L, cg, D, B);
    ctx->stats.kernel_launches += 1 + (B.splits > 0 ? (cg ? 2 * (P.cg_steps + 1) : 1) : 0);
  }
}

// One side solved from the other (P.implicit: after the counterpart's Gram matrix), by Cholesky, with
// P.nnls by the non-negative solve in its place or, with P.cg_steps > 0, by conjugate gradients on the
// same work lists, batches and partial slots.
// only_row >= 0 (the testing hooks): that row's work items alone, and s.als_dump takes the row's system
// (Cholesky), x with its iteration count and reason code (the non-negative solve) or A v and b for the v
// in s.als_cg_v (conjugate gradients) instead of the row being solved; false if the row has no rating.
// rows != null (mf_als_run_rows): those rows alone -- ascending, distinct, each with a rating -- from work
// lists of their own, cut as the side's are (fresh slot numbers for the long rows, launches by the same
// batch and slot limits); the kernels, the CSR and G are the full half-sweep's.
bool als_half(mf_ctx* ctx, int side, const AlsParams& P, int64_t only_row = -1,
              const std::vector<int32_t>* rows = nullptr) {
  Shard& s = ctx->shards[0];
  DeviceGuard g(s.device);
  mf_ctx::AlsSide& A = ctx->als[side];
  const int k = ctx->P.num_factors;
  const bool cg = P.cg_steps > 0;
  const int other = side == kSideU ? MF_SIDE_ITEM : kSideU;
  mf_ctx::AlsSide sub;
  if (rows) {
    AlsCutter cut{sub.items, sub.splits, sub.batches, sub.max_slots, ctx->als_chunk, ctx->als_batch};
    for (const int32_t row : *rows) cut.add(row, A.off[row], A.off[row + 1] - A.off[row], A.npos[row]);
    cut.close();
    als_upload(s.als_sub_items, sub.items.data(), sub.items.size() * sizeof(AlsItem));
    als_upload(s.als_sub_splits, sub.splits.data(), sub.splits.size() * sizeof(AlsSplit));
    if (cg) {
      als_cg_work(sub.items, sub.splits, sub.batches, sub.cg_work, sub.cg_work0, sub.cg_max_splits);
      als_upload(s.als_sub_work, sub.cg_work.data(), sub.cg_work.size() * sizeof(AlsCgWork));
    }
  } else if (cg) {
    als_cg_lists(ctx, s, side);
  }
  const mf_ctx::AlsSide& W = rows ? sub : A;  // the work of this call
  const AlsWork D{rows ? s.als_sub_items.as<AlsItem>() : s.als_items[side].as<AlsItem>(),
                  rows ? s.als_sub_splits.as<AlsSplit>() : s.als_splits[side].as<AlsSplit>(),
                  rows ? s.als_sub_work.as<AlsCgWork>() : s.als_cg_work[side].as<AlsCgWork>()};
  AlsLaunch L;
  L.st = s.stream;
  L.cols = s.als_cols[side].as<int32_t>();
  L.vals = s.als_vals[side].get();
  L.Q = side == kSideU ? s.itf.get() : s.uf.get();
  L.X = side == kSideU ? s.uf.get() : s.itf.get();
  L.nnls_stats = s.als_nnls_stats.get();
  als_launch_setup(ctx, s, L, P, W, ctx->als_slabs);
  const std::function<void()> gram = [&] {
    als_gram_launch(ctx, s, other);
    L.gram = s.als_gram.get();
  };
  if (only_row >= 0) {
    const mf_ctx::AlsBatch row = als_row_span(A, only_row);
    if (row.items == 0) return false;
    if (cg && row.splits) {  // the row's chunks, as items [0, n) of the launch and long row 0
      std::vector<AlsCgWork> w(static_cast<size_t>(row.items));
      for (int32_t x = 0; x < row.items; ++x) w[static_cast<size_t>(x)] = {x, 0};
      s.als_cg_hook_work.alloc(w.size() * sizeof(AlsCgWork));
      MF_HIP(hipMemcpy(s.als_cg_hook_work.get(), w.data(), w.size() * sizeof(AlsCgWork), hipMemcpyHostToDevice));
      L.work = s.als_cg_hook_work.as<AlsCgWork>();
      L.n_work = static_cast<int>(row.items);
    }
    s.als_dump.alloc(std::max<size_t>((static_cast<size_t>(k) * k + k + 2) * ctx->es, 16));
    L.dump = s.als_dump.get();
    L.hook_v = s.als_cg_v.get();
    if (P.implicit) gram();
    als_launch_one(L, cg, D, row);
    return true;
  }
  als_launch_batches(ctx, s, L, P, W, D, P.implicit ? &gram : nullptr);
  return true;
}

// The hooks' row: the id's row on `side`, solved as als_half's only_row.
void als_hook_row(mf_ctx* ctx, int side, int32_t id, const AlsParams& P) {
  const int32_t row = side_of(ctx, side).index.find(id);
  MF_REQUIRE(row >= 0, "unknown id");
  MF_REQUIRE(als_half(ctx, side, P, row), "the id has no rating in the prepared data");
  DeviceGuard g(ctx->shards[0].device);
  MF_HIP(hipStreamSynchronize(ctx->shards[0].stream));
}

}  // namespace

void als_run(mf_ctx* ctx, int64_t half_sweeps, const AlsParams& P) {
  if (P.implicit) als_check_alpha(P.alpha);
  MF_REQUIRE(half_sweeps >= 0, "negative half-sweep count");
  als_check_run(P);
  als_enter(ctx, std::string("mf_als_run") + (P.implicit ? "_implicit" : "") + (P.cg_steps ? "_cg" : "") +
                     (P.nnls ? "_nonneg" : ""));
  for (int64_t h = 0; h < half_sweeps; ++h) {
    // MLlib's order: the item side from the user factors first
    als_half(ctx, ctx->als_half_sweeps % 2 == 0 ? MF_SIDE_ITEM : kSideU, P);
    ++ctx->als_half_sweeps;
  }
  DeviceGuard g(ctx->shards[0].device);
  MF_HIP(hipStreamSynchronize(ctx->shards[0].stream));
}

// ---------------------------------------------------------------------------------------
// The objective (mf_als_objective, kernels_als_objective.hip): a gather-and-reduce pass over the user side's
// CSR and work list, a row-norm pass per side, and with P.implicit the two Gram matrices and their trace.
// Everything is queued on the shard's stream and four doubles come back behind one synchronisation; nothing
// of the context changes but scratch.
void als_check_objective(const AlsParams& P) {
  MF_REQUIRE(P.lambda >= 0.0 && std::isfinite(P.lambda), "the ALS objective needs a finite lambda >= 0");
  MF_REQUIRE(P.reg == MF_ALS_REG_WEIGHTED || P.reg == MF_ALS_REG_PLAIN, "unknown ALS regularisation (reg)");
  if (P.implicit) als_check_alpha(P.alpha);
}

namespace {

// The call on an entered context (als_enter): mf_als_objective, and every J of mf_als_run_until.
void als_objective_entered(mf_ctx* ctx, Shard& s, const AlsParams& P, struct mf_als_loss* out) {
  std::memset(out, 0, sizeof(*out));
  const mf_ctx::AlsSide& AU = ctx->als[kSideU];
  const mf_ctx::AlsSide& AI = ctx->als[MF_SIDE_ITEM];
  const int64_t n = AU.off.empty() ? 0 : AU.off.back();
  out->ratings = n;
  out->user_rows = AU.rated;
  out->item_rows = AI.rated;
  if (n == 0) return;
  DeviceGuard g(s.device);
  const int k = ctx->P.num_factors;
  const int64_t n_items = static_cast<int64_t>(AU.items.size());
  // (the stream is drained here: scratch may grow)
  s.als_obj_part.alloc(static_cast<size_t>(std::max({n_items, AU.rated, AI.rated})) * 8);
  s.als_obj_out.alloc(4 * 8);
  double* const part = s.als_obj_part.as<double>();
  double* const res = s.als_obj_out.as<double>();  // fit, unobserved, R_user, R_item
  // MFHIP_TIMING=1: the parts on stderr, the stream drained after each (a diagnostic run)
  PhaseClock clk;
  auto lap = [&](const char* what) {
    if (!clk.on) return;
    MF_HIP(hipStreamSynchronize(s.stream));
    clk.lap(what);
  };
  MF_HIP(hipMemsetAsync(res, 0, 4 * 8, s.stream));
  launch_als_objective_fit({s.stream, s.als_items[kSideU].as<AlsItem>(), n_items, s.als_cols[kSideU].as<int32_t>(),
                            s.als_vals[kSideU].get(), s.uf.get(), s.itf.get(), k, ctx->f64, P.implicit, P.alpha, part});
  launch_sum64(s.stream, part, n_items, res + 0);
  MF_HIP(hipGetLastError());
  lap("objective fit");
  const int weight = P.reg == MF_ALS_REG_WEIGHTED ? (P.implicit ? 2 : 1) : 0;
  for (int side = 0; side < 2; ++side) {
    const int64_t m = ctx->als[side].rated;
    launch_als_objective_norms(s.stream, s.als_rated[side].as<int32_t>(), m, s.als_off[side].as<int64_t>(),
                               s.als_vals[side].get(), side == kSideU ? s.uf.get() : s.itf.get(), k, ctx->f64, weight,
                               part);
    launch_sum64(s.stream, part, m, res + 2 + side);
  }
  MF_HIP(hipGetLastError());
  lap("objective norms");
  ctx->stats.kernel_launches += 6;
  if (P.implicit) {
    const size_t ge = als_gram_elems(k) * ctx->es;
    s.als_obj_gram.alloc(ge);
    als_gram_launch(ctx, s, kSideU);
    MF_HIP(hipMemcpyAsync(s.als_obj_gram.get(), s.als_gram.get(), ge, hipMemcpyDeviceToDevice, s.stream));
    als_gram_launch(ctx, s, MF_SIDE_ITEM);
    launch_als_objective_trace(s.stream, s.als_obj_gram.get(), s.als_gram.get(), k, ctx->f64, res + 1);
    MF_HIP(hipGetLastError());
    ctx->stats.kernel_launches += 5;
    lap("objective gram + trace");
  }
  double h[4];
  MF_HIP(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, s.stream));
  MF_HIP(hipStreamSynchronize(s.stream));
  const double lam = ctx->f64 ? P.lambda : static_cast<double>(static_cast<float>(P.lambda));
  out->fit = h[0];
  out->unobserved = h[1];
  out->reg_user = lam * h[2];
  out->reg_item = lam * h[3];
  out->total = ((out->fit + out->unobserved) + out->reg_user) + out->reg_item;
}

}  // namespace

void als_objective(mf_ctx* ctx, const AlsParams& P, struct mf_als_loss* out) {
  als_check_objective(P);
  Shard& s = als_enter(ctx, "mf_als_objective");
  als_objective_entered(ctx, s, P, out);
}

int32_t als_run_until(mf_ctx* ctx, const AlsParams& P, int32_t max_iterations, double rel_tol, double* history) {
  als_check_objective(P);
  als_check_run(P);
  MF_REQUIRE(max_iterations >= 0, "negative iteration count");
  MF_REQUIRE(rel_tol >= 0.0 && std::isfinite(rel_tol), "rel_tol must be finite and >= 0");
  Shard& s = als_enter(ctx, "mf_als_run_until");
  struct mf_als_loss loss;
  als_objective_entered(ctx, s, P, &loss);
  double prev = loss.total;
  if (history) history[0] = prev;
  int32_t t = 0;
  while (t < max_iterations) {
    als_run(ctx, 2, P);
    als_objective_entered(ctx, s, P, &loss);
    ++t;
    const double now = loss.total;
    if (history) history[t] = now;
    if (!std::isfinite(now) || prev - now <= rel_tol * std::fabs(prev)) break;
    prev = now;
  }
  return t;
}

// The normal equations of one row as the kernel accumulates them (mf_debug_als_normal_eq, and with
// P.implicit mf_debug_als_normal_eq_implicit).
void als_normal_eq(mf_ctx* ctx, int side, int32_t id, const AlsParams& P, double* A_out, double* b_out) {
  if (P.implicit) als_check_alpha(P.alpha);
  als_check_run(P);
  Shard& s = als_enter(ctx, std::string("mf_debug_als_normal_eq") + (P.implicit ? "_implicit" : ""));
  als_hook_row(ctx, side, id, P);
  DeviceGuard g(s.device);
  const size_t k = static_cast<size_t>(ctx->P.num_factors);
  const std::vector<double> h = read_as_f64(ctx, s.als_dump, k * k + k);
  std::memcpy(A_out, h.data(), k * k * 8);
  std::memcpy(b_out, h.data() + k * k, k * 8);
}

// A v and b of one row through the conjugate-gradient half-sweep's own kernels (mf_debug_als_cg_matvec).
void als_cg_matvec(mf_ctx* ctx, int side, int32_t id, const AlsParams& P, const double* v, double* Av_out,
                   double* b_out) {
  if (P.implicit) als_check_alpha(P.alpha);
  als_check_run(P);
  Shard& s = als_enter(ctx, "mf_debug_als_cg_matvec");
  DeviceGuard g(s.device);
  const size_t k = static_cast<size_t>(ctx->P.num_factors);
  write_from_f64(ctx, s.als_cg_v, v, k);
  als_hook_row(ctx, side, id, P);
  const std::vector<double> h = read_as_f64(ctx, s.als_dump, 2 * k);
  std::memcpy(Av_out, h.data(), k * 8);
  std::memcpy(b_out, h.data() + k, k * 8);
}

// One row through the non-negative half-sweep's own kernels (mf_debug_als_nnls_row): x, its iteration
// count and its reason code.
void als_nnls_row(mf_ctx* ctx, int side, int32_t id, const AlsParams& P, double* x_out, int32_t* iters_out,
                  int32_t* reason_out) {
  if (P.implicit) als_check_alpha(P.alpha);
  als_check_run(P);
  Shard& s = als_enter(ctx, "mf_debug_als_nnls_row");
  als_hook_row(ctx, side, id, P);
  DeviceGuard g(s.device);
  const size_t k = static_cast<size_t>(ctx->P.num_factors);
  const std::vector<double> h = read_as_f64(ctx, s.als_dump, k + 2);
  std::memcpy(x_out, h.data(), k * 8);
  *iters_out = static_cast<int32_t>(h[k]);
  *reason_out = static_cast<int32_t>(h[k + 1]);
}

// The device counters of the non-negative half-sweeps since mf_als_prepare (mf_als_nonneg_stats).
void als_nonneg_stats(mf_ctx* ctx, struct mf_als_nonneg_stats* out) {
  Shard& s = als_enter(ctx, "mf_als_nonneg_stats");
  DeviceGuard g(s.device);
  MF_HIP(hipMemcpy(out, s.als_nnls_stats.get(), sizeof(struct mf_als_nonneg_stats), hipMemcpyDeviceToHost));
}

// G of one side's rated rows through the half-sweep's own launches (mf_debug_als_gram).
void als_gram(mf_ctx* ctx, int side, double* G_out) {
  Shard& s = als_enter(ctx, "mf_debug_als_gram");
  DeviceGuard g(s.device);
  {
    LaunchTimer t(s, ctx->profiling);
    als_gram_launch(ctx, s, side);
  }
  MF_HIP(hipStreamSynchronize(s.stream));
  const size_t k = static_cast<size_t>(ctx->P.num_factors), kp = (k + 31) / 32 * 32;
  const std::vector<double> h = read_as_f64(ctx, s.als_gram, kp * kp);
  for (size_t a = 0; a < k; ++a) std::memcpy(G_out + a * k, h.data() + a * kp, k * 8);
}

// ---------------------------------------------------------------------------------------
// Incremental ALS: mf_als_append repacks both CSRs on the device with the batch in (kernels_als_append.hip),
// mf_als_run_rows solves named rows through als_half, mf_als_update is the two in sequence.

void als_append_placement(const int64_t* old_off, int64_t old_rows, const uint32_t* batch_row, int64_t n,
                          int64_t new_rows, int64_t* new_off, int64_t* batch_pos) {
  std::vector<int64_t> add(static_cast<size_t>(new_rows), 0);
  for (int64_t j = 0; j < n; ++j) ++add[batch_row[j]];
  new_off[0] = 0;
  for (int64_t x = 0; x < new_rows; ++x)
    new_off[x + 1] = new_off[x] + (x < old_rows ? old_off[x + 1] - old_off[x] : 0) + add[x];
  if (!batch_pos) return;
  for (int64_t x = 0; x < new_rows; ++x) add[x] = new_off[x + 1] - add[x];  // where the row's new entries begin
  for (int64_t j = 0; j < n; ++j) batch_pos[j] = add[batch_row[j]]++;
}

namespace {

// One side of mf_als_append: its new offsets and n+ on the host, its entries moved on the device into fresh
// arrays (the old ones go to `retired`, to be freed once the stream is done), its work lists rebuilt.
template <typename T>
void als_append_side(mf_ctx* ctx, Shard& s, int side, const std::vector<uint32_t>& xr, const T* vals, int64_t n,
                     const uint32_t* d_xr, const uint32_t* d_yr, std::vector<DevBuf>& retired) {
  mf_ctx::AlsSide& A = ctx->als[side];
  const int64_t old_rows = static_cast<int64_t>(A.off.size()) - 1, new_rows = side_of(ctx, side).rows();
  std::vector<int64_t> off(static_cast<size_t>(new_rows) + 1);
  als_append_placement(A.off.data(), old_rows, xr.data(), n, new_rows, off.data(), nullptr);
  std::vector<int32_t> npos(A.npos);
  npos.resize(static_cast<size_t>(new_rows), 0);
  for (int64_t j = 0; j < n; ++j) npos[xr[j]] += vals[j] > T(0);
  DevBuf d_off, d_cols, d_vals;
  als_upload(d_off, off.data(), off.size() * 8);
  d_cols.alloc(std::max<size_t>(static_cast<size_t>(off.back()) * 4, 16));
  d_vals.alloc(std::max<size_t>(static_cast<size_t>(off.back()) * sizeof(T), 16));
  launch_als_append({s.stream, s.als_off[side].as<int64_t>(), old_rows, A.off.back(), d_off.as<int64_t>(), new_rows,
                     s.als_cols[side].as<int32_t>(), s.als_vals[side].get(), d_cols.as<int32_t>(), d_vals.get(),
                     static_cast<int>(sizeof(T)), d_xr, d_yr, s.als_app.val.get(), n},
                    s.als_app);
  als_adopt_arrays(ctx, s, side, d_off, d_cols, d_vals, std::move(off), std::move(npos));
  retired.push_back(std::move(d_off));
  retired.push_back(std::move(d_cols));
  retired.push_back(std::move(d_vals));
}

template <typename T>
void als_append_both(mf_ctx* ctx, Shard& s, const std::vector<uint32_t>& ur, const std::vector<uint32_t>& ir,
                     const double* r, int64_t n) {
  std::vector<T> vals(static_cast<size_t>(n));
  for (int64_t j = 0; j < n; ++j) vals[static_cast<size_t>(j)] = static_cast<T>(r[j]);  // the context's precision
  DeviceGuard g(s.device);
  als_upload(s.als_app.urow, ur.data(), static_cast<size_t>(n) * 4);
  als_upload(s.als_app.irow, ir.data(), static_cast<size_t>(n) * 4);
  als_upload(s.als_app.val, vals.data(), static_cast<size_t>(n) * sizeof(T));
  const uint32_t* d_ur = s.als_app.urow.as<uint32_t>();
  const uint32_t* d_ir = s.als_app.irow.as<uint32_t>();
  // One side at a time, the stream drained between them: the side's old arrays are freed before the other
  // side's new ones are allocated (the transient is a second copy of one side, not of both), and the sort's
  // scratch in s.als_app, which the second side may reallocate, is idle by then.
  for (int side = 0; side < 2; ++side) {
    std::vector<DevBuf> retired;
    if (side == kSideU) als_append_side<T>(ctx, s, kSideU, ur, vals.data(), n, d_ur, d_ir, retired);
    else als_append_side<T>(ctx, s, MF_SIDE_ITEM, ir, vals.data(), n, d_ir, d_ur, retired);
    MF_HIP(hipStreamSynchronize(s.stream));  // `retired` is freed behind the moves
  }
}

}  // namespace

void als_append(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n) {
  MF_REQUIRE(n >= 0, "negative rating count");
  MF_REQUIRE(n < (int64_t{1} << 31), "mf_als_append takes fewer than 2^31 ratings in one call");
  MF_REQUIRE(n == 0 || (u && i && r), "null rating arrays");
  Shard& s = als_enter(ctx, "mf_als_append");
  if (n == 0) return;
  std::vector<uint32_t> ur, ir;
  lookup_rows(ctx->U, u, n, ur);
  lookup_rows(ctx->I, i, n, ir);
  bool fresh = false;
  for (int side = 0; side < 2; ++side) {  // nothing has changed yet: no row may pass 2^31 - 1 ratings
    const mf_ctx::AlsSide& A = ctx->als[side];
    const std::vector<uint32_t>& xr = side == kSideU ? ur : ir;
    const int64_t have = static_cast<int64_t>(A.off.size()) - 1;
    std::vector<int64_t> cnt(static_cast<size_t>(side_of(ctx, side).rows()), 0);
    for (int64_t j = 0; j < n; ++j) {
      if (xr[j] == kRowMiss) {  // (a new row holds at most the n < 2^31 ratings of this call)
        fresh = true;
        continue;
      }
      const int64_t x = xr[j];
      if (cnt[x] == 0 && x < have) cnt[x] = A.off[x + 1] - A.off[x];
      MF_REQUIRE(++cnt[x] <= INT32_MAX, "ALS: a row has more than 2^31 - 1 ratings");
    }
  }
  if (fresh) det_spec_wait(ctx, true);  // new ids change the layouts the builds read
  als_insert_rows(ctx, s, u, i, n, ur, ir);
  ctx->f64 ? als_append_both<double>(ctx, s, ur, ir, r, n) : als_append_both<float>(ctx, s, ur, ir, r, n);
}

int64_t als_run_rows(mf_ctx* ctx, int side, const int32_t* ids, int64_t n_ids, const AlsParams& P) {
  if (P.implicit) als_check_alpha(P.alpha);
  als_check_run(P);
  MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
  MF_REQUIRE(n_ids >= 0, "negative id count");
  MF_REQUIRE(n_ids == 0 || ids, "null id array");
  Shard& s = als_enter(ctx, "mf_als_run_rows");
  const mf_ctx::AlsSide& A = ctx->als[side];
  const SideLayout& S = side_of(ctx, side);
  const int64_t have = static_cast<int64_t>(A.off.size()) - 1;
  std::vector<uint8_t> named(static_cast<size_t>(have), 0);
  for (int64_t j = 0; j < n_ids; ++j) {  // ids the model does not hold and rows without a rating are skipped
    const int32_t row = S.index.find(ids[j]);
    if (row >= 0 && row < have && A.off[row + 1] > A.off[row]) named[row] = 1;
  }
  std::vector<int32_t> rows;  // ascending row order, each row once: no trace of the order of ids[]
  for (int64_t row = 0; row < have; ++row)
    if (named[row]) rows.push_back(static_cast<int32_t>(row));
  if (rows.empty()) return 0;
  als_half(ctx, side, P, -1, &rows);
  DeviceGuard g(s.device);
  MF_HIP(hipStreamSynchronize(s.stream));
  return static_cast<int64_t>(rows.size());
}

void als_update(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, const AlsParams& P,
                int32_t rounds, int64_t* solved_users, int64_t* solved_items) {
  MF_REQUIRE(rounds >= 0, "negative round count");
  if (P.implicit) als_check_alpha(P.alpha);
  als_check_run(P);
  als_append(ctx, u, i, r, n);  // (checks the rest before it changes anything)
  int64_t su = 0, si = 0;
  for (int32_t t = 0; t < rounds; ++t) {
    // users first: a new user's row is random until solved, and items solved from it would be pulled to noise
    su = als_run_rows(ctx, kSideU, u, n, P);
    si = als_run_rows(ctx, MF_SIDE_ITEM, i, n, P);
  }
  if (solved_users) *solved_users = su;
  if (solved_items) *solved_items = si;
}

// ---------------------------------------------------------------------------------------
// Removal: mf_als_remove / mf_als_remove_rows repack both CSRs on the device without the entries that go
// (kernels_als_remove.hip), mf_als_retract is a remove followed by mf_als_run_rows of what it named.

void als_remove_select(const int64_t* off, int64_t rows, const int32_t* cols, const int32_t* batch_row,
                       const int32_t* batch_col, int64_t n, int64_t* pos_out) {
  std::vector<uint8_t> gone(static_cast<size_t>(off[rows]), 0);
  for (int64_t j = 0; j < n; ++j) {  // in ascending j: the oldest remaining instance of the pair
    pos_out[j] = -1;
    for (int64_t p = off[batch_row[j]]; p < off[batch_row[j] + 1]; ++p) {
      if (cols[p] != batch_col[j] || gone[p]) continue;
      gone[p] = 1;
      pos_out[j] = p;
      break;
    }
  }
}

namespace {

// One side of a removal.  The selection runs first and changes nothing; when entries go, the survivors move
// into fresh arrays on the device, the host takes the new offsets and the per-row removed ratings > 0 (it
// holds the shape, never the entries), and the work lists are rebuilt.  Returns the entries that went.
int64_t als_remove_side(mf_ctx* ctx, Shard& s, int side, const uint64_t* d_bkey, int64_t nb, const uint8_t* rowmark,
                        const uint8_t* colmark, uint8_t* d_found) {
  mf_ctx::AlsSide& A = ctx->als[side];
  const int64_t rows = static_cast<int64_t>(A.off.size()) - 1, nnz = A.off.back();
  AlsRemoveScratch& sc = s.als_rem;
  sc.rempos.alloc(std::max<size_t>(static_cast<size_t>(rows) * 4, 16));
  const AlsRemoveLaunch L{s.stream, s.als_off[side].as<int64_t>(), rows, nnz, s.als_cols[side].as<int32_t>(),
                          s.als_vals[side].get(), static_cast<int>(ctx->es), d_bkey, nb, rowmark, colmark};
  const int64_t gone = launch_als_remove_select(L, sc, d_found, sc.rempos.as<int32_t>());
  if (gone == 0) return 0;
  DevBuf d_off, d_cols, d_vals;
  d_off.alloc(static_cast<size_t>(rows + 1) * 8);
  d_cols.alloc(std::max<size_t>(static_cast<size_t>(nnz - gone) * 4, 16));
  d_vals.alloc(std::max<size_t>(static_cast<size_t>(nnz - gone) * ctx->es, 16));
  launch_als_remove_move(L, sc, d_off.as<int64_t>(), d_cols.as<int32_t>(), d_vals.get());
  std::vector<int64_t> off(static_cast<size_t>(rows) + 1);
  std::vector<int32_t> npos(A.npos), rempos(static_cast<size_t>(rows));
  MF_HIP(hipMemcpyAsync(off.data(), d_off.get(), off.size() * 8, hipMemcpyDeviceToHost, s.stream));
  MF_HIP(hipMemcpyAsync(rempos.data(), sc.rempos.get(), rempos.size() * 4, hipMemcpyDeviceToHost, s.stream));
  MF_HIP(hipStreamSynchronize(s.stream));  // the old arrays are freed behind the move
  for (int64_t x = 0; x < rows; ++x) npos[x] -= rempos[x];
  als_adopt_arrays(ctx, s, side, d_off, d_cols, d_vals, std::move(off), std::move(npos));
  return gone;
}

void als_remove_args(const int32_t* u, const int32_t* i, int64_t n, const char* api) {
  MF_REQUIRE(n >= 0, "negative rating count");
  MF_REQUIRE(n < (int64_t{1} << 31), std::string(api) + " takes fewer than 2^31 entries in one call");
  MF_REQUIRE(n == 0 || (u && i), "null rating arrays");
}

}  // namespace

int64_t als_remove(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, uint8_t* found) {
  als_remove_args(u, i, n, "mf_als_remove");
  Shard& s = als_enter(ctx, "mf_als_remove");
  if (n == 0) return 0;
  if (found) std::memset(found, 0, static_cast<size_t>(n));
  std::vector<uint32_t> ur, ir;
  lookup_rows(ctx->U, u, n, ur);
  lookup_rows(ctx->I, i, n, ir);
  // the entries that can name a stored rating: both ids known, both rows inside the CSRs
  const int64_t have_u = static_cast<int64_t>(ctx->als[kSideU].off.size()) - 1;
  const int64_t have_i = static_cast<int64_t>(ctx->als[MF_SIDE_ITEM].off.size()) - 1;
  std::vector<int64_t> at;
  std::vector<uint64_t> key;
  for (int64_t j = 0; j < n; ++j) {
    if (ur[j] == kRowMiss || ir[j] == kRowMiss || ur[j] >= have_u || ir[j] >= have_i) continue;
    at.push_back(j);
    key.push_back((static_cast<uint64_t>(ur[j]) << 32) | ir[j]);
  }
  const int64_t nb = static_cast<int64_t>(at.size());
  if (nb == 0) return 0;
  DeviceGuard g(s.device);
  AlsRemoveScratch& sc = s.als_rem;
  // One side at a time, as mf_als_append: the transient is a second copy of one side.  CSR order is arrival
  // order on both sides, so the m oldest instances of a pair in its user row are the m oldest in its item row.
  als_upload(sc.in, key.data(), key.size() * 8);
  sc.found.alloc(static_cast<size_t>(nb));
  const int64_t gone = als_remove_side(ctx, s, kSideU, sc.in.as<uint64_t>(), nb, nullptr, nullptr, sc.found.as<uint8_t>());
  if (gone == 0) return 0;  // every entry a miss: nothing has changed
  if (found) {
    std::vector<uint8_t> f(static_cast<size_t>(nb));
    MF_HIP(hipMemcpy(f.data(), sc.found.get(), f.size(), hipMemcpyDeviceToHost));
    for (int64_t t = 0; t < nb; ++t) found[at[t]] = f[t];
  }
  for (int64_t t = 0; t < nb; ++t) key[t] = (key[t] << 32) | (key[t] >> 32);
  als_upload(sc.in, key.data(), key.size() * 8);
  const int64_t gone_i = als_remove_side(ctx, s, MF_SIDE_ITEM, sc.in.as<uint64_t>(), nb, nullptr, nullptr, nullptr);
  if (gone_i != gone) fail(MF_ERR_STATE, "mf_als_remove: the two CSRs did not hold the same ratings");
  return gone;
}

int64_t als_remove_rows(mf_ctx* ctx, int side, const int32_t* ids, int64_t n_ids) {
  MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
  MF_REQUIRE(n_ids >= 0, "negative id count");
  MF_REQUIRE(n_ids == 0 || ids, "null id array");
  Shard& s = als_enter(ctx, "mf_als_remove_rows");
  const mf_ctx::AlsSide& A = ctx->als[side];
  const SideLayout& S = side_of(ctx, side);
  const int64_t have = static_cast<int64_t>(A.off.size()) - 1;
  std::vector<uint8_t> mark(static_cast<size_t>(have), 0);
  int64_t want = 0;
  for (int64_t j = 0; j < n_ids; ++j) {  // ids the model does not hold and rows without a rating are skipped
    const int32_t row = S.index.find(ids[j]);
    if (row < 0 || row >= have || mark[row]) continue;
    const int64_t c = A.off[row + 1] - A.off[row];
    if (c == 0) continue;
    mark[row] = 1;
    want += c;
  }
  if (want == 0) return 0;
  MF_REQUIRE(want < (int64_t{1} << 31) - 1, "mf_als_remove_rows removes fewer than 2^31 - 1 ratings in one call");
  DeviceGuard g(s.device);
  AlsRemoveScratch& sc = s.als_rem;
  als_upload(sc.mark, mark.data(), mark.size());
  const int64_t gone = als_remove_side(ctx, s, side, nullptr, 0, sc.mark.as<uint8_t>(), nullptr, nullptr);
  const int64_t gone_o = als_remove_side(ctx, s, 1 - side, nullptr, 0, nullptr, sc.mark.as<uint8_t>(), nullptr);
  if (gone != want || gone_o != want) fail(MF_ERR_STATE, "mf_als_remove_rows: the two CSRs did not hold the same ratings");
  return want;
}

int64_t als_retract(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, const AlsParams& P, int32_t rounds,
                    uint8_t* found, int64_t* solved_users, int64_t* solved_items) {
  MF_REQUIRE(rounds >= 0, "negative round count");
  if (P.implicit) als_check_alpha(P.alpha);
  als_check_run(P);
  const int64_t gone = als_remove(ctx, u, i, n, found);  // (checks the rest before it changes anything)
  int64_t su = 0, si = 0;
  for (int32_t t = 0; t < rounds; ++t) {  // rows that lost their last rating fall out by mf_als_run_rows' own rule
    su = als_run_rows(ctx, kSideU, u, n, P);
    si = als_run_rows(ctx, MF_SIDE_ITEM, i, n, P);
  }
  if (solved_users) *solved_users = su;
  if (solved_items) *solved_items = si;
  return gone;
}

// ---------------------------------------------------------------------------------------
// Fold-in (mf_als_foldin / mf_recommend_foldin): rows of `side` solved from lists the callers hand over, as
// mf_als_run_rows would solve rows that held exactly those ratings, and nothing of the context changes.  Per
// batch of queries the lists are uploaded as they are; the device resolves the ids over the counterpart's id
// mirror, compacts the kept entries stably into a transient CSR (kernels_foldin.hip) and hands back two int32
// per query; the host cuts those with AlsCutter, and the launch loop of the half-sweeps runs with cols / vals
// = the transient CSR, X = a zeroed scratch slab and item.row = the query's position in the batch.  The fused
// call turns the kept entries into the exclusion CSR on the device and scores the slab where it lies.
constexpr int64_t kFoldinBatch = 8192;           // queries per batch (MFHIP_TEST foldin_batch=B)
constexpr int64_t kFoldinEntries = int64_t{1} << 22;  // ... and entries, unless one list alone is longer

void als_foldin(mf_ctx* ctx, int side, const int64_t* off, const int32_t* ids, const double* r, int64_t nq,
                const AlsParams& P, const FoldinRecommend* rec, double* vecs_out, int32_t* used_out) {
  als_check(ctx);
  if (!ctx->have_model)
    fail(MF_ERR_NOT_FITTED, "The MatrixFactorization model has not been fitted to data. "
                            "Prior to folding in, it has to be trained on data or loaded.");
  require_healthy(ctx);
  if (nq == 0) return;
  sync_all(ctx);
  Shard& s = ctx->shards[0];
  DeviceGuard g(s.device);
  FoldinScratch& sc = s.fold;
  const int other = side == kSideU ? MF_SIDE_ITEM : kSideU;
  const int k = ctx->P.num_factors;
  const size_t kk = static_cast<size_t>(k), es = ctx->es;
  const size_t N = rec ? static_cast<size_t>(rec->top_n) : 0;
  const AlsCuts cuts = ctx->als_prepared
                           ? AlsCuts{ctx->als_chunk, ctx->als_batch, ctx->als_gram_slice, ctx->als_slabs}
                           : als_cuts_now(ctx, s);
  int64_t B = kFoldinBatch;
  if (const std::string v = test_knob("foldin_batch"); !v.empty()) B = std::max<int64_t>(1, std::atoll(v.c_str()));
  B = std::min(B, nq);

  DevIndex& mirror = s.didx[other];
  sync_dev_index(s, side_of(ctx, other).index, mirror);
  sc.stats.alloc(sizeof(struct mf_als_nonneg_stats));  // counters of the fold-in launches' own, never read
  MF_HIP(hipMemsetAsync(sc.stats.get(), 0, sizeof(struct mf_als_nonneg_stats), s.stream));
  // G once per call: the counterpart's factors do not change under it.  With prepared data over the rated-row
  // list as it stands (a prepare with n = 0: no row, G = 0), without over every row the counterpart holds.
  const void* gram = nullptr;
  if (P.implicit) {
    if (ctx->als_prepared) {
      als_gram_launch(ctx, s, other);
    } else {
      const int64_t C = side_of(ctx, other).rows();
      sc.iota.alloc(std::max<size_t>(static_cast<size_t>(C) * 4, 16));
      launch_iota(s.stream, sc.iota.as<int32_t>(), C);
      als_gram_launch(ctx, s, other, sc.iota.as<int32_t>(), C, cuts.gram_slice);
    }
    ctx->stats.kernel_launches += 2;
    gram = s.als_gram.get();
    MF_HIP(hipStreamSynchronize(s.stream));  // the batches below grow scratch only on a drained stream
  }

  // MFHIP_TIMING=1: the phases of every batch on stderr, the stream drained after each (a diagnostic run)
  PhaseClock clk;
  auto lap = [&](const char* what) {
    if (!clk.on) return;
    MF_HIP(hipStreamSynchronize(s.stream));
    clk.lap(what);
  };
  for (int64_t q0 = 0, q1 = 0; q0 < nq; q0 = q1) {
    for (q1 = q0 + 1; q1 < nq && q1 - q0 < B && off[q1 + 1] - off[q0] <= kFoldinEntries;) ++q1;
    const int64_t nb = q1 - q0, e0 = off[q0], n = off[q1] - e0;
    const bool keys = rec && rec->exclude_rated && n > 0;
    // the stream is drained here (sync_all, or the previous batch's read-back): scratch may grow
    const size_t b_r = static_cast<size_t>(n) * 8, b_off = static_cast<size_t>(nb + 1) * 8, b_id = static_cast<size_t>(n) * 4;
    sc.pin.alloc(b_r + b_off + b_id);
    sc.in.alloc(b_r + b_off + 2 * b_id);
    sc.back.alloc(static_cast<size_t>(nb) * 8);
    sc.cnt.alloc(static_cast<size_t>(nb) * 8);
    sc.cols.alloc(std::max<size_t>(b_id, 16));
    sc.vals.alloc(std::max<size_t>(static_cast<size_t>(n) * es, 16));
    sc.x.alloc(std::max<size_t>(static_cast<size_t>(nb) * kk * es, 16));
    if (keys) rank_keys_reserve(s.rank_sc, n);
    if (rec) {
      s.rec_eoff.alloc(b_off);
      s.rec_erows.alloc(std::max<size_t>(b_id, 16));
    }
    // 1. the lists through the pinned stage: ratings, batch-local offsets, ids
    char* const pin = sc.pin.as<char>();
    if (n) std::memcpy(pin, r + e0, b_r);
    int64_t* const poff = reinterpret_cast<int64_t*>(pin + b_r);
    for (int64_t j = 0; j <= nb; ++j) poff[j] = off[q0 + j] - e0;
    if (n) std::memcpy(pin + b_r + b_off, ids + e0, b_id);
    char* const din = sc.in.as<char>();
    MF_HIP(hipMemcpyAsync(din, pin, b_r + b_off + b_id, hipMemcpyHostToDevice, s.stream));
    lap("foldin upload");
    // 2. + 3. resolve and compact on the device; 4. two int32 per query come back
    launch_foldin_compact({s.stream, reinterpret_cast<const int64_t*>(din + b_r), nb, n,
                           reinterpret_cast<uint32_t*>(din + b_r + b_off), reinterpret_cast<const double*>(din),
                           mirror.cap ? mirror.slots.get() : nullptr, mirror.cap - 1, ctx->f64, sc.cols.as<int32_t>(),
                           sc.vals.get(), sc.cnt.as<int32_t>(), keys ? s.rank_sc.key.as<uint64_t>() : nullptr},
                          sc);
    const int32_t* const cnt = sc.back.as<int32_t>();
    MF_HIP(hipMemcpyAsync(sc.back.as<char>(), sc.cnt.get(), static_cast<size_t>(nb) * 8, hipMemcpyDeviceToHost, s.stream));
    MF_HIP(hipStreamSynchronize(s.stream));
    mf_ctx::AlsSide W;
    AlsCutter cut{W.items, W.splits, W.batches, W.max_slots, cuts.chunk, cuts.batch};
    int64_t nk = 0;
    for (int64_t j = 0; j < nb; ++j) {
      const int64_t c = cnt[2 * j];
      if (c > 0) cut.add(j, nk, c, cnt[2 * j + 1]);
      nk += c;
    }
    cut.close();
    lap("foldin table");
    // 5. the half-sweeps' launches over the transient CSR into the zeroed slab
    MF_HIP(hipMemsetAsync(sc.x.get(), 0, std::max<size_t>(static_cast<size_t>(nb) * kk * es, 16), s.stream));
    if (!W.batches.empty()) {
      als_upload(s.als_sub_items, W.items.data(), W.items.size() * sizeof(AlsItem));
      als_upload(s.als_sub_splits, W.splits.data(), W.splits.size() * sizeof(AlsSplit));
      if (P.cg_steps > 0) {
        als_cg_work(W.items, W.splits, W.batches, W.cg_work, W.cg_work0, W.cg_max_splits);
        als_upload(s.als_sub_work, W.cg_work.data(), W.cg_work.size() * sizeof(AlsCgWork));
      }
      AlsLaunch L;
      L.st = s.stream;
      L.cols = sc.cols.as<int32_t>();
      L.vals = sc.vals.get();
      L.Q = side == kSideU ? s.itf.get() : s.uf.get();
      L.X = sc.x.get();
      L.nnls_stats = sc.stats.get();
      L.gram = gram;
      als_launch_setup(ctx, s, L, P, W, cuts.slabs);
      als_launch_batches(ctx, s, L, P, W,
                         {s.als_sub_items.as<AlsItem>(), s.als_sub_splits.as<AlsSplit>(), s.als_sub_work.as<AlsCgWork>()},
                         nullptr);
    }
    lap("foldin solve");
    // 6. the fused call: the kept entries' keys -> the exclusion CSR, the slab scored where it lies
    if (rec) {
      if (keys && nk > 0) {
        rank_keys_sort(s.stream, s.rank_sc, nk, nb);
        rank_keys_csr(s.stream, s.rank_sc, nk, nb, false, s.rec_eoff.as<int64_t>(), s.rec_erows.as<int32_t>());
      } else {
        MF_HIP(hipMemsetAsync(s.rec_eoff.get(), 0, b_off, s.stream));
      }
      int32_t* const io = rec->ids_out + static_cast<size_t>(q0) * N;
      double* const so = rec->scores_out ? rec->scores_out + static_cast<size_t>(q0) * N : nullptr;
      recommend_scored(ctx, s, TopNQueries::of_slab(s, sc.x.get(), nb), TopNCandidates::of_side(ctx, other), rec->top_n,
                       MF_METRIC_DOT, ExclSource::csr(s.rec_eoff.as<int64_t>(), s.rec_erows.as<int32_t>()),
                       TopNSink{io, so, rec->counts_out + q0, nullptr});
      for (int64_t j = 0; j < nb; ++j) {  // a query with no kept entry has no list
        if (cnt[2 * j] > 0) continue;
        rec->counts_out[q0 + j] = 0;
        std::fill(io + static_cast<size_t>(j) * N, io + static_cast<size_t>(j + 1) * N, 0);
        if (so) std::fill(so + static_cast<size_t>(j) * N, so + static_cast<size_t>(j + 1) * N, 0.0);
      }
    }
    MF_HIP(hipStreamSynchronize(s.stream));
    if (rec) lap("foldin select");
    if (vecs_out) {
      const std::vector<double> h = read_as_f64(ctx, sc.x, static_cast<size_t>(nb) * kk);
      std::memcpy(vecs_out + static_cast<size_t>(q0) * kk, h.data(), h.size() * 8);
    }
    if (used_out)
      for (int64_t j = 0; j < nb; ++j) used_out[q0 + j] = cnt[2 * j];
  }
}

// The resident CSR of a side copied back (mf_debug_als_csr): the offsets and entries from the device, the
// per-row n+ from the host list the work items are cut from.
void als_debug_csr(mf_ctx* ctx, int side, int64_t* off_out, int32_t* cols_out, double* vals_out, int32_t* npos_out,
                   int64_t cap_rows, int64_t cap_nnz, int64_t* rows_out, int64_t* nnz_out) {
  Shard& s = als_enter(ctx, "mf_debug_als_csr");
  const mf_ctx::AlsSide& A = ctx->als[side];
  const int64_t rows = static_cast<int64_t>(A.off.size()) - 1, nnz = A.off.back();
  *rows_out = rows;
  *nnz_out = nnz;
  if (cap_rows < rows || cap_nnz < nnz) fail(MF_ERR_CAPACITY, "mf_debug_als_csr: the output arrays are too short");
  DeviceGuard g(s.device);
  MF_HIP(hipMemcpy(off_out, s.als_off[side].get(), static_cast<size_t>(rows + 1) * 8, hipMemcpyDeviceToHost));
  std::copy(A.npos.begin(), A.npos.end(), npos_out);
  if (nnz == 0) return;
  MF_HIP(hipMemcpy(cols_out, s.als_cols[side].get(), static_cast<size_t>(nnz) * 4, hipMemcpyDeviceToHost));
  const std::vector<double> v = read_as_f64(ctx, s.als_vals[side], static_cast<size_t>(nnz));
  std::memcpy(vals_out, v.data(), static_cast<size_t>(nnz) * 8);
}

}  // namespace mfhip
