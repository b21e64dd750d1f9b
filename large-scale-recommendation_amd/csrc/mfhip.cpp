// mfhip.cpp -- the context and its shards, the helpers every feature uses (slabs, health, sync),
// model construction, and the top of the DSGD driver: prepare, which dispatches to the mode's
// preparation, and run_supersteps.  The deterministic supersteps are dsgd_det.cpp, the fast ones
// dsgd_fast.cpp, the item-block ring between GPUs ring.cpp, the persistent sweeps' launch tables
// placement.cpp.  The C ABI is abi.cpp; online micro-batches and mf_block_update are online.cpp,
// evaluation eval.cpp, top-N lists recommend.cpp, ALS als.cpp; context.hpp declares what they share.
//
// Execution model:
//  * A context owns G shards.  Shard g owns user blocks [g*c, (g+1)*c), c = numBlocks / G, and
//    the rating blocks of those rows, resident in HBM for the whole fit.
//  * Superstep s (1-based, DSGDforMF.scala:341-344, :476) runs rating blocks (p, (p+s-1) mod n)
//    for the shard's p on the shard's stream; afterwards the shard hands item block
//    (g*c + s - 1) mod n to shard g-1 and receives ((g+1)*c + s - 1) mod n from shard g+1 --
//    the nextRatingBlock rotation (:611-619).  In-process shards use peer copies; one process
//    per GPU (mf_create_rank) uses RCCL send/recv over xGMI.
//  * Every shard keeps full-size factor slabs with the global row numbering, so a block moves
//    by copying its row range; only the rows a shard currently owns are current.
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
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

thread_local std::string g_last_error;

double bytes_per_update(const mf_ctx* ctx) {
  const double k = ctx->P.num_factors;
  return ctx->f64 ? 32.0 * k + 24.0 : 16.0 * k + 20.0;
}

namespace {

void validate_params(const mf_params* p) {
  MF_REQUIRE(p, "params is null");
  MF_REQUIRE(p->num_factors >= 1 && p->num_factors <= 512, "num_factors must be in [1, 512]");
  MF_REQUIRE(p->iterations >= 0, "iterations must be >= 0");
  MF_REQUIRE(p->num_blocks >= 1, "num_blocks must be >= 1");
  MF_REQUIRE(p->mode == MF_MODE_DETERMINISTIC_F64 || p->mode == MF_MODE_FAST_F32, "unknown mode");
  MF_REQUIRE(p->lr_method >= MF_LR_DEFAULT && p->lr_method <= MF_LR_XU, "unknown lr_method");
  MF_REQUIRE(p->fast_blocking == MF_BLOCKING_BALANCED || p->fast_blocking == MF_BLOCKING_REFERENCE,
             "unknown fast_blocking");
}

void init_shard(Shard& s, int device, int index) {
  s.device = device;
  s.index = index;
  DeviceGuard g(device);
  MF_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  MF_HIP(hipStreamCreateWithFlags(&s.copy_stream, hipStreamNonBlocking));
  MF_HIP(hipStreamCreateWithFlags(&s.aux, hipStreamNonBlocking));
  MF_HIP(hipStreamCreateWithFlags(&s.comm, hipStreamNonBlocking));
  MF_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  for (hipEvent_t* e : {&s.ev_front, &s.ev_last, &s.ev_moved}) MF_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  for (auto& b : s.det_buf) {
    MF_HIP(hipEventCreateWithFlags(&b.copied, hipEventDisableTiming));
    MF_HIP(hipEventCreateWithFlags(&b.swept, hipEventDisableTiming));
  }
}

void destroy_shard(Shard& s) {
  if (!s.stream) return;
  (void)hipSetDevice(s.device);
  (void)hipStreamSynchronize(s.stream);
  (void)hipStreamSynchronize(s.copy_stream);
  (void)hipStreamSynchronize(s.aux);
  (void)hipStreamSynchronize(s.comm);
  for (hipEvent_t e : {s.ev_front, s.ev_last, s.ev_moved})
    if (e) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(s.aux);
  (void)hipStreamDestroy(s.comm);
  for (auto e : s.ev) (void)hipEventDestroy(e);
  s.ev.clear();
  for (auto& b : s.det_buf) {
    if (b.copied) (void)hipEventDestroy(b.copied);
    if (b.swept) (void)hipEventDestroy(b.swept);
  }
  (void)hipEventDestroy(s.done);
  (void)hipStreamDestroy(s.copy_stream);
  (void)hipStreamDestroy(s.stream);
  s.stream = nullptr;
}

}  // namespace

// Grow a factor slab (and its regularisation column) to hold `rows`, keeping the contents.
void ensure_rows(mf_ctx* ctx, Shard& s, int side, int64_t rows) {
  int64_t& cap = side == kSideU ? s.cap_u : s.cap_i;
  if (rows <= cap) return;
  DeviceGuard g(s.device);
  const int64_t ncap = std::max<int64_t>({rows, cap * 2, 1024});
  const size_t k = static_cast<size_t>(ctx->P.num_factors);
  DevBuf f, rg;
  f.alloc(static_cast<size_t>(ncap) * k * ctx->es);
  rg.alloc(static_cast<size_t>(ncap) * ctx->es);
  MF_HIP(hipMemsetAsync(rg.get(), 0, static_cast<size_t>(ncap) * ctx->es, s.stream));
  DevBuf& of = side == kSideU ? s.uf : s.itf;
  DevBuf& og = side == kSideU ? s.regu : s.regi;
  if (cap > 0) {
    MF_HIP(hipMemcpyAsync(f.get(), of.get(), static_cast<size_t>(cap) * k * ctx->es, hipMemcpyDeviceToDevice, s.stream));
    MF_HIP(hipMemcpyAsync(rg.get(), og.get(), static_cast<size_t>(cap) * ctx->es, hipMemcpyDeviceToDevice, s.stream));
  }
  MF_HIP(hipStreamSynchronize(s.stream));
  of = std::move(f);
  og = std::move(rg);
  cap = ncap;
}

// Host f64 rows -> device slab rows [row0, row0+n) in the context's precision.
void upload_rows(mf_ctx* ctx, Shard& s, int side, int64_t row0, const double* src, int64_t n) {
  if (n <= 0) return;
  DeviceGuard g(s.device);
  const size_t k = static_cast<size_t>(ctx->P.num_factors);
  DevBuf& slab = side == kSideU ? s.uf : s.itf;
  char* dst = slab.as<char>() + static_cast<size_t>(row0) * k * ctx->es;
  if (ctx->f64) {
    MF_HIP(hipMemcpy(dst, src, static_cast<size_t>(n) * k * 8, hipMemcpyHostToDevice));
  } else {
    std::vector<float> tmp(static_cast<size_t>(n) * k);
    parallel_for(static_cast<int64_t>(tmp.size()), [&](int64_t b, int64_t e, int) {
      for (int64_t x = b; x < e; ++x) tmp[x] = static_cast<float>(src[x]);
    });
    MF_HIP(hipMemcpy(dst, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
  }
}

void upload_regs(mf_ctx* ctx, Shard& s, int side, int64_t row0, const double* src, int64_t n) {
  if (n <= 0) return;
  DeviceGuard g(s.device);
  DevBuf& reg = side == kSideU ? s.regu : s.regi;
  char* dst = reg.as<char>() + static_cast<size_t>(row0) * ctx->es;
  if (ctx->f64) {
    MF_HIP(hipMemcpy(dst, src, static_cast<size_t>(n) * 8, hipMemcpyHostToDevice));
  } else {
    std::vector<float> tmp(n);
    for (int64_t x = 0; x < n; ++x) tmp[x] = static_cast<float>(src[x]);
    MF_HIP(hipMemcpy(dst, tmp.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
  }
}

// Device slab rows [row0, row0+n) -> host f64.
void download_rows(mf_ctx* ctx, Shard& s, int side, int64_t row0, int64_t n, double* out) {
  if (n <= 0) return;
  DeviceGuard g(s.device);
  const size_t k = static_cast<size_t>(ctx->P.num_factors);
  DevBuf& slab = side == kSideU ? s.uf : s.itf;
  const char* src = slab.as<char>() + static_cast<size_t>(row0) * k * ctx->es;
  MF_HIP(hipStreamSynchronize(s.stream));
  if (ctx->f64) {
    MF_HIP(hipMemcpy(out, src, static_cast<size_t>(n) * k * 8, hipMemcpyDeviceToHost));
  } else {
    std::vector<float> tmp(static_cast<size_t>(n) * k);
    MF_HIP(hipMemcpy(tmp.data(), src, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (size_t x = 0; x < tmp.size(); ++x) out[x] = static_cast<double>(tmp[x]);
  }
}

// Initial factors: k x nextDouble of new Random(id ^ seed) (DSGDforMF.scala:548-549), or of
// new Random(id) for PseudoRandomFactorInitializer (core/FactorInitializer.scala:23-27).
void init_vectors(const int32_t* ids, int64_t n, int k, bool xor_seed, int64_t seed, std::vector<double>& out) {
  out.resize(static_cast<size_t>(n) * k);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t x = b; x < e; ++x) {
      JavaRandom rng(xor_seed ? (static_cast<int64_t>(ids[x]) ^ seed) : static_cast<int64_t>(ids[x]));
      double* v = out.data() + static_cast<size_t>(x) * k;
      for (int f = 0; f < k; ++f) v[f] = rng.nextDouble();
    }
  }, 0, 1024);
}

namespace {

void collect_profile(mf_ctx* ctx) {
  for (auto& s : ctx->shards) {
    if (s.ev_used == 0) continue;
    DeviceGuard g(s.device);
    MF_HIP(hipStreamSynchronize(s.stream));
    double ms = 0.0;
    for (size_t x = 0; x + 1 < s.ev_used; x += 2) {
      float t = 0.f;
      MF_HIP(hipEventElapsedTime(&t, s.ev[x], s.ev[x + 1]));
      ms += t;
    }
    ctx->stats.kernel_ms += ms;
    s.ev_used = 0;
  }
}

}  // namespace

// (does not wait for det_run's speculative builds: they touch no device state, and a caller's
// sync must not pay for the next run's host work)
void sync_all(mf_ctx* ctx) {
  for (auto& s : ctx->shards) {
    DeviceGuard g(s.device);
    MF_HIP(hipStreamSynchronize(s.stream));
    MF_HIP(hipStreamSynchronize(s.aux));
    MF_HIP(hipStreamSynchronize(s.comm));
    for (DevBuf* eb : {&s.fast_err, &s.det_err}) {
      if (!eb->get()) continue;
      int32_t err4[4] = {0, 0, 0, 0};
      MF_HIP(hipMemcpy(err4, eb->get(), std::min<size_t>(sizeof(err4), eb->bytes()), hipMemcpyDeviceToHost));
      const int32_t err = err4[0];
      if (err) {
        MF_HIP(hipMemsetAsync(eb->get(), 0, std::min<size_t>(sizeof(err4), eb->bytes()), s.stream));
        MF_HIP(hipStreamSynchronize(s.stream));
        if (std::getenv("MFHIP_DEBUG_PLAN") && eb->bytes() > 16) {
          std::vector<uint32_t> dg(eb->bytes() / 4);
          MF_HIP(hipMemcpy(dg.data(), eb->get(), eb->bytes(), hipMemcpyDeviceToHost));
          for (size_t w = 0; 4 + 4 * w + 3 < dg.size(); ++w)
            if (dg[4 + 4 * w + 3])
              std::fprintf(stderr, "[mfhip] sweep timeout: wave slot %zu seen %u want %u published %u\n", w,
                           dg[4 + 4 * w], dg[4 + 4 * w + 1], dg[4 + 4 * w + 2]);
          MF_HIP(hipMemsetAsync(eb->get(), 0, eb->bytes(), s.stream));
          MF_HIP(hipStreamSynchronize(s.stream));
        }
        // waves that gave up skipped the rest of their work: the model is partly updated, so
        // the context refuses further supersteps and reads until the fit is prepared again
        ctx->failed = eb == &s.fast_err
                          ? "fast sweep: a wave waited > 1 s for its neighbour (workgroups not co-resident?); "
                            "set MFHIP_TEST=pair_sys=0 (or fast_kernel=cell; INTEGRATION.md section 5)"
                          : "deterministic sweep: a wave waited > 1 s for a user ticket (waves not co-resident?); "
                            "set MFHIP_TEST=det_kernel=level (INTEGRATION.md section 5)";
        fail(MF_ERR_TIMEOUT, ctx->failed);
      }
    }
  }
  collect_profile(ctx);
}

void require_healthy(const mf_ctx* ctx) {
  if (!ctx->failed.empty())
    fail(MF_ERR_STATE, "the context failed earlier (" + ctx->failed + "); prepare the fit again");
}

namespace {

// ---------------------------------------------------------------------------------------
// Model construction for a fit.
// Slab rows [0, n) := initial factors of ids[0..n) generated on the device (launch_jvm_init_rows):
// only the ids cross PCIe (4 B per row instead of k doubles), bit-exact with init_vectors.
void init_rows_on_device(mf_ctx* ctx, Shard& s, int side, const int32_t* ids, int64_t n, bool xor_seed, int64_t seed) {
  if (n <= 0) return;
  DeviceGuard g(s.device);
  const int k = ctx->P.num_factors;
  std::vector<uint64_t> jump(4 * static_cast<size_t>(k));  // (mult, add) after m = 1..2k LCG steps
  constexpr uint64_t kMult = 0x5DEECE66DULL, kMask = (1ULL << 48) - 1;
  uint64_t m = 1, a = 0;
  for (int step = 0; step < 2 * k; ++step) {
    m = (m * kMult) & kMask;
    a = (a * kMult + 0xBULL) & kMask;
    jump[2 * step] = m;
    jump[2 * step + 1] = a;
  }
  DevBuf dids, djump;
  dids.alloc(static_cast<size_t>(n) * 4);
  djump.alloc(jump.size() * 8);
  MF_HIP(hipMemcpyAsync(dids.get(), ids, static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, s.stream));
  MF_HIP(hipMemcpyAsync(djump.get(), jump.data(), jump.size() * 8, hipMemcpyHostToDevice, s.stream));
  DevBuf& slab = side == kSideU ? s.uf : s.itf;
  launch_jvm_init_rows(s.stream, dids.as<int32_t>(), n, k, xor_seed, seed, djump.as<uint64_t>(), slab.get(), ctx->f64);
  MF_HIP(hipGetLastError());
  MF_HIP(hipStreamSynchronize(s.stream));  // the temporaries die here
}

}  // namespace

// Every shard's slabs := the initial factors of every row (fitSGD's starting point).
void init_factors(mf_ctx* ctx) {
  for (int side = 0; side < 2; ++side) {
    SideLayout& S = side == kSideU ? ctx->U : ctx->I;
    for (auto& s : ctx->shards) init_rows_on_device(ctx, s, side, S.row_id.data(), S.rows(), true, ctx->init_seed);
  }
}

namespace {

// sides_built: ctx->U / ctx->I already hold the blocking (device_blocking).
void build_model(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, bool sides_built) {
  const bool seeded = ctx->P.has_seed != 0;
  const Blocking bl = !ctx->f64 && ctx->P.fast_blocking == MF_BLOCKING_BALANCED ? Blocking::kBalanced : Blocking::kJvm;
  if (!sides_built) {
    build_side(ctx->U, u, n, ctx->nb, ctx->P.seed, seeded, bl);
    build_side(ctx->I, i, n, ctx->nb, ctx->P.seed, seeded, bl);
  }
  for (int side = 0; side < 2; ++side) {
    SideLayout& S = side == kSideU ? ctx->U : ctx->I;
    std::vector<double> reg(S.rows());
    for (int64_t x = 0; x < S.rows(); ++x) reg[x] = ctx->P.lambda / static_cast<double>(S.omega[x]);
    for (auto& s : ctx->shards) {
      ensure_rows(ctx, s, side, std::max<int64_t>(S.rows(), 1));
      upload_regs(ctx, s, side, 0, reg.data(), S.rows());
    }
  }
  ctx->init_seed = ctx->P.seed;
  if (!seeded) {
    std::random_device rd;
    ctx->init_seed = (static_cast<int64_t>(rd()) << 32) ^ rd();
  }
  init_factors(ctx);
  ctx->have_model = true;
  ctx->order_dirty = true;
  ++ctx->layout_gen;
}

}  // namespace

void ensure_order(mf_ctx* ctx) {
  if (!ctx->order_dirty) return;
  for (int side = 0; side < 2; ++side) {
    SideLayout& S = side_of(ctx, side);
    auto& ord = side == kSideU ? ctx->rows_by_id_u : ctx->rows_by_id_i;
    ord.resize(S.rows());
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return S.row_id[a] < S.row_id[b]; });
  }
  ctx->order_dirty = false;
}

void run_supersteps(mf_ctx* ctx, int64_t count) {
  MF_REQUIRE(ctx->prepared, "mf_dsgd_run before mf_dsgd_prepare");
  require_healthy(ctx);
  if (ctx->f64 && ctx->det_sweep) {
    if (count > 0) det_run(ctx, count);
    return;
  }
  for (int64_t x = 0; x < count; ++x) {
    const int64_t s = ctx->superstep_done + 1;
    const int32_t iteration = static_cast<int32_t>(s / ctx->nb);  // getSuperstepNumber / numBlocks (:476)
    const double eta = learning_rate(ctx->P.lr_method, ctx->P.learning_rate, iteration + 1, ctx->P.lambda,
                                     ctx->P.lr_arg);  // :383-386
    for (auto& sh : ctx->shards) {
      if (ctx->f64) det_superstep(ctx, sh, s, eta);
      else fast_superstep(ctx, sh, s, eta);
    }
    ring_shift(ctx, s);
    ctx->superstep_done = s;
    ctx->stats.supersteps++;
  }
  ctx->stats.algorithmic_bytes = static_cast<double>(ctx->stats.updates) * bytes_per_update(ctx);
}

void prepare(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n) {
  MF_REQUIRE(n >= 0, "negative rating count");
  MF_REQUIRE(n == 0 || (u && i && r), "null rating arrays");
  det_spec_wait(ctx, true);
  ctx->failed.clear();
  ctx->als_prepared = false;  // the layouts are rebuilt: an ALS CSR names rows of the old ones
  seen_clear(ctx);            // ... and so does the seen set
  sync_all(ctx);
  PhaseClock clk;
  ctx->item_split = 0;
  if (const char* v = exp_knob("MFHIP_ITEM_SPLIT")) ctx->item_split = std::max(0, std::atoi(v));  // replicas
  ctx->reaper.join();
  DevRatingBlocks dev_rb;  // the device copy of the rating blocks (full device schedule only)
  ctx->nb = std::max(1, ctx->P.num_blocks);
  MF_REQUIRE(ctx->nb % ctx->G == 0, "num_blocks must be a multiple of the device count");
  ctx->c = ctx->nb / ctx->G;
  int32_t lo = 0, hi = ctx->nb;
  if (ctx->rank_mode) { lo = ctx->shards[0].index * ctx->c; hi = lo + ctx->c; }
  // the reference's seeded blocking runs on the device (MFHIP_TEST host_blocking=1: on the host)
  const std::string hb = test_knob("host_blocking");
  const bool on_device = ctx->P.has_seed && (ctx->f64 || ctx->P.fast_blocking == MF_BLOCKING_REFERENCE) &&
                         !(!hb.empty() && hb != "0") && n < (int64_t{1} << 31);
  if (on_device) {
    Shard& s0 = ctx->shards[0];
    DeviceGuard g(s0.device);
    const std::string dpv0 = test_knob("device_plan");
    const bool keep = !ctx->f64 && ctx->shards.size() == 1 && ctx->item_split == 0 &&
                      choose_fast_kernel(ctx->P.num_factors) == FastKernel::kPair && dpv0 != "0" && dpv0 != "1";
    device_blocking(s0.stream, u, i, r, n, ctx->nb, ctx->P.seed, lo, hi, ctx->f64, ctx->U, ctx->I, ctx->rb,
                    keep ? &dev_rb : nullptr, !keep);
    clk.lap("blocking + rating blocks (device)");
  }
  build_model(ctx, u, i, n, on_device);
  clk.lap("factor init + H2D");
  if (!on_device) {
    build_rating_blocks(ctx->rb, ctx->U, ctx->I, u, i, r, n, lo, hi, ctx->f64 && ctx->P.has_seed);
    clk.lap("rating blocks");
  }
  ctx->det_sweep = false;
  ctx->ring_overlap = false;
  if (ctx->f64) prepare_det_sweep(ctx);
  clk.lap("deterministic sweep layout");
  if (!ctx->f64) prepare_fast(ctx, dev_rb, clk, lo, hi);
  clk.lap("release host blocks");
  // hipMemset on device memory returns before the fill is done and the legacy stream does not
  // order the non-blocking sweep streams (tools/micro/memset_order.hip: a 4-GiB memset returns
  // in 3 us and a kernel on another stream still reads the old bytes), so the zeroing above is
  // issued on the shard streams, and the device drains here: the first superstep's launches
  // (aux included, which waits on no event yet) see every table, zeroed row and progress word.
  // A run of 8 ranks sharing one GPU raced here (stale progress words let waves skip a hand-off).
  for (auto& s : ctx->shards) {
    DeviceGuard g(s.device);
    MF_HIP(hipDeviceSynchronize());
  }
  ctx->superstep_done = 0;
  reset_item_loc(ctx);
  ctx->prepared = true;
}

int32_t online_row(mf_ctx* ctx, SideLayout& S, int32_t id, std::vector<int32_t>& fresh) {
  const int32_t row = S.index.find(id);
  if (row >= 0) return row;
  const int32_t nr = static_cast<int32_t>(S.rows());
  S.index.insert(id, nr);
  S.row_id.push_back(id);
  S.omega.push_back(0);
  S.row_block.push_back(-1);
  fresh.push_back(id);
  ctx->order_dirty = true;
  ++ctx->layout_gen;
  return nr;
}

namespace {

mf_ctx* new_ctx(const mf_params* p) {
  validate_params(p);
  auto* ctx = new mf_ctx();
  ctx->P = *p;
  ctx->f64 = p->mode == MF_MODE_DETERMINISTIC_F64;
  ctx->es = ctx->f64 ? 8 : 4;
  ctx->fast_persistent = choose_fast_kernel(p->num_factors) == FastKernel::kPersistent;
  return ctx;
}

}  // namespace

mf_ctx* create_ctx(const mf_params* p, const int* device_ids, int n_devices) {
  MF_REQUIRE(n_devices >= 1, "n_devices must be >= 1");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
    fail(MF_ERR_NO_DEVICE, "no HIP device available (libmfhip has no CPU fallback)");
  std::unique_ptr<mf_ctx> ctx(new_ctx(p));
  ctx->G = n_devices;
  { std::vector<Shard> tmp(n_devices); ctx->shards.swap(tmp); }
  for (int d = 0; d < n_devices; ++d) {
    const int dev = device_ids ? device_ids[d] : d % count;  // shards may share a device
    MF_REQUIRE(dev >= 0 && dev < count, "device id out of range");
    init_shard(ctx->shards[d], dev, d);
  }
  // enable peer access between distinct devices (ignore "already enabled")
  for (auto& a : ctx->shards)
    for (auto& b : ctx->shards)
      if (a.device != b.device) {
        int ok = 0;
        (void)hipDeviceCanAccessPeer(&ok, a.device, b.device);
        if (ok) {
          DeviceGuard g(a.device);
          (void)hipDeviceEnablePeerAccess(b.device, 0);
          (void)hipGetLastError();
        }
      }
  return ctx.release();
}

mf_ctx* create_rank_ctx(const mf_params* p, int device_id, int nranks, int rank, const uint8_t* uid) {
  MF_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank / nranks");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
    fail(MF_ERR_NO_DEVICE, "no HIP device available (libmfhip has no CPU fallback)");
  MF_REQUIRE(device_id >= 0 && device_id < count, "device id out of range");
  std::unique_ptr<mf_ctx> ctx(new_ctx(p));
  ctx->G = nranks;
  ctx->rank_mode = true;
  { std::vector<Shard> tmp(1); ctx->shards.swap(tmp); }
  init_shard(ctx->shards[0], device_id, rank);
  if (nranks > 1) {
    DeviceGuard g(device_id);
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof(id));
    MF_NCCL(ncclCommInitRank(&ctx->comm, nranks, id, rank));
  }
  return ctx.release();
}

void destroy_ctx(mf_ctx* ctx) {
  try {
    det_spec_wait(ctx, true);
  } catch (...) {  // a failed speculative build only matters to a run that would have used it
  }
  for (auto& s : ctx->shards) {
    DeviceGuard g(s.device);
    (void)hipStreamSynchronize(s.stream);
  }
  dump_wave_trace(ctx);
  for (auto& s : ctx->shards) destroy_shard(s);
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  delete ctx;
}

// The testing hooks of include/mfhip_testing.h that read the driver's schedules.
void debug_levels(const uint32_t* urow, const uint32_t* irow, const int32_t* order, int64_t n, int32_t* level_out) {
  MF_REQUIRE(n >= 0 && (n == 0 || (urow && irow && level_out)), "bad argument");
  if (n == 0) return;
  uint32_t umax = 0, imax = 0;
  for (int64_t j = 0; j < n; ++j) { umax = std::max(umax, urow[j]); imax = std::max(imax, irow[j]); }
  std::vector<double> zero(n, 0.0);
  OrderedSeq sq{urow, irow, zero.data(), order, n, 0, umax + 1, 0, imax + 1};
  // levels in sequence order: replay the same recurrence build_level_plan uses
  LevelPlan lp;
  build_level_plan({sq}, lp);
  std::vector<int32_t> lu(umax + 1, 0), li(imax + 1, 0);
  for (int64_t j = 0; j < n; ++j) {
    const int64_t e = order ? order[j] : j;
    const int32_t l = std::max(lu[urow[e]], li[irow[e]]) + 1;
    lu[urow[e]] = l;
    li[irow[e]] = l;
    level_out[j] = l;
  }
  MF_REQUIRE(lp.levels() == (n ? *std::max_element(level_out, level_out + n) : 0), "level count mismatch");
}

}  // namespace mfhip
