// bpr.cpp -- BPR ranking training (mf_bpr_run / mf_bpr_step_triples / mf_bpr_fit): synchronous minibatch
// steps on the resident seen set, the table the positives are drawn from and the drawn negatives are checked
// against.  Nothing but the caller's triples (mf_bpr_step_triples) is uploaded.  The steps of one call are queued
// on the shard's stream with no host synchronisation between them: the scratch is sized once, before the
// first (bpr_reserve), launch sizes follow from the batch alone, and the counters of mf_bpr_stats are summed
// on the device and read once at the end.  The kernels are kernels_bpr.hip; the draw is bpr_draw.hpp.
//
// MFHIP_TIMING: the phases of every step on stderr (scratch, draw, then the step's own, named by launch_bpr_step); the
// stream is then drained after every phase, so the steps no longer overlap their launches.
#include <cmath>
#include <string>
#include <vector>

#include "bpr_draw.hpp"
#include "common.hpp"
#include "context.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mfhip {
namespace {

void bpr_check_ctx(const mf_ctx* ctx, const char* who) {
  if (ctx->rank_mode || ctx->shards.size() != 1)
    fail(MF_ERR_STATE, std::string(who) + " runs on a single-process context on one device");
  MF_REQUIRE(ctx->P.num_factors <= kBprMaxRank, "BPR supports a rank of at most " + std::to_string(kBprMaxRank) +
                                                    "; this context has k = " + std::to_string(ctx->P.num_factors));
}

int64_t chunk_now() {
  if (const std::string v = test_knob("bpr_chunk"); !v.empty())
    return std::min<int64_t>(std::max<int64_t>(1, std::atoll(v.c_str())), int64_t{1} << 30);
  return kBprChunk;
}

BprStep step_of(mf_ctx* ctx, Shard& s, const mf_bpr_params& p, int64_t batch) {
  return BprStep{s.stream,
                 batch,
                 s.uf.get(),
                 s.itf.get(),
                 static_cast<uint32_t>(ctx->U.rows()),
                 static_cast<uint32_t>(ctx->I.rows()),
                 ctx->P.num_factors,
                 ctx->f64,
                 p.lr,
                 p.lambda,
                 p.scale == MF_BPR_SCALE_MEAN,
                 chunk_now()};
}

void zero_stats(Shard& s) {
  s.bpr.stats.alloc(4 * 8);
  MF_HIP(hipMemsetAsync(s.bpr.stats.get(), 0, 4 * 8, s.stream));
}

// The device counters, read once; slots is the host's own count.
void read_stats(Shard& s, int64_t slots, mf_bpr_stats* out) {
  int64_t c[4] = {0, 0, 0, 0};
  MF_HIP(hipMemcpyAsync(c, s.bpr.stats.get(), sizeof(c), hipMemcpyDeviceToHost, s.stream));
  MF_HIP(hipStreamSynchronize(s.stream));
  if (out) *out = mf_bpr_stats{slots, c[1], c[2], c[3]};
}

}  // namespace

void bpr_check_params(const mf_bpr_params& p, bool sampled) {
  MF_REQUIRE(std::isfinite(p.lr) && p.lr > 0.0, "BPR needs a finite lr > 0");
  MF_REQUIRE(std::isfinite(p.lambda) && p.lambda >= 0.0, "BPR needs a finite lambda >= 0");
  MF_REQUIRE(p.scale == MF_BPR_SCALE_SUM || p.scale == MF_BPR_SCALE_MEAN, "unknown BPR scale rule (scale)");
  if (!sampled) return;
  MF_REQUIRE(p.batch >= 1 && p.batch <= kBprMaxBatch, "batch must lie in 1 .. 2^24");
  MF_REQUIRE(p.redraws >= 0 && p.redraws <= kBprMaxRedraws,
             "redraws must lie in 0 .. " + std::to_string(kBprMaxRedraws));
}

void bpr_check_steps(int64_t first_step, int64_t steps) {
  MF_REQUIRE(first_step >= 0 && steps >= 0, "first_step and steps must not be negative");
  MF_REQUIRE(first_step <= kBprMaxSteps && steps <= kBprMaxSteps - first_step, "steps run up to step 2^26");
}

void bpr_run(mf_ctx* ctx, const mf_bpr_params& p, int64_t first_step, int64_t steps, mf_bpr_stats* out) {
  bpr_check_ctx(ctx, "mf_bpr_run");
  Shard& s = ctx->shards[0];
  if (!s.seen.have) fail(MF_ERR_STATE, "mf_bpr_run without a seen set (mf_seen_set, mf_seen_add or mf_seen_from_als)");
  require_healthy(ctx);
  if (out) *out = mf_bpr_stats{0, 0, 0, 0};
  if (steps == 0) return;
  const int64_t pairs = seen_count(ctx), pool = ctx->I.rows();
  const int64_t slots = steps * static_cast<int64_t>(p.batch);
  if (pairs == 0 || pool < 2) {  // no positive to draw, or no row a negative could be: every slot is void
    s.bpr.last_n = -1;
    if (out) *out = mf_bpr_stats{slots, slots, 0, 0};
    return;
  }
  consolidate(ctx, s);
  sync_all(ctx);
  DeviceGuard g(s.device);
  PhaseClock clk;
  const SeenView v = seen_view(ctx, s, kSideU);
  const BprStep L = step_of(ctx, s, p, p.batch);
  bpr_reserve(s.stream, s.bpr, L.batch, L.user_rows, L.k, ctx->es, L.chunk);
  zero_stats(s);
  clk.lap("bpr_run: scratch");
  BprLap lap;  // MFHIP_TIMING: every phase of every step drained and timed by the one phase clock
  if (clk.on)
    lap = [&](const char* what) {
      MF_HIP(hipStreamSynchronize(s.stream));
      clk.lap(what);
    };
  for (int64_t t = first_step; t < first_step + steps; ++t) {
    launch_bpr_draw(L, s.bpr, v.off, v.ent, ctx->U.rows(), pairs, p.seed, t, p.redraws);
    if (lap) lap("bpr_run: draw");
    launch_bpr_step(L, s.bpr, lap);
  }
  s.bpr.last_n = L.batch;
  read_stats(s, slots, out);
}

void bpr_step_triples(mf_ctx* ctx, const mf_bpr_params& p, const int32_t* u, const int32_t* pos, const int32_t* neg,
                      int64_t n, mf_bpr_stats* out) {
  bpr_check_ctx(ctx, "mf_bpr_step_triples");
  if (!ctx->have_model)
    fail(MF_ERR_NOT_FITTED, "The MatrixFactorization model has not been fitted to data. "
                            "Fit the model before training it on triples.");
  require_healthy(ctx);
  if (out) *out = mf_bpr_stats{n, n, 0, 0};
  Shard& s = ctx->shards[0];
  if (n == 0 || ctx->U.rows() == 0 || ctx->I.rows() == 0) {  // (an empty side holds no id: every triple is void)
    s.bpr.last_n = -1;
    return;
  }
  consolidate(ctx, s);
  sync_all(ctx);
  DeviceGuard g(s.device);
  const BprStep L = step_of(ctx, s, p, n);
  bpr_reserve(s.stream, s.bpr, n, L.user_rows, L.k, ctx->es, L.chunk);
  zero_stats(s);
  sync_dev_index(s, ctx->U.index, s.didx[0]);
  sync_dev_index(s, ctx->I.index, s.didx[1]);
  uint32_t* trip = s.bpr.trip.as<uint32_t>();
  const size_t nb = static_cast<size_t>(n) * 4;
  MF_HIP(hipMemcpyAsync(trip, u, nb, hipMemcpyHostToDevice, s.stream));
  MF_HIP(hipMemcpyAsync(trip + n, pos, nb, hipMemcpyHostToDevice, s.stream));
  MF_HIP(hipMemcpyAsync(trip + 2 * n, neg, nb, hipMemcpyHostToDevice, s.stream));
  launch_id_lookup_one(s.stream, trip, n, s.didx[0].cap ? s.didx[0].slots.get() : nullptr, s.didx[0].cap - 1);
  launch_id_lookup_one(s.stream, trip + n, 2 * n, s.didx[1].cap ? s.didx[1].slots.get() : nullptr, s.didx[1].cap - 1);
  launch_bpr_resolve(L, s.bpr);
  launch_bpr_step(L, s.bpr);
  s.bpr.last_n = n;
  read_stats(s, n, out);  // (drains the stream: the caller's arrays have been read)
}

void bpr_fit(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, double init_scale, const mf_bpr_params& p,
             int64_t steps, mf_bpr_stats* out) {
  bpr_check_ctx(ctx, "mf_bpr_fit");
  require_healthy(ctx);
  det_spec_wait(ctx, true);  // new ids change the layouts the builds read
  sync_all(ctx);
  Shard& s = ctx->shards[0];
  if (!ctx->have_model) {
    ctx->U = SideLayout();
    ctx->I = SideLayout();
    ctx->have_model = true;
    ++ctx->layout_gen;
  }
  std::vector<uint32_t> ur, ir;
  lookup_rows(ctx->U, u, n, ur);
  lookup_rows(ctx->I, i, n, ir);
  als_insert_rows(ctx, s, u, i, n, ur, ir, init_scale);
  seen_put(ctx, u, i, n, false, nullptr);
  bpr_run(ctx, p, 0, steps, out);
}

void bpr_debug_triples(mf_ctx* ctx, int32_t* u, int32_t* pos, int32_t* neg, int64_t cap, int64_t* n_out) {
  bpr_check_ctx(ctx, "mf_debug_bpr_triples");
  Shard& s = ctx->shards[0];
  const int64_t n = s.bpr.last_n;
  if (n < 0) fail(MF_ERR_STATE, "mf_debug_bpr_triples: no BPR step has run kernels on this context");
  *n_out = n;
  if (cap < n) fail(MF_ERR_CAPACITY, "output capacity too small");
  DeviceGuard g(s.device);
  MF_HIP(hipStreamSynchronize(s.stream));
  std::vector<uint32_t> t(3 * static_cast<size_t>(n));
  MF_HIP(hipMemcpy(t.data(), s.bpr.trip.get(), t.size() * 4, hipMemcpyDeviceToHost));
  for (int64_t x = 0; x < n; ++x) {
    const bool is_void = t[x] == kRowMiss;
    u[x] = is_void ? -1 : static_cast<int32_t>(t[x]);
    pos[x] = is_void ? -1 : static_cast<int32_t>(t[n + x]);
    neg[x] = is_void ? -1 : static_cast<int32_t>(t[2 * n + x]);
  }
}

}  // namespace mfhip
