// dsgd_det.cpp -- deterministic-mode supersteps: the level launches (det_superstep, one launch per
// dependency level; MFHIP_TEST det_kernel=level) and the persistent sweep (kernels_detsweep.hip):
// its preparation (prepare_det_sweep, prepare_det_device_build), the per-superstep build on host
// worker threads (det_build) or on the device, and det_run's three-slot pipeline that builds
// supersteps s+1 and s+2 while the device runs s.  The slot table is placement.cpp's
// det_slot_table; the ring step between supersteps is ring.cpp's.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <future>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "common.hpp"
#include "context.hpp"
#include "jvm_random.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mfhip {

namespace {

// Fixed SoA layout of a DetBuf for at most n entries and nw waves (256-B aligned regions).
struct DetOffsets {
  size_t waves, u, i, qf, r, total;
};
DetOffsets det_offsets(int64_t n, int64_t nw) {
  auto up = [](size_t x) { return (x + 255) & ~static_cast<size_t>(255); };
  DetOffsets o;
  const size_t ne = static_cast<size_t>(n + kDetPad);  // the sweep reads whole chunks past a wave's end
  o.waves = 0;
  o.u = up(static_cast<size_t>(det_slot_room(nw)) * sizeof(DetWave));  // room for the split sweep's slot table
  o.i = o.u + up(ne * 4);
  o.qf = o.i + up(ne * 4);
  o.r = o.qf + up(ne * 4);
  o.total = o.r + up(ne * 8);
  return o;
}
// The regions of a buffer (pinned or device) laid out so.
DetStepOut det_regions(void* buf, const DetOffsets& o) {
  char* base = static_cast<char*>(buf);
  return {reinterpret_cast<DetWave*>(base + o.waves), reinterpret_cast<uint32_t*>(base + o.u),
          reinterpret_cast<uint32_t*>(base + o.i), reinterpret_cast<uint32_t*>(base + o.qf),
          reinterpret_cast<double*>(base + o.r)};
}

// The rating blocks shard s runs in superstep `superstep` and their shuffle seeds
// (new Random(iteration ^ ratingBlockId ^ seed), DSGDforMF.scala:392).
void det_blocks(const mf_ctx* ctx, const Shard& s, int64_t superstep, std::vector<int64_t>& blocks,
                std::vector<int64_t>& seeds) {
  const int32_t n = ctx->nb;
  const int32_t iteration = static_cast<int32_t>(superstep / n);
  blocks.clear();
  seeds.clear();
  for (int32_t j = 0; j < ctx->c; ++j) {
    const int32_t p = s.index * ctx->c + j;
    const int32_t q = static_cast<int32_t>((p + superstep - 1) % n);
    const int64_t b = static_cast<int64_t>(p) * n + q;  // toRatingBlockId (:597-601)
    if (ctx->rb.size(b) == 0) continue;
    blocks.push_back(b);
    seeds.push_back(static_cast<int64_t>(iteration ^ static_cast<int32_t>(b)) ^ ctx->P.seed);
  }
}

// MFHIP_TIMING=1: where a det_run call's host time goes (build time, waits for builds and for
// staging copies), on stderr at the end of the call
struct DetRunClock {
  std::atomic<int64_t> build_ns{0}, builds{0};
};
DetRunClock g_det_clock;
const bool g_det_timing = std::getenv("MFHIP_TIMING") != nullptr;

}  // namespace

// ---------------------------------------------------------------------------------------
// One superstep on one shard, one launch per dependency level.
void det_superstep(mf_ctx* ctx, Shard& s, int64_t superstep, double eta) {
  const int32_t n = ctx->nb;
  std::vector<std::vector<int32_t>> orders;
  std::vector<OrderedSeq> seqs;
  std::vector<int64_t> rbids, seeds;
  det_blocks(ctx, s, superstep, rbids, seeds);
  orders.resize(rbids.size());
  parallel_tasks(static_cast<int64_t>(rbids.size()), [&](int64_t x) {
    const int64_t len = ctx->rb.size(rbids[x]);
    orders[x].resize(len);
    if (ctx->P.has_seed) {
      JavaRandom rng(seeds[x]);                   // :392
      scala_shuffle(rng, orders[x].data(), len);  // :393
    } else {
      std::random_device rd;
      JavaRandom rng((static_cast<int64_t>(rd()) << 32) ^ rd());
      scala_shuffle(rng, orders[x].data(), len);
    }
  });
  for (size_t x = 0; x < rbids.size(); ++x) {
    const int64_t b = rbids[x];
    const int32_t p = static_cast<int32_t>(b / n), q = static_cast<int32_t>(b % n);
    const int64_t st = ctx->rb.start[b];
    OrderedSeq sq;
    sq.u = ctx->rb.urow.data() + st;
    sq.i = ctx->rb.irow.data() + st;
    sq.r = ctx->rb.r.data() + st;
    sq.order = orders[x].data();
    sq.len = ctx->rb.size(b);
    sq.u_lo = static_cast<uint32_t>(ctx->U.block_start[p]);
    sq.u_hi = static_cast<uint32_t>(ctx->U.block_start[p + 1]);
    sq.i_lo = static_cast<uint32_t>(ctx->I.block_start[q]);
    sq.i_hi = static_cast<uint32_t>(ctx->I.block_start[q + 1]);
    seqs.push_back(sq);
  }
  if (seqs.empty()) return;
  LevelPlan lp;
  build_level_plan(seqs, lp);
  DeviceGuard g(s.device);
  const size_t bytes = lp.entries.size() * sizeof(DetEntry);
  MF_HIP(hipStreamSynchronize(s.stream));  // the pinned staging buffer is reused
  s.det_pin.alloc(bytes);
  s.det_dev.alloc(bytes);
  std::memcpy(s.det_pin.as<void>(), lp.entries.data(), bytes);
  MF_HIP(hipMemcpyAsync(s.det_dev.get(), s.det_pin.as<void>(), bytes, hipMemcpyHostToDevice, s.stream));
  const DetEntry* dev = s.det_dev.as<DetEntry>();
  for (int64_t l = 0; l < lp.levels(); ++l) {
    const int64_t b0 = lp.level_start[l], cnt = lp.level_start[l + 1] - b0;
    LaunchTimer t(s, ctx->profiling);
    launch_level(s.stream, dev + b0, cnt, s.uf.get(), s.itf.get(), s.regu.get(), s.regi.get(),
                 ctx->P.num_factors, eta, Arith::kDsgd, true);
  }
  MF_HIP(hipGetLastError());
  ctx->stats.levels += lp.levels();
  ctx->stats.updates += static_cast<int64_t>(lp.entries.size());
  ctx->stats.kernel_launches += lp.levels();
  // per update: two f64 rows read and written, the 16-B entry, the two lambda/omega values
  ctx->stats.moved_bytes += static_cast<double>(lp.entries.size()) * (32.0 * ctx->P.num_factors + 32.0);
}

// Joins the speculative builds of det_run.  invalidate: the training data, the layouts or the
// superstep changes, so the builds are dropped (otherwise a later run may still use them).
// A failed build is never used: its slot is marked empty before the error can surface, and when the
// builds are being dropped (invalidate) their errors are dropped with them (MFHIP_DEBUG_PLAN logs
// them) -- only a run that would take a build over reports its failure (det_run).
void det_spec_wait(mf_ctx* ctx, bool invalidate) {
  std::exception_ptr first;
  for (int slot = 0; slot < kDetSlots; ++slot) {
    if (ctx->det_spec[slot].valid()) {
      try {
        ctx->det_spec[slot].get();
      } catch (const std::exception& e) {
        ctx->det_spec_s[slot] = -1;
        if (invalidate) {
          if (std::getenv("MFHIP_DEBUG_PLAN")) std::fprintf(stderr, "[mfhip] dropped speculative build: %s\n", e.what());
        } else if (!first) {
          first = std::current_exception();
        }
      } catch (...) {
        ctx->det_spec_s[slot] = -1;
        if (!invalidate && !first) first = std::current_exception();
      }
    }
    if (invalidate) ctx->det_spec_s[slot] = -1;
  }
  if (first) std::rethrow_exception(first);
}

// The device's CU count: the period of det_slot_table (blocks b and b + period share a CU).
int64_t device_cu_count(int dev) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
  return cus;
}

namespace {

// Host side of one superstep for every local shard, into det_buf[slot] (runs on a worker thread
// while the device runs the previous superstep).
void det_build(mf_ctx* ctx, int64_t superstep, int slot) {
  const auto t_build = std::chrono::steady_clock::now();
  struct Done {
    std::chrono::steady_clock::time_point t;
    ~Done() {
      if (g_det_timing) {
        g_det_clock.build_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t).count();
        g_det_clock.builds += 1;
      }
    }
  } done{t_build};
  std::vector<int64_t> blocks, seeds;
  if (ctx->det_dev_build || ctx->det_switch.load(std::memory_order_acquire)) {
    // the device builds the entries (det_run): here only each block's JVM shuffle, written as the
    // uploaded permutation, and the superstep index's fixed slot table
    const int64_t sm = (superstep - 1) % ctx->nb;
    for (auto& s : ctx->shards) {
      DetBuf& db = s.det_buf[slot];
      det_blocks(ctx, s, superstep, blocks, seeds);
      db.dev_built = true;
      db.n = s.det_sm_n[sm];
      db.nw = static_cast<int64_t>(s.det_sm_slots[sm].size());
      if (db.n == 0) continue;
      const DetStepOut out = det_regions(db.pin.as<void>(), det_offsets(s.det_n_max, s.det_nw_max));
      std::memcpy(out.waves, s.det_sm_slots[sm].data(), static_cast<size_t>(db.nw) * sizeof(DetWave));
      int32_t* ord = reinterpret_cast<int32_t*>(out.u);  // (the host path's u region)
      std::vector<int64_t> e0(blocks.size() + 1, 0);
      for (size_t x = 0; x < blocks.size(); ++x) e0[x + 1] = e0[x] + ctx->rb.size(blocks[x]);
      std::vector<uint64_t> rseeds(blocks.size());
      if (!ctx->P.has_seed) {
        std::random_device rd;
        for (auto& v : rseeds) v = (static_cast<uint64_t>(rd()) << 32) ^ rd();
      }
      parallel_tasks(static_cast<int64_t>(blocks.size()), [&](int64_t x) {
        JavaRandom rng(ctx->P.has_seed ? seeds[x] : static_cast<int64_t>(rseeds[x]));
        scala_shuffle(rng, ord + e0[x], e0[x + 1] - e0[x]);  // DSGDforMF.scala:392-393
      });
    }
    return;
  }
  for (auto& s : ctx->shards) {
    DetBuf& db = s.det_buf[slot];
    det_blocks(ctx, s, superstep, blocks, seeds);
    db.dev_built = false;
    db.n = db.nw = 0;
    for (int64_t b : blocks) {
      db.n += ctx->rb.size(b);
      db.nw += s.det_layout.block_waves[b];
    }
    if (db.n == 0) continue;
    const DetStepOut out = det_regions(db.pin.as<void>(), det_offsets(s.det_n_max, s.det_nw_max));
    build_det_step(ctx->rb, ctx->U, ctx->I, s.det_layout, blocks, seeds, ctx->P.has_seed != 0, out, &db.scratch);
    if (ctx->det_split)
      db.nw = det_slot_table(out.waves, db.nw, ctx->det_split_blocks, ctx->det_alone, ctx->det_cu_period);
  }
}

}  // namespace

// Deterministic supersteps with the persistent sweep: the host builds supersteps s+1 and s+2
// while the device runs superstep s.
void det_run(mf_ctx* ctx, int64_t count) {
  const int k = ctx->P.num_factors;
  const int64_t s0 = ctx->superstep_done + 1;
  using clk = std::chrono::steady_clock;
  const auto t_run = clk::now();
  const int64_t b_ns0 = g_det_clock.build_ns, b_n0 = g_det_clock.builds;
  int64_t wait_build_ns = 0, wait_copy_ns = 0;
  auto since = [](clk::time_point t) { return std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - t).count(); };
  auto reclaim = [&](int slot) {  // the staging copy out of this slot's pinned buffer has finished
    const auto t = clk::now();
    for (auto& sh : ctx->shards) {
      DetBuf& db = sh.det_buf[slot];
      if (!db.pending) continue;
      DeviceGuard g(sh.device);
      MF_HIP(hipEventSynchronize(db.copied));
      db.pending = false;
    }
    wait_copy_ns += since(t);
  };
  std::future<void> builds[kDetSlots];
  constexpr int kAhead = kDetSlots - 1;  // supersteps built ahead of the one launched
  // the previous run's speculative builds of supersteps s0 .. s0+kAhead-1 (slots 0 ..) are taken over;
  // any other is joined and dropped (a taken-over build is waited for like the run's own)
  bool prebuilt[kDetSlots] = {};
  for (int slot = 0; slot < kDetSlots; ++slot) {
    const int64_t built = ctx->det_spec_s[slot];
    ctx->det_spec_s[slot] = -1;  // before anything can throw: a slot is never taken over twice
    if (slot < kAhead && slot < count && built == s0 + slot && ctx->det_spec[slot].valid()) {
      builds[slot] = std::move(ctx->det_spec[slot]);  // joined (and its error raised) below, like a fresh build
      prebuilt[slot] = true;
    } else if (ctx->det_spec[slot].valid()) {
      try {
        ctx->det_spec[slot].get();  // a build this run does not use: its failure does not matter
      } catch (...) {
      }
    }
  }
  for (int slot = 0; slot < kDetSlots; ++slot) reclaim(slot);  // a previous call's last copies
  for (int64_t x = 0; x < std::min<int64_t>(count, kAhead); ++x)
    if (!prebuilt[x % kDetSlots])
      builds[x % kDetSlots] = std::async(std::launch::async, det_build, ctx, s0 + x, static_cast<int>(x % kDetSlots));
  for (int64_t x = 0; x < count; ++x) {
    const int64_t s = s0 + x;
    const int slot = static_cast<int>(x % kDetSlots);
    {
      const auto t = clk::now();
      builds[slot].get();  // every superstep of the run has a build (taken over or started here)
      wait_build_ns += since(t);
    }
    // auto mode: when the device has already finished the previous superstep twice in a row by the
    // time its host build is done, the host is the bottleneck (a busy or small host): from then on
    // the builds leave the gather / sorts / scatter to the device (det_device_build), whose host
    // part is the shuffle alone.  Either build gives the same entries, so the factors do not change.
    if (ctx->det_dev_ready && !ctx->det_dev_build && !ctx->det_switch.load() && x >= 2) {
      bool idle = true;
      for (auto& sh : ctx->shards) {
        const DetBuf& pb = sh.det_buf[(slot + kDetSlots - 1) % kDetSlots];
        if (pb.n == 0) continue;
        DeviceGuard g(sh.device);
        idle = idle && hipEventQuery(pb.swept) == hipSuccess;
      }
      ctx->det_idle = idle || ctx->det_mixed ? ctx->det_idle + 1 : 0;
      if (ctx->det_idle >= 2) {
        ctx->det_switch.store(true, std::memory_order_release);
        if (g_det_timing)
          std::fprintf(stderr, "[mfhip] det_run: host builds fell behind at superstep %lld: device builds from now on\n",
                       static_cast<long long>(s));
      }
    }
    const int32_t iteration = static_cast<int32_t>(s / ctx->nb);  // :476
    const double eta = learning_rate(ctx->P.lr_method, ctx->P.learning_rate, iteration + 1, ctx->P.lambda,
                                     ctx->P.lr_arg);  // :383-386
    for (auto& sh : ctx->shards) {
      DetBuf& db = sh.det_buf[slot];
      if (db.n == 0) continue;
      DeviceGuard g(sh.device);
      const DetOffsets o = det_offsets(sh.det_n_max, sh.det_nw_max);
      const DetStepOut h = det_regions(db.pin.as<void>(), o), d = det_regions(db.dev.get(), o);
      const size_t wave_bytes = static_cast<size_t>(db.nw) * sizeof(DetWave), n = static_cast<size_t>(db.n);
      // staging copy on the copy stream, after the sweep that last read this buffer (s-3), so it
      // overlaps the sweeps still running on the compute stream
      MF_HIP(hipStreamWaitEvent(sh.copy_stream, db.swept, 0));
      if (db.dev_built) {
        // the slot table and the shuffle permutation go up; the entries are built on the device
        // (det_device_build), on the same stream
        const int64_t sm = (s - 1) % ctx->nb;
        MF_HIP(hipMemcpyAsync(d.waves, h.waves, wave_bytes, hipMemcpyHostToDevice, sh.copy_stream));
        MF_HIP(hipMemcpyAsync(sh.det_ord.get(), h.u, n * 4, hipMemcpyHostToDevice, sh.copy_stream));
        det_device_build(sh.copy_stream, sh.det_bs, sh.det_ord.as<int32_t>(), db.n,
                         sh.det_bt.as<DetBuildBlock>() + static_cast<size_t>(sm) * ctx->c, sh.det_sm_nblk[sm],
                         sh.det_aos_dev.as<DetEntry>(), sh.det_iw.as<int32_t>(), sh.det_wave_bound,
                         static_cast<uint32_t>(ctx->U.rows()), d.u, d.i, d.qf, d.r);
      } else {
        const std::tuple<void*, const void*, size_t> regions[] = {
            {d.waves, h.waves, wave_bytes}, {d.u, h.u, n * 4}, {d.i, h.i, n * 4}, {d.qf, h.qf, n * 4}, {d.r, h.r, n * 8}};
        for (const auto& [dst, src, bytes] : regions)
          MF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, sh.copy_stream));
      }
      MF_HIP(hipEventRecord(db.copied, sh.copy_stream));
      db.pending = true;
      MF_HIP(hipStreamWaitEvent(sh.stream, db.copied, 0));
      MF_HIP(hipMemsetAsync(sh.det_ticket.get(), 0, sh.det_ticket.bytes(), sh.stream));
      LaunchTimer tm(sh, ctx->profiling, true);
      if (ctx->det_split)
        launch_det_sweep_split(sh.stream, d.waves, static_cast<int>(db.nw), d.u, d.i, d.qf, d.r, sh.uf.as<double>(),
                               sh.itf.as<double>(), sh.uf.bytes(), sh.itf.bytes(), sh.regu.as<double>(),
                               sh.regi.as<double>(), k, eta, sh.det_ticket.as<int32_t>(), sh.det_err.as<int32_t>(),
                               tm.start(), tm.stop());
      else
        launch_det_sweep(sh.stream, d.waves, static_cast<int>(db.nw), d.u, d.i, d.qf, d.r, sh.uf.as<double>(),
                         sh.itf.as<double>(), sh.uf.bytes(), sh.itf.bytes(), sh.regu.as<double>(),
                         sh.regi.as<double>(), k, eta, sh.det_ticket.as<int32_t>(), sh.det_scratch.as<int32_t>(),
                         sh.det_err.as<int32_t>(), tm.start(), tm.stop());
      MF_HIP(hipGetLastError());
      MF_HIP(hipEventRecord(db.swept, sh.stream));
      ctx->stats.updates += db.n;
      ctx->stats.kernel_launches += 1;
      // rows: user in + out and item in + out per update (an upper bound: an item row kept in
      // registers across consecutive entries of its item moves once); per update the 20-B entry,
      // two lambda/omega doubles and the ticket poll + store
      ctx->stats.moved_bytes += 8.0 * k * static_cast<double>(4 * db.n) + 44.0 * db.n;
    }
    ring_shift(ctx, s);
    ctx->superstep_done = s;
    ctx->stats.supersteps++;
    if (x + kAhead < count) {  // superstep s+kAhead goes where s-1 was staged: its copy must be done
      const int other = static_cast<int>((x + kAhead) % kDetSlots);
      reclaim(other);
      builds[other] = std::async(std::launch::async, det_build, ctx, s + kAhead, other);
    }
  }
  ctx->stats.algorithmic_bytes = static_cast<double>(ctx->stats.updates) * bytes_per_update(ctx);
  if (g_det_timing)
    std::fprintf(stderr,
                 "[mfhip] det_run: %lld supersteps enqueued in %.1f ms; waited %.1f ms for host builds, %.1f ms for "
                 "staging copies; %lld builds finished meanwhile, %.2f ms each\n",
                 static_cast<long long>(count), since(t_run) / 1e6, wait_build_ns / 1e6, wait_copy_ns / 1e6,
                 static_cast<long long>(g_det_clock.builds - b_n0),
                 g_det_clock.builds > b_n0 ? (g_det_clock.build_ns - b_ns0) / 1e6 / (g_det_clock.builds - b_n0) : 0.0);
  if (g_det_timing && g_det_clock.builds > 0)
    std::fprintf(stderr, "[mfhip] det builds so far, ms each: shuffle %.2f gather %.2f prefix %.2f scatter %.2f flags %.2f\n",
                 det_build_phase_ns(0) / 1e6 / g_det_clock.builds, det_build_phase_ns(1) / 1e6 / g_det_clock.builds,
                 det_build_phase_ns(2) / 1e6 / g_det_clock.builds, det_build_phase_ns(3) / 1e6 / g_det_clock.builds,
                 det_build_phase_ns(4) / 1e6 / g_det_clock.builds);
  // the next run's first supersteps, built in the background while the caller syncs, evaluates or
  // returns: a run's start no longer waits for its first host build (~36 ms of an NFLX call).  A builder
  // first waits for the staging copy that last read its slot's pinned buffer.
  for (int64_t x = 0; x < kAhead; ++x) {
    const int slot = static_cast<int>(x);
    const int64_t s = s0 + count + x;
    ctx->det_spec[slot] = std::async(std::launch::async, [ctx, slot, s] {
      for (auto& sh : ctx->shards) {
        if (!sh.det_buf[slot].copied) continue;
        DeviceGuard g(sh.device);
        MF_HIP(hipEventSynchronize(sh.det_buf[slot].copied));
      }
      det_build(ctx, s, slot);
    });
    ctx->det_spec_s[slot] = s;
  }
}

namespace {

// The device build of the det sweep's input (kernels.hpp det_device_build): per shard, the rating
// blocks' records and item -> wave maps on the device, and per superstep index its block table and
// wave / slot table.  A wave's entries are its items' ratings of the block, so its count -- and
// with it the wave table and the slot table -- is the same every time the block comes round; only
// the order inside the waves (the shuffle) changes.
void prepare_det_device_build(mf_ctx* ctx) {
  const int32_t n = ctx->nb;
  const DetEntry* aos = ctx->rb.det_aos.data();
  const int64_t total = static_cast<int64_t>(ctx->rb.det_aos.size());
  for (auto& s : ctx->shards) {
    DeviceGuard g(s.device);
    const DetSweepLayout& L = s.det_layout;
    const int64_t nb2 = static_cast<int64_t>(n) * n;
    // per rating block of this shard: its wave counts and its item -> wave map's offset
    std::vector<std::vector<int64_t>> wcnt(nb2);
    std::vector<int64_t> iwoff(nb2, -1);
    std::vector<int32_t> iw;
    for (int64_t b = 0; b < nb2; ++b)
      if (L.block_waves[b] > 0 && !L.item_wave[b].empty()) {
        iwoff[b] = static_cast<int64_t>(iw.size());
        iw.insert(iw.end(), L.item_wave[b].begin(), L.item_wave[b].end());
      }
    parallel_tasks(nb2, [&](int64_t b) {
      if (L.block_waves[b] <= 0 || ctx->rb.size(b) == 0) return;
      const int64_t i0 = ctx->I.block_start[b % n];
      wcnt[b].assign(L.block_waves[b], 0);
      for (int64_t e = ctx->rb.start[b]; e < ctx->rb.start[b + 1]; ++e) wcnt[b][L.item_wave[b][aos[e].i - i0]]++;
    });
    s.det_sm_slots.assign(n, {});
    s.det_sm_n.assign(n, 0);
    s.det_sm_nblk.assign(n, 0);
    std::vector<DetBuildBlock> bt(static_cast<size_t>(n) * std::max(ctx->c, 1));
    std::vector<int64_t> blocks, seeds;
    for (int32_t sm = 0; sm < n; ++sm) {
      det_blocks(ctx, s, sm + 1, blocks, seeds);  // the blocks of superstep s depend on (s-1) mod n
      std::vector<DetWave> waves;
      int64_t e0 = 0;
      for (size_t x = 0; x < blocks.size(); ++x) {
        const int64_t b = blocks[x];
        MF_REQUIRE(iwoff[b] >= 0 && static_cast<int64_t>(wcnt[b].size()) == L.block_waves[b],
                   "det device build: a block without its wave layout");
        bt[static_cast<size_t>(sm) * ctx->c + x] =
            DetBuildBlock{e0, ctx->rb.start[b], iwoff[b], static_cast<uint32_t>(ctx->I.block_start[b % n]),
                          static_cast<uint32_t>(waves.size())};
        int64_t at = e0;
        for (int32_t w = 0; w < L.block_waves[b]; ++w) {
          waves.push_back(DetWave{at, static_cast<int32_t>(wcnt[b][w]), L.wave_single[b][w] ? kDetWaveSingleItem : 0});
          at += wcnt[b][w];
        }
        e0 = at;
      }
      const int64_t nw = static_cast<int64_t>(waves.size());
      waves.resize(static_cast<size_t>(det_slot_room(nw)));
      const int64_t nslots =
          ctx->det_split ? det_slot_table(waves.data(), nw, ctx->det_split_blocks, ctx->det_alone, ctx->det_cu_period)
                         : nw;
      waves.resize(static_cast<size_t>(nslots));
      s.det_sm_slots[sm] = std::move(waves);
      s.det_sm_n[sm] = e0;
      s.det_sm_nblk[sm] = static_cast<int32_t>(blocks.size());
    }
    s.det_aos_dev.alloc(static_cast<size_t>(std::max<int64_t>(total, 1)) * sizeof(DetEntry));
    if (total > 0)
      MF_HIP(hipMemcpy(s.det_aos_dev.get(), aos, static_cast<size_t>(total) * sizeof(DetEntry), hipMemcpyHostToDevice));
    s.det_iw.alloc(std::max<size_t>(iw.size(), 1) * 4);
    if (!iw.empty()) MF_HIP(hipMemcpy(s.det_iw.get(), iw.data(), iw.size() * 4, hipMemcpyHostToDevice));
    s.det_bt.alloc(bt.size() * sizeof(DetBuildBlock));
    MF_HIP(hipMemcpy(s.det_bt.get(), bt.data(), bt.size() * sizeof(DetBuildBlock), hipMemcpyHostToDevice));
    s.det_ord.alloc(static_cast<size_t>(std::max<int64_t>(s.det_n_max, 1)) * 4);
    s.det_wave_bound = static_cast<uint32_t>(std::max<int64_t>(s.det_nw_max, 1));
    det_device_build_reserve(s.det_bs, s.det_n_max, s.det_wave_bound, static_cast<uint32_t>(ctx->U.rows()));
  }
}

}  // namespace

// Deterministic mode: the persistent sweep's item -> wave layout and staging buffers, unless
// MFHIP_TEST det_kernel=level (one launch per dependency level, det_superstep) or the device
// cannot hold a superstep's waves.  Waves per superstep and shard: half the device's resident
// capacity (shared by the shards on that device; MFHIP_TEST det_waves= overrides).
void prepare_det_sweep(mf_ctx* ctx) {
  if (test_knob("det_kernel") == "level") return;
  // single-item chains split over two waves where k allows (MFHIP_TEST det_split=0: one wave each)
  const bool split = test_knob("det_split") != "0" && det_split_capacity(ctx->P.num_factors) > 0;
  int cap = 1 << 30;
  for (auto& s : ctx->shards) {
    DeviceGuard g(s.device);
    int sharers = 0;
    for (auto& o : ctx->shards) sharers += o.device == s.device;
    if (const char* v = std::getenv("MFHIP_DEVICE_SHARERS"))
      if (ctx->rank_mode) sharers = std::max(sharers, std::atoi(v));
    // in wave slots; the split sweep's helpers take one each, at most one per wave of the layout
    // (waves = cap / 2 below), so the slot table stays within the resident capacity
    cap = std::min(cap, (split ? det_split_capacity(ctx->P.num_factors) : det_sweep_capacity(ctx->P.num_factors)) /
                            std::max(1, sharers));
  }
  if (cap < 1) return;
  const uint64_t k8 = static_cast<uint64_t>(ctx->P.num_factors) * 8;
  if (static_cast<uint64_t>(ctx->U.rows()) * k8 >= kSlabLimit || static_cast<uint64_t>(ctx->I.rows()) * k8 >= kSlabLimit)
    return;  // the sweep addresses each f64 slab with 32-bit offsets
  // k not a multiple of 64: lanes past k use voffset 0x80000000, and with the out-of-range row
  // offset kOffOOB in soffset the 32-bit sum wraps to 0x7FFFF000 -- inside a slab of 2 GiB or more
  if (ctx->P.num_factors % 64 != 0 &&
      (static_cast<uint64_t>(ctx->U.rows()) * k8 >= 0x7FFFF000ull || static_cast<uint64_t>(ctx->I.rows()) * k8 >= 0x7FFFF000ull))
    return;
  int32_t waves = std::max(1, cap / 2);
  // the split sweep's slot table holds at most one block (two slots) per wave of the layout, and
  // at most cap / 2 blocks are resident: so at most cap / 2 waves there
  if (const std::string v = test_knob("det_waves"); !v.empty())
    waves = std::clamp(std::atoi(v.c_str()), 1, split ? std::max(1, cap / 2) : cap);
  const int32_t n = ctx->nb;
  {  // the build's shuffle-order gather reads one 16-B record per rating
    const int64_t total = ctx->rb.start.empty() ? 0 : ctx->rb.start.back();
    resize_huge(ctx->rb.det_aos, static_cast<size_t>(total));  // random reads: fewer TLB misses
    DetEntry* a = ctx->rb.det_aos.data();
    parallel_for(total, [&](int64_t b, int64_t e, int) {
      for (int64_t x = b; x < e; ++x) a[x] = DetEntry{ctx->rb.urow[x], ctx->rb.irow[x], ctx->rb.r[x]};
    });
  }
  for (auto& s : ctx->shards) {
    build_det_layout(s.det_layout, ctx->rb, ctx->U, ctx->I, ctx->c, s.index, waves);
    s.det_n_max = s.det_nw_max = 0;
    for (int32_t sm = 0; sm < n; ++sm) {
      int64_t cnt = 0, nw = 0;
      for (int32_t j = 0; j < ctx->c; ++j) {
        const int64_t b = rating_block_of(ctx, s.index, sm, j);
        cnt += ctx->rb.size(b);
        nw += s.det_layout.block_waves[b];
      }
      s.det_n_max = std::max(s.det_n_max, cnt);
      s.det_nw_max = std::max(s.det_nw_max, nw);
    }
    DeviceGuard g(s.device);
    const size_t bytes = std::max<size_t>(det_offsets(s.det_n_max, s.det_nw_max).total, 256);
    for (auto& db : s.det_buf) {
      if (db.pending) { MF_HIP(hipEventSynchronize(db.copied)); db.pending = false; }
      db.pin.alloc(bytes);
      db.dev.alloc(bytes);
    }
    s.det_ticket.alloc(static_cast<size_t>(std::max<int64_t>(ctx->U.rows(), 1)) * 4);
    s.det_scratch.alloc(static_cast<size_t>(s.det_nw_max) * 64);  // one scratch line per wave
    s.det_err.alloc(16);
    MF_HIP(hipMemsetAsync(s.det_err.get(), 0, 16, s.stream));
  }
  // the sweep's host build reads only det_aos from here on: release the (user row, item row,
  // rating) arrays it was made from (16 B per rating; ~11.5 GB at full YAHOO)
  ctx->reaper.drop(ctx->rb.urow);
  ctx->reaper.drop(ctx->rb.irow);
  ctx->reaper.drop(ctx->rb.r);
  ctx->reaper.release();
  ctx->det_sweep = true;
  ctx->det_split = split;
  ctx->det_split_blocks = cap / 2;
  ctx->det_alone = test_knob("det_alone") != "0";
  ctx->det_cu_period = device_cu_count(ctx->shards[0].device);
  // The sweep's input is built on the host while the device keeps up with it; the device build
  // (4% slower on a free host: its traffic slows the running chain, profiles/r06_det_device_build_ab.txt)
  // takes over when the host falls behind (det_run).  MFHIP_TEST det_build=device / host: always
  // that one; mixed: the switch from the third superstep on (tests).
  const std::string dbk = test_knob("det_build");
  ctx->det_dev_build = dbk == "device";
  ctx->det_dev_ready = dbk != "host";
  ctx->det_mixed = dbk == "mixed";
  ctx->det_switch = false;
  ctx->det_idle = 0;
  if (ctx->det_dev_ready) prepare_det_device_build(ctx);
}

}  // namespace mfhip
