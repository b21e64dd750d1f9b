// dsgd_fast.cpp -- fast-mode supersteps: the choice among the four launch shapes (systolic pair
// sweep, per-sub-step pair sweep, cell, persistent; choose_fast_kernel, want_pair_sys),
// prepare_fast with the group model, the cell / pair schedule and every shard's device tables,
// fast_superstep's launches, and the hooks that read the schedule (debug_fast_plan, plan_digest,
// the wave trace).  The systolic launches' block -> wave maps are placement.cpp's sys_placement;
// the ring step that overlaps the split launches is ring.cpp's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"
#include "context.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mfhip {

// Fast sweep kernel: pair (default where k is 64, 128 or 256; kernels_pair.hip) | cell (one
// update per step, any k; kernels_fast.hip) | persistent (kernels_fast.hip, one launch per
// superstep); MFHIP_TEST fast_kernel= overrides.
// Pair cells as one systolic launch per superstep (default; MFHIP_TEST pair_sys=0: one launch per
// sub-step).  Falls back to per-sub-step launches when a superstep's waves cannot all be resident.
bool want_pair_sys() { return test_knob("pair_sys") != "0"; }

FastKernel choose_fast_kernel(int k) {
  const std::string want = test_knob("fast_kernel");
  if (want == "persistent") return FastKernel::kPersistent;
  if (want == "cell") return FastKernel::kCell;
  if (pair_kernel_supports(k)) return FastKernel::kPair;
  return FastKernel::kCell;
}

// The pair sweep's plan window for k (plan.hpp pair_window, plan_window_pack): MFHIP_TEST
// pair_window=N overrides the mixed cells' window for the window sweeps (clamped to the ring's
// minimum 2 * pair_ring), run_window=N the single-item cells' (plan.hpp pair_run_window; 0 = the
// same window, forwarded repeats allowed).
int32_t plan_window(int32_t k) {
  int32_t w = pair_window(k), rw = pair_run_window(k);
  if (const std::string v = test_knob("pair_window"); !v.empty())
    w = std::max<int32_t>(2 * pair_ring(pair_kpl(k)), std::atoi(v.c_str()));
  if (const std::string v = test_knob("run_window"); !v.empty()) rw = std::atoi(v.c_str());
  if (rw != 0) rw = std::clamp<int32_t>(rw, w, 0x7FFF);
  return plan_window_pack(w, rw);
}

// MFHIP_WAVE_TRACE=<file>: per wave of the per-cell schedules "shard sm t wave steps cells start
// end" (100 MHz clock) of the last time every sub-step ran; written when the context is destroyed.
// The systolic sweep adds a 9th column: the cell's shader-clock cycles (s_memtime), so the clock
// the wave actually ran at is cycles / ((end - start) x 10 ns), and a 10th: where the wave ran,
// XCC_ID << 32 | HW_ID (SIMD bits 5:4, CU 11:8, SH 12, SE 15:13).
void dump_wave_trace(mf_ctx* ctx) {
  const char* path = exp_knob("MFHIP_WAVE_TRACE");
  if (!path) return;
  FILE* f = nullptr;
  for (auto& s : ctx->shards) {
    if (s.st_trace.get() && !s.st_sys_host.empty()) {  // systolic: one row per cell, wave = index in superstep
      DeviceGuard g(s.device);
      std::vector<uint64_t> tr(s.st_sys_host.size() * 4);
      MF_HIP(hipMemcpy(tr.data(), s.st_trace.get(), tr.size() * 8, hipMemcpyDeviceToHost));
      if (!f) f = std::fopen(path, "w");
      if (!f) return;
      for (int32_t sm = 0; sm < ctx->nb; ++sm)
        for (int64_t w = s.st_sys_off[sm]; w < s.st_sys_off[sm + 1]; ++w) {
          const SysWave& sw = s.st_sysw_host[w];
          for (int32_t t = 0; t < sw.G; ++t) {
            const int64_t x = sw.cell0 + t;
            std::fprintf(f, "%d %d %d %lld %d %d %llu %llu %llu %llu\n", s.index, sm, t, (long long)(w - s.st_sys_off[sm]),
                         s.st_sys_host[x].steps, s.st_sys_host[x].cells, (unsigned long long)tr[4 * x],
                         (unsigned long long)tr[4 * x + 1], (unsigned long long)tr[4 * x + 2],
                         (unsigned long long)tr[4 * x + 3]);
          }
        }
      continue;
    }
    if (!s.st_trace.get() || s.st_waves_host.empty()) continue;
    DeviceGuard g(s.device);
    std::vector<uint64_t> tr(s.st_waves_host.size() * 2);
    MF_HIP(hipMemcpy(tr.data(), s.st_trace.get(), tr.size() * 8, hipMemcpyDeviceToHost));
    if (!f) f = std::fopen(path, "w");
    if (!f) return;
    const int64_t G = ctx->G_fast;
    for (size_t x = 0; x + 1 < s.st_sub_off.size(); ++x)
      for (int64_t w = s.st_sub_off[x]; w < s.st_sub_off[x + 1]; ++w)
        std::fprintf(f, "%d %lld %lld %lld %d %d %llu %llu\n", s.index, (long long)(x / G), (long long)(x % G),
                     (long long)(w - s.st_sub_off[x]), s.st_waves_host[w].steps, s.st_waves_host[w].cells,
                     (unsigned long long)tr[2 * w], (unsigned long long)tr[2 * w + 1]);
  }
  if (f) std::fclose(f);
}

// ---------------------------------------------------------------------------------------
// One superstep on one shard.
void fast_superstep(mf_ctx* ctx, Shard& s, int64_t superstep, double eta) {
  const int32_t n = ctx->nb;
  const int64_t smod = (superstep - 1) % n;
  DeviceGuard g(s.device);
  const FastBlk* blks = s.fast_blks.as<FastBlk>() + smod * ctx->c;
  int64_t ups = 0;
  for (int32_t j = 0; j < ctx->c; ++j) {
    ups += ctx->fast_rb_size[rating_block_of(ctx, s.index, smod, j)];
  }
  if (ups == 0) return;
  const int64_t sp0 = s.st_split_off.empty() ? 0 : s.st_split_off[smod];
  const int nsplit = s.st_split_off.empty() ? 0 : static_cast<int>(s.st_split_off[smod + 1] - sp0);
  launch_split_fork(s.stream, s.st_split.as<SplitItem>() + sp0, nsplit, s.itf.as<float>(), ctx->P.num_factors);
  if (ctx->fast_pair && ctx->fast_sys) {
    const int64_t w0 = s.st_sys_off[smod], nw = s.st_sys_off[smod + 1] - w0;
    auto sweep = [&](hipStream_t st, int64_t a, int64_t z) {  // waves [a, z) of the superstep
      if (z <= a) return;
      LaunchTimer tm(s, ctx->profiling, true);
      // with a placement table the launch has its empty blocks too (sys_placement pad)
      const bool placed = s.st_place.get() != nullptr;
      const int64_t blocks = z - a + (placed && a == 0 && z == nw ? 8 * s.st_place_pad[smod] : 0);
      launch_sweep_pair_sys(st, s.st_sysw.as<SysWave>() + w0 + a, s.st_sys.as<WaveDesc>(), static_cast<int>(blocks),
                            static_cast<int>(a), s.st_recs.as<PairRec>(), s.uf.as<float>(), s.itf.as<float>(),
                            s.uf.bytes(), s.itf.bytes(), ctx->P.num_factors, static_cast<float>(eta),
                            s.fast_prog.as<int32_t>(), s.sys_base, s.fast_err.as<int32_t>(),
                            s.st_trace.get() ? s.st_trace.as<uint64_t>() : nullptr, tm.start(), tm.stop(),
                            placed ? s.st_place.as<int32_t>() + s.st_place_off[smod] + a : nullptr);
      ctx->stats.kernel_launches += 1;
    };
    if (ctx->ring_overlap) {
      // A: local blocks 0..c-2 on the compute stream, behind the previous superstep's block c-1
      // (its item block is A's last one now); B: block c-1 on aux, behind the item block the
      // ring step delivered.  Both may run at once (disjoint rows, all waves resident).
      const int64_t split = s.st_sys_block_off[static_cast<size_t>(smod) * (ctx->c + 1) + ctx->c - 1];
      MF_HIP(hipStreamWaitEvent(s.stream, s.ev_last, 0));
      sweep(s.stream, 0, split);
      MF_HIP(hipEventRecord(s.ev_front, s.stream));
      MF_HIP(hipStreamWaitEvent(s.aux, s.ev_moved, 0));
      sweep(s.aux, split, nw);
      MF_HIP(hipEventRecord(s.ev_last, s.aux));
    } else {
      sweep(s.stream, 0, nw);
    }
    if (nw > 0) s.sys_base += s.sys_step;
  } else if (ctx->fast_pair) {
    for (int32_t t = 0; t < ctx->G_fast; ++t) {
      const int64_t x = smod * ctx->G_fast + t;
      const int64_t w0 = s.st_sub_off[x], nw = s.st_sub_off[x + 1] - w0;
      if (nw == 0) continue;
      LaunchTimer tm(s, ctx->profiling, true);
      launch_sweep_pair(s.stream, s.st_waves.as<WaveDesc>() + w0, static_cast<int>(nw), s.st_recs.as<PairRec>(),
                        s.uf.as<float>(), s.itf.as<float>(), s.uf.bytes(), s.itf.bytes(), ctx->P.num_factors,
                        static_cast<float>(eta), s.st_trace.get() ? s.st_trace.as<uint64_t>() + 2 * w0 : nullptr,
                        tm.start(), tm.stop());
      ctx->stats.kernel_launches += 1;
    }
  } else if (ctx->fast_persistent) {
    MF_HIP(hipMemsetAsync(s.fast_prog.get(), 0, s.fast_prog.bytes(), s.stream));
    LaunchTimer tm(s, ctx->profiling);
    launch_fast_superstep(s.stream, blks, ctx->c, ctx->G_fast, s.fast_recs.as<FastRec>(), s.fast_cells.as<int32_t>(),
                          s.uf.as<float>(), s.itf.as<float>(), ctx->P.num_factors, static_cast<float>(eta),
                          s.uf.bytes(), s.itf.bytes(), (ctx->fast_dummy_u + 1) * 4u * ctx->P.num_factors,
                          ctx->fast_dummy_i * 4u * ctx->P.num_factors, s.fast_prog.as<int32_t>(),
                          s.fast_err.as<int32_t>());
    ctx->stats.kernel_launches += 1;
  } else {
    for (int32_t t = 0; t < ctx->G_fast; ++t) {
      LaunchTimer tm(s, ctx->profiling);
      launch_fast_substep(s.stream, blks, ctx->c, ctx->G_fast, t, s.fast_recs.as<FastRec>(),
                          s.fast_cells.as<int32_t>(), s.uf.as<float>(), s.itf.as<float>(), ctx->P.num_factors,
                          static_cast<float>(eta), s.uf.bytes(), s.itf.bytes(),
                          (ctx->fast_dummy_u + 1) * 4u * ctx->P.num_factors,
                          ctx->fast_dummy_i * 4u * ctx->P.num_factors, ctx->fast_prio_len);
    }
    ctx->stats.kernel_launches += ctx->G_fast;
  }
  static const bool keep_join = [] { const char* v = exp_knob("MFHIP_SPLIT_JOIN"); return v && std::string(v) == "keep"; }();
  if (!keep_join)  // MFHIP_SPLIT_JOIN=keep: the item keeps replica 0's chain (the others are dropped)
    launch_split_join(s.stream, s.st_split.as<SplitItem>() + sp0, nsplit, s.itf.as<float>(), ctx->P.num_factors);
  MF_HIP(hipGetLastError());
  ctx->stats.updates += ups;
  if (!s.sm_bytes.empty()) ctx->stats.moved_bytes += s.sm_bytes[smod];
}

namespace {

// The systolic pair sweep's group model and residency check: one G_j per rating block (automatic G)
// into block_groups, and ctx->fast_sys when every wave of a superstep can be resident at once.
// Returns the blocks of one systolic launch that can be resident at once.
int64_t choose_sys_groups(mf_ctx* ctx, DevRatingBlocks& dev_rb, std::vector<int32_t>& block_groups) {
  const int k = ctx->P.num_factors;
  const int64_t nb2 = static_cast<int64_t>(ctx->nb) * ctx->nb;
  int64_t sys_cap = 0;                // blocks of one systolic launch that can be resident at once
  if (!(ctx->fast_pair && want_pair_sys())) return sys_cap;
  int cap = 1 << 30, simds = 1 << 30;
  for (auto& s : ctx->shards) {
    DeviceGuard g(s.device);
    int cus = 0;
    MF_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s.device));
    cap = std::min(cap, sweep_pair_sys_capacity(k));
    simds = std::min(simds, 4 * cus);
  }
  // the group model's wave budget: one wave per SIMD.  (With the round-4 ring of 7 pairs a budget
  // of two waves per CU at k <= 128 and three at k = 256 was faster -- a pair step slowed sharply
  // with the waves sharing its CU; with the per-width rings of round 5 (plan.hpp pair_ring) the
  // model's own choice is best again: NFLX 20.0 ms with 656 waves vs 20.24 with 512, YAHOO 223.7
  // vs 232.0 ms with 1004 vs 768; profiles/r05_wave_budget.txt.)
  if (const std::string v = test_knob("sys_waves"); !v.empty()) simds = std::max(8, std::atoi(v.c_str()));
  if (ctx->P.fast_waves == 0 && test_knob("block_groups") != "0") {
    block_groups.assign(nb2, 0);
    for (auto& s : ctx->shards) {
      std::vector<int32_t> gb;
      if (ctx->rb.urow.empty() && dev_rb.urow.get()) {  // rating blocks on the device only
        DeviceGuard g(s.device);
        std::vector<int64_t> size(nb2, 0);
        for (int64_t b = 0; b < nb2; ++b) size[b] = ctx->rb.size(b);
        gb = choose_block_groups(size, device_block_tops(s.stream, dev_rb, ctx->rb, ctx->I), ctx->nb, ctx->c,
                                 s.index, simds, sys_cell_ns(k), sys_run_pair_ns(k));
      } else {
        gb = choose_block_groups(ctx->rb, ctx->I, ctx->c, s.index, simds, ctx->item_split, sys_cell_ns(k),
                                 sys_run_pair_ns(k));
      }
      for (int64_t b = 0; b < nb2; ++b)
        if (gb[b] > 0) block_groups[b] = gb[b];
    }
  }
  // every wave of a superstep must be resident at once -- on a device shared by several
  // shards (their streams run concurrently) or, in rank mode, by MFHIP_DEVICE_SHARERS ranks
  // (the one-GPU rehearsal of the ring), all of theirs together
  if (const char* v = std::getenv("MFHIP_DEVICE_SHARERS"))
    if (ctx->rank_mode && std::atoi(v) > 1) cap /= std::atoi(v);
  sys_cap = cap;
  bool fits = cap > 0;
  for (int32_t sm = 0; sm < ctx->nb && fits; ++sm) {
    std::vector<std::pair<int, int64_t>> per_dev;  // (device, waves of superstep sm)
    for (auto& s : ctx->shards) {
      int64_t waves = 0;
      for (int32_t j = 0; j < ctx->c; ++j) {
        const int64_t b = rating_block_of(ctx, s.index, sm, j);
        waves += block_groups.empty() || block_groups[b] == 0 ? ctx->G_fast : block_groups[b];
      }
      auto it = std::find_if(per_dev.begin(), per_dev.end(), [&](const auto& e) { return e.first == s.device; });
      if (it == per_dev.end()) per_dev.emplace_back(s.device, waves);
      else it->second += waves;
    }
    for (const auto& e : per_dev) fits = fits && e.second <= cap;
  }
  ctx->fast_sys = fits;
  if (!fits) block_groups.clear();
  return sys_cap;
}

// The cell plan (and, for the default systolic pair sweep of one shard, the pair schedule) on the
// device or on the host; true when dev_pp / dev_pairs hold the pair schedule.
bool build_fast_schedule(mf_ctx* ctx, DevRatingBlocks& dev_rb, PhaseClock& clk, std::vector<int32_t>& block_groups,
                         uint32_t dummy, FastPlan& fp, PairPlan& dev_pp, DevBuf& dev_pairs) {
  const int k = ctx->P.num_factors;
  const int64_t nb2 = static_cast<int64_t>(ctx->nb) * ctx->nb;
  // the per-cell emission and the pair records on the device (kernels_plan.hip) for the default
  // systolic pair sweep of one shard; MFHIP_TEST device_plan=0 keeps them on the host
  const std::string dpv = test_knob("device_plan");
  // (a rank whose user blocks hold no rating -- the reference's blocking can leave a block
  // empty -- plans on the host: its schedule is empty)
  const bool dev_plan = ctx->fast_pair && ctx->fast_sys && ctx->item_split == 0 &&
                        ctx->shards.size() == 1 && ctx->rb.start[nb2] > 0 && dpv != "0";
  std::vector<FastBlockWork> entries;
  // MFHIP_TEST device_plan: unset / 2 = the whole schedule on the device, 1 = host phase 1 + device
  // emission, 0 = host
  const bool dev_full = dev_plan && dev_rb.total == ctx->rb.start[nb2] && dev_rb.urow.get();
  if (dev_full) {
    std::vector<int32_t> Gb(nb2, ctx->G_fast);
    if (!block_groups.empty())
      for (int64_t b = 0; b < nb2; ++b) Gb[b] = block_groups[b] > 0 ? block_groups[b] : ctx->G_fast;
    Shard& s0 = ctx->shards[0];
    DeviceGuard g(s0.device);
    device_fast_schedule(s0.stream, dev_rb, ctx->rb, ctx->U, ctx->I, Gb, ctx->P.lambda,
                         static_cast<uint64_t>(ctx->P.seed) * 0x9E3779B97F4A7C15ULL + 1, fp, ctx->c, s0.index, k,
                         dummy, plan_window(k), dev_pp, dev_pairs);
    dev_rb = DevRatingBlocks();
  } else {
    if (ctx->rb.urow.empty() && dev_rb.urow.get()) {  // a host-built plan after all
      Shard& s0 = ctx->shards[0];
      DeviceGuard g(s0.device);
      fetch_rating_blocks(s0.stream, dev_rb, ctx->rb);
    }
    build_fast_plan(fp, ctx->rb, ctx->U, ctx->I, ctx->G_fast, k, ctx->P.lambda,
                    static_cast<uint64_t>(ctx->P.seed) * 0x9E3779B97F4A7C15ULL + 1, dummy, nullptr,
                    ctx->fast_pair ? plan_window(k) : kHazardWindow, block_groups.empty() ? nullptr : &block_groups,
                    ctx->item_split, static_cast<uint32_t>(ctx->I.rows() + 1), dev_plan ? &entries : nullptr);
  }
  MF_REQUIRE(static_cast<uint64_t>(ctx->I.rows() + 1 + fp.scratch_rows) * k * 4 < (1ull << 32),
             "hot-item replica rows exceed the 32-bit item slab offsets");
  if (dev_plan && !dev_full) {
    Shard& s0 = ctx->shards[0];
    DeviceGuard g(s0.device);
    clk.lap("cell order (host)");
    device_pair_schedule(s0.stream, entries, fp, ctx->nb, ctx->c, s0.index, k, dummy, plan_window(k), false, dev_pp,
                         dev_pairs);
    ctx->reaper.drop(entries);
  }
  ctx->stats.pads = fp.pads;
  ctx->reaper.drop(fp.scratch);
  clk.lap(dev_full ? "schedule (device)" : dev_plan ? "cell emission + pairs (device)" : "cell plan");
  return dev_plan;
}

// The systolic launches' block -> wave maps of one shard (placement.cpp sys_placement, which checks
// each to be a permutation), on the device.
void upload_sys_placement(mf_ctx* ctx, Shard& s, const PairPlan& pp, int64_t sys_cap) {
  s.st_place.release();
  s.st_place_off.assign(ctx->nb + 1, 0);
  s.st_place_pad.assign(ctx->nb, 0);
  if (test_knob("sys_place") == "0" || pp.sys_waves.empty()) return;
  // empty blocks isolate each XCD's heaviest wave (one launch per superstep, one shard:
  // the co-residency check above counted this shard's waves alone); MFHIP_TEST sys_iso=N:
  // its N heaviest (0: none).  Default: k <= 128 (NFLX -0.7%, ML20M even; YAHOO's four-wave
  // CUs lose 0.3% to the slots the empty blocks take, profiles/r06_sys_isolation_ab.txt)
  int32_t iso = !ctx->ring_overlap && ctx->shards.size() == 1 && ctx->P.num_factors <= 128 ? 1 : 0;
  if (const std::string v = test_knob("sys_iso"); !v.empty() && iso) iso = std::clamp(std::atoi(v.c_str()), 0, 8);
  std::vector<int32_t> place;
  sys_placement(pp, ctx->nb, ctx->c, ctx->ring_overlap, iso, sys_cap, place, s.st_place_off, s.st_place_pad);
  s.st_place.alloc(place.size() * sizeof(int32_t));
  MF_HIP(hipMemcpy(s.st_place.get(), place.data(), place.size() * sizeof(int32_t), hipMemcpyHostToDevice));
}

// One shard's pair schedule on the device: records, wave tables, systolic tables and placement.
void upload_pair_tables(mf_ctx* ctx, Shard& s, FastPlan& fp, bool dev_plan, PairPlan& dev_pp, DevBuf& dev_pairs,
                        int64_t sys_cap, PhaseClock& clk) {
  const int k = ctx->P.num_factors;
  PairPlan pp;
  if (dev_plan) {
    pp = std::move(dev_pp);
    s.st_recs = std::move(dev_pairs);
  } else {
    build_pair_plan(pp, fp, ctx->nb, ctx->c, s.index, k, !ctx->fast_sys);
  }
  ctx->stats.pads += pp.noop_halves - fp.pads;  // run padding on top of the planner's
  s.sm_bytes = pp.sm_bytes;
  s.st_nrecs = 0;
  for (const WaveDesc& wd : pp.waves) s.st_nrecs = std::max<int64_t>(s.st_nrecs, wd.base + wd.steps);
  if (!dev_plan) s.st_recs.alloc(std::max<size_t>(pp.recs.size(), 1) * sizeof(PairRec));
  s.st_waves.alloc(std::max<size_t>(pp.waves.size(), 1) * sizeof(WaveDesc));
  if (!pp.recs.empty())
    MF_HIP(hipMemcpy(s.st_recs.get(), pp.recs.data(), pp.recs.size() * sizeof(PairRec), hipMemcpyHostToDevice));
  if (!pp.waves.empty())
    MF_HIP(hipMemcpy(s.st_waves.get(), pp.waves.data(), pp.waves.size() * sizeof(WaveDesc), hipMemcpyHostToDevice));
  s.st_sub_off = std::move(pp.sub_off);
  s.st_sys_host.clear();
  s.sys_base = 0;
  if (ctx->fast_sys) {
    s.st_sys.alloc(std::max<size_t>(pp.sys.size(), 1) * sizeof(WaveDesc));
    if (!pp.sys.empty())
      MF_HIP(hipMemcpy(s.st_sys.get(), pp.sys.data(), pp.sys.size() * sizeof(WaveDesc), hipMemcpyHostToDevice));
    s.st_sysw.alloc(std::max<size_t>(pp.sys_waves.size(), 1) * sizeof(SysWave));
    if (!pp.sys_waves.empty())
      MF_HIP(hipMemcpy(s.st_sysw.get(), pp.sys_waves.data(), pp.sys_waves.size() * sizeof(SysWave),
                       hipMemcpyHostToDevice));
    s.st_sys_off = pp.sys_off;
    s.st_sys_block_off = pp.sys_block_off;
    upload_sys_placement(ctx, s, pp, sys_cap);
    s.sys_step = static_cast<uint32_t>(fp.G) + 1u;
    int64_t max_waves = 1;
    for (int32_t sm = 0; sm < ctx->nb; ++sm) max_waves = std::max(max_waves, pp.sys_off[sm + 1] - pp.sys_off[sm]);
    s.fast_prog.alloc(static_cast<size_t>(max_waves) * kProgStride * sizeof(int32_t));
    MF_HIP(hipMemsetAsync(s.fast_prog.get(), 0, s.fast_prog.bytes(), s.stream));
    s.fast_err.alloc(16);
    MF_HIP(hipMemsetAsync(s.fast_err.get(), 0, 16, s.stream));
  }
  clk.lap("pair plan + H2D");
  ctx->reaper.drop(pp.recs);
  if (exp_knob("MFHIP_WAVE_TRACE")) {
    const size_t n = ctx->fast_sys ? pp.sys.size() : pp.waves.size();
    const size_t per = ctx->fast_sys ? 32 : 16;  // systolic: realtime and shader-clock stamps
    s.st_trace.alloc(std::max<size_t>(n, 1) * per);
    MF_HIP(hipMemsetAsync(s.st_trace.get(), 0, std::max<size_t>(n, 1) * per, s.stream));
    if (ctx->fast_sys) {
      s.st_sys_host = pp.sys;
      s.st_sysw_host = pp.sys_waves;
    }
    else s.st_waves_host = pp.waves;
  }
}

// One shard's per-cell schedule on the device (the cell and persistent kernels).
void upload_cell_tables(mf_ctx* ctx, Shard& s, const FastPlan& fp) {
  const int k = ctx->P.num_factors;
  {  // requested bytes per superstep: 32-B record, user row in + out, item row per run in + out
    s.sm_bytes.assign(ctx->nb, 0.0);
    const double row_bytes = 4.0 * k;
    for (int32_t sm = 0; sm < ctx->nb; ++sm)
      for (int32_t j = 0; j < ctx->c; ++j) {
        const int64_t b = rating_block_of(ctx, s.index, sm, j);
        if (fp.cell_base[b] < 0) continue;
        const int32_t* o = fp.cell_off.data() + fp.cell_base[b];
        const int64_t GG = static_cast<int64_t>(fp.Gb[b]) * fp.Gb[b];
        const FastRec* f = fp.recs.data() + fp.rec_base[b];
        int64_t runs = 0;
        for (int64_t cc = 0; cc < GG; ++cc)
          for (int32_t x = o[cc]; x < o[cc + 1]; ++x)
            runs += x == o[cc] || ((f[x].i ^ f[x - 1].i) & ~kPadBit) != 0;
        s.sm_bytes[sm] += (32.0 + 2.0 * row_bytes) * o[GG] + 2.0 * row_bytes * static_cast<double>(runs);
      }
  }
  s.fast_recs.alloc(std::max<size_t>(fp.recs.size(), 1) * sizeof(FastRec));
  s.fast_cells.alloc(std::max<size_t>(fp.cell_off.size(), 1) * sizeof(int32_t));
  if (!fp.recs.empty())
    MF_HIP(hipMemcpy(s.fast_recs.get(), fp.recs.data(), fp.recs.size() * sizeof(FastRec), hipMemcpyHostToDevice));
  if (!fp.cell_off.empty())
    MF_HIP(hipMemcpy(s.fast_cells.get(), fp.cell_off.data(), fp.cell_off.size() * sizeof(int32_t),
                     hipMemcpyHostToDevice));
  std::vector<FastBlk> blks(static_cast<size_t>(ctx->nb) * ctx->c);
  for (int32_t sm = 0; sm < ctx->nb; ++sm)
    for (int32_t j = 0; j < ctx->c; ++j) {
      const int64_t b = rating_block_of(ctx, s.index, sm, j);
      blks[static_cast<size_t>(sm) * ctx->c + j] = FastBlk{fp.rec_base[b], fp.cell_base[b] < 0 ? 0 : fp.cell_base[b]};
    }
  s.fast_prog.alloc(static_cast<size_t>(ctx->c) * ctx->G_fast * kProgStride * sizeof(int32_t));
  s.fast_err.alloc(16);
  MF_HIP(hipMemsetAsync(s.fast_err.get(), 0, 16, s.stream));
  s.fast_blks.alloc(blks.size() * sizeof(FastBlk));
  MF_HIP(hipMemcpy(s.fast_blks.get(), blks.data(), blks.size() * sizeof(FastBlk), hipMemcpyHostToDevice));
}

}  // namespace

// Fast mode: the schedule model, the cell / pair plan and every shard's device tables.
void prepare_fast(mf_ctx* ctx, DevRatingBlocks& dev_rb, PhaseClock& clk, int32_t lo, int32_t hi) {
  const int64_t nb2 = static_cast<int64_t>(ctx->nb) * ctx->nb;
  const int64_t local = ctx->rb.start[nb2];
  const int64_t blocks_local = static_cast<int64_t>(hi - lo) * ctx->nb;
  const FastKernel fk = choose_fast_kernel(ctx->P.num_factors);
  ctx->G_fast = choose_groups(local / std::max<int64_t>(blocks_local, 1), ctx->c, ctx->P.fast_waves,
                              fk == FastKernel::kPair ? 40.0 : 150.0, fk == FastKernel::kPair ? 1024 : 2048);
  FastPlan fp;
  const uint32_t dummy = static_cast<uint32_t>(ctx->U.rows());  // zeroed row used by padding records
  MF_REQUIRE(static_cast<uint64_t>(ctx->U.rows() + 2) * ctx->P.num_factors * 4 < (1ull << 32) &&
                 static_cast<uint64_t>(ctx->I.rows() + 1) * ctx->P.num_factors * 4 < (1ull << 32),
             "fast mode addresses each factor slab with 32-bit offsets (< 4 GiB)");
  ctx->fast_pair = fk == FastKernel::kPair;
  ctx->fast_sys = false;
  std::vector<int32_t> block_groups;  // systolic sweep, automatic G: one G_j per rating block
  const int64_t sys_cap = choose_sys_groups(ctx, dev_rb, block_groups);
  clk.lap("schedule model (groups)");
  PairPlan dev_pp;
  DevBuf dev_pairs;
  const bool dev_plan = build_fast_schedule(ctx, dev_rb, clk, block_groups, dummy, fp, dev_pp, dev_pairs);
  {  // priority threshold: 3x the mean non-empty cell length
    int64_t cells = 0, recs = 0;
    for (int64_t b = 0; b < nb2; ++b)
      if (fp.cell_base[b] >= 0) {
        const int32_t* o = fp.cell_off.data() + fp.cell_base[b];
        const int64_t gg = static_cast<int64_t>(fp.Gb[b]) * fp.Gb[b];
        for (int64_t c2 = 0; c2 < gg; ++c2) cells += o[c2 + 1] > o[c2];
        recs += o[gg];
      }
    ctx->fast_prio_len = cells ? static_cast<int32_t>(std::max<int64_t>(16, 3 * recs / cells)) : (1 << 30);
    if (const char* v = exp_knob("MFHIP_PRIO_LEN")) ctx->fast_prio_len = std::atoi(v);
  }
  ctx->fast_rb_size.assign(nb2, 0);
  for (int64_t b = 0; b < nb2; ++b) ctx->fast_rb_size[b] = ctx->rb.size(b);
  ctx->stats.groups = ctx->G_fast;
  if (!block_groups.empty()) {  // report the mean G_j of the non-empty rating blocks
    int64_t sum = 0, cnt = 0;
    for (int64_t b = 0; b < nb2; ++b)
      if (fp.cell_base[b] >= 0) { sum += fp.Gb[b]; ++cnt; }
    ctx->stats.groups = cnt ? static_cast<int32_t>((sum + cnt / 2) / cnt) : ctx->G_fast;
  }
  ctx->fast_dummy_u = dummy;
  ctx->fast_dummy_i = static_cast<uint32_t>(ctx->I.rows());
  {
    ctx->ring_overlap = ctx->fast_pair && ctx->fast_sys && ctx->G > 1 && ctx->c >= 2 &&
                        ctx->item_split == 0 && test_knob("ring_overlap") != "0";
  }
  for (auto& s : ctx->shards) {
    ensure_rows(ctx, s, kSideU, ctx->U.rows() + 2);
    ensure_rows(ctx, s, MF_SIDE_ITEM, ctx->I.rows() + 1 + fp.scratch_rows);
    DeviceGuard g(s.device);
    {  // hot-item replicas of this shard's rating blocks, per superstep
      std::vector<SplitItem> tab;
      s.st_split_off.assign(ctx->nb + 1, 0);
      for (int32_t sm = 0; sm < ctx->nb; ++sm) {
        for (int32_t j = 0; j < ctx->c; ++j) {
          const int64_t b = rating_block_of(ctx, s.index, sm, j);
          tab.insert(tab.end(), fp.splits.begin() + fp.split_off[b], fp.splits.begin() + fp.split_off[b + 1]);
        }
        s.st_split_off[sm + 1] = static_cast<int64_t>(tab.size());
      }
      s.st_split.alloc(std::max<size_t>(tab.size(), 1) * sizeof(SplitItem));
      if (!tab.empty())
        MF_HIP(hipMemcpy(s.st_split.get(), tab.data(), tab.size() * sizeof(SplitItem), hipMemcpyHostToDevice));
    }
    const size_t row_bytes = static_cast<size_t>(ctx->P.num_factors) * ctx->es;
    MF_HIP(hipMemsetAsync(s.uf.as<char>() + static_cast<size_t>(dummy) * row_bytes, 0, 2 * row_bytes, s.stream));
    MF_HIP(hipMemsetAsync(s.itf.as<char>() + static_cast<size_t>(ctx->fast_dummy_i) * row_bytes, 0, row_bytes,
                          s.stream));
    if (ctx->fast_pair) {
      upload_pair_tables(ctx, s, fp, dev_plan, dev_pp, dev_pairs, sys_cap, clk);
      continue;
    }
    upload_cell_tables(ctx, s, fp);
  }
  clk.lap("device tables");
  // the device holds the schedule; release the host copies in the background
  ctx->reaper.drop(fp.recs);
  ctx->reaper.drop(ctx->rb.urow);
  ctx->reaper.drop(ctx->rb.irow);
  ctx->reaper.drop(ctx->rb.r);
  ctx->rb = RatingBlocks();
  ctx->rb.n_blocks = ctx->nb;
  ctx->reaper.release();
}

// The testing hooks of include/mfhip_testing.h that read the fast schedule.
int debug_fast_plan(const int32_t* u, const int32_t* i, int64_t n, int32_t n_blocks, int64_t seed, int32_t groups,
                    int32_t blocking, int32_t window, int32_t k, int32_t item_split, int32_t* block_out, int32_t* substep_out, int32_t* group_out, int64_t* pos_out,
                    int32_t* replica_out) {
  return guarded([&] {
    MF_REQUIRE(n >= 0 && n_blocks >= 1 && groups != 0 && item_split >= 0 && k >= 1, "bad argument");
    MF_REQUIRE(n == 0 || (u && i && block_out && substep_out && group_out && pos_out), "null argument");
    SideLayout U, I;
    const Blocking bl = blocking == MF_BLOCKING_BALANCED ? Blocking::kBalanced : Blocking::kJvm;
    build_side(U, u, n, n_blocks, seed, true, bl);
    build_side(I, i, n, n_blocks, seed, true, bl);
    std::vector<double> r(n, 1.0);
    RatingBlocks rb;
    build_rating_blocks(rb, U, I, u, i, r.data(), n, 0, n_blocks, false, true);
    FastPlan fp;
    std::vector<int64_t> src;
    std::vector<int32_t> block_groups;  // groups < 0: the systolic per-block choice for -groups waves
    if (groups < 0)
      block_groups = choose_block_groups(rb, I, n_blocks, 0, -groups, item_split, sys_cell_ns(k), sys_run_pair_ns(k));
    const uint32_t scratch_base = static_cast<uint32_t>(I.rows() + 1);
    build_fast_plan(fp, rb, U, I, groups > 0 ? groups : 8, 1, 1.0,
                    static_cast<uint64_t>(seed) * 0x9E3779B97F4A7C15ULL + 1, static_cast<uint32_t>(U.rows()), &src,
                    window > 0 ? window : kHazardWindow, block_groups.empty() ? nullptr : &block_groups, item_split,
                    scratch_base);
    const int64_t nb2 = static_cast<int64_t>(n_blocks) * n_blocks;
    for (int64_t b = 0; b < nb2; ++b) {
      if (fp.rec_base[b] < 0) continue;
      const int32_t G = fp.Gb[b];
      const int64_t GG = static_cast<int64_t>(G) * G;
      const int32_t* off = fp.cell_off.data() + fp.cell_base[b];
      for (int64_t cidx = 0; cidx < GG; ++cidx)
        for (int64_t x = off[cidx]; x < off[cidx + 1]; ++x) {
          if (src[fp.rec_base[b] + x] < 0) continue;  // padding
          const int64_t j = rb.src[src[fp.rec_base[b] + x]];
          block_out[j] = static_cast<int32_t>(b);
          substep_out[j] = static_cast<int32_t>(cidx / G);
          group_out[j] = static_cast<int32_t>(cidx % G);
          pos_out[j] = x - off[cidx];
          if (replica_out) {  // 0: the item's own row; r: its replica r (scratch row)
            const uint32_t row = fp.recs[fp.rec_base[b] + x].i & ~kPadBit;
            int32_t rep = 0;
            if (row >= scratch_base)
              for (int64_t h = fp.split_off[b]; h < fp.split_off[b + 1]; ++h)
                if (row >= fp.splits[h].scratch_row && row < fp.splits[h].scratch_row + fp.splits[h].R - 1)
                  rep = static_cast<int32_t>(row - fp.splits[h].scratch_row) + 1;
            replica_out[j] = rep;
          }
        }
    }
  });
}

void plan_digest(mf_ctx* ctx, uint64_t out[2]) {
  MF_REQUIRE(ctx->prepared && !ctx->f64 && ctx->fast_pair && ctx->shards.size() == 1,
             "mf_debug_plan_digest needs a prepared fast-mode pair fit on one shard");
  sync_all(ctx);
  Shard& s = ctx->shards[0];
  DeviceGuard g(s.device);
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const DevBuf& d, size_t bytes) {
    std::vector<unsigned char> v(bytes);
    if (bytes) MF_HIP(hipMemcpy(v.data(), d.get(), bytes, hipMemcpyDeviceToHost));
    for (unsigned char c : v) { h ^= c; h *= 1099511628211ull; }
  };
  mix(s.st_recs, static_cast<size_t>(s.st_nrecs) * sizeof(PairRec));
  mix(s.st_waves, s.st_sub_off.empty() ? 0 : static_cast<size_t>(s.st_sub_off.back()) * sizeof(WaveDesc));
  if (ctx->fast_sys) {
    mix(s.st_sys, s.st_sys.bytes());
    mix(s.st_sysw, s.st_sysw.bytes());
  }
  out[0] = h;
  out[1] = static_cast<uint64_t>(s.st_nrecs);
}

}  // namespace mfhip
