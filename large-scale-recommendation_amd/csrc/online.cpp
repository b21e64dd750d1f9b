// online.cpp -- online micro-batches (mf_online_update / mf_online_update_out, and
// mf_online_update_sampled, which follows every event with sampled negatives), mf_block_update,
// which runs one rating block through the same device plan, and mf_set_factors.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "common.hpp"
#include "context.hpp"
#include "jvm_random.hpp"
#include "kernels.hpp"
#include "neg_sample.hpp"
#include "plan.hpp"

namespace mfhip {

// ---------------------------------------------------------------------------------------
// Online micro-batches (single shard).
// Brings the device mirror d up to the host table ix: the whole table after a rehash / clear / a
// table of its own (generation changed), else only the slots written since the last sync.
void sync_dev_index(Shard& s, const IdIndex& ix, DevIndex& d) {
  const uint64_t cap = ix.capacity();
  const auto& log = ix.log();
  if (cap == 0) {
    d.gen = ix.gen();
    d.cap = 0;
    d.applied = log.size();
    return;
  }
  if (d.gen != ix.gen() || d.cap != cap) {
    d.slots.alloc(cap * sizeof(IdIndex::Slot));
    MF_HIP(hipMemcpyAsync(d.slots.get(), ix.slots(), cap * sizeof(IdIndex::Slot), hipMemcpyHostToDevice, s.stream));
    MF_HIP(hipStreamSynchronize(s.stream));  // pageable source
    d.gen = ix.gen();
    d.cap = cap;
    d.applied = log.size();
    return;
  }
  const size_t m = log.size() - d.applied;
  if (m == 0) return;
  std::vector<uint32_t> pos(log.begin() + static_cast<std::ptrdiff_t>(d.applied), log.end());
  std::vector<IdIndex::Slot> val(m);
  for (size_t j = 0; j < m; ++j) val[j] = ix.slots()[pos[j]];
  d.upd_pos.alloc(m * 4);
  d.upd_val.alloc(m * sizeof(IdIndex::Slot));
  MF_HIP(hipMemcpyAsync(d.upd_pos.get(), pos.data(), m * 4, hipMemcpyHostToDevice, s.stream));
  MF_HIP(hipMemcpyAsync(d.upd_val.get(), val.data(), m * sizeof(IdIndex::Slot), hipMemcpyHostToDevice, s.stream));
  launch_id_scatter(s.stream, d.slots.get(), d.upd_pos.as<uint32_t>(), d.upd_val.get(), static_cast<int64_t>(m));
  MF_HIP(hipStreamSynchronize(s.stream));  // pos / val are released on return
  d.applied = log.size();
}

namespace {

// The sweep's device plan leaves the batch's entries and, behind them, each entry's ticket value in
// det_dev.
uint32_t* plan_tickets(Shard& s, int64_t n) {
  return reinterpret_cast<uint32_t*>(s.det_dev.as<char>() + static_cast<size_t>(n) * sizeof(DetEntry));
}

// Queues the sweep's device plan (online_sweep_plan, kernels_online.hip) of the n updates in sc.in
// (user rows, item rows, ratings -- floats when rf32) over W waves; returns the number of leading
// single-item waves.
uint32_t queue_sweep_plan(Shard& s, int64_t n, int64_t W, int64_t user_rows, int64_t item_rows, bool rf32) {
  OnlineSweepScratch& sc = s.online_sc;
  const size_t ebytes = static_cast<size_t>(n) * sizeof(DetEntry), qbytes = static_cast<size_t>(n) * 4;
  s.det_dev.alloc(ebytes + qbytes);
  sc.wbeg.alloc(static_cast<size_t>(W + 1) * 8);
  sc.touched.alloc(8);
  const uint32_t* du = sc.in.as<uint32_t>();
  return online_sweep_plan(s.stream, sc, du, du + n, reinterpret_cast<const double*>(du + 2 * n), n,
                           static_cast<uint32_t>(W), static_cast<uint32_t>(user_rows), static_cast<uint32_t>(item_rows),
                           s.det_dev.as<DetEntry>(), plan_tickets(s, n), sc.wbeg.as<int64_t>(), sc.touched.as<int32_t>(),
                           rf32 ? reinterpret_cast<const float*>(du + 2 * n) : nullptr);
}

// The deterministic split sweep's input from a queued plan, in two halves around a stream sync.
// queue_det_entries: the sweep's entry arrays and wave table; the table (W descriptors) is read back
// into `host` (room for det_slot_room(W)), valid after the next sync of s.stream.
// finish_det_slots: det_slot_table pairs each single-item wave with its helper and gives the longest
// chains a CU each, in place in `host`; the slots go back up.  Returns the slot count.
struct DetEntries {
  uint32_t *eu = nullptr, *ei = nullptr, *eq = nullptr;
  double* er = nullptr;
};
void queue_det_entries(Shard& s, int64_t n, int64_t W, DetEntries& e, DetWave* host) {
  OnlineSweepScratch& sc = s.online_sc;
  sc.waves.alloc(static_cast<size_t>(det_slot_room(W)) * sizeof(DetWave));
  online_det_entries(s.stream, sc, s.det_dev.as<DetEntry>(), plan_tickets(s, n), sc.wbeg.as<int64_t>(), n,
                     static_cast<uint32_t>(W), e.eu, e.ei, e.eq, e.er, sc.waves.as<DetWave>());
  MF_HIP(hipMemcpyAsync(host, sc.waves.get(), static_cast<size_t>(W) * sizeof(DetWave), hipMemcpyDeviceToHost,
                        s.stream));
}
int64_t finish_det_slots(Shard& s, DetWave* host, int64_t W, int cap) {
  const int64_t nslots = det_slot_table(host, W, cap / 2, test_knob("det_alone") != "0", device_cu_count(s.device));
  MF_HIP(hipMemcpyAsync(s.online_sc.waves.get(), host, static_cast<size_t>(nslots) * sizeof(DetWave),
                        hipMemcpyHostToDevice, s.stream));
  return nslots;
}

// Clears the per-user tickets and the sweep's error word.
void reset_tickets(OnlineSweepScratch& sc, int64_t rows, hipStream_t stream) {
  const size_t ub = static_cast<size_t>(std::max<int64_t>(rows, 1)) * 4;
  sc.uticket.alloc(ub);
  MF_HIP(hipMemsetAsync(sc.uticket.get(), 0, ub, stream));
  sc.err.alloc(4);
  MF_HIP(hipMemsetAsync(sc.err.get(), 0, 4, stream));
}

// A ticket sweep set its error word: waves that gave up skipped the rest of their updates (and an
// online batch's new ids are already in the index), so the model is partly updated and the context
// refuses further work (as the DSGD sweeps do, sync_all) until a fit is prepared again.
[[noreturn]] void fail_ticket_timeout(mf_ctx* ctx, const char* path, const char* knob) {
  ctx->failed = std::string(path) + ": a wave waited > 1 s for a user ticket (waves not co-resident?); "
                "set MFHIP_TEST=" + knob + " (INTEGRATION.md section 5)";
  fail(MF_ERR_TIMEOUT, ctx->failed);
}

// One persistent launch (the default; MFHIP_TEST online_kernel=level forces the level-by-level
// replay, which is also the path with per-rating outputs): NFLX 1M-rating batches 1.1e8 vs
// 0.5e8 ratings/s end to end.
enum class OnlinePath {
  kF32Sweep,     // k_online_f32: f32 at k <= 256
  kDetSweep,     // the deterministic split sweep with nextFactors' update: f64 at k = 64 / 128 / 256
  kTicketSweep,  // k_online_sweep: any k, size_t addressing
  kLevels,       // one launch per dependency level
};


// One online batch on its way through online_update's stages: the caller's arrays, the kernel
// chosen for it, the upload's layout, the factor rows of its ratings and what is queued on the
// shard's stream so far.
// A batch has n_in events (the caller's arrays: what is staged, looked up and given new rows) and n
// updates (what is planned, swept and counted).  They differ only for a sampled batch (neg.negatives
// > 0, n = n_in * (1 + negatives)): its expansion -- on the device behind the id lookup, else on
// the host (expand_host) -- turns the events' rows into the updates, and from there it is an ordinary
// batch of n.
struct OnlineBatch {
  mf_ctx* ctx;
  Shard& s;
  const int32_t* u;
  const int32_t* i;
  const double* r;
  int64_t n_in, n;
  int flavour, num_partitions;
  int64_t *tu, *ti;
  double *uout, *iout;
  NegSampling neg;
  int k = ctx->P.num_factors;
  int64_t u0 = ctx->U.rows(), i0 = ctx->I.rows();  // rows before this batch
  PhaseClock clk;
  OnlinePath path = OnlinePath::kLevels;
  int cap = 0;    // wave slots of the sweep's kernel
  int64_t W = 1;  // waves of the sweep
  // the sweep in arrival order takes the rows straight into its pinned upload buffer (user rows,
  // item rows, ratings: 16 B per rating), with no staging pass; otherwise they go to on_ur / on_ir
  bool direct = false;
  // the direct path looks the ids up on the device (a mirror of each side's IdIndex, kept in step
  // by sync_dev_index): the host only copies the batch into the pinned upload, and resolves misses
  // (ids first seen in this batch) itself, in rating order, when there are any.  MFHIP_TEST
  // online_lookup=host keeps the host lookup (the tests compare the two bit for bit).
  bool dev_lookup = false;
  // the f32 sweep's upload carries the ratings as floats (12 B per rating instead of 16): the
  // sweep rounds each rating to float first in any case (online_f32.hpp), so the bits are the same
  bool rf32 = false;
  size_t in_bytes = 0;
  uint32_t *ur = nullptr, *ir = nullptr;  // factor rows per rating (kRowMiss: not known yet)
  int64_t misses = 0;
  std::vector<int32_t> fu, fi;  // ids first seen in this batch, in order of appearance
  int32_t* pin4 = nullptr;      // pinned: {lookup misses, sweep error, touched users, touched items}
  // queued on the stream: the batch in sc.in; its device plan (on the device-lookup path right
  // behind the lookup, before the host waits for the miss count, so the host's ~100 plan launches
  // overlap the upload's DMA; misses void it and it runs again after the host has given them rows);
  // the f64 sweep's entries and wave table from that plan
  bool uploaded = false, planned = false, det_queued = false;
  uint32_t nsingle = 0;  // waves [0, nsingle) hold one item each: k_online_f32's lean single-item path
  DetEntries det;

  std::vector<uint32_t> xu, xi;  // a sampled batch expanded for the level replay: rows and ratings
  std::vector<double> xr;

  bool outs() const { return uout || iout; }
  bool sweeps() const { return path != OnlinePath::kLevels; }
  bool sampled() const { return neg.negatives > 0; }
  // the expansion runs on the device, behind the lookup that found the events' rows there
  bool dev_expand() const { return sampled() && dev_lookup; }
  size_t event_bytes() const { return static_cast<size_t>(n_in) * (rf32 ? 12 : 16); }
  // the events' ratings [lo, hi) into the upload's rating array
  void stage_ratings(void* dst, int64_t lo, int64_t hi) const {
    if (rf32) {
      float* f = static_cast<float*>(dst);
      for (int64_t x = lo; x < hi; ++x) f[x] = static_cast<float>(r[x]);
    } else {
      std::memcpy(static_cast<double*>(dst) + lo, r + lo, static_cast<size_t>(hi - lo) * 8);
    }
  }
  void plan() {
    nsingle = queue_sweep_plan(s, n, W, ctx->U.rows(), ctx->I.rows(), rf32);
    planned = true;
  }
};

// The kernel for the batch, its wave count, and with them the upload's layout.
// f64 at k = 64 / 128 / 256: the deterministic sweep's kernel with nextFactors' update (split
// hot-item chains, kernels_detsweep.hip), while every row offset fits its 32-bit buffer offsets
// (rows after this batch's new ids at most rows + n); MFHIP_TEST online_kernel=ticket keeps
// k_online_sweep
// f32 at k <= 256: k_online_f32, whose row offsets are 32-bit as well (u * k * 4 bytes); a slab
// that would pass 4 GiB with this batch's new rows takes k_online_sweep (size_t addressing).
// MFHIP_TEST offset_limit=<bytes> lowers the limit so the tests reach that fallback.
void choose_online_path(OnlineBatch& b) {
  mf_ctx* ctx = b.ctx;
  const int k = b.k;
  if (b.n > 0 && !b.outs() && test_knob("online_kernel") != "level") {
    DeviceGuard g(b.s.device);
    double limit = kSlabLimit;  // raw_rsrc's clamp
    if (const std::string v = test_knob("offset_limit"); !v.empty()) limit = std::stod(v);
    const auto fits = [&](int64_t rows, int eb) { return static_cast<double>(rows + b.n) * k * eb <= limit; };
    const bool det_online = ctx->f64 && test_knob("online_kernel") != "ticket" && online_det_capacity(k) > 0 &&
                            fits(ctx->U.rows(), 8) && fits(ctx->I.rows(), 8);
    const bool f32_online = !ctx->f64 && online_f32_supports(k) && fits(ctx->U.rows(), 4) && fits(ctx->I.rows(), 4);
    // 0 (occupancy query failed): the level replay
    b.cap = det_online ? online_det_capacity(k)
            : f32_online ? online_f32_capacity(k) : online_sweep_capacity(k, ctx->f64);
    if (b.cap > 0)
      b.path = det_online ? OnlinePath::kDetSweep : f32_online ? OnlinePath::kF32Sweep : OnlinePath::kTicketSweep;
  }
  if (b.sweeps()) {
    int64_t wmax = 4096;
    if (const char* v = exp_knob("MFHIP_ONLINE_WAVES")) wmax = std::max(1, std::atoi(v));
    // MFHIP_TEST online_waves=<W>: at most W waves, so that a small batch puts many items and many
    // updates on each wave (tests/test_gpu_online_ranks.py)
    if (const std::string v = test_knob("online_waves"); !v.empty())
      wmax = std::min<int64_t>(wmax, std::max(1, std::atoi(v.c_str())));
    b.W = std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(b.cap / 2), wmax, b.n}));
  }
  b.direct = b.sweeps() && b.flavour != MF_ONLINE_SPARK_SWEEP;
  b.dev_lookup = b.direct && test_knob("online_lookup") != "host";
  b.rf32 = b.path == OnlinePath::kF32Sweep;
  b.in_bytes = static_cast<size_t>(b.n) * (b.rf32 ? 12 : 16);
}

// Where the batch's factor rows go: the pinned upload buffer (direct) or the context's row arrays.
void open_row_arrays(OnlineBatch& b) {
  mf_ctx* ctx = b.ctx;
  Shard& s = b.s;
  const int64_t n = b.n_in;
  // (a sampled batch expanded on the host keeps its events' rows in the context's arrays: the pinned
  // upload takes the expanded batch, expand_host)
  if (b.direct && (!b.sampled() || b.dev_lookup)) {
    DeviceGuard g(s.device);
    MF_HIP(hipStreamSynchronize(s.stream));  // det_pin may still feed an earlier copy
    s.det_pin.alloc(static_cast<size_t>(n) * 16);
    b.ur = s.det_pin.as<uint32_t>();
    b.ir = b.ur + n;
  } else {
    if (static_cast<int64_t>(ctx->on_ur.size()) < n) {
      ctx->on_ur.resize(n);
      ctx->on_ir.resize(n);
    }
    b.ur = ctx->on_ur.data();
    b.ir = ctx->on_ir.data();
  }
  s.small_pin.alloc(16);
  b.pin4 = s.small_pin.as<int32_t>();
}

// The f32 sweep of the planned batch, queued with its error word and touched counts read back into
// pinned memory (pin4[1..3]); skip: the lookup's miss count (the launch does nothing when non-zero)
void queue_f32_sweep(OnlineBatch& b, const int32_t* skip) {
  mf_ctx* ctx = b.ctx;
  Shard& s = b.s;
  OnlineSweepScratch& sc = s.online_sc;
  reset_tickets(sc, ctx->U.rows(), s.stream);
  sc.dummy.alloc(static_cast<size_t>(b.W) * 64);
  {
    LaunchTimer t(s, ctx->profiling, true);
    launch_online_f32(s.stream, static_cast<int>(b.W), sc.wbeg.as<int64_t>(), s.det_dev.as<DetEntry>(),
                      plan_tickets(s, b.n), s.uf.as<float>(), s.itf.as<float>(), s.uf.bytes(), s.itf.bytes(), b.k,
                      ctx->P.online_learning_rate, sc.uticket.as<int32_t>(), sc.dummy.as<int32_t>(),
                      sc.err.as<int32_t>(), test_knob("online_single") == "0" ? 0 : static_cast<int>(b.nsingle), skip,
                      t.start(), t.stop());
  }
  MF_HIP(hipGetLastError());
  MF_HIP(hipMemcpyAsync(b.pin4 + 1, sc.err.get(), 4, hipMemcpyDeviceToHost, s.stream));
  MF_HIP(hipMemcpyAsync(b.pin4 + 2, sc.touched.get(), 8, hipMemcpyDeviceToHost, s.stream));
}

// The f64 split sweep's entries from the queued plan; the wave table comes back to the host
// (pinned) for det_slot_table, read after the next stream sync.
void queue_online_det_entries(OnlineBatch& b) {
  b.s.slots_pin.alloc(static_cast<size_t>(det_slot_room(b.W)) * sizeof(DetWave));
  queue_det_entries(b.s, b.n, b.W, b.det, b.s.slots_pin.as<DetWave>());
  b.det_queued = true;
}

// The sweep has run (the stream is synced): its error word, the touched-row counts the plan
// counted on the device, the stats.
void finish_sweep(OnlineBatch& b) {
  b.clk.lap("online: sweep (device)");
  if (b.pin4[1]) fail_ticket_timeout(b.ctx, "online sweep", "online_kernel=level");
  if (b.tu) *b.tu = b.pin4[2];
  if (b.ti) *b.ti = b.pin4[3];
  b.ctx->stats.kernel_launches += 1;
  b.ctx->stats.updates += b.n;
}

// A sampled batch's events in sc.pos (rows as the lookup left them, or as the host has completed them)
// into the n updates in sc.in, with the model's item rows as they stand now as the pool; skip: the
// lookup's miss count, as queue_f32_sweep takes it.
void queue_expansion(OnlineBatch& b, const int32_t* skip) {
  OnlineSweepScratch& sc = b.s.online_sc;
  launch_neg_expand(b.s.stream, sc.pos.as<uint32_t>(), b.n_in, b.neg.negatives, static_cast<uint32_t>(b.ctx->I.rows()),
                    b.neg.seed, b.neg.first_event, b.neg.rating, b.rf32, sc.in.as<uint32_t>(), skip);
}

// The direct path with the device lookup: the ids go up as they are, the device replaces them by
// their rows and counts the misses; the plan and -- f32 -- the sweep, or -- f64 -- the sweep's
// entries, are queued behind the lookup, and one sync brings back the miss count with whatever
// they read back.  A sampled batch's events go to sc.pos instead, and its expansion into sc.in is
// queued between the lookup and the plan.  True when the batch is done (f32, no new id).
bool stage_and_lookup_device(OnlineBatch& b) {
  mf_ctx* ctx = b.ctx;
  Shard& s = b.s;
  const int64_t n = b.n_in;
  uint32_t *ur = b.ur, *ir = b.ir;
  DeviceGuard g(s.device);
  OnlineSweepScratch& sc = s.online_sc;
  sync_dev_index(s, ctx->U.index, s.didx[0]);
  sync_dev_index(s, ctx->I.index, s.didx[1]);
  sc.in.alloc(b.in_bytes);
  DevBuf& up = b.sampled() ? sc.pos : sc.in;
  up.alloc(b.event_bytes());
  // (staging in pieces with each piece's upload queued behind it was slower: 2-3 ms against ~1 ms
  // per NFLX batch, gpurun_out/r6d)
  parallel_for(n, [&](int64_t lo2, int64_t hi2, int) {
    const size_t c = static_cast<size_t>(hi2 - lo2);
    std::memcpy(ur + lo2, b.u + lo2, c * 4);
    std::memcpy(ir + lo2, b.i + lo2, c * 4);
    b.stage_ratings(ir + n, lo2, hi2);
  });
  MF_HIP(hipMemcpyAsync(up.get(), ur, b.event_bytes(), hipMemcpyHostToDevice, s.stream));
  b.clk.lap("online: staging + upload");
  sc.miss.alloc(4);
  MF_HIP(hipMemsetAsync(sc.miss.get(), 0, 4, s.stream));
  const DevIndex &du = s.didx[0], &di = s.didx[1];
  launch_id_lookup(s.stream, up.as<uint32_t>(), n, du.cap ? du.slots.get() : nullptr, du.cap - 1,
                   di.cap ? di.slots.get() : nullptr, di.cap - 1, sc.miss.as<int32_t>());
  MF_HIP(hipMemcpyAsync(b.pin4, sc.miss.get(), 4, hipMemcpyDeviceToHost, s.stream));
  if (b.sampled()) queue_expansion(b, sc.miss.as<int32_t>());  // (void with the plan when there are misses)
  b.plan();  // (the plan's kernels skip rows past the tables: the misses)
  // f32: the sweep goes right behind the plan, so the batch runs through without the host in the
  // loop; a batch with misses skips it on the device and takes the host's path
  const bool queued = b.path == OnlinePath::kF32Sweep;
  if (queued) {
    ensure_rows(ctx, s, kSideU, std::max<int64_t>(ctx->U.rows(), 1));
    ensure_rows(ctx, s, MF_SIDE_ITEM, std::max<int64_t>(ctx->I.rows(), 1));
    queue_f32_sweep(b, sc.miss.as<int32_t>());
  } else if (b.path == OnlinePath::kDetSweep) {
    queue_online_det_entries(b);  // (void with the plan when there are misses)
  }
  b.clk.lap("online: lookup + plan queued");
  MF_HIP(hipStreamSynchronize(s.stream));
  const int32_t m = b.pin4[0];
  b.misses = m;
  if (queued && m == 0) {
    finish_sweep(b);
    return true;
  }
  if (m > 0) {  // the rows as found (kRowMiss where absent) back into the pinned buffer
    b.planned = b.det_queued = false;
    MF_HIP(hipMemcpyAsync(ur, up.get(), static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, s.stream));
    MF_HIP(hipStreamSynchronize(s.stream));
  }
  b.uploaded = m == 0;
  return false;
}

// Rows of known ids in parallel (the index is only read; kRowMiss marks the others).
void lookup_host(OnlineBatch& b) {
  mf_ctx* ctx = b.ctx;
  const int64_t n = b.n_in;
  uint32_t *ur = b.ur, *ir = b.ir;
  std::atomic<int64_t> misses{0};
  parallel_for(n, [&](int64_t lo2, int64_t hi2, int) {
    ctx->U.index.find_many(b.u + lo2, hi2 - lo2, ur + lo2);
    ctx->I.index.find_many(b.i + lo2, hi2 - lo2, ir + lo2);
    if (b.direct && !b.sampled()) b.stage_ratings(ir + n, lo2, hi2);
    int64_t m = 0;
    for (int64_t j = lo2; j < hi2; ++j) m += (ur[j] == kRowMiss) + (ir[j] == kRowMiss);
    misses += m;
  });
  b.misses = misses;
}

// In rating order, the ids first seen in this batch get new rows in order of appearance, exactly
// as one sequential scan would.
void assign_new_rows(OnlineBatch& b) {
  mf_ctx* ctx = b.ctx;
  if (b.misses > 0)
    for (int64_t j = 0; j < b.n_in; ++j) {
      if (b.ur[j] == kRowMiss) b.ur[j] = static_cast<uint32_t>(online_row(ctx, ctx->U, b.u[j], b.fu));
      if (b.ir[j] == kRowMiss) b.ir[j] = static_cast<uint32_t>(online_row(ctx, ctx->I, b.i[j], b.fi));
    }
  b.clk.lap("online: id lookup");
}

// A sampled batch off the device-lookup path (MFHIP_TEST online_lookup=host, the level replay): the
// events' final rows into the n updates, the draws of k_neg_expand (neg_sample.hpp) -- into the pinned
// upload for a sweep, into the batch's own arrays for the levels.  From here b.ur / b.ir / b.r are the
// updates'.
void expand_host(OnlineBatch& b) {
  Shard& s = b.s;
  const int64_t N = b.n, per = 1 + b.neg.negatives;
  const uint32_t pool = static_cast<uint32_t>(b.ctx->I.rows());
  uint32_t *pu, *pi;
  double* pr = nullptr;
  float* prf = nullptr;
  if (b.direct) {
    DeviceGuard g(s.device);
    MF_HIP(hipStreamSynchronize(s.stream));  // det_pin may still feed an earlier copy
    s.det_pin.alloc(b.in_bytes);
    pu = s.det_pin.as<uint32_t>();
    pi = pu + N;
    if (b.rf32) prf = reinterpret_cast<float*>(pi + N);
    else pr = reinterpret_cast<double*>(pi + N);
  } else {
    b.xu.resize(N);
    b.xi.resize(N);
    b.xr.resize(N);
    pu = b.xu.data();
    pi = b.xi.data();
    pr = b.xr.data();
  }
  const uint32_t *eu = b.ur, *ei = b.ir;
  const double* er = b.r;
  const uint64_t seed = static_cast<uint64_t>(b.neg.seed), t0 = static_cast<uint64_t>(b.neg.first_event);
  parallel_for(N, [&](int64_t lo2, int64_t hi2, int) {
    for (int64_t x = lo2; x < hi2; ++x) {
      const int64_t j = x / per, sx = x - j * per;
      pu[x] = eu[j];
      pi[x] = sx == 0 ? ei[j] : neg_row(seed, t0 + static_cast<uint64_t>(j), static_cast<uint32_t>(sx - 1), pool, ei[j]);
      const double rv = sx == 0 ? er[j] : b.neg.rating;
      if (prf) prf[x] = static_cast<float>(rv);
      else pr[x] = rv;
    }
  });
  b.ur = pu;
  b.ir = pi;
  if (!b.direct) b.r = pr;
  b.clk.lap("online: negatives (host)");
}

// Touched-row counts (UpdateSeparatedHashMap.updates, OfflineSpark.scala:33-67) on the host; the
// sweeps' plan counts them on the device.
void count_touched_host(OnlineBatch& b) {
  mf_ctx* ctx = b.ctx;
  const uint32_t *ur = b.ur, *ir = b.ir;
  std::vector<uint8_t> seen_u, seen_i;
  seen_u.assign(ctx->U.rows(), 0);
  seen_i.assign(ctx->I.rows(), 0);
  // flags set with plain relaxed stores, and only when still clear (a locked exchange per rating
  // kept the flag lines bouncing between cores: 8 ms per 1M ratings), then counted
  parallel_for(b.n, [&](int64_t lo2, int64_t hi2, int) {
    for (int64_t j = lo2; j < hi2; ++j) {
      if (!__atomic_load_n(&seen_u[ur[j]], __ATOMIC_RELAXED)) __atomic_store_n(&seen_u[ur[j]], 1, __ATOMIC_RELAXED);
      if (!__atomic_load_n(&seen_i[ir[j]], __ATOMIC_RELAXED)) __atomic_store_n(&seen_i[ir[j]], 1, __ATOMIC_RELAXED);
    }
  });
  std::atomic<int64_t> acu{0}, aci{0};
  parallel_for(static_cast<int64_t>(std::max(seen_u.size(), seen_i.size())), [&](int64_t lo2, int64_t hi2, int) {
    int64_t lu = 0, li = 0;
    for (int64_t x = lo2; x < hi2; ++x) {
      if (x < static_cast<int64_t>(seen_u.size())) lu += seen_u[x];
      if (x < static_cast<int64_t>(seen_i.size())) li += seen_i[x];
    }
    acu += lu;
    aci += li;
  });
  if (b.tu) *b.tu = acu;
  if (b.ti) *b.ti = aci;
  b.clk.lap("online: touched rows");
}

// First-touch initialisation of the ids first seen in this batch.
void init_new_rows(OnlineBatch& b) {
  mf_ctx* ctx = b.ctx;
  // new rows take the slab rows the fast DSGD schedule keeps zeroed (padding / idle prefetch
  // rows past the real ones): that schedule is void now, a further fit must prepare again
  if (ctx->prepared && !ctx->f64 && (!b.fu.empty() || !b.fi.empty())) ctx->prepared = false;
  const bool xor_seed = ctx->P.online_init == MF_INIT_SEEDED;
  for (int side = 0; side < 2; ++side) {
    const std::vector<int32_t>& fresh = side == kSideU ? b.fu : b.fi;
    const int64_t row0 = side == kSideU ? b.u0 : b.i0;
    const SideLayout& S = side_of(ctx, side);
    ensure_rows(ctx, b.s, side, std::max<int64_t>(S.rows(), 1));
    if (fresh.empty()) continue;
    std::vector<double> vec;
    init_vectors(fresh.data(), static_cast<int64_t>(fresh.size()), b.k, xor_seed, ctx->P.seed, vec);
    upload_rows(ctx, b.s, side, row0, vec.data(), static_cast<int64_t>(fresh.size()));
  }
}

// The sequential order of the flavour: arrival order, or the Spark sweep's.
void spark_sweep_order(const OnlineBatch& b, std::vector<int32_t>& order) {
  const int64_t n = b.n;
  order.resize(n);
  std::iota(order.begin(), order.end(), 0);
  if (b.flavour != MF_ONLINE_SPARK_SWEEP) return;
  // OfflineSpark.scala:135-147,163-203: user partition id % P, item rating block abs(i) % P;
  // sub-epoch s (1-based) pairs partition p with item block (p - (s-1)) mod P; each cell in
  // insertion order.  One iteration per micro-batch (OnlineSpark.scala:191-194).
  MF_REQUIRE(b.num_partitions >= 1, "num_partitions must be >= 1 for MF_ONLINE_SPARK_SWEEP");
  const int P = b.num_partitions;
  std::vector<std::vector<int32_t>> cells(static_cast<size_t>(P) * P);
  for (int64_t j = 0; j < n; ++j) {
    MF_REQUIRE(b.u[j] >= 0 && b.i[j] != INT32_MIN, "Spark sweep needs non-negative user ids");
    const int up = b.u[j] % P, ib = std::abs(b.i[j]) % P;
    cells[static_cast<size_t>(up) * P + ib].push_back(static_cast<int32_t>(j));
  }
  order.clear();
  for (int sub = 1; sub <= P; ++sub)
    for (int p = 0; p < P; ++p) {
      const int q = ((p - (sub - 1)) % P + P) % P;
      const auto& c = cells[static_cast<size_t>(p) * P + q];
      order.insert(order.end(), c.begin(), c.end());
    }
}

// The batch in the Spark-sweep order into the pinned upload buffer.
void stage_in_order(OnlineBatch& b, const std::vector<int32_t>& order) {
  Shard& s = b.s;
  const int64_t n = b.n;
  MF_HIP(hipStreamSynchronize(s.stream));  // det_pin may still feed an earlier copy
  s.det_pin.alloc(b.in_bytes);
  uint32_t* pu = s.det_pin.as<uint32_t>();
  uint32_t* pi = pu + n;
  double* pr = reinterpret_cast<double*>(pi + n);
  float* prf = reinterpret_cast<float*>(pi + n);
  parallel_for(n, [&](int64_t lo2, int64_t hi2, int) {
    for (int64_t x = lo2; x < hi2; ++x) {
      const int32_t j = order[x];
      pu[x] = b.ur[j];
      pi[x] = b.ir[j];
      if (b.rf32) prf[x] = static_cast<float>(b.r[j]);
      else pr[x] = b.r[j];
    }
  });
  b.clk.lap("online: sweep staging");
}

// One persistent launch: items spread over the waves, each wave's updates in sequence order, and
// per update the number of earlier updates of its user (its ticket value).  The batch in sequence
// order goes up as is (16 bytes an update); the per-wave lists and the tickets are built on the
// device (online_sweep_plan, kernels_online.hip).
void run_sweep(OnlineBatch& b, const std::vector<int32_t>& order) {
  mf_ctx* ctx = b.ctx;
  Shard& s = b.s;
  DeviceGuard g(s.device);
  OnlineSweepScratch& sc = s.online_sc;
  if (!b.direct) stage_in_order(b, order);
  if (!b.uploaded && b.dev_expand()) {
    // the events' rows, now complete, beside their ratings in sc.pos; expanded again with the final pool
    MF_HIP(hipMemcpyAsync(sc.pos.get(), s.det_pin.as<uint32_t>(), static_cast<size_t>(b.n_in) * 8,
                          hipMemcpyHostToDevice, s.stream));
    queue_expansion(b, nullptr);
  } else if (!b.uploaded) {  // (the device lookup left the batch's rows in sc.in already)
    sc.in.alloc(b.in_bytes);
    MF_HIP(hipMemcpyAsync(sc.in.get(), s.det_pin.as<uint32_t>(), b.in_bytes, hipMemcpyHostToDevice, s.stream));
  }
  if (!b.planned) b.plan();
  if (b.path == OnlinePath::kF32Sweep) {
    queue_f32_sweep(b, nullptr);
  } else if (b.path == OnlinePath::kDetSweep) {
    reset_tickets(sc, ctx->U.rows(), s.stream);
    // the wave table goes through the host once (W descriptors; queued behind the device lookup on
    // that path, so that one sync brings back the miss count and the table)
    if (!b.det_queued) {
      queue_online_det_entries(b);
      MF_HIP(hipStreamSynchronize(s.stream));
    }
    const int64_t nslots = finish_det_slots(s, s.slots_pin.as<DetWave>(), b.W, b.cap);
    LaunchTimer t(s, ctx->profiling, true);
    launch_online_det(s.stream, sc.waves.as<DetWave>(), static_cast<int>(nslots), b.det.eu, b.det.ei, b.det.eq,
                      b.det.er, s.uf.as<double>(), s.itf.as<double>(), s.uf.bytes(), s.itf.bytes(), b.k,
                      ctx->P.online_learning_rate, sc.uticket.as<int32_t>(), sc.err.as<int32_t>(), t.start(),
                      t.stop());
  } else {
    reset_tickets(sc, ctx->U.rows(), s.stream);
    LaunchTimer t(s, ctx->profiling);
    launch_online_sweep(s.stream, static_cast<int>(b.W), sc.wbeg.as<int64_t>(), s.det_dev.as<DetEntry>(),
                        plan_tickets(s, b.n), s.uf.get(), s.itf.get(), b.k, ctx->P.online_learning_rate, ctx->f64,
                        sc.uticket.as<int32_t>(), sc.err.as<int32_t>());
  }
  MF_HIP(hipGetLastError());
  if (b.path != OnlinePath::kF32Sweep) {
    MF_HIP(hipMemcpyAsync(b.pin4 + 1, sc.err.get(), 4, hipMemcpyDeviceToHost, s.stream));
    MF_HIP(hipMemcpyAsync(b.pin4 + 2, sc.touched.get(), 8, hipMemcpyDeviceToHost, s.stream));
  }
  MF_HIP(hipStreamSynchronize(s.stream));
  finish_sweep(b);
}

// The level-by-level replay: one launch per dependency level (no two updates of a level share a
// row), with the per-rating output records when asked for.
void run_levels(OnlineBatch& b, const std::vector<int32_t>& order) {
  mf_ctx* ctx = b.ctx;
  Shard& s = b.s;
  const int64_t n = b.n;
  const int k = b.k;
  double *uout = b.uout, *iout = b.iout;
  const bool outs = b.outs();
  std::vector<double> rr(b.r, b.r + n);
  OrderedSeq sq;
  sq.u = b.ur;
  sq.i = b.ir;
  sq.r = rr.data();
  sq.order = order.data();
  sq.len = n;
  sq.u_lo = 0;
  sq.u_hi = static_cast<uint32_t>(ctx->U.rows());
  sq.i_lo = 0;
  sq.i_hi = static_cast<uint32_t>(ctx->I.rows());
  LevelPlan lp;
  std::vector<int32_t> src;
  b.clk.lap("online: new rows + order");
  build_level_plan({sq}, lp, outs ? &src : nullptr);
  b.clk.lap("online: level plan");
  DeviceGuard g(s.device);
  const size_t bytes = lp.entries.size() * sizeof(DetEntry);
  MF_HIP(hipStreamSynchronize(s.stream));
  s.det_pin.alloc(bytes);
  s.det_dev.alloc(bytes);
  std::memcpy(s.det_pin.as<void>(), lp.entries.data(), bytes);
  MF_HIP(hipMemcpyAsync(s.det_dev.get(), s.det_pin.as<void>(), bytes, hipMemcpyHostToDevice, s.stream));
  DevBuf dsrc, duo, dio;
  const size_t obytes = static_cast<size_t>(n) * k * sizeof(double);
  if (outs) {
    dsrc.alloc(src.size() * sizeof(int32_t));
    MF_HIP(hipMemcpyAsync(dsrc.get(), src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    if (uout) duo.alloc(obytes);
    if (iout) dio.alloc(obytes);
  }
  const OnlineOut om = b.flavour == MF_ONLINE_DELTA ? OnlineOut::kOutDelta : OnlineOut::kOutNext;
  for (int64_t l = 0; l < lp.levels(); ++l) {
    const int64_t b0 = lp.level_start[l], cnt = lp.level_start[l + 1] - b0;
    LaunchTimer t(s, ctx->profiling);
    if (outs)
      launch_level_out(s.stream, s.det_dev.as<DetEntry>() + b0, cnt, s.uf.get(), s.itf.get(), k,
                       ctx->P.online_learning_rate, ctx->f64, om, dsrc.as<int32_t>() + b0,
                       uout ? duo.as<double>() : nullptr, iout ? dio.as<double>() : nullptr);
    else
      launch_level(s.stream, s.det_dev.as<DetEntry>() + b0, cnt, s.uf.get(), s.itf.get(), s.regu.get(),
                   s.regi.get(), k, ctx->P.online_learning_rate, Arith::kSgdNext, ctx->f64);
  }
  MF_HIP(hipGetLastError());
  b.clk.lap("online: H2D + level launches queued");
  MF_HIP(hipStreamSynchronize(s.stream));
  b.clk.lap("online: kernels done");
  if (uout) MF_HIP(hipMemcpy(uout, duo.get(), obytes, hipMemcpyDeviceToHost));
  if (iout) MF_HIP(hipMemcpy(iout, dio.get(), obytes, hipMemcpyDeviceToHost));
  ctx->stats.levels += lp.levels();
  ctx->stats.kernel_launches += lp.levels();
  ctx->stats.updates += n;
}

void check_online_call(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour) {
  MF_REQUIRE(ctx->shards.size() == 1 && !ctx->rank_mode, "online updates run on a single-device context");
  MF_REQUIRE(flavour >= MF_ONLINE_NEXT_FACTORS && flavour <= MF_ONLINE_SPARK_SWEEP, "unknown online flavour");
  MF_REQUIRE(n >= 0 && (n == 0 || (u && i && r)), "bad rating arrays");
}

// The batch through its stages; neg.negatives > 0: every event followed by its sampled negatives.
void run_online_batch(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                      int num_partitions, int64_t* tu, int64_t* ti, double* uout, double* iout,
                      const NegSampling& neg) {
  if (!ctx->have_model) {
    ctx->U = SideLayout();
    ctx->I = SideLayout();
    ctx->have_model = true;
    ++ctx->layout_gen;
  }
  OnlineBatch b{ctx, ctx->shards[0], u, i, r, n, n * (1 + neg.negatives), flavour, num_partitions, tu, ti, uout, iout,
                neg};
  choose_online_path(b);
  open_row_arrays(b);
  if (b.dev_lookup) {
    if (stage_and_lookup_device(b)) return;
  } else {
    lookup_host(b);
  }
  assign_new_rows(b);
  if (b.sampled() && !b.dev_expand()) expand_host(b);
  if (!b.sweeps()) count_touched_host(b);
  init_new_rows(b);
  if (n == 0) return;
  std::vector<int32_t> order;  // the sequence, where it is not the arrival order of a direct upload
  if (!b.direct) spark_sweep_order(b, order);
  if (b.sweeps()) run_sweep(b, order);
  else run_levels(b, order);
}

// True when the model will hold a single item row once the batch's new ids have theirs: no row to
// draw a negative from.  Only a model of at most one item can end so, and then only when every event
// names the same item.
bool single_item_pool(const mf_ctx* ctx, const int32_t* i, int64_t n) {
  if (!ctx->have_model || ctx->I.rows() == 0) return std::all_of(i, i + n, [&](int32_t x) { return x == i[0]; });
  if (ctx->I.rows() > 1) return false;
  const int32_t only = ctx->I.row_id[0];
  return std::all_of(i, i + n, [&](int32_t x) { return x == only; });
}
}  // namespace

void online_update(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                   int num_partitions, int64_t* tu, int64_t* ti, double* uout, double* iout) {
  check_online_call(ctx, u, i, r, n, flavour);
  MF_REQUIRE(!(uout || iout) || flavour != MF_ONLINE_SPARK_SWEEP,
             "MF_ONLINE_SPARK_SWEEP emits touched rows only (OfflineSpark.scala:33-67): no per-rating outputs");
  require_healthy(ctx);
  run_online_batch(ctx, u, i, r, n, flavour, num_partitions, tu, ti, uout, iout, NegSampling{});
}

void check_negative_sampling(const NegSampling& neg) {
  MF_REQUIRE(neg.negatives >= 0 && neg.negatives <= kNegMax,
             "negatives must be in [0, " + std::to_string(kNegMax) + "]");
  MF_REQUIRE(std::isfinite(neg.rating), "negative_rating must be finite");
  MF_REQUIRE(neg.first_event >= 0, "first_event must not be negative");
}

void online_update_sampled(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                           const NegSampling& neg, int32_t* sampled_out, int64_t* tu, int64_t* ti) {
  check_negative_sampling(neg);
  check_online_call(ctx, u, i, r, n, flavour);
  MF_REQUIRE(flavour != MF_ONLINE_SPARK_SWEEP,
             "MF_ONLINE_SPARK_SWEEP has no sampled form: its sequence is not the arrival order");
  MF_REQUIRE(n < (int64_t{1} << 31) && n * (1 + neg.negatives) < (int64_t{1} << 31),
             "a sampled batch holds fewer than 2^31 updates");
  require_healthy(ctx);
  NegSampling use = neg;
  if (n == 0 || single_item_pool(ctx, i, n)) use.negatives = 0;  // nothing to draw (from): the plain batch
  run_online_batch(ctx, u, i, r, n, flavour, 0, tu, ti, nullptr, nullptr, use);
  if (!sampled_out || use.negatives == 0) return;
  // the drawn rows as ids: the events' rows again (the device path never brought them to the host)
  const SideLayout& I = ctx->I;
  const uint32_t pool = static_cast<uint32_t>(I.rows());
  const uint64_t seed = static_cast<uint64_t>(neg.seed), t0 = static_cast<uint64_t>(neg.first_event);
  const int64_t per = neg.negatives;
  parallel_for(n, [&](int64_t lo2, int64_t hi2, int) {
    std::vector<uint32_t> rows(static_cast<size_t>(hi2 - lo2));
    I.index.find_many(i + lo2, hi2 - lo2, rows.data());
    for (int64_t j = lo2; j < hi2; ++j)
      for (int64_t sx = 0; sx < per; ++sx)
        sampled_out[j * per + sx] =
            I.row_id[neg_row(seed, t0 + static_cast<uint64_t>(j), static_cast<uint32_t>(sx), pool, rows[j - lo2])];
  });
}

// mf_block_update: one rating block's updateLocalFactors (DSGDforMF.scala:378-418) on caller
// buffers, as a Flink-resident task would call it.  The block's shuffle (new Random(iteration ^
// ratingBlockId ^ seed), :392-393) runs on the host; the block then runs as ONE persistent launch of
// the deterministic split sweep (k_det_sweep_split, kernels_detsweep.hip) -- the superstep's kernel
// with a one-block superstep: every item's updates in shuffle order inside one wave (the hottest
// items as chain + helper pairs on CUs of their own), every user's through per-user tickets -- with
// its wave lists and tickets built on the device by the online plan (kernels_online.hip
// online_sweep_plan / online_det_entries: any item -> wave map gives the same factors).  Bitwise the
// sequential reference order (tests/test_gpu_dsgd.py test_block_update_*).  k outside 64 / 128 /
// 256, slabs past the 32-bit row offsets, or MFHIP_TEST det_kernel=level: one launch per dependency
// level (k_level), the same factors.
namespace {
void block_update_levels(Shard& s, const std::vector<int32_t>& order, const double* r, const int32_t* uidx,
                         const int32_t* iidx, int64_t len, DevBuf& du, DevBuf& di, DevBuf& dru, DevBuf& dri, int64_t nu,
                         int64_t ni, int k, double eta, int64_t& levels) {
  std::vector<uint32_t> uu(uidx, uidx + len), ii(iidx, iidx + len);
  OrderedSeq sq{uu.data(), ii.data(), r, order.data(), len, 0, static_cast<uint32_t>(nu), 0, static_cast<uint32_t>(ni)};
  LevelPlan lp;
  build_level_plan({sq}, lp);
  DevBuf de;
  de.alloc(lp.entries.size() * sizeof(DetEntry));
  MF_HIP(hipMemcpyAsync(de.get(), lp.entries.data(), lp.entries.size() * sizeof(DetEntry), hipMemcpyHostToDevice,
                        s.stream));
  for (int64_t l = 0; l < lp.levels(); ++l) {
    const int64_t b0 = lp.level_start[l], cnt = lp.level_start[l + 1] - b0;
    launch_level(s.stream, de.as<DetEntry>() + b0, cnt, du.get(), di.get(), dru.get(), dri.get(), k, eta, Arith::kDsgd,
                 true);
  }
  MF_HIP(hipGetLastError());
  MF_HIP(hipStreamSynchronize(s.stream));  // lp and de are released on return
  levels = lp.levels();
}
}  // namespace

void block_update(mf_ctx* ctx, const double* r, const int32_t* uidx, const int32_t* iidx, int64_t len, double* users,
                  const int32_t* uomega, int64_t nu, double* items, const int32_t* iomega, int64_t ni, int k,
                  int iteration, int rating_block_id, int64_t seed, double lr, int lr_method, double lr_arg,
                  double lambda) {
  MF_REQUIRE(len >= 0 && nu >= 0 && ni >= 0 && k >= 1 && k <= 512, "bad sizes");
  MF_REQUIRE(len == 0 || (r && uidx && iidx && users && items && uomega && iomega), "null argument");
  MF_REQUIRE(len < (int64_t{1} << 31), "a rating block holds fewer than 2^31 ratings");
  std::atomic<int64_t> bad{0};
  parallel_for(len, [&](int64_t b, int64_t e, int) {
    int64_t m = 0;
    for (int64_t j = b; j < e; ++j) m += !(uidx[j] >= 0 && uidx[j] < nu && iidx[j] >= 0 && iidx[j] < ni);
    bad += m;
  });
  MF_REQUIRE(bad == 0, "rating index out of block range");
  if (len == 0) return;
  require_healthy(ctx);
  Shard& s = ctx->shards[0];
  DeviceGuard g(s.device);
  PhaseClock clk;
  std::vector<int32_t> order(len);
  JavaRandom rng(static_cast<int64_t>(iteration ^ rating_block_id) ^ seed);  // DSGDforMF.scala:392
  scala_shuffle(rng, order.data(), len);
  clk.lap("block_update: shuffle");
  const double eta = learning_rate(lr_method, lr, iteration + 1, lambda, lr_arg);  // :383-386
  const size_t ub = static_cast<size_t>(nu) * k * 8, ib = static_cast<size_t>(ni) * k * 8;
  // the block's rows and reg vectors live in the shard's scratch across calls (grow-only)
  DevBuf &du = s.blk_u, &di = s.blk_i, &dru = s.blk_ru, &dri = s.blk_ri;
  du.alloc(std::max<size_t>(ub, 8));
  di.alloc(std::max<size_t>(ib, 8));
  dru.alloc(static_cast<size_t>(std::max<int64_t>(nu, 1)) * 8);
  dri.alloc(static_cast<size_t>(std::max<int64_t>(ni, 1)) * 8);
  {
    std::vector<double> ru(nu), ri(ni);
    for (int64_t x = 0; x < nu; ++x) ru[x] = lambda / static_cast<double>(uomega[x]);
    for (int64_t x = 0; x < ni; ++x) ri[x] = lambda / static_cast<double>(iomega[x]);
    MF_HIP(hipMemcpyAsync(du.get(), users, ub, hipMemcpyHostToDevice, s.stream));
    MF_HIP(hipMemcpyAsync(di.get(), items, ib, hipMemcpyHostToDevice, s.stream));
    MF_HIP(hipMemcpyAsync(dru.get(), ru.data(), static_cast<size_t>(nu) * 8, hipMemcpyHostToDevice, s.stream));
    MF_HIP(hipMemcpyAsync(dri.get(), ri.data(), static_cast<size_t>(ni) * 8, hipMemcpyHostToDevice, s.stream));
    MF_HIP(hipStreamSynchronize(s.stream));  // ru / ri are released here
  }
  const int cap = det_split_capacity(k);
  const bool sweep = cap >= 2 && test_knob("det_kernel") != "level" && ub < kSlabLimit && ib < kSlabLimit;
  int64_t levels = 0;
  if (!sweep) {
    block_update_levels(s, order, r, uidx, iidx, len, du, di, dru, dri, nu, ni, k, eta, levels);
  } else {
    // the block in shuffle order, as the online plan takes a batch: rows, rows, ratings (16 B each)
    const size_t in_bytes = static_cast<size_t>(len) * 16;
    MF_HIP(hipStreamSynchronize(s.stream));  // det_pin may still feed an earlier copy
    s.det_pin.alloc(in_bytes);
    uint32_t* pu = s.det_pin.as<uint32_t>();
    uint32_t* pi = pu + len;
    double* pr = reinterpret_cast<double*>(pi + len);
    parallel_for(len, [&](int64_t b, int64_t e, int) {
      for (int64_t x = b; x < e; ++x) {
        const int32_t j = order[x];
        pu[x] = static_cast<uint32_t>(uidx[j]);
        pi[x] = static_cast<uint32_t>(iidx[j]);
        pr[x] = r[j];
      }
    });
    clk.lap("block_update: gather");
    OnlineSweepScratch& sc = s.online_sc;
    sc.in.alloc(in_bytes);
    MF_HIP(hipMemcpyAsync(sc.in.get(), pu, in_bytes, hipMemcpyHostToDevice, s.stream));
    const int64_t W = std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(cap / 2), 4096, len}));
    queue_sweep_plan(s, len, W, nu, ni, false);
    DetEntries e;
    std::vector<DetWave> slots(static_cast<size_t>(det_slot_room(W)));
    queue_det_entries(s, len, W, e, slots.data());
    MF_HIP(hipStreamSynchronize(s.stream));
    const int64_t nslots = finish_det_slots(s, slots.data(), W, cap);
    reset_tickets(sc, nu, s.stream);
    {
      LaunchTimer t(s, ctx->profiling, true);
      launch_det_sweep_split(s.stream, sc.waves.as<DetWave>(), static_cast<int>(nslots), e.eu, e.ei, e.eq, e.er,
                             du.as<double>(), di.as<double>(), ub, ib, dru.as<double>(), dri.as<double>(), k, eta,
                             sc.uticket.as<int32_t>(), sc.err.as<int32_t>(), t.start(), t.stop());
    }
    MF_HIP(hipGetLastError());
    int32_t err = 0;
    MF_HIP(hipMemcpyAsync(&err, sc.err.get(), 4, hipMemcpyDeviceToHost, s.stream));
    MF_HIP(hipStreamSynchronize(s.stream));
    clk.lap("block_update: plan + sweep");
    if (err) fail_ticket_timeout(ctx, "block update sweep", "det_kernel=level");
    ctx->stats.kernel_launches += 1;
  }
  MF_HIP(hipMemcpyAsync(users, du.get(), ub, hipMemcpyDeviceToHost, s.stream));
  MF_HIP(hipMemcpyAsync(items, di.get(), ib, hipMemcpyDeviceToHost, s.stream));
  MF_HIP(hipStreamSynchronize(s.stream));
  clk.lap("block_update: download");
  ctx->stats.updates += len;
  ctx->stats.levels += levels;
}

// Rows of the given ids := vecs; unseen ids get rows as in an online batch (mf_set_factors).
void set_factors(mf_ctx* ctx, int side, const int32_t* ids, const double* vecs, int64_t n) {
  det_spec_wait(ctx, true);  // rows may be added: the layouts change
  if (!ctx->have_model) { ctx->U = SideLayout(); ctx->I = SideLayout(); ctx->have_model = true; ++ctx->layout_gen; }
  SideLayout& S = side_of(ctx, side);
  std::vector<int32_t> fresh;
  std::vector<int32_t> rows(n);
  for (int64_t j = 0; j < n; ++j) rows[j] = online_row(ctx, S, ids[j], fresh);
  const int k = ctx->P.num_factors;
  sync_all(ctx);
  for (auto& s : ctx->shards) {
    ensure_rows(ctx, s, side, std::max<int64_t>(S.rows(), 1));
    if (n < 64) {
      for (int64_t j = 0; j < n; ++j) upload_rows(ctx, s, side, rows[j], vecs + static_cast<size_t>(j) * k, 1);
      continue;
    }
    // many rows: patch a host copy of the slab and upload it once
    std::vector<double> all(static_cast<size_t>(S.rows()) * k);
    download_rows(ctx, s, side, 0, S.rows(), all.data());
    for (int64_t j = 0; j < n; ++j)
      std::memcpy(all.data() + static_cast<size_t>(rows[j]) * k, vecs + static_cast<size_t>(j) * k, k * sizeof(double));
    upload_rows(ctx, s, side, 0, all.data(), S.rows());
  }
}

}  // namespace mfhip
