// eval.cpp -- reading the model out: evaluation (mf_predict / mf_rmse / mf_empirical_risk),
// top-N lists (mf_recommend, mf_similar, mf_recommend_vectors, mf_recommend_among) and the factor read-outs
// (mf_get_factors, mf_lookup).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
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

// Rank mode: broadcast each item block from its holder so every rank has all items.
void allgather_items(mf_ctx* ctx) {
  if (!ctx->rank_mode || ctx->G <= 1) return;
  // The last superstep may still be running: with the ring overlap its second launch is on
  // `aux` and the item block's send/recv on `comm`.  The broadcast below reads and writes item
  // rows on `stream`, and two RCCL operations of one communicator must not run on unordered
  // streams, so every stream of the rank drains first (and a sweep timeout surfaces here).
  sync_all(ctx);
  require_healthy(ctx);
  Shard& s = ctx->shards[0];
  DeviceGuard g(s.device);
  const size_t k = static_cast<size_t>(ctx->P.num_factors);
  MF_NCCL(ncclGroupStart());
  for (int32_t b = 0; b < ctx->nb; ++b) {
    const int64_t r0 = ctx->I.block_start[b], cnt = ctx->I.block_start[b + 1] - r0;
    if (cnt == 0) continue;
    char* p = s.itf.as<char>() + static_cast<size_t>(r0) * k * ctx->es;
    MF_NCCL(ncclBroadcast(p, p, cnt * k, ctx->f64 ? ncclFloat64 : ncclFloat32, ctx->item_loc[b], ctx->comm, s.stream));
  }
  MF_NCCL(ncclGroupEnd());
  MF_HIP(hipStreamSynchronize(s.stream));
  // item_loc keeps tracking the ring (all ranks simulate it identically); copies made here
  // are read-only snapshots for evaluation.
}

EvalOut evaluate(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                 const int32_t* mult, double lambda, double* pred_out, uint8_t* found_out) {
  MF_REQUIRE(ctx->have_model, "The MatrixFactorization model has not been fitted to data. "
                              "Prior to predicting values, it has to be trained on data.");
  MF_REQUIRE(n >= 0, "negative count");
  require_healthy(ctx);
  EvalOut res;
  if (n == 0) return res;
  Shard& s = ctx->shards[0];
  if (ctx->rank_mode) allgather_items(ctx);
  else consolidate(ctx, s);
  std::vector<uint32_t> ur, ir;
  lookup_rows(ctx->U, u, n, ur);
  lookup_rows(ctx->I, i, n, ir);
  std::vector<int32_t> urow(n), irow(n);
  const int me = s.index;
  for (int64_t j = 0; j < n; ++j) {
    int32_t a = static_cast<int32_t>(ur[j]), b = static_cast<int32_t>(ir[j]);
    if (ctx->rank_mode && a >= 0 && ctx->U.row_block[a] / ctx->c != me) a = -1;  // not my user
    urow[j] = a;
    irow[j] = b;
  }
  DeviceGuard g(s.device);
  MF_HIP(hipStreamSynchronize(s.stream));
  s.ev_u.alloc(n * 4);
  s.ev_i.alloc(n * 4);
  MF_HIP(hipMemcpy(s.ev_u.get(), urow.data(), n * 4, hipMemcpyHostToDevice));
  MF_HIP(hipMemcpy(s.ev_i.get(), irow.data(), n * 4, hipMemcpyHostToDevice));
  double* dout = nullptr;
  if (pred_out) { s.ev_out.alloc(n * 8); dout = s.ev_out.as<double>(); }
  const double* dr = nullptr;
  const int32_t* dm = nullptr;
  double* dpart = nullptr;
  const int grid = predict_grid(n);
  if (r) {
    s.ev_r.alloc(n * 8);
    MF_HIP(hipMemcpy(s.ev_r.get(), r, n * 8, hipMemcpyHostToDevice));
    dr = s.ev_r.as<double>();
    s.ev_part.alloc(static_cast<size_t>(grid) * 3 * 8);
    dpart = s.ev_part.as<double>();
    if (mult) {
      s.ev_mult.alloc(n * 4);
      MF_HIP(hipMemcpy(s.ev_mult.get(), mult, n * 4, hipMemcpyHostToDevice));
      dm = s.ev_mult.as<int32_t>();
    }
  }
  launch_predict(s.stream, s.ev_u.as<int32_t>(), s.ev_i.as<int32_t>(), n, s.uf.get(), s.itf.get(),
                 ctx->P.num_factors, ctx->f64, dout, dr, dm, lambda, dpart);
  MF_HIP(hipGetLastError());
  MF_HIP(hipStreamSynchronize(s.stream));
  if (pred_out) {
    MF_HIP(hipMemcpy(pred_out, dout, n * 8, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < n; ++j) found_out[j] = (urow[j] >= 0 && irow[j] >= 0) ? 1 : 0;
  }
  if (r) {
    std::vector<double> part(static_cast<size_t>(grid) * 3);
    MF_HIP(hipMemcpy(part.data(), dpart, part.size() * 8, hipMemcpyDeviceToHost));
    for (int w = 0; w < grid; ++w) {
      res.sse += part[3 * w];
      res.cnt += part[3 * w + 1];
      res.risk += part[3 * w + 2];
    }
  }
  if (ctx->rank_mode && ctx->G > 1) {
    // combine per-rank results: predictions (owner rank writes, others contribute 0), sums
    DevBuf red;
    const int64_t m = 3 + (pred_out ? 2 * n : 0);
    std::vector<double> h(m, 0.0);
    h[0] = res.sse; h[1] = res.cnt; h[2] = res.risk;
    if (pred_out)
      for (int64_t j = 0; j < n; ++j) { h[3 + j] = found_out[j] ? pred_out[j] : 0.0; h[3 + n + j] = found_out[j]; }
    red.alloc(m * 8);
    MF_HIP(hipMemcpy(red.get(), h.data(), m * 8, hipMemcpyHostToDevice));
    MF_NCCL(ncclAllReduce(red.get(), red.get(), m, ncclFloat64, ncclSum, ctx->comm, s.stream));
    MF_HIP(hipStreamSynchronize(s.stream));
    MF_HIP(hipMemcpy(h.data(), red.get(), m * 8, hipMemcpyDeviceToHost));
    res.sse = h[0]; res.cnt = h[1]; res.risk = h[2];
    if (pred_out)
      for (int64_t j = 0; j < n; ++j) { pred_out[j] = h[3 + j]; found_out[j] = h[3 + n + j] > 0.5 ? 1 : 0; }
  }
  return res;
}

// ---------------------------------------------------------------------------------------
// Top-N lists (mf_recommend, mf_recommend_seen, mf_similar, mf_recommend_vectors): a front resolves the
// call's queries and exclusions to rows, one core scores and selects on the device
// (kernels_recommend.hip), on shard 0 like evaluate.  The query rows are scored in batches that bound the
// device scratch at batch x S x top_n keys (S = candidate splits, chosen so that a small batch against a
// large catalogue still fills the device).  MFHIP_TEST rec_batch=B / rec_split=S override both.
namespace {


// The row -> id table of a side on the device, current with the layout.
void sync_row_ids(mf_ctx* ctx, Shard& s, int side) {
  const SideLayout& L = side_of(ctx, side);
  const size_t bytes = static_cast<size_t>(L.rows()) * 4;
  if (s.rec_id_gen[side] != ctx->layout_gen || s.rec_id[side].bytes() < bytes) {
    s.rec_id[side].alloc(bytes);
    MF_HIP(hipMemcpy(s.rec_id[side].get(), L.row_id.data(), bytes, hipMemcpyHostToDevice));
    s.rec_id_gen[side] = ctx->layout_gen;
  }
}

// (query position << 32 | candidate row) pairs -> the exclusion CSR of nu queries: sorted distinct rows
void exclusion_csr(std::vector<uint64_t>& pairs, int64_t nu, std::vector<int64_t>& eoff, std::vector<int32_t>& erows) {
  eoff.assign(static_cast<size_t>(nu) + 1, 0);
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  erows.resize(pairs.size());
  for (size_t x = 0; x < pairs.size(); ++x) {
    ++eoff[(pairs[x] >> 32) + 1];
    erows[x] = static_cast<int32_t>(pairs[x] & 0xFFFFFFFFu);
  }
  for (int64_t u = 0; u < nu; ++u) eoff[u + 1] += eoff[u];
}

// The core.  nu queries against every row of side cside, minus each query's exclusions (the CSR d_eoff [nu + 1]
// / d_erows on the device, or with seen_qside >= 0 the resident seen set of that query side): ids [nu][top_n],
// scores (may be null), counts [nu] on the host.  The queries are either the rows s.rec_q[0 .. nu) of a
// resident factor slab Q of q_rows rows (which may be the candidate slab itself: mf_similar), or, with Q null,
// the caller's nu x k f64 vectors hvecs (s.rec_q = 0 .. nu-1): those are converted as upload_rows converts
// factor rows and staged one batch ahead, so the conversion of batch b + 1 runs on the host while the device
// scores batch b.
// among >= 0 (mf_recommend_among's shared list; MF_METRIC_DOT): the candidates are only the rows s.am_rows[0 ..
// among) of the side, distinct and ascending (on the device).  They are gathered into a compact slab with their
// ids, the kernels walk that slab, and the row list itself maps a slab position back to the factor row the
// exclusion tables name.
void recommend_scored(mf_ctx* ctx, Shard& s, const void* Q, int64_t q_rows, const double* hvecs, int64_t nu, int cside,
                      int32_t top_n, int metric, const int64_t* d_eoff, const int32_t* d_erows, int seen_qside,
                      int32_t* uid, double* usc, int32_t* ucnt, int64_t among = -1) {
  const SideLayout& CS = side_of(ctx, cside);
  const int64_t C = among >= 0 ? among : CS.rows();
  const int k = ctx->P.num_factors;
  const size_t N = static_cast<size_t>(top_n);
  if (nu == 0) return;
  if (C == 0) {
    std::fill(uid, uid + static_cast<size_t>(nu) * N, 0);
    if (usc) std::fill(usc, usc + static_cast<size_t>(nu) * N, 0.0);
    std::fill(ucnt, ucnt + nu, 0);
    return;
  }
  sync_row_ids(ctx, s, cside);

  int64_t batch = 8192;
  if (const std::string v = test_knob("rec_batch"); !v.empty()) batch = std::max<int64_t>(1, std::atoll(v.c_str()));
  batch = std::min(batch, nu);
  // S: enough workgroups for two per CU, each split at least one candidate tile of 128 rows
  const int qt = recommend_query_tile(top_n, ctx->f64);
  const int64_t qtiles = (batch + qt - 1) / qt;
  int64_t S = std::min<int64_t>((512 + qtiles - 1) / qtiles, (C + 127) / 128);
  if (const std::string v = test_knob("rec_split"); !v.empty()) S = std::atoll(v.c_str());
  S = std::max<int64_t>(1, std::min<int64_t>({S, 64, C}));

  s.rec_part.alloc(static_cast<size_t>(batch) * S * N * recommend_key_bytes(ctx->f64));
  s.rec_ids.alloc(static_cast<size_t>(batch) * N * 4);
  s.rec_scores.alloc(static_cast<size_t>(batch) * N * 8);
  s.rec_counts.alloc(static_cast<size_t>(batch) * 4);
  const void* Cf = cside == kSideU ? s.uf.get() : s.itf.get();
  const int32_t* cand_id = s.rec_id[cside].as<int32_t>();
  const int32_t* pos_row = nullptr;
  if (among >= 0) {
    s.am_id.alloc(static_cast<size_t>(C) * 4);
    s.am_slab.alloc(static_cast<size_t>(C) * k * ctx->es);
    launch_among_gather(s.stream, Cf, s.am_rows.as<int32_t>(), C, k, ctx->f64, cand_id, s.am_slab.get(),
                        s.am_id.as<int32_t>());
    MF_HIP(hipGetLastError());
    Cf = s.am_slab.get();
    cand_id = s.am_id.as<int32_t>();
    pos_row = s.am_rows.as<int32_t>();
  }
  // cosine: the inverse norms of this call (never kept: the rows may change before the next one)
  const bool cosine = metric == MF_METRIC_COSINE;
  const void *q_inv = nullptr, *c_inv = nullptr;
  if (cosine) {
    s.rec_cinv.alloc(static_cast<size_t>(C) * ctx->es);
    launch_row_inv_norm(s.stream, Cf, C, k, ctx->f64, s.rec_cinv.get());
    q_inv = c_inv = s.rec_cinv.get();
    if (Q != Cf) {
      s.rec_qinv.alloc(static_cast<size_t>(Q ? q_rows : batch) * ctx->es);
      if (Q) launch_row_inv_norm(s.stream, Q, q_rows, k, ctx->f64, s.rec_qinv.get());
      q_inv = s.rec_qinv.get();
    }
    MF_HIP(hipGetLastError());
  }
  // host vectors: batch [b0, b0 + nb) -> the pinned stage in the context's precision -> rec_qvec, queued
  // behind whatever the stream holds (the previous batch's kernels still read rec_qvec)
  const size_t kk = static_cast<size_t>(k);
  auto stage_vectors = [&](int64_t b0, int64_t nb) {
    const double* src = hvecs + static_cast<size_t>(b0) * kk;
    const int64_t n = nb * k;
    if (ctx->f64) {
      std::memcpy(s.rec_pin.as<double>(), src, static_cast<size_t>(n) * 8);
    } else {
      float* dst = s.rec_pin.as<float>();
      parallel_for(n, [&](int64_t b, int64_t e, int) {
        for (int64_t x = b; x < e; ++x) dst[x] = static_cast<float>(src[x]);
      });
    }
    MF_HIP(hipMemcpyAsync(s.rec_qvec.get(), s.rec_pin.as<char>(), static_cast<size_t>(n) * ctx->es,
                          hipMemcpyHostToDevice, s.stream));
  };
  if (!Q) {
    s.rec_qvec.alloc(static_cast<size_t>(batch) * kk * ctx->es);
    s.rec_pin.alloc(static_cast<size_t>(batch) * kk * ctx->es);
    stage_vectors(0, batch);
    MF_HIP(hipStreamSynchronize(s.stream));  // the stage is rewritten while batch 0 runs
  }
  // the seen set: a batch's exclusion ranges are gathered from the resident offsets through its rows
  const SeenView sv = seen_qside >= 0 ? seen_view(ctx, s, seen_qside) : SeenView{};
  if (sv.any) {
    s.seen.qbeg.alloc(static_cast<size_t>(batch) * 8);
    s.seen.qend.alloc(static_cast<size_t>(batch) * 8);
  }
  for (int64_t b0 = 0; b0 < nu; b0 += batch) {
    const int64_t nb = std::min(batch, nu - b0);
    const int64_t *ebeg = d_eoff + b0, *eend = ebeg + 1;
    const int32_t* erows_d = d_erows;
    if (sv.any) {
      launch_seen_gather(s.stream, sv.off, s.rec_q.as<int32_t>() + b0, static_cast<int>(nb), s.seen.qbeg.as<int64_t>(),
                         s.seen.qend.as<int64_t>());
      ebeg = s.seen.qbeg.as<int64_t>();
      eend = s.seen.qend.as<int64_t>();
      erows_d = sv.ent;
    }
    // a staged batch is rows 0 .. nb-1 of rec_qvec: the head of the identity list in rec_q names them
    const int32_t* rows_d = s.rec_q.as<int32_t>() + (Q ? b0 : 0);
    if (!Q && cosine) launch_row_inv_norm(s.stream, s.rec_qvec.get(), nb, k, ctx->f64, s.rec_qinv.get());
    launch_recommend(s.stream, Q ? Q : s.rec_qvec.get(), Cf, rows_d, static_cast<int>(nb), static_cast<int32_t>(C),
                     static_cast<int>(S), k, top_n, ctx->f64, cand_id, ebeg, eend, erows_d, s.rec_part.get(),
                     s.rec_ids.as<int32_t>(), s.rec_scores.as<double>(), s.rec_counts.as<int32_t>(), q_inv, c_inv,
                     pos_row);
    MF_HIP(hipGetLastError());
    if (!Q && b0 + batch < nu) {
      // the stage is free: its last copy finished with the previous batch's synchronisation
      stage_vectors(b0 + batch, std::min(batch, nu - b0 - batch));
    }
    MF_HIP(hipStreamSynchronize(s.stream));
    MF_HIP(hipMemcpy(uid + static_cast<size_t>(b0) * N, s.rec_ids.get(), static_cast<size_t>(nb) * N * 4,
                     hipMemcpyDeviceToHost));
    if (usc)
      MF_HIP(hipMemcpy(usc + static_cast<size_t>(b0) * N, s.rec_scores.get(), static_cast<size_t>(nb) * N * 8,
                       hipMemcpyDeviceToHost));
    MF_HIP(hipMemcpy(ucnt + b0, s.rec_counts.get(), static_cast<size_t>(nb) * 4, hipMemcpyDeviceToHost));
  }
}

// The same for queries and exclusions the host holds: the rows qrows[0 .. nu) and the CSR eoff / erows are
// uploaded, the rest is recommend_scored's.
void recommend_core(mf_ctx* ctx, Shard& s, const void* Q, int64_t q_rows, const double* hvecs,
                    const std::vector<int32_t>& qrows, int cside, int32_t top_n, int metric,
                    const std::vector<int64_t>& eoff, const std::vector<int32_t>& erows, int seen_qside, int32_t* uid,
                    double* usc, int32_t* ucnt, int64_t among = -1) {
  const int64_t nu = static_cast<int64_t>(qrows.size());
  if (nu == 0) return;
  DeviceGuard g(s.device);
  if (side_of(ctx, cside).rows() > 0) {
    s.rec_q.alloc(static_cast<size_t>(nu) * 4);
    s.rec_eoff.alloc(eoff.size() * 8);
    s.rec_erows.alloc(std::max<size_t>(erows.size(), 1) * 4);
    MF_HIP(hipMemcpy(s.rec_q.get(), qrows.data(), static_cast<size_t>(nu) * 4, hipMemcpyHostToDevice));
    MF_HIP(hipMemcpy(s.rec_eoff.get(), eoff.data(), eoff.size() * 8, hipMemcpyHostToDevice));
    if (!erows.empty()) MF_HIP(hipMemcpy(s.rec_erows.get(), erows.data(), erows.size() * 4, hipMemcpyHostToDevice));
  }
  recommend_scored(ctx, s, Q, q_rows, hvecs, nu, cside, top_n, metric, s.rec_eoff.as<int64_t>(),
                   s.rec_erows.as<int32_t>(), seen_qside, uid, usc, ucnt, among);
}

// The queries of a call by id: qr[j] = the row of queries[j] (kRowMiss: unknown id), uniq = the distinct known
// rows, ascending, pos(row) = a row's index among them (-1: unknown id).
struct QuerySet {
  std::vector<uint32_t> qr;
  std::vector<int32_t> uniq;
  QuerySet(const SideLayout& QS, const int32_t* queries, int64_t nq) {
    lookup_rows(QS, queries, nq, qr);
    uniq.reserve(qr.size());
    for (uint32_t r : qr)
      if (r != kRowMiss) uniq.push_back(static_cast<int32_t>(r));
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  }
  int64_t pos(uint32_t row) const {
    if (row == kRowMiss) return -1;
    auto it = std::lower_bound(uniq.begin(), uniq.end(), static_cast<int32_t>(row));
    return it != uniq.end() && *it == static_cast<int32_t>(row) ? it - uniq.begin() : -1;
  }
};

// The call's exclusion pairs (ids) as a CSR: one row per distinct query, sorted candidate rows inside it.
// no_self: each query's own row joins its exclusions.
void call_exclusions(const SideLayout& QS, const SideLayout& CS, const QuerySet& qs, bool no_self, const int32_t* eq,
                     const int32_t* ec, int64_t ne, std::vector<int64_t>& eoff, std::vector<int32_t>& erows) {
  const std::vector<int32_t>& uniq = qs.uniq;
  const int64_t nu = static_cast<int64_t>(uniq.size());
  eoff.assign(static_cast<size_t>(nu) + 1, 0);
  erows.clear();
  if (!((ne > 0 || no_self) && nu > 0 && CS.rows() > 0)) return;
  std::vector<uint64_t> pairs;
  pairs.reserve(static_cast<size_t>(ne) + (no_self ? static_cast<size_t>(nu) : 0));
  if (ne > 0) {
    std::vector<uint32_t> er_q, er_c;
    lookup_rows(QS, eq, ne, er_q);
    lookup_rows(CS, ec, ne, er_c);
    for (int64_t e = 0; e < ne; ++e) {
      const int64_t u = qs.pos(er_q[e]);
      if (u < 0 || er_c[e] == kRowMiss) continue;
      pairs.push_back((static_cast<uint64_t>(u) << 32) | er_c[e]);
    }
  }
  if (no_self)
    for (int64_t u = 0; u < nu; ++u) pairs.push_back((static_cast<uint64_t>(u) << 32) | static_cast<uint32_t>(uniq[u]));
  exclusion_csr(pairs, nu, eoff, erows);
}

// The front of the calls whose queries are ids of side qside, candidates the rows of side cside (the other
// side: mf_recommend; the same side: mf_similar).  Distinct known query rows are scored once; every position
// of queries[] then takes its row's result.  no_self: each query's own row joins its exclusions (it is a
// candidate only when qside == cside) -- no kernel knows about "self".  among: recommend_scored's.
void recommend_ids(mf_ctx* ctx, int qside, int cside, const int32_t* queries, int64_t nq, int32_t top_n, int metric,
                   bool no_self, const int32_t* eq, const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out,
                   int32_t* counts_out, bool seen, int64_t among = -1) {
  Shard& s = ctx->shards[0];
  if (seen) ne = 0;  // the resident set stands in for the call's own CSR
  consolidate(ctx, s);
  sync_all(ctx);  // a run may still be sweeping (mf_dsgd_run returns early)
  const SideLayout& QS = side_of(ctx, qside);
  const SideLayout& CS = side_of(ctx, cside);
  const size_t N = static_cast<size_t>(top_n);

  const QuerySet qs(QS, queries, nq);
  const std::vector<uint32_t>& qr = qs.qr;
  const std::vector<int32_t>& uniq = qs.uniq;
  const int64_t nu = static_cast<int64_t>(uniq.size());
  auto upos = [&](uint32_t row) { return qs.pos(row); };
  std::vector<int64_t> eoff;
  std::vector<int32_t> erows;
  call_exclusions(QS, CS, qs, no_self, eq, ec, ne, eoff, erows);

  std::vector<int32_t> uid(static_cast<size_t>(nu) * N, 0), ucnt(static_cast<size_t>(nu), 0);
  std::vector<double> usc(scores_out ? static_cast<size_t>(nu) * N : 0, 0.0);
  recommend_core(ctx, s, qside == kSideU ? s.uf.get() : s.itf.get(), QS.rows(), nullptr, uniq, cside, top_n, metric,
                 eoff, erows, seen ? qside : -1, uid.data(), scores_out ? usc.data() : nullptr, ucnt.data(), among);
  parallel_for(nq, [&](int64_t b, int64_t e, int) {
    for (int64_t j = b; j < e; ++j) {
      const int64_t u = upos(qr[j]);
      int32_t* io = ids_out + static_cast<size_t>(j) * N;
      if (u < 0) {
        counts_out[j] = 0;
        std::fill(io, io + N, 0);
        if (scores_out) std::fill(scores_out + static_cast<size_t>(j) * N, scores_out + static_cast<size_t>(j + 1) * N, 0.0);
        continue;
      }
      counts_out[j] = ucnt[u];
      std::memcpy(io, uid.data() + static_cast<size_t>(u) * N, N * 4);
      if (scores_out) std::memcpy(scores_out + static_cast<size_t>(j) * N, usc.data() + static_cast<size_t>(u) * N, N * 8);
    }
  });
}

}  // namespace

void recommend(mf_ctx* ctx, int qside, const int32_t* queries, int64_t nq, int32_t top_n, const int32_t* eq,
               const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out, int32_t* counts_out,
               bool seen) {
  recommend_ids(ctx, qside, 1 - qside, queries, nq, top_n, MF_METRIC_DOT, false, eq, ec, ne, ids_out, scores_out,
                counts_out, seen);
}

namespace {

// mf_recommend_among with per-query lists: position j owns cand[off[j] .. off[j + 1]).  Nothing is shared
// between positions, so every position is scored on its own (duplicate queries included) and the outputs are
// written in place.  The lists go up as they are and are resolved on the device (launch_id_lookup_one over
// the candidate side's id mirror); the host only cuts them into tasks from the offsets: a list of n entries takes
// ceil(n / E) parts, at most 64, of equal length rounded up to whole 64-entry groups -- so long lists get longer
// parts -- and E = 512 entries (MFHIP_TEST among_chunk=E).  Positions are taken in batches that bound the
// device scratch (MFHIP_TEST among_batch=B: at most B positions per batch).
void among_lists(mf_ctx* ctx, int qside, const int32_t* queries, int64_t nq, int32_t top_n, const int64_t* off,
                 const int32_t* cand, bool seen, const int32_t* eq, const int32_t* ec, int64_t ne, int32_t* ids_out,
                 double* scores_out, int32_t* counts_out) {
  Shard& s = ctx->shards[0];
  consolidate(ctx, s);
  sync_all(ctx);
  const int cside = 1 - qside;
  const SideLayout& QS = side_of(ctx, qside);
  const SideLayout& CS = side_of(ctx, cside);
  const size_t N = static_cast<size_t>(top_n);
  const int k = ctx->P.num_factors;
  std::fill(ids_out, ids_out + static_cast<size_t>(nq) * N, 0);
  if (scores_out) std::fill(scores_out, scores_out + static_cast<size_t>(nq) * N, 0.0);
  std::fill(counts_out, counts_out + nq, 0);
  if (CS.rows() == 0 || QS.rows() == 0 || off[nq] == 0) return;

  const QuerySet qs(QS, queries, nq);
  std::vector<int64_t> eoff;
  std::vector<int32_t> erows;
  call_exclusions(QS, CS, qs, false, eq, ec, seen ? 0 : ne, eoff, erows);

  // A batch is bounded by its scratch, 256 MB each of: the lists as uploaded (4 B an entry: 2^26 entries; a
  // longer single list is a batch of its own), the partial lists (top_n keys a task), and the results (12 B a
  // slot: 256 MB / (12 top_n) positions, 1.7M at top 10, 175k at top 128).
  const int64_t scratch = int64_t{256} << 20;
  int64_t E = 512, max_pos = scratch / (12 * static_cast<int64_t>(N));
  if (const std::string v = test_knob("among_chunk"); !v.empty()) E = std::max<int64_t>(1, std::atoll(v.c_str()));
  if (const std::string v = test_knob("among_batch"); !v.empty()) max_pos = std::max<int64_t>(1, std::atoll(v.c_str()));
  const size_t kb = recommend_key_bytes(ctx->f64);
  const int64_t max_tasks = std::max<int64_t>(64, scratch / static_cast<int64_t>(N * kb));  // (a list: <= 64 tasks)
  const int64_t max_entries = scratch / 4;

  DeviceGuard g(s.device);
  sync_row_ids(ctx, s, cside);
  DevIndex& mirror = s.didx[cside];
  sync_dev_index(s, CS.index, mirror);
  s.rec_erows.alloc(std::max<size_t>(erows.size(), 1) * 4);
  if (!erows.empty()) MF_HIP(hipMemcpy(s.rec_erows.get(), erows.data(), erows.size() * 4, hipMemcpyHostToDevice));
  const SeenView sv = seen ? seen_view(ctx, s, qside) : SeenView{};
  const void* Q = qside == kSideU ? s.uf.get() : s.itf.get();
  const void* Cf = cside == kSideU ? s.uf.get() : s.itf.get();

  std::vector<AmongTask> tasks;
  std::vector<int64_t> pbeg, ebeg, eend;
  std::vector<int32_t> qrow;
  for (int64_t j0 = 0; j0 < nq;) {
    // the batch [j0, j1): its tasks, and per position the query row and the exclusion range
    tasks.clear();
    pbeg.assign(1, 0);
    qrow.clear();
    ebeg.clear();
    eend.clear();
    int64_t j1 = j0;
    for (; j1 < nq && j1 - j0 < max_pos; ++j1) {
      const int64_t n = off[j1 + 1] - off[j1];
      const int64_t u = qs.pos(qs.qr[j1]);
      int64_t parts = 0, plen = 0;
      if (u >= 0 && n > 0) {
        parts = std::min<int64_t>(64, (n + E - 1) / E);
        plen = ((n + parts - 1) / parts + 63) / 64 * 64;
        MF_REQUIRE(plen < (int64_t{1} << 31), "a candidate list is too long");
      }
      if (j1 > j0 && (static_cast<int64_t>(tasks.size()) + parts > max_tasks || off[j1 + 1] - off[j0] > max_entries)) break;
      for (int64_t b = 0; b < n && parts > 0; b += plen)
        tasks.push_back(AmongTask{off[j1] - off[j0] + b, static_cast<int32_t>(std::min(plen, n - b)),
                                  static_cast<int32_t>(j1 - j0)});
      pbeg.push_back(static_cast<int64_t>(tasks.size()));
      qrow.push_back(u >= 0 ? qs.uniq[u] : 0);
      ebeg.push_back(u >= 0 ? eoff[u] : 0);
      eend.push_back(u >= 0 ? eoff[u + 1] : 0);
    }
    const int64_t nb = j1 - j0, ntasks = static_cast<int64_t>(tasks.size()), nent = off[j1] - off[j0];
    if (ntasks > 0) {  // (else every count of the batch is 0, as the outputs already say)
      s.am_in.alloc(static_cast<size_t>(nent) * 4);
      s.am_tasks.alloc(static_cast<size_t>(ntasks) * sizeof(AmongTask));
      s.am_pbeg.alloc(static_cast<size_t>(nb + 1) * 8);
      s.am_qrow.alloc(static_cast<size_t>(nb) * 4);
      s.am_ebeg.alloc(static_cast<size_t>(nb) * 8);
      s.am_eend.alloc(static_cast<size_t>(nb) * 8);
      s.rec_part.alloc(static_cast<size_t>(ntasks) * N * kb);
      s.rec_ids.alloc(static_cast<size_t>(nb) * N * 4);
      s.rec_scores.alloc(static_cast<size_t>(nb) * N * 8);
      s.rec_counts.alloc(static_cast<size_t>(nb) * 4);
      MF_HIP(hipMemcpyAsync(s.am_in.get(), cand + off[j0], static_cast<size_t>(nent) * 4, hipMemcpyHostToDevice, s.stream));
      MF_HIP(hipMemcpyAsync(s.am_tasks.get(), tasks.data(), static_cast<size_t>(ntasks) * sizeof(AmongTask),
                            hipMemcpyHostToDevice, s.stream));
      MF_HIP(hipMemcpyAsync(s.am_pbeg.get(), pbeg.data(), static_cast<size_t>(nb + 1) * 8, hipMemcpyHostToDevice, s.stream));
      MF_HIP(hipMemcpyAsync(s.am_qrow.get(), qrow.data(), static_cast<size_t>(nb) * 4, hipMemcpyHostToDevice, s.stream));
      if (sv.any) {
        launch_seen_gather(s.stream, sv.off, s.am_qrow.as<int32_t>(), static_cast<int>(nb), s.am_ebeg.as<int64_t>(),
                           s.am_eend.as<int64_t>());
      } else {
        MF_HIP(hipMemcpyAsync(s.am_ebeg.get(), ebeg.data(), static_cast<size_t>(nb) * 8, hipMemcpyHostToDevice, s.stream));
        MF_HIP(hipMemcpyAsync(s.am_eend.get(), eend.data(), static_cast<size_t>(nb) * 8, hipMemcpyHostToDevice, s.stream));
      }
      launch_id_lookup_one(s.stream, s.am_in.as<uint32_t>(), nent, mirror.cap ? mirror.slots.get() : nullptr,
                           mirror.cap - 1);
      launch_among(s.stream, Q, Cf, s.am_tasks.as<AmongTask>(), ntasks, s.am_pbeg.as<int64_t>(), static_cast<int>(nb),
                   s.am_in.as<uint32_t>(), s.am_qrow.as<int32_t>(), s.rec_id[cside].as<int32_t>(), s.am_ebeg.as<int64_t>(),
                   s.am_eend.as<int64_t>(), sv.any ? sv.ent : s.rec_erows.as<int32_t>(), k, top_n, ctx->f64,
                   s.rec_part.get(), s.rec_ids.as<int32_t>(), s.rec_scores.as<double>(), s.rec_counts.as<int32_t>());
      MF_HIP(hipGetLastError());
      MF_HIP(hipStreamSynchronize(s.stream));  // (the host vectors are rebuilt for the next batch)
      MF_HIP(hipMemcpy(ids_out + static_cast<size_t>(j0) * N, s.rec_ids.get(), static_cast<size_t>(nb) * N * 4,
                       hipMemcpyDeviceToHost));
      if (scores_out)
        MF_HIP(hipMemcpy(scores_out + static_cast<size_t>(j0) * N, s.rec_scores.get(), static_cast<size_t>(nb) * N * 8,
                         hipMemcpyDeviceToHost));
      MF_HIP(hipMemcpy(counts_out + j0, s.rec_counts.get(), static_cast<size_t>(nb) * 4, hipMemcpyDeviceToHost));
    }
    j0 = j1;
  }
}

}  // namespace

// mf_recommend_among.  One shared list (off == null) is resolved to its distinct held rows on the device and
// handed to the fused kernels as their candidate slab; per-query lists take the gather path above.
void recommend_among(mf_ctx* ctx, int qside, const int32_t* queries, int64_t nq, int32_t top_n, const int64_t* off,
                     const int32_t* cand, int64_t n_cand, bool seen, const int32_t* eq, const int32_t* ec, int64_t ne,
                     int32_t* ids_out, double* scores_out, int32_t* counts_out) {
  if (off) {
    among_lists(ctx, qside, queries, nq, top_n, off, cand, seen, eq, ec, ne, ids_out, scores_out, counts_out);
    return;
  }
  // the list goes up as it is: ids -> rows (the candidate side's id mirror), then sort, first occurrences, scan
  // and compaction leave its distinct held rows, ascending, in s.am_rows
  Shard& s = ctx->shards[0];
  consolidate(ctx, s);
  sync_all(ctx);
  const SideLayout& CS = side_of(ctx, 1 - qside);
  int64_t held = 0;
  if (n_cand > 0 && CS.rows() > 0) {
    DeviceGuard g(s.device);
    DevIndex& mirror = s.didx[1 - qside];
    sync_dev_index(s, CS.index, mirror);
    s.am_in.alloc(static_cast<size_t>(n_cand) * 4);
    s.am_rows.alloc(static_cast<size_t>(n_cand) * 4);
    MF_HIP(hipMemcpyAsync(s.am_in.get(), cand, static_cast<size_t>(n_cand) * 4, hipMemcpyHostToDevice, s.stream));
    launch_id_lookup_one(s.stream, s.am_in.as<uint32_t>(), n_cand, mirror.cap ? mirror.slots.get() : nullptr,
                         mirror.cap - 1);
    held = among_distinct_rows(s.stream, s.rank_sc, s.am_in.as<uint32_t>(), n_cand, s.am_rows.as<int32_t>());
  }
  recommend_ids(ctx, qside, 1 - qside, queries, nq, top_n, MF_METRIC_DOT, false, eq, ec, ne, ids_out, scores_out,
                counts_out, seen, held);
}

// mf_similar: the nearest rows of the queries' own side.
void similar(mf_ctx* ctx, int side, const int32_t* queries, int64_t nq, int32_t top_n, int metric, bool include_self,
             const int32_t* eq, const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out,
             int32_t* counts_out) {
  recommend_ids(ctx, side, side, queries, nq, top_n, metric, !include_self, eq, ec, ne, ids_out, scores_out, counts_out,
                false);
}

// mf_recommend_vectors: the queries are the caller's vectors; query j is row j of vecs, exclusions name j.
void recommend_vectors(mf_ctx* ctx, int cside, const double* vecs, int64_t nq, int32_t top_n, int metric,
                       const int64_t* eqi, const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out,
                       int32_t* counts_out) {
  Shard& s = ctx->shards[0];
  consolidate(ctx, s);
  sync_all(ctx);
  const SideLayout& CS = side_of(ctx, cside);
  MF_REQUIRE(nq < (int64_t{1} << 31), "too many query vectors for one call");
  std::vector<int32_t> rows(static_cast<size_t>(nq));
  std::iota(rows.begin(), rows.end(), 0);
  std::vector<int64_t> eoff(static_cast<size_t>(nq) + 1, 0);
  std::vector<int32_t> erows;
  if (ne > 0 && CS.rows() > 0) {
    std::vector<uint32_t> er_c;
    lookup_rows(CS, ec, ne, er_c);
    std::vector<uint64_t> pairs;
    pairs.reserve(static_cast<size_t>(ne));
    for (int64_t e = 0; e < ne; ++e) {
      if (eqi[e] < 0 || eqi[e] >= nq || er_c[e] == kRowMiss) continue;
      pairs.push_back((static_cast<uint64_t>(eqi[e]) << 32) | er_c[e]);
    }
    exclusion_csr(pairs, nq, eoff, erows);
  }
  recommend_core(ctx, s, nullptr, 0, vecs, rows, cside, top_n, metric, eoff, erows, -1, ids_out, scores_out,
                 counts_out);
}

// mf_recommend_foldin's entry: the queries are the identity rows of a slab that kernels queued on the stream
// are still writing; the identity list is made on the device.
void recommend_resident(mf_ctx* ctx, Shard& s, const void* Q, int64_t nu, int cside, int32_t top_n,
                        const int64_t* d_eoff, const int32_t* d_erows, int32_t* ids_out, double* scores_out,
                        int32_t* counts_out) {
  if (nu > 0 && side_of(ctx, cside).rows() > 0) {
    s.rec_q.alloc(static_cast<size_t>(nu) * 4);
    launch_iota(s.stream, s.rec_q.as<int32_t>(), nu);
  }
  recommend_scored(ctx, s, Q, nu, nullptr, nu, cside, top_n, MF_METRIC_DOT, d_eoff, d_erows, -1, ids_out, scores_out,
                   counts_out);
}

// Every row of a side (rank mode: the rank's own users), ascending by id (mf_get_factors).
void get_factors(mf_ctx* ctx, int side, int32_t* ids, double* vecs, int64_t cap, int64_t* written) {
  MF_REQUIRE(ctx->have_model, "The MatrixFactorization model has not been fitted to data.");
  require_healthy(ctx);
  Shard& s = ctx->shards[0];
  if (ctx->rank_mode) { if (side == MF_SIDE_ITEM) allgather_items(ctx); }
  else consolidate(ctx, s);
  sync_all(ctx);
  ensure_order(ctx);
  const SideLayout& S = side_of(ctx, side);
  const int k = ctx->P.num_factors;
  std::vector<double> all(static_cast<size_t>(std::max<int64_t>(S.rows(), 1)) * k);
  download_rows(ctx, s, side, 0, S.rows(), all.data());
  const auto& ord = side == kSideU ? ctx->rows_by_id_u : ctx->rows_by_id_i;
  int64_t w = 0;
  const int me = s.index;
  for (int64_t x = 0; x < S.rows(); ++x) {
    const int32_t row = ord[x];
    if (ctx->rank_mode && side == kSideU && S.row_block[row] / ctx->c != me) continue;
    if (w >= cap) fail(MF_ERR_CAPACITY, "output capacity too small");
    if (ids) ids[w] = S.row_id[row];
    if (vecs) std::memcpy(vecs + static_cast<size_t>(w) * k, all.data() + static_cast<size_t>(row) * k, sizeof(double) * k);
    ++w;
  }
  if (written) *written = w;
}

void lookup_factors(mf_ctx* ctx, int side, const int32_t* ids, int64_t n, double* vecs_out, uint8_t* found) {
  MF_REQUIRE(ctx->have_model, "no model");
  Shard& s = ctx->shards[0];
  if (!ctx->rank_mode) consolidate(ctx, s);
  else if (side == MF_SIDE_ITEM) allgather_items(ctx);
  sync_all(ctx);
  const SideLayout& S = side_of(ctx, side);
  const int k = ctx->P.num_factors;
  std::vector<double> row(k);
  for (int64_t j = 0; j < n; ++j) {
    const int32_t x = S.index.find(ids[j]);
    found[j] = x >= 0;
    if (x < 0) { std::fill(vecs_out + j * k, vecs_out + (j + 1) * k, 0.0); continue; }
    download_rows(ctx, s, side, x, 1, vecs_out + static_cast<size_t>(j) * k);
  }
}

}  // namespace mfhip
