// rank_eval.cpp -- ranking metrics of held-out pairs against the model's top-N lists (mf_rank_eval):
// ids resolved on the host, everything after that on the device (kernels_rank.hip for the pair tables,
// the metrics and their sums; kernels_recommend.hip for the lists), on shard 0 like recommend().  Only
// the totals cross back, and the per-query rows when the caller asks for them.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "common.hpp"
#include "context.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mfhip {
namespace {


// One pair list on the device: the query rows in rk_in[0, n), the candidate column in rk_in[n, 2n).
// The stream is drained first: an earlier table build may still read the buffer.
void upload_pairs(Shard& s, const uint32_t* qrow, const void* cand, int64_t n) {
  MF_HIP(hipStreamSynchronize(s.stream));
  s.rk_in.alloc(static_cast<size_t>(std::max<int64_t>(n, 1)) * 8);
  if (n == 0) return;
  MF_HIP(hipMemcpy(s.rk_in.get(), qrow, static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
  MF_HIP(hipMemcpy(s.rk_in.as<uint32_t>() + n, cand, static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
}

// The evaluated queries of a ground-truth list (into rec_q) and its CSR (rk_goff / rk_gent); returns nq.
int64_t build_truth(Shard& s, const SideLayout& QS, const int32_t* gq, const int32_t* gc, int64_t ng,
                    std::vector<uint32_t>& qr) {
  lookup_rows(QS, gq, ng, qr);
  upload_pairs(s, qr.data(), gc, ng);
  const uint32_t rows = static_cast<uint32_t>(QS.rows());
  const uint32_t* in = s.rk_in.as<uint32_t>();
  const int64_t nq = rank_query_set(s.stream, s.rank_sc, in, ng, rows, s.rec_q);
  rank_pair_csr(s.stream, s.rank_sc, in, in + ng, ng, rows, nq, true, s.rk_goff, s.rk_gent);
  return nq;
}

// The exclusion CSR of the evaluated queries (rec_eoff / rec_erows), after build_truth.
void build_exclusions(Shard& s, const SideLayout& QS, const SideLayout& CS, const int32_t* eq,
                      const int32_t* ec, int64_t ne, int64_t nq) {
  if (ne > 0 && CS.rows() > 0 && nq > 0) {
    std::vector<uint32_t> er_q, er_c;
    lookup_rows(QS, eq, ne, er_q);
    lookup_rows(CS, ec, ne, er_c);
    upload_pairs(s, er_q.data(), er_c.data(), ne);
  } else {
    ne = 0;
  }
  const uint32_t* in = s.rk_in.as<uint32_t>();
  rank_pair_csr(s.stream, s.rank_sc, in, in + ne, ne, static_cast<uint32_t>(QS.rows()), nq, false, s.rec_eoff,
                s.rec_erows);
}

}  // namespace

// 128 gains 1 / log(i + 2), then idcg[m] = gain_0 + ... + gain_{m-1} summed in that order, m = 0 .. 128
const std::vector<double>& gain_table() {
  static const std::vector<double> tab = [] {
    std::vector<double> t(MF_RECOMMEND_MAX_TOP + MF_RECOMMEND_MAX_TOP + 1, 0.0);
    for (int i = 0; i < MF_RECOMMEND_MAX_TOP; ++i) t[i] = 1.0 / std::log(static_cast<double>(i + 2));
    double* idcg = t.data() + MF_RECOMMEND_MAX_TOP;
    for (int m = 1; m <= MF_RECOMMEND_MAX_TOP; ++m) idcg[m] = idcg[m - 1] + t[m - 1];
    return t;
  }();
  return tab;
}

void rank_eval(mf_ctx* ctx, int qside, const int32_t* gq, const int32_t* gc, int64_t ng, int32_t top_n,
               const int32_t* eq, const int32_t* ec, int64_t ne, mf_rank_metrics* out, int32_t* q_ids_out,
               int32_t* q_counts_out, double* q_metrics_out, int64_t cap, bool seen) {
  *out = mf_rank_metrics{};
  if (ng == 0) return;
  Shard& s = ctx->shards[0];
  consolidate(ctx, s);
  sync_all(ctx);  // a run may still be sweeping (mf_dsgd_run returns early)
  PhaseClock clk;
  const int cside = 1 - qside;
  const SideLayout& QS = side_of(ctx, qside);
  const SideLayout& CS = side_of(ctx, cside);
  DeviceGuard g(s.device);

  // the seen set stands in for the exclusion table of the call (taken first: it may build its item-major
  // table with the scratch build_truth uses)
  const SeenView sv = seen ? seen_view(ctx, s, qside) : SeenView{};
  if (seen) ne = 0;
  std::vector<uint32_t> qr;
  const int64_t nq = build_truth(s, QS, gq, gc, ng, qr);
  {
    // the distinct unknown query ids, while the device builds the ground-truth table
    std::vector<int32_t> unknown;
    std::mutex mu;
    parallel_for(ng, [&](int64_t b, int64_t e, int) {
      std::vector<int32_t> mine;
      for (int64_t j = b; j < e; ++j)
        if (qr[j] == kRowMiss) mine.push_back(gq[j]);
      if (mine.empty()) return;
      std::lock_guard<std::mutex> lk(mu);
      unknown.insert(unknown.end(), mine.begin(), mine.end());
    });
    std::sort(unknown.begin(), unknown.end());
    out->unknown_queries = std::unique(unknown.begin(), unknown.end()) - unknown.begin();
  }
  out->queries = nq;
  if (q_ids_out && cap < nq)
    fail(MF_ERR_CAPACITY, "per-query outputs hold " + std::to_string(cap) + " rows, " + std::to_string(nq) + " needed");
  if (nq == 0) {
    MF_HIP(hipStreamSynchronize(s.stream));
    return;
  }
  if (!sv.any) build_exclusions(s, QS, CS, eq, ec, ne, nq);
  if (clk.on) MF_HIP(hipStreamSynchronize(s.stream));
  clk.lap("rank_eval: pair tables");

  const std::vector<double>& tab = gain_table();
  s.rk_tab.alloc(tab.size() * 8);
  MF_HIP(hipMemcpyAsync(s.rk_tab.get(), tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s.stream));

  const int64_t slices = rank_reduce_slices(nq);
  s.rk_met.alloc(static_cast<size_t>(nq) * MF_RANK_NMETRICS * 8);
  s.rk_cnt.alloc(static_cast<size_t>(nq) * 2 * 8);
  s.rk_part.alloc(static_cast<size_t>(slices) * (MF_RANK_NMETRICS + 2) * 8);
  s.rk_res.alloc((MF_RANK_NMETRICS + 2) * 8);
  double* part = s.rk_part.as<double>();
  int64_t* ipart = reinterpret_cast<int64_t*>(part + slices * MF_RANK_NMETRICS);
  double* sums = s.rk_res.as<double>();
  int64_t* isums = reinterpret_cast<int64_t*>(sums + MF_RANK_NMETRICS);
  // the driver's batches (lists of no candidate side: empty), each followed by its metrics.  No copy and no wait
  // inside the loop: stream order makes the reuse of a batch's scratch safe
  TopNSink sink;
  sink.on_batch = [&](int64_t b0, int64_t nb) {
    launch_rank_metrics(s.stream, s.rec_ids.as<int32_t>(), s.rec_counts.as<int32_t>(), static_cast<int>(nb), top_n,
                        s.rk_goff.as<int64_t>() + b0, s.rk_gent.as<int32_t>(), s.rk_tab.as<double>(),
                        s.rk_met.as<double>() + b0 * MF_RANK_NMETRICS, s.rk_cnt.as<int64_t>() + b0 * 2);
  };
  recommend_scored(ctx, s, TopNQueries::of_side(ctx, s, qside, nq), TopNCandidates::of_side(ctx, cside), top_n,
                   MF_METRIC_DOT,
                   sv.any ? ExclSource::seen(sv, s.seen.qbeg, s.seen.qend)
                          : ExclSource::csr(s.rec_eoff.as<int64_t>(), s.rec_erows.as<int32_t>()),
                   sink);
  launch_rank_reduce(s.stream, s.rk_met.as<double>(), s.rk_cnt.as<int64_t>(), nq, part, ipart, sums, isums);
  MF_HIP(hipGetLastError());
  MF_HIP(hipStreamSynchronize(s.stream));
  clk.lap("rank_eval: batch loop");

  double hs[MF_RANK_NMETRICS + 2];
  MF_HIP(hipMemcpy(hs, sums, sizeof(hs), hipMemcpyDeviceToHost));
  int64_t hi[2];
  std::memcpy(hi, hs + MF_RANK_NMETRICS, sizeof(hi));
  const double dn = static_cast<double>(nq);
  out->hits = hi[0];
  out->gt_pairs = hi[1];
  out->precision = hs[0] / dn;
  out->recall = hs[1] / dn;
  out->map = hs[2] / dn;
  out->ndcg = hs[3] / dn;
  out->mrr = hs[4] / dn;
  out->hit_rate = hs[5] / dn;
  if (q_ids_out) {
    // device rows are in ascending factor-row order; the caller's in ascending id
    std::vector<int32_t> rows(nq), order(nq);
    std::vector<int64_t> cnt(static_cast<size_t>(nq) * 2);
    std::vector<double> met(static_cast<size_t>(nq) * MF_RANK_NMETRICS);
    MF_HIP(hipMemcpy(rows.data(), s.rec_q.get(), static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost));
    MF_HIP(hipMemcpy(cnt.data(), s.rk_cnt.get(), cnt.size() * 8, hipMemcpyDeviceToHost));
    MF_HIP(hipMemcpy(met.data(), s.rk_met.get(), met.size() * 8, hipMemcpyDeviceToHost));
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(),
              [&](int32_t a, int32_t b) { return QS.row_id[rows[a]] < QS.row_id[rows[b]]; });
    for (int64_t x = 0; x < nq; ++x) {
      const int32_t p = order[x];
      q_ids_out[x] = QS.row_id[rows[p]];
      q_counts_out[2 * x] = static_cast<int32_t>(cnt[2 * static_cast<size_t>(p)]);
      q_counts_out[2 * x + 1] = static_cast<int32_t>(cnt[2 * static_cast<size_t>(p) + 1]);
      std::memcpy(q_metrics_out + x * MF_RANK_NMETRICS, met.data() + static_cast<size_t>(p) * MF_RANK_NMETRICS,
                  MF_RANK_NMETRICS * 8);
    }
  }
  clk.lap("rank_eval: results");
}

void debug_rank_csr(mf_ctx* ctx, int qside, bool gt, const int32_t* q, const int32_t* c, int64_t n, int32_t* q_ids_out,
                    int64_t* off_out, int32_t* entries_out, int64_t cap_q, int64_t cap_e, int64_t* nq_out,
                    int64_t* ne_out) {
  Shard& s = ctx->shards[0];
  consolidate(ctx, s);
  sync_all(ctx);
  const SideLayout& QS = side_of(ctx, qside);
  const SideLayout& CS = side_of(ctx, 1 - qside);
  DeviceGuard g(s.device);
  *nq_out = *ne_out = 0;
  off_out[0] = 0;
  if (n == 0) return;
  std::vector<uint32_t> qr;
  DevBuf *off = &s.rk_goff, *ent = &s.rk_gent;
  const int64_t nq = build_truth(s, QS, q, c, n, qr);
  if (!gt) {
    build_exclusions(s, QS, CS, q, c, n, nq);
    off = &s.rec_eoff;
    ent = &s.rec_erows;
  }
  MF_HIP(hipStreamSynchronize(s.stream));
  int64_t m = 0;
  MF_HIP(hipMemcpy(&m, off->as<int64_t>() + nq, 8, hipMemcpyDeviceToHost));
  *nq_out = nq;
  *ne_out = m;
  if (cap_q < nq || cap_e < m) fail(MF_ERR_CAPACITY, "output capacity too small");
  std::vector<int32_t> rows(nq);
  if (nq > 0) MF_HIP(hipMemcpy(rows.data(), s.rec_q.get(), static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost));
  for (int64_t x = 0; x < nq; ++x) q_ids_out[x] = QS.row_id[rows[x]];
  MF_HIP(hipMemcpy(off_out, off->get(), static_cast<size_t>(nq + 1) * 8, hipMemcpyDeviceToHost));
  if (m > 0) MF_HIP(hipMemcpy(entries_out, ent->get(), static_cast<size_t>(m) * 4, hipMemcpyDeviceToHost));
}

}  // namespace mfhip
