// pair_rank.cpp -- the rank of given (query, candidate) pairs in the query's complete list
// (mf_pair_ranks) and the prequential evaluation of an online micro-batch built on it
// (mf_online_prequential): ids resolved on the host, everything after that on the device
// (kernels_pairrank.hip for the targets, the score-and-count walk, the exclusion subtraction and the
// per-event metrics; kernels_rank.hip for the exclusion table and the fixed-order sums), on shard 0 like
// recommend().
//
// Exclusions are subtracted, not tested in the walk: the walk counts every candidate row that beats the
// target, and a second small kernel scores only the query's excluded rows and takes those that beat it
// off again.  The table is rank_eval's: rank_query_set over the pairs' query rows gives
// every row's position, rank_pair_csr the sorted distinct excluded rows per position.
//
// Pairs are walked in batches (MFHIP_TEST pr_batch=B; pr_split=S the candidate splits, pr_nw=1|2|4 the
// waves per workgroup of the f32 walk); the loop holds no copy and no host wait, and a rank depends on
// none of the three.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "context.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mfhip {

int64_t pair_ranks(mf_ctx* ctx, int qside, const int32_t* q, const int32_t* c, int64_t n, const int32_t* eq,
                   const int32_t* ec, int64_t ne, int32_t* rank_out, int32_t* valid_out, double* score_out,
                   bool seen) {
  if (n == 0) return 0;
  if (seen) ne = 0;  // the resident set stands in for the call's own table (below)
  MF_REQUIRE(n < (int64_t{1} << 31) - 1, "mf_pair_ranks: fewer than 2^31 - 1 pairs per call");
  Shard& s = ctx->shards[0];
  consolidate(ctx, s);
  sync_all(ctx);  // a run may still be sweeping (mf_dsgd_run returns early)
  PhaseClock clk;
  const int cside = 1 - qside;
  const SideLayout& QS = side_of(ctx, qside);
  const SideLayout& CS = side_of(ctx, cside);
  const int64_t C = CS.rows();
  const int k = ctx->P.num_factors;

  std::vector<uint32_t> qr, cr;
  lookup_rows(QS, q, n, qr);
  lookup_rows(CS, c, n, cr);
  std::atomic<int64_t> cold_sum{0};
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    int64_t m = 0;
    for (int64_t j = b; j < e; ++j) m += (qr[j] == kRowMiss || cr[j] == kRowMiss) ? 1 : 0;
    cold_sum += m;
  });
  const int64_t cold = cold_sum.load();
  if (cold == n) {  // nothing to rank: the device is not needed (a side may hold no row at all)
    if (rank_out) std::fill(rank_out, rank_out + n, MF_PAIR_RANK_COLD);
    if (valid_out) std::fill(valid_out, valid_out + n, 0);
    if (score_out) std::fill(score_out, score_out + n, 0.0);
    return cold;
  }

  DeviceGuard g(s.device);
  MF_HIP(hipStreamSynchronize(s.stream));  // an earlier call may still read the buffers
  s.pr_in.alloc(static_cast<size_t>(n) * 8);
  uint32_t* d_q = s.pr_in.as<uint32_t>();
  uint32_t* d_c = d_q + n;
  MF_HIP(hipMemcpy(d_q, qr.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
  MF_HIP(hipMemcpy(d_c, cr.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));

  // the seen set is keyed by factor row: a row's position in it is the row itself, and nothing is built
  const SeenView sv = seen ? seen_view(ctx, s, qside) : SeenView{};
  // the exclusion table over the distinct query rows of the pairs
  const uint32_t rows = static_cast<uint32_t>(QS.rows());
  if (!sv.any) {
    const int64_t nq = rank_query_set(s.stream, s.rank_sc, d_q, n, rows, s.rec_q);
    if (ne > 0) {
      std::vector<uint32_t> er_q, er_c;
      lookup_rows(QS, eq, ne, er_q);
      lookup_rows(CS, ec, ne, er_c);
      MF_HIP(hipStreamSynchronize(s.stream));
      s.rk_in.alloc(static_cast<size_t>(ne) * 8);
      MF_HIP(hipMemcpy(s.rk_in.get(), er_q.data(), static_cast<size_t>(ne) * 4, hipMemcpyHostToDevice));
      MF_HIP(hipMemcpy(s.rk_in.as<uint32_t>() + ne, er_c.data(), static_cast<size_t>(ne) * 4, hipMemcpyHostToDevice));
    } else {
      s.rk_in.alloc(8);
    }
    const uint32_t* ein = s.rk_in.as<uint32_t>();
    rank_pair_csr(s.stream, s.rank_sc, ein, ein + ne, ne, rows, nq, false, s.rec_eoff, s.rec_erows);
  }
  if (clk.on) MF_HIP(hipStreamSynchronize(s.stream));
  clk.lap("pair_ranks: tables");

  sync_row_ids(ctx, s, cside);
  const size_t ob = pair_rank_ord_bytes(ctx->f64);
  s.pr_ord.alloc(static_cast<size_t>(n) * ob);
  s.pr_tid.alloc(static_cast<size_t>(n) * 4);
  s.pr_rank.alloc(static_cast<size_t>(n) * 4);
  s.pr_valid.alloc(static_cast<size_t>(n) * 4);
  s.pr_score.alloc(static_cast<size_t>(n) * 8);
  const void* Q = qside == kSideU ? s.uf.get() : s.itf.get();
  const void* Cf = cside == kSideU ? s.uf.get() : s.itf.get();
  const int32_t* cand_id = s.rec_id[cside].as<int32_t>();
  const int32_t* qpos = sv.any ? sv.iota : s.rank_sc.pos.as<int32_t>();
  const int64_t* eoff = sv.any ? sv.off : s.rec_eoff.as<int64_t>();
  const int32_t* erows = sv.any ? sv.ent : s.rec_erows.as<int32_t>();
  launch_pair_targets(s.stream, Q, Cf, d_q, d_c, n, static_cast<int32_t>(C), k, ctx->f64, cand_id, qpos, eoff, erows,
                      s.pr_ord.get(), s.pr_tid.as<uint32_t>(), s.pr_rank.as<int32_t>(), s.pr_valid.as<int32_t>(),
                      s.pr_score.as<double>());

  // batches and candidate splits, sized as recommend()'s (topn_shape)
  int nw = 4;
  if (const std::string v = test_knob("pr_nw"); !v.empty()) nw = std::atoi(v.c_str());
  nw = nw >= 4 ? 4 : nw >= 2 ? 2 : 1;
  const TopNShape sh = topn_shape(n, C, pair_rank_tile(ctx->f64, nw), 32768, "pr_batch", "pr_split");
  const int64_t batch = sh.batch, S = sh.S;
  // no copy and no wait inside the loop
  for (int64_t b0 = 0; b0 < n; b0 += batch) {
    const int64_t nb = std::min(batch, n - b0);
    launch_pair_count(s.stream, Q, Cf, d_q + b0, static_cast<int>(nb), static_cast<int32_t>(C), static_cast<int>(S), k,
                      ctx->f64, nw, cand_id, qpos, eoff, erows, sv.any || ne > 0,
                      s.pr_ord.as<char>() + static_cast<size_t>(b0) * ob, s.pr_tid.as<uint32_t>() + b0,
                      s.pr_rank.as<int32_t>() + b0);
  }
  MF_HIP(hipGetLastError());
  MF_HIP(hipStreamSynchronize(s.stream));
  clk.lap("pair_ranks: batch loop");
  if (rank_out) MF_HIP(hipMemcpy(rank_out, s.pr_rank.get(), static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  if (valid_out) MF_HIP(hipMemcpy(valid_out, s.pr_valid.get(), static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  if (score_out) MF_HIP(hipMemcpy(score_out, s.pr_score.get(), static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost));
  return cold;
}

// Step 1: the events' ranks (pair_ranks), their metrics and the fixed-order sums, all complete before
// step 2, the online update, queues its first kernel.
namespace {
void prequential_ranks(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, int32_t top_n, const int32_t* eu,
                       const int32_t* ei, int64_t ne, mf_prequential* out, int32_t* rank_out, bool seen = false) {
  *out = mf_prequential{};
  out->events = n;
  out->cold = n;
  if (n > 0 && !ctx->have_model) {
    if (rank_out) std::fill(rank_out, rank_out + n, MF_PAIR_RANK_COLD);
  } else if (n > 0) {
    out->cold = pair_ranks(ctx, kSideU, u, i, n, eu, ei, ne, rank_out, nullptr, nullptr, seen);
    if (out->cold < n) {  // the ranks are on the device
      Shard& s = ctx->shards[0];
      DeviceGuard g(s.device);
      const std::vector<double>& tab = gain_table();
      s.rk_tab.alloc(tab.size() * 8);
      MF_HIP(hipMemcpyAsync(s.rk_tab.get(), tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s.stream));
      const int64_t slices = rank_reduce_slices(n);
      s.rk_met.alloc(static_cast<size_t>(n) * MF_RANK_NMETRICS * 8);
      s.rk_cnt.alloc(static_cast<size_t>(n) * 2 * 8);
      s.rk_part.alloc(static_cast<size_t>(slices) * (MF_RANK_NMETRICS + 2) * 8);
      s.rk_res.alloc((MF_RANK_NMETRICS + 2) * 8);
      double* part = s.rk_part.as<double>();
      int64_t* ipart = reinterpret_cast<int64_t*>(part + slices * MF_RANK_NMETRICS);
      double* sums = s.rk_res.as<double>();
      int64_t* isums = reinterpret_cast<int64_t*>(sums + MF_RANK_NMETRICS);
      launch_pair_metrics(s.stream, s.pr_rank.as<int32_t>(), s.pr_valid.as<int32_t>(), n, top_n, s.rk_tab.as<double>(),
                          s.rk_met.as<double>(), s.rk_cnt.as<int64_t>());
      launch_rank_reduce(s.stream, s.rk_met.as<double>(), s.rk_cnt.as<int64_t>(), n, part, ipart, sums, isums);
      MF_HIP(hipGetLastError());
      MF_HIP(hipStreamSynchronize(s.stream));
      double hs[MF_RANK_NMETRICS + 2];
      MF_HIP(hipMemcpy(hs, sums, sizeof(hs), hipMemcpyDeviceToHost));
      int64_t hi[2];
      std::memcpy(hi, hs + MF_RANK_NMETRICS, sizeof(hi));
      out->hits = hi[0];
      out->evaluated = hi[1];
      out->sum_ndcg = hs[0];
      out->sum_rr = hs[1];
      out->sum_pr = hs[2];
    }
  }
  out->excluded = n - out->evaluated - out->cold;
  if (out->evaluated > 0) {
    const double de = static_cast<double>(out->evaluated);
    out->ndcg = out->sum_ndcg / de;
    out->mrr = out->sum_rr / de;
    out->hit_rate = static_cast<double>(out->hits) / de;
    out->mpr = out->sum_pr / de;
  }
}
}  // namespace

void online_prequential(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                        int num_partitions, int32_t top_n, const int32_t* eu, const int32_t* ei, int64_t ne,
                        mf_prequential* out, int32_t* rank_out, int64_t* tu, int64_t* ti) {
  prequential_ranks(ctx, u, i, n, top_n, eu, ei, ne, out, rank_out);
  online_update(ctx, u, i, r, n, flavour, num_partitions, tu, ti);
}

void online_prequential_sampled(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                                int flavour, int32_t top_n, const int32_t* eu, const int32_t* ei, int64_t ne,
                                const NegSampling& neg, int32_t* sampled_out, mf_prequential* out, int32_t* rank_out,
                                int64_t* tu, int64_t* ti) {
  prequential_ranks(ctx, u, i, n, top_n, eu, ei, ne, out, rank_out);
  online_update_sampled(ctx, u, i, r, n, flavour, neg, sampled_out, tu, ti);
}

void online_prequential_seen(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                             int32_t top_n, const NegSampling& neg, int32_t* sampled_out, mf_prequential* out,
                             int32_t* rank_out, int64_t* tu, int64_t* ti, bool add_events) {
  prequential_ranks(ctx, u, i, n, top_n, nullptr, nullptr, 0, out, rank_out, true);
  online_update_sampled(ctx, u, i, r, n, flavour, neg, sampled_out, tu, ti);
  // every id of the batch has a row now: its events are seen from the next batch on
  if (add_events) seen_put(ctx, u, i, n, true, nullptr);
}

}  // namespace mfhip
