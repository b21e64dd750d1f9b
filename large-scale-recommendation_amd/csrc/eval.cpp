// eval.cpp -- reading the model out: evaluation (mf_predict / mf_rmse / mf_empirical_risk) and the factor
// read-outs (mf_get_factors, mf_lookup).  The top-N lists are recommend.cpp's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "context.hpp"
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
