// abi.cpp -- the C ABI of libmfhip.so: every entry point of include/mfhip.h and
// include/mfhip_testing.h, as a thin wrapper that checks its arguments and calls the feature's
// function (mfhip.cpp, dsgd_det.cpp, dsgd_fast.cpp, ring.cpp, online.cpp, eval.cpp, rank_eval.cpp,
// pair_rank.cpp, als.cpp, declared in context.hpp; placement.cpp, declared in plan.hpp) under `guarded`.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "bpr_draw.hpp"
#include "common.hpp"
#include "context.hpp"
#include "jvm_random.hpp"
#include "kernels.hpp"
#include "neg_sample.hpp"
#include "plan.hpp"

using namespace mfhip;

extern "C" {

void mf_params_init(mf_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->num_factors = 10;        // MatrixFactorization.scala:201-203
  p->iterations = 10;         // :209-211
  p->lambda = 1.0;            // :205-207
  p->learning_rate = 0.001;   // DSGDforMF.scala:163-165
  p->lr_method = MF_LR_DEFAULT;  // :167-169
  p->lr_arg = 0.0;
  p->num_blocks = 1;          // Blocks None -> getOrElse(1) (:270)
  p->seed = 0;                // Seed Some(0L) (:217-219)
  p->has_seed = 1;
  p->mode = MF_MODE_DETERMINISTIC_F64;
  p->online_learning_rate = 0.01;  // SparkExample.scala:33 SGDUpdater(0.01)
  p->online_init = MF_INIT_PSEUDO_RANDOM;
  p->fast_waves = 0;
}

const char* mf_last_error(void) { return g_last_error.c_str(); }
const char* mf_version(void) { return "mfhip 0.1.0 (gfx950)"; }

int mf_device_count(int* n) {
  return guarded([&] {
    MF_REQUIRE(n, "null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = (e == hipSuccess) ? c : 0;
  });
}

int mf_create(const mf_params* p, const int* device_ids, int n_devices, mf_ctx** out) {
  return guarded([&] {
    MF_REQUIRE(out, "out is null");
    *out = nullptr;
    *out = create_ctx(p, device_ids, n_devices);
  });
}

int mf_comm_unique_id(uint8_t uid_out[MF_UID_BYTES]) {
  return guarded([&] {
    MF_REQUIRE(uid_out, "null");
    static_assert(sizeof(ncclUniqueId) <= MF_UID_BYTES, "uid size");
    ncclUniqueId id;
    MF_NCCL(ncclGetUniqueId(&id));
    std::memset(uid_out, 0, MF_UID_BYTES);
    std::memcpy(uid_out, &id, sizeof(id));
  });
}

int mf_create_rank(const mf_params* p, int device_id, int nranks, int rank, const uint8_t uid[MF_UID_BYTES],
                   mf_ctx** out) {
  return guarded([&] {
    MF_REQUIRE(out && uid, "null argument");
    *out = nullptr;
    *out = create_rank_ctx(p, device_id, nranks, rank, uid);
  });
}

int mf_destroy(mf_ctx* ctx) {
  return guarded([&] {
    if (ctx) destroy_ctx(ctx);
  });
}

int mf_dsgd_prepare(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    prepare(ctx, u, i, r, n);
  });
}

int mf_dsgd_run(mf_ctx* ctx, int64_t supersteps) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(supersteps >= 0, "negative superstep count");
    run_supersteps(ctx, supersteps);
  });
}

int mf_dsgd_superstep(mf_ctx* ctx, int64_t* done) {
  return guarded([&] {
    MF_REQUIRE(ctx && done, "null argument");
    *done = ctx->superstep_done;
  });
}

int mf_dsgd_set_superstep(mf_ctx* ctx, int64_t done) {
  return guarded([&] {
    MF_REQUIRE(ctx && done >= 0, "bad argument");
    MF_REQUIRE(ctx->prepared, "mf_dsgd_set_superstep before mf_dsgd_prepare");
    det_spec_wait(ctx, true);
    sync_all(ctx);
    ctx->superstep_done = done;
    reset_item_loc(ctx);
  });
}

int mf_dsgd_restart(mf_ctx* ctx) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(ctx->prepared, "mf_dsgd_restart before mf_dsgd_prepare");
    det_spec_wait(ctx, true);
    ctx->failed.clear();
    sync_all(ctx);
    init_factors(ctx);
    ctx->superstep_done = 0;
    reset_item_loc(ctx);
  });
}

int mf_sync(mf_ctx* ctx) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    sync_all(ctx);
  });
}

int mf_dsgd_fit(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    prepare(ctx, u, i, r, n);
    run_supersteps(ctx, static_cast<int64_t>(ctx->P.iterations) * ctx->nb);
    sync_all(ctx);
  });
}

int mf_num_factors(mf_ctx* ctx, int side, int64_t* count) {
  return guarded([&] {
    MF_REQUIRE(ctx && count, "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    const SideLayout& S = side_of(ctx, side);
    if (!ctx->rank_mode || side == MF_SIDE_ITEM || !ctx->prepared) { *count = S.rows(); return; }
    const int me = ctx->shards[0].index;
    *count = S.block_start[(me + 1) * ctx->c] - S.block_start[me * ctx->c];
  });
}

int mf_get_factors(mf_ctx* ctx, int side, int32_t* ids, double* vecs, int64_t cap, int64_t* written) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    get_factors(ctx, side, ids, vecs, cap, written);
  });
}

int mf_set_factors(mf_ctx* ctx, int side, const int32_t* ids, const double* vecs, int64_t n) {
  return guarded([&] {
    MF_REQUIRE(ctx && (n == 0 || (ids && vecs)), "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    set_factors(ctx, side, ids, vecs, n);
  });
}

int mf_get_params(mf_ctx* ctx, mf_params* out) {
  return guarded([&] {
    MF_REQUIRE(ctx && out, "null argument");
    *out = ctx->P;
  });
}

int mf_predict(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, double* out, uint8_t* found) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(n == 0 || (u && i && out && found), "null argument");
    evaluate(ctx, u, i, nullptr, n, nullptr, 0.0, out, found);
  });
}

int mf_rmse(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, double* rmse,
            int64_t* matched) {
  return guarded([&] {
    MF_REQUIRE(ctx && rmse, "null argument");
    MF_REQUIRE(n == 0 || (u && i && r), "null argument");
    EvalOut e = evaluate(ctx, u, i, r, n, nullptr, 0.0, nullptr, nullptr);
    *rmse = e.cnt > 0 ? std::sqrt(e.sse / e.cnt) : std::nan("");
    if (matched) *matched = static_cast<int64_t>(e.cnt);
  });
}

int mf_empirical_risk(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                      double lambda, double* risk) {
  return guarded([&] {
    MF_REQUIRE(ctx && risk, "null argument");
    MF_REQUIRE(n == 0 || (u && i && r), "null argument");
    // the (user, item)-keyed join multiplies duplicate pairs (MatrixFactorization.scala:175)
    std::vector<uint64_t> key(n);
    for (int64_t j = 0; j < n; ++j)
      key[j] = (static_cast<uint64_t>(static_cast<uint32_t>(u[j])) << 32) | static_cast<uint32_t>(i[j]);
    std::vector<uint64_t> sorted = key;
    std::sort(sorted.begin(), sorted.end());
    std::vector<int32_t> mult(n);
    for (int64_t j = 0; j < n; ++j) {
      auto rg = std::equal_range(sorted.begin(), sorted.end(), key[j]);
      mult[j] = static_cast<int32_t>(rg.second - rg.first);
    }
    EvalOut e = evaluate(ctx, u, i, r, n, mult.data(), lambda, nullptr, nullptr);
    *risk = e.risk;
  });
}

int mf_recommend(mf_ctx* ctx, int query_side, const int32_t* queries, int64_t n_queries, int32_t top_n,
                 const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl, int32_t* ids_out,
                 double* scores_out, int32_t* counts_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(query_side == MF_SIDE_USER || query_side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n_queries >= 0 && n_excl >= 0, "negative count");
    MF_REQUIRE(n_excl == 0 || (excl_query && excl_cand), "null exclusion list");
    if (ctx->rank_mode)
      fail(MF_ERR_STATE, "mf_recommend runs on a single-process context; a rank-mode context (mf_create_rank) "
                         "holds only its own users' rows");
    if (!ctx->have_model)
      fail(MF_ERR_NOT_FITTED, "The MatrixFactorization model has not been fitted to data. "
                              "Prior to predicting values, it has to be trained on data.");
    require_healthy(ctx);
    if (n_queries == 0) return;
    MF_REQUIRE(queries && ids_out && counts_out, "null argument");
    recommend(ctx, query_side, queries, n_queries, top_n, excl_query, excl_cand, n_excl, ids_out, scores_out,
              counts_out);
  });
}

namespace {
// the checks mf_similar and mf_recommend_vectors share with mf_recommend
void top_list_check(mf_ctx* ctx, int side, int32_t top_n, int32_t metric, int64_t n_queries, int64_t n_excl,
                    const char* who) {
  MF_REQUIRE(ctx, "null context");
  MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
  MF_REQUIRE(metric == MF_METRIC_DOT || metric == MF_METRIC_COSINE, "bad metric");
  MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
             "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
  MF_REQUIRE(n_queries >= 0 && n_excl >= 0, "negative count");
  if (ctx->rank_mode)
    fail(MF_ERR_STATE, std::string(who) + " runs on a single-process context; a rank-mode context (mf_create_rank) "
                                          "holds only its own users' rows");
  if (!ctx->have_model)
    fail(MF_ERR_NOT_FITTED, "The MatrixFactorization model has not been fitted to data. "
                            "Prior to predicting values, it has to be trained on data.");
  require_healthy(ctx);
}
}  // namespace

int mf_similar(mf_ctx* ctx, int side, const int32_t* queries, int64_t n_queries, int32_t top_n, int32_t metric,
               int32_t include_self, const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl,
               int32_t* ids_out, double* scores_out, int32_t* counts_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(include_self == 0 || include_self == 1, "include_self must be 0 or 1");
    top_list_check(ctx, side, top_n, metric, n_queries, n_excl, "mf_similar");
    MF_REQUIRE(n_excl == 0 || (excl_query && excl_cand), "null exclusion list");
    if (n_queries == 0) return;
    MF_REQUIRE(queries && ids_out && counts_out, "null argument");
    similar(ctx, side, queries, n_queries, top_n, metric, include_self != 0, excl_query, excl_cand, n_excl, ids_out,
            scores_out, counts_out);
  });
}

int mf_recommend_vectors(mf_ctx* ctx, int cand_side, const double* vecs, int64_t n_queries, int32_t top_n,
                         int32_t metric, const int64_t* excl_query_index, const int32_t* excl_cand, int64_t n_excl,
                         int32_t* ids_out, double* scores_out, int32_t* counts_out) {
  return guarded([&] {
    top_list_check(ctx, cand_side, top_n, metric, n_queries, n_excl, "mf_recommend_vectors");
    MF_REQUIRE(n_excl == 0 || (excl_query_index && excl_cand), "null exclusion list");
    if (n_queries == 0) return;
    MF_REQUIRE(vecs && ids_out && counts_out, "null argument");
    recommend_vectors(ctx, cand_side, vecs, n_queries, top_n, metric, excl_query_index, excl_cand, n_excl, ids_out,
                      scores_out, counts_out);
  });
}

namespace {
// the checks mf_rank_eval and its testing hook share with mf_recommend
void rank_check(mf_ctx* ctx, int query_side, const char* who) {
  MF_REQUIRE(ctx, "null context");
  MF_REQUIRE(query_side == MF_SIDE_USER || query_side == MF_SIDE_ITEM, "bad side");
  if (ctx->rank_mode)
    fail(MF_ERR_STATE, std::string(who) + " runs on a single-process context; a rank-mode context (mf_create_rank) "
                                          "holds only its own users' rows");
  if (!ctx->have_model)
    fail(MF_ERR_NOT_FITTED, "The MatrixFactorization model has not been fitted to data. "
                            "Prior to predicting values, it has to be trained on data.");
  require_healthy(ctx);
}
}  // namespace

int mf_recommend_among(mf_ctx* ctx, int query_side, const int32_t* queries, int64_t n_queries, int32_t top_n,
                       const int64_t* offsets, const int32_t* cand_ids, int64_t n_cand, int32_t exclude_seen,
                       const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl, int32_t* ids_out,
                       double* scores_out, int32_t* counts_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(query_side == MF_SIDE_USER || query_side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n_queries >= 0 && n_cand >= 0 && n_excl >= 0, "negative count");
    MF_REQUIRE(n_queries < (int64_t{1} << 31), "n_queries must be below 2^31");
    MF_REQUIRE(n_cand < (int64_t{1} << 31), "n_cand must be below 2^31");
    MF_REQUIRE(exclude_seen == 0 || exclude_seen == 1, "exclude_seen must be 0 or 1");
    MF_REQUIRE(exclude_seen == 0 || n_excl == 0, "n_excl must be 0 with exclude_seen = 1: the seen set is the exclusion list");
    MF_REQUIRE(n_excl == 0 || (excl_query && excl_cand), "null exclusion list");
    MF_REQUIRE(n_queries == 0 || (queries && ids_out && counts_out), "null argument: queries, ids_out and counts_out");
    MF_REQUIRE(n_cand == 0 || cand_ids, "null argument: cand_ids");
    if (offsets) {
      MF_REQUIRE(offsets[0] == 0, "offsets[0] must be 0");
      for (int64_t j = 0; j < n_queries; ++j)
        MF_REQUIRE(offsets[j + 1] >= offsets[j], "offsets must not decrease (at query " + std::to_string(j) + ")");
      MF_REQUIRE(offsets[n_queries] == n_cand, "offsets[n_queries] must equal n_cand");
    }
    rank_check(ctx, query_side, "mf_recommend_among");
    if (n_queries == 0) return;
    recommend_among(ctx, query_side, queries, n_queries, top_n, offsets, cand_ids, n_cand, exclude_seen != 0, excl_query,
                    excl_cand, n_excl, ids_out, scores_out, counts_out);
  });
}

int mf_rank_eval(mf_ctx* ctx, int query_side, const int32_t* gt_query, const int32_t* gt_cand, int64_t n_gt,
                 int32_t top_n, const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl,
                 mf_rank_metrics* out, int32_t* q_ids_out, int32_t* q_counts_out, double* q_metrics_out, int64_t cap) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(out, "out is null");
    MF_REQUIRE(query_side == MF_SIDE_USER || query_side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n_gt >= 0 && n_excl >= 0, "negative count");
    MF_REQUIRE(n_gt == 0 || (gt_query && gt_cand), "null ground-truth list");
    MF_REQUIRE(n_excl == 0 || (excl_query && excl_cand), "null exclusion list");
    const int given = (q_ids_out != nullptr) + (q_counts_out != nullptr) + (q_metrics_out != nullptr);
    MF_REQUIRE(given == 0 || given == 3, "per-query outputs: give all three arrays or none");
    MF_REQUIRE(given == 0 || cap >= 0, "negative count");
    rank_check(ctx, query_side, "mf_rank_eval");
    rank_eval(ctx, query_side, gt_query, gt_cand, n_gt, top_n, excl_query, excl_cand, n_excl, out, q_ids_out,
              q_counts_out, q_metrics_out, cap);
  });
}

int mf_pair_ranks(mf_ctx* ctx, int query_side, const int32_t* queries, const int32_t* cands, int64_t n,
                  const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl, int32_t* rank_out,
                  int32_t* valid_out, double* score_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(query_side == MF_SIDE_USER || query_side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(n >= 0 && n_excl >= 0, "negative count");
    MF_REQUIRE(n == 0 || (queries && cands && rank_out), "null argument");
    MF_REQUIRE(n_excl == 0 || (excl_query && excl_cand), "null exclusion list");
    rank_check(ctx, query_side, "mf_pair_ranks");
    pair_ranks(ctx, query_side, queries, cands, n, excl_query, excl_cand, n_excl, rank_out, valid_out, score_out);
  });
}

int mf_online_prequential(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                          int num_partitions, int32_t top_n, const int32_t* excl_user, const int32_t* excl_item,
                          int64_t n_excl, mf_prequential* out, int32_t* rank_out, int64_t* touched_users,
                          int64_t* touched_items) {
  return guarded([&] {
    // everything mf_online_update would refuse is refused here, before the model is touched
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(out, "out is null");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n >= 0 && n_excl >= 0, "negative count");
    MF_REQUIRE(n == 0 || (u && i && r), "bad rating arrays");
    MF_REQUIRE(n_excl == 0 || (excl_user && excl_item), "null exclusion list");
    if (ctx->rank_mode)
      fail(MF_ERR_STATE, "mf_online_prequential runs on a single-process context; a rank-mode context "
                         "(mf_create_rank) holds only its own users' rows");
    MF_REQUIRE(ctx->shards.size() == 1, "online updates run on a single-device context");
    MF_REQUIRE(flavour >= MF_ONLINE_NEXT_FACTORS && flavour <= MF_ONLINE_SPARK_SWEEP, "unknown online flavour");
    if (flavour == MF_ONLINE_SPARK_SWEEP && n > 0) {
      MF_REQUIRE(num_partitions >= 1, "num_partitions must be >= 1 for MF_ONLINE_SPARK_SWEEP");
      for (int64_t j = 0; j < n; ++j)
        MF_REQUIRE(u[j] >= 0 && i[j] != INT32_MIN, "Spark sweep needs non-negative user ids");
    }
    require_healthy(ctx);
    det_spec_wait(ctx, true);  // new ids change the layouts the builds read
    online_prequential(ctx, u, i, r, n, flavour, num_partitions, top_n, excl_user, excl_item, n_excl, out, rank_out,
                       touched_users, touched_items);
  });
}

int mf_online_prequential_sampled(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                                  int flavour, int32_t top_n, const int32_t* excl_user, const int32_t* excl_item,
                                  int64_t n_excl, mf_prequential* out, int32_t* rank_out, int64_t* touched_users,
                                  int64_t* touched_items, int32_t negatives, double negative_rating, int64_t seed,
                                  int64_t first_event, int32_t* sampled_items_out) {
  return guarded([&] {
    // everything mf_online_update_sampled would refuse is refused here, before the model is touched
    const NegSampling neg{negatives, negative_rating, seed, first_event};
    check_negative_sampling(neg);
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(out, "out is null");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n >= 0 && n_excl >= 0, "negative count");
    MF_REQUIRE(n == 0 || (u && i && r), "bad rating arrays");
    MF_REQUIRE(n_excl == 0 || (excl_user && excl_item), "null exclusion list");
    if (ctx->rank_mode)
      fail(MF_ERR_STATE, "mf_online_prequential_sampled runs on a single-process context; a rank-mode context "
                         "(mf_create_rank) holds only its own users' rows");
    MF_REQUIRE(ctx->shards.size() == 1, "online updates run on a single-device context");
    MF_REQUIRE(flavour >= MF_ONLINE_NEXT_FACTORS && flavour < MF_ONLINE_SPARK_SWEEP,
               "MF_ONLINE_NEXT_FACTORS or MF_ONLINE_DELTA: MF_ONLINE_SPARK_SWEEP has no sampled form");
    MF_REQUIRE(n < (int64_t{1} << 31) && n * (1 + negatives) < (int64_t{1} << 31),
               "a sampled batch holds fewer than 2^31 updates");
    require_healthy(ctx);
    det_spec_wait(ctx, true);  // new ids change the layouts the builds read
    online_prequential_sampled(ctx, u, i, r, n, flavour, top_n, excl_user, excl_item, n_excl, neg, sampled_items_out,
                               out, rank_out, touched_users, touched_items);
  });
}

int mf_debug_rank_csr(mf_ctx* ctx, int query_side, int ground_truth, const int32_t* query, const int32_t* cand,
                      int64_t n, int32_t* q_ids_out, int64_t* off_out, int32_t* entries_out, int64_t cap_q,
                      int64_t cap_e, int64_t* nq_out, int64_t* ne_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(nq_out && ne_out && q_ids_out && off_out && entries_out, "null argument");
    MF_REQUIRE(n >= 0 && cap_q >= 0 && cap_e >= 0, "negative count");
    MF_REQUIRE(n == 0 || (query && cand), "null pair list");
    rank_check(ctx, query_side, "mf_debug_rank_csr");
    debug_rank_csr(ctx, query_side, ground_truth != 0, query, cand, n, q_ids_out, off_out, entries_out, cap_q, cap_e,
                   nq_out, ne_out);
  });
}

// ---- the resident seen set and its four readers ----------------------------------------------------------
namespace {
// what the set calls share: a single-process context whose first shard holds the table
void seen_check(mf_ctx* ctx, const char* who) {
  MF_REQUIRE(ctx, "null context");
  if (ctx->rank_mode)
    fail(MF_ERR_STATE, std::string(who) + " runs on a single-process context; a rank-mode context (mf_create_rank) "
                                          "holds only its own users' rows");
}
int seen_put_entry(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, bool add, int64_t* ignored_out,
                   const char* who) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(n >= 0, "negative count");
    MF_REQUIRE(n == 0 || (u && i), "null pair list");
    MF_REQUIRE(n < (int64_t{1} << 31) - 1, "fewer than 2^31 - 1 pairs per call");
    seen_check(ctx, who);
    require_healthy(ctx);
    seen_put(ctx, u, i, n, add, ignored_out);
  });
}
}  // namespace

int mf_seen_set(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, int64_t* ignored_out) {
  return seen_put_entry(ctx, users, items, n, false, ignored_out, "mf_seen_set");
}

int mf_seen_add(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, int64_t* ignored_out) {
  return seen_put_entry(ctx, users, items, n, true, ignored_out, "mf_seen_add");
}

int mf_seen_remove(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, int64_t* removed_out,
                   int64_t* ignored_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(n >= 0, "negative count");
    MF_REQUIRE(n == 0 || (users && items), "null pair list");
    MF_REQUIRE(n < (int64_t{1} << 31) - 1, "fewer than 2^31 - 1 pairs per call");
    seen_check(ctx, "mf_seen_remove");
    require_healthy(ctx);
    seen_remove(ctx, users, items, n, removed_out, ignored_out);
  });
}

int mf_seen_from_als(mf_ctx* ctx) {
  return guarded([&] {
    seen_check(ctx, "mf_seen_from_als");
    seen_from_als(ctx);
  });
}

int mf_seen_clear(mf_ctx* ctx) {
  return guarded([&] {
    seen_check(ctx, "mf_seen_clear");
    seen_clear(ctx);
  });
}

int mf_seen_count(mf_ctx* ctx, int64_t* pairs) {
  return guarded([&] {
    MF_REQUIRE(ctx && pairs, "null argument");
    seen_check(ctx, "mf_seen_count");
    *pairs = seen_count(ctx);
  });
}

int mf_recommend_seen(mf_ctx* ctx, int query_side, const int32_t* queries, int64_t n_queries, int32_t top_n,
                      int32_t* ids_out, double* scores_out, int32_t* counts_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(query_side == MF_SIDE_USER || query_side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n_queries >= 0, "negative count");
    MF_REQUIRE(n_queries == 0 || (queries && ids_out && counts_out), "null argument");
    rank_check(ctx, query_side, "mf_recommend_seen");
    if (n_queries == 0) return;
    recommend(ctx, query_side, queries, n_queries, top_n, nullptr, nullptr, 0, ids_out, scores_out, counts_out, true);
  });
}

int mf_rank_eval_seen(mf_ctx* ctx, int query_side, const int32_t* gt_query, const int32_t* gt_cand, int64_t n_gt,
                      int32_t top_n, mf_rank_metrics* out, int32_t* q_ids_out, int32_t* q_counts_out,
                      double* q_metrics_out, int64_t cap) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(out, "out is null");
    MF_REQUIRE(query_side == MF_SIDE_USER || query_side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n_gt >= 0, "negative count");
    MF_REQUIRE(n_gt == 0 || (gt_query && gt_cand), "null ground-truth list");
    const int given = (q_ids_out != nullptr) + (q_counts_out != nullptr) + (q_metrics_out != nullptr);
    MF_REQUIRE(given == 0 || given == 3, "per-query outputs: give all three arrays or none");
    MF_REQUIRE(given == 0 || cap >= 0, "negative count");
    rank_check(ctx, query_side, "mf_rank_eval_seen");
    rank_eval(ctx, query_side, gt_query, gt_cand, n_gt, top_n, nullptr, nullptr, 0, out, q_ids_out, q_counts_out,
              q_metrics_out, cap, true);
  });
}

int mf_pair_ranks_seen(mf_ctx* ctx, int query_side, const int32_t* queries, const int32_t* cands, int64_t n,
                       int32_t* rank_out, int32_t* valid_out, double* score_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(query_side == MF_SIDE_USER || query_side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(n >= 0, "negative count");
    MF_REQUIRE(n == 0 || (queries && cands && rank_out), "null argument");
    rank_check(ctx, query_side, "mf_pair_ranks_seen");
    pair_ranks(ctx, query_side, queries, cands, n, nullptr, nullptr, 0, rank_out, valid_out, score_out, true);
  });
}

int mf_online_prequential_seen(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                               int32_t top_n, mf_prequential* out, int32_t* rank_out, int64_t* touched_users,
                               int64_t* touched_items, int32_t negatives, double negative_rating, int64_t seed,
                               int64_t first_event, int32_t* sampled_items_out, int add_events) {
  return guarded([&] {
    // everything mf_online_prequential_sampled would refuse is refused here, before anything changes
    const NegSampling neg{negatives, negative_rating, seed, first_event};
    check_negative_sampling(neg);
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(out, "out is null");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n >= 0, "negative count");
    MF_REQUIRE(n == 0 || (u && i && r), "bad rating arrays");
    if (ctx->rank_mode)
      fail(MF_ERR_STATE, "mf_online_prequential_seen runs on a single-process context; a rank-mode context "
                         "(mf_create_rank) holds only its own users' rows");
    MF_REQUIRE(ctx->shards.size() == 1, "online updates run on a single-device context");
    MF_REQUIRE(flavour >= MF_ONLINE_NEXT_FACTORS && flavour < MF_ONLINE_SPARK_SWEEP,
               "MF_ONLINE_NEXT_FACTORS or MF_ONLINE_DELTA: MF_ONLINE_SPARK_SWEEP has no sampled form");
    MF_REQUIRE(n < (int64_t{1} << 31) - 1 && n * (1 + negatives) < (int64_t{1} << 31),
               "a sampled batch holds fewer than 2^31 updates");
    require_healthy(ctx);
    det_spec_wait(ctx, true);  // new ids change the layouts the builds read
    online_prequential_seen(ctx, u, i, r, n, flavour, top_n, neg, sampled_items_out, out, rank_out, touched_users,
                            touched_items, add_events != 0);
  });
}

int mf_debug_seen_csr(mf_ctx* ctx, int side, int32_t* row_ids_out, int64_t* off_out, int32_t* entries_out,
                      int32_t* entry_ids_out, int64_t cap_rows, int64_t cap_nnz, int64_t* rows_out, int64_t* nnz_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && row_ids_out && off_out && entries_out && rows_out && nnz_out, "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(cap_rows >= 0 && cap_nnz >= 0, "negative count");
    seen_check(ctx, "mf_debug_seen_csr");
    seen_debug_csr(ctx, side, row_ids_out, off_out, entries_out, entry_ids_out, cap_rows, cap_nnz, rows_out, nnz_out);
  });
}

int mf_debug_seen_merge_placement(const uint64_t* old_keys, int64_t n_old, const uint64_t* batch_keys, int64_t n_batch,
                                  int64_t* old_pos_out, int64_t* novel_pos_out, int64_t* n_novel_out) {
  return guarded([&] {
    MF_REQUIRE(n_old >= 0 && n_batch >= 0, "negative count");
    MF_REQUIRE(n_novel_out && (n_old == 0 || (old_keys && old_pos_out)) && (n_batch == 0 || (batch_keys && novel_pos_out)),
               "null argument");
    seen_merge_placement(old_keys, n_old, batch_keys, n_batch, old_pos_out, novel_pos_out, n_novel_out);
  });
}

// ---- BPR training on the seen set ---------------------------------------------------------------------------
int mf_bpr_run(mf_ctx* ctx, const mf_bpr_params* params, int64_t first_step, int64_t steps, mf_bpr_stats* out) {
  return guarded([&] {
    MF_REQUIRE(ctx && params, "null argument");
    bpr_check_params(*params, true);
    bpr_check_steps(first_step, steps);
    bpr_run(ctx, *params, first_step, steps, out);
  });
}

int mf_bpr_step_triples(mf_ctx* ctx, const mf_bpr_params* params, const int32_t* users, const int32_t* pos_items,
                        const int32_t* neg_items, int64_t n, mf_bpr_stats* out) {
  return guarded([&] {
    MF_REQUIRE(ctx && params, "null argument");
    MF_REQUIRE(n >= 0, "negative count");
    MF_REQUIRE(n <= kBprMaxBatch, "at most 2^24 triples per step");
    MF_REQUIRE(n == 0 || (users && pos_items && neg_items), "null triple list");
    bpr_check_params(*params, false);
    bpr_step_triples(ctx, *params, users, pos_items, neg_items, n, out);
  });
}

int mf_bpr_draws(int64_t seed, int64_t step, int32_t batch, int32_t redraws, int64_t pairs, int64_t pool,
                 uint64_t* z_out) {
  return guarded([&] {
    MF_REQUIRE(batch >= 1 && batch <= kBprMaxBatch, "batch must lie in 1 .. 2^24");
    MF_REQUIRE(redraws >= 0 && redraws <= kBprMaxRedraws, "redraws must lie in 0 .. " + std::to_string(kBprMaxRedraws));
    MF_REQUIRE(step >= 0 && step < kBprMaxSteps, "step must lie in 0 .. 2^26 - 1");
    MF_REQUIRE(pairs >= 0, "negative pair count");
    MF_REQUIRE(pool >= 1 && pool <= (int64_t{1} << 31), "pool must be in [1, 2^31]");
    MF_REQUIRE(z_out, "null argument");
    const int per = 2 + redraws;
    for (int32_t s = 0; s < batch; ++s) {
      uint64_t* z = z_out + static_cast<size_t>(s) * per;
      const auto bits = [&](int r) {
        return bpr_draw_bits(static_cast<uint64_t>(seed), static_cast<uint64_t>(step), static_cast<uint32_t>(s),
                             static_cast<uint32_t>(r));
      };
      z[0] = bpr_entry(bits(0), static_cast<uint64_t>(pairs));
      for (int r = 1; r < per; ++r) z[r] = pool >= 2 ? bpr_neg_rank(bits(r), static_cast<uint32_t>(pool)) : 0;
    }
  });
}

int mf_bpr_fit(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, double init_scale,
               const mf_bpr_params* params, int64_t steps, mf_bpr_stats* out) {
  return guarded([&] {
    MF_REQUIRE(ctx && params, "null argument");
    MF_REQUIRE(n >= 0, "negative count");
    MF_REQUIRE(n == 0 || (users && items), "null pair list");
    MF_REQUIRE(n < (int64_t{1} << 31) - 1, "fewer than 2^31 - 1 pairs per call");
    MF_REQUIRE(std::isfinite(init_scale), "init_scale must be finite");
    bpr_check_params(*params, true);
    bpr_check_steps(0, steps);
    bpr_fit(ctx, users, items, n, init_scale, *params, steps, out);
  });
}

int mf_debug_bpr_triples(mf_ctx* ctx, int32_t* users_out, int32_t* pos_out, int32_t* neg_out, int64_t cap,
                         int64_t* n_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && n_out, "null argument");
    MF_REQUIRE(cap >= 0 && (cap == 0 || (users_out && pos_out && neg_out)), "null argument");
    bpr_debug_triples(ctx, users_out, pos_out, neg_out, cap, n_out);
  });
}

int mf_als_prepare(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    als_prepare(ctx, u, i, r, n);
  });
}

namespace {

// The cg_steps of a conjugate-gradient entry as AlsParams::cg_steps, where 0 selects Cholesky: the
// caller's 0 stays out of range.
int32_t als_cg_entry_steps(int32_t cg_steps) { return cg_steps == 0 ? -1 : cg_steps; }

int als_run_entry(mf_ctx* ctx, int64_t half_sweeps, const AlsParams& P) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    als_run(ctx, half_sweeps, P);
  });
}

// mf_als_fit and its variants: prepare + 2 * iterations half-sweeps, every argument checked first.
int als_fit_entry(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int32_t iterations,
                  const AlsParams& P) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    MF_REQUIRE(n >= 0 && iterations >= 0, "negative count");
    if (P.implicit) als_check_alpha(P.alpha);
    als_check_run(P);
    als_check(ctx);
    if (n == 0) return;
    als_prepare(ctx, u, i, r, n);
    als_run(ctx, 2 * static_cast<int64_t>(iterations), P);
  });
}

}  // namespace

int mf_als_run(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg) {
  return als_run_entry(ctx, half_sweeps, {lambda, reg});
}

int mf_als_fit(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int32_t iterations,
               double lambda, int32_t reg) {
  return als_fit_entry(ctx, u, i, r, n, iterations, {lambda, reg});
}

int mf_als_run_implicit(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg, double alpha) {
  return als_run_entry(ctx, half_sweeps, {lambda, reg, true, alpha});
}

int mf_als_fit_implicit(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                        int32_t iterations, double lambda, int32_t reg, double alpha) {
  return als_fit_entry(ctx, u, i, r, n, iterations, {lambda, reg, true, alpha});
}

int mf_als_run_cg(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg, int32_t cg_steps) {
  return als_run_entry(ctx, half_sweeps, {lambda, reg, false, 0.0, als_cg_entry_steps(cg_steps)});
}

int mf_als_fit_cg(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int32_t iterations,
                  double lambda, int32_t reg, int32_t cg_steps) {
  return als_fit_entry(ctx, u, i, r, n, iterations, {lambda, reg, false, 0.0, als_cg_entry_steps(cg_steps)});
}

int mf_als_run_implicit_cg(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg, double alpha,
                           int32_t cg_steps) {
  return als_run_entry(ctx, half_sweeps, {lambda, reg, true, alpha, als_cg_entry_steps(cg_steps)});
}

int mf_als_fit_implicit_cg(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                           int32_t iterations, double lambda, int32_t reg, double alpha, int32_t cg_steps) {
  return als_fit_entry(ctx, u, i, r, n, iterations, {lambda, reg, true, alpha, als_cg_entry_steps(cg_steps)});
}

int mf_als_run_nonneg(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg) {
  return als_run_entry(ctx, half_sweeps, {lambda, reg, false, 0.0, 0, true});
}

int mf_als_fit_nonneg(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int32_t iterations,
                      double lambda, int32_t reg) {
  return als_fit_entry(ctx, u, i, r, n, iterations, {lambda, reg, false, 0.0, 0, true});
}

int mf_als_run_implicit_nonneg(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg, double alpha) {
  return als_run_entry(ctx, half_sweeps, {lambda, reg, true, alpha, 0, true});
}

int mf_als_fit_implicit_nonneg(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n,
                               int32_t iterations, double lambda, int32_t reg, double alpha) {
  return als_fit_entry(ctx, u, i, r, n, iterations, {lambda, reg, true, alpha, 0, true});
}

extern "C++" {
namespace {

// mf_als_solve as the AlsParams of the run call it names.
AlsParams als_params_of(const mf_als_solve* how) {
  MF_REQUIRE(how, "null mf_als_solve");
  MF_REQUIRE(how->solver == MF_ALS_SOLVER_CHOLESKY || how->solver == MF_ALS_SOLVER_CG ||
                 how->solver == MF_ALS_SOLVER_NNLS,
             "unknown ALS solver");
  AlsParams P{how->lambda, how->reg, how->implicit != 0, how->implicit != 0 ? how->alpha : 0.0};
  if (how->solver == MF_ALS_SOLVER_CG) P.cg_steps = als_cg_entry_steps(how->cg_steps);
  P.nnls = how->solver == MF_ALS_SOLVER_NNLS;
  return P;
}

}  // namespace
}  // extern "C++"

int mf_als_append(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    als_append(ctx, u, i, r, n);
  });
}

int mf_als_run_rows(mf_ctx* ctx, int side, const int32_t* ids, int64_t n_ids, const mf_als_solve* how,
                    int64_t* solved_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    const int64_t solved = als_run_rows(ctx, side, ids, n_ids, als_params_of(how));
    if (solved_out) *solved_out = solved;
  });
}

int mf_als_update(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, const mf_als_solve* how,
                  int32_t rounds, int64_t* solved_users_out, int64_t* solved_items_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    als_update(ctx, u, i, r, n, als_params_of(how), rounds, solved_users_out, solved_items_out);
  });
}

int mf_als_objective(mf_ctx* ctx, const mf_als_solve* how, mf_als_loss* out) {
  return guarded([&] {
    MF_REQUIRE(ctx && how && out, "null argument");
    // solver and cg_steps are not read
    als_objective(ctx, {how->lambda, how->reg, how->implicit != 0, how->implicit != 0 ? how->alpha : 0.0}, out);
  });
}

int mf_als_run_until(mf_ctx* ctx, const mf_als_solve* how, int32_t max_iterations, double rel_tol,
                     int32_t* iterations_out, double* history_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    const int32_t t = als_run_until(ctx, als_params_of(how), max_iterations, rel_tol, history_out);
    if (iterations_out) *iterations_out = t;
  });
}

extern "C++" {
namespace {

// The checks of the two fold-in calls that read nothing of the context; returns the solve's parameters.
AlsParams foldin_check(mf_ctx* ctx, int side, const int64_t* off, const int32_t* ids, const double* r, int64_t nq,
                       const mf_als_solve* how) {
  MF_REQUIRE(ctx, "null context");
  MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
  MF_REQUIRE(nq >= 0, "negative n_queries");
  const AlsParams P = als_params_of(how);
  if (P.implicit) als_check_alpha(P.alpha);
  als_check_run(P);
  MF_REQUIRE(off, "null offsets");
  MF_REQUIRE(off[0] == 0, "offsets[0] must be 0");
  for (int64_t j = 0; j < nq; ++j) MF_REQUIRE(off[j + 1] >= off[j], "offsets must not decrease");
  MF_REQUIRE(off[nq] < (int64_t{1} << 31), "the lists hold 2^31 entries or more: total entries must stay below 2^31");
  MF_REQUIRE(off[nq] == 0 || (ids && r), "null cand_ids or ratings with entries in the lists");
  return P;
}

}  // namespace
}  // extern "C++"

int mf_als_foldin(mf_ctx* ctx, int side, const int64_t* offsets, const int32_t* cand_ids, const double* ratings,
                  int64_t n_queries, const mf_als_solve* how, double* vecs_out, int32_t* used_out) {
  return guarded([&] {
    const AlsParams P = foldin_check(ctx, side, offsets, cand_ids, ratings, n_queries, how);
    MF_REQUIRE(n_queries == 0 || vecs_out, "null vecs_out");
    als_foldin(ctx, side, offsets, cand_ids, ratings, n_queries, P, nullptr, vecs_out, used_out);
  });
}

int mf_recommend_foldin(mf_ctx* ctx, int side, const int64_t* offsets, const int32_t* cand_ids, const double* ratings,
                        int64_t n_queries, const mf_als_solve* how, int32_t top_n, int32_t exclude_rated,
                        int32_t* ids_out, double* scores_out, int32_t* counts_out, double* vecs_out,
                        int32_t* used_out) {
  return guarded([&] {
    const AlsParams P = foldin_check(ctx, side, offsets, cand_ids, ratings, n_queries, how);
    MF_REQUIRE(exclude_rated == 0 || exclude_rated == 1, "exclude_rated must be 0 or 1");
    MF_REQUIRE(top_n >= 1 && top_n <= MF_RECOMMEND_MAX_TOP,
               "top_n must be in [1, " + std::to_string(MF_RECOMMEND_MAX_TOP) + "]");
    MF_REQUIRE(n_queries == 0 || (ids_out && counts_out), "null ids_out or counts_out");
    const FoldinRecommend rec{top_n, exclude_rated != 0, ids_out, scores_out, counts_out};
    als_foldin(ctx, side, offsets, cand_ids, ratings, n_queries, P, &rec, vecs_out, used_out);
  });
}

int mf_als_remove(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, uint8_t* found_out, int64_t* removed_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    const int64_t removed = als_remove(ctx, u, i, n, found_out);
    if (removed_out) *removed_out = removed;
  });
}

int mf_als_remove_rows(mf_ctx* ctx, int side, const int32_t* ids, int64_t n_ids, int64_t* removed_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    const int64_t removed = als_remove_rows(ctx, side, ids, n_ids);
    if (removed_out) *removed_out = removed;
  });
}

int mf_als_retract(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, const mf_als_solve* how, int32_t rounds,
                   uint8_t* found_out, int64_t* removed_out, int64_t* solved_users_out, int64_t* solved_items_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    const int64_t removed =
        als_retract(ctx, u, i, n, als_params_of(how), rounds, found_out, solved_users_out, solved_items_out);
    if (removed_out) *removed_out = removed;
  });
}

int mf_debug_als_remove_select(const int64_t* off, int64_t rows, const int32_t* cols, const int32_t* batch_row,
                               const int32_t* batch_col, int64_t n, int64_t* pos_out) {
  return guarded([&] {
    MF_REQUIRE(off && rows >= 0 && n >= 0, "null offsets or a negative count");
    MF_REQUIRE(off[0] == 0, "off[0] must be 0");
    for (int64_t x = 0; x < rows; ++x) MF_REQUIRE(off[x + 1] >= off[x], "off must not descend");
    MF_REQUIRE((off[rows] == 0 || cols) && (n == 0 || (batch_row && batch_col && pos_out)), "null argument");
    for (int64_t j = 0; j < n; ++j) MF_REQUIRE(batch_row[j] >= 0 && batch_row[j] < rows, "a batch row is out of range");
    als_remove_select(off, rows, cols, batch_row, batch_col, n, pos_out);
  });
}

int mf_debug_als_csr(mf_ctx* ctx, int side, int64_t* off_out, int32_t* cols_out, double* vals_out, int32_t* npos_out,
                     int64_t cap_rows, int64_t cap_nnz, int64_t* rows_out, int64_t* nnz_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && off_out && cols_out && vals_out && npos_out && rows_out && nnz_out, "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    MF_REQUIRE(cap_rows >= 0 && cap_nnz >= 0, "negative count");
    als_debug_csr(ctx, side, off_out, cols_out, vals_out, npos_out, cap_rows, cap_nnz, rows_out, nnz_out);
  });
}

int mf_debug_als_append_placement(const int64_t* old_off, int64_t old_rows, const int32_t* batch_row, int64_t n,
                                  int64_t new_rows, int64_t* new_off_out, int64_t* batch_pos_out) {
  return guarded([&] {
    MF_REQUIRE(old_off && new_off_out && batch_pos_out && (n == 0 || batch_row), "null argument");
    MF_REQUIRE(old_rows >= 0 && n >= 0 && new_rows >= old_rows, "bad counts");
    MF_REQUIRE(old_off[0] == 0, "old_off[0] must be 0");
    for (int64_t x = 0; x < old_rows; ++x) MF_REQUIRE(old_off[x + 1] >= old_off[x], "old_off must not descend");
    for (int64_t j = 0; j < n; ++j) MF_REQUIRE(batch_row[j] >= 0 && batch_row[j] < new_rows, "a batch row is out of range");
    als_append_placement(old_off, old_rows, reinterpret_cast<const uint32_t*>(batch_row), n, new_rows, new_off_out,
                         batch_pos_out);
  });
}

int mf_als_nonneg_stats(mf_ctx* ctx, struct mf_als_nonneg_stats* out) {
  return guarded([&] {
    MF_REQUIRE(ctx && out, "null argument");
    als_nonneg_stats(ctx, out);
  });
}

int mf_nnls_solve(int32_t k, const double* A, const double* b, int f64, double* x_out, int32_t* iters_out,
                  int32_t* reason_out) {
  return guarded([&] { nnls_solve_host(k, A, b, f64 != 0, x_out, iters_out, reason_out); });
}

// (alpha < 0: the explicit system; any other alpha, NaN included, is the implicit one's and is checked as such)
int mf_debug_als_nnls_row(mf_ctx* ctx, int side, int32_t id, double lambda, int32_t reg, double alpha, double* x_out,
                          int32_t* iters_out, int32_t* reason_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && x_out && iters_out && reason_out, "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    als_nnls_row(ctx, side, id, {lambda, reg, !(alpha < 0.0), alpha, 0, true}, x_out, iters_out, reason_out);
  });
}

int mf_debug_als_cg_matvec(mf_ctx* ctx, int side, int32_t id, double lambda, int32_t reg, double alpha, const double* v,
                           double* Av_out, double* b_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && v && Av_out && b_out, "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    als_cg_matvec(ctx, side, id, {lambda, reg, !(alpha < 0.0), alpha, 1}, v, Av_out, b_out);
  });
}

int mf_debug_als_cg_capacity(mf_ctx* ctx, int32_t* ratings_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && ratings_out, "null argument");
    als_check(ctx);
    *ratings_out = als_cg_capacity(ctx->P.num_factors, ctx->f64);
  });
}

int mf_debug_als_gram(mf_ctx* ctx, int side, double* G_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && G_out, "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    als_gram(ctx, side, G_out);
  });
}

int mf_debug_als_normal_eq_implicit(mf_ctx* ctx, int side, int32_t id, double lambda, int32_t reg, double alpha,
                                    double* A_out, double* b_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && A_out && b_out, "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    als_normal_eq(ctx, side, id, {lambda, reg, true, alpha}, A_out, b_out);
  });
}

int mf_debug_als_normal_eq(mf_ctx* ctx, int side, int32_t id, double lambda, int32_t reg, double* A_out,
                           double* b_out) {
  return guarded([&] {
    MF_REQUIRE(ctx && A_out && b_out, "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    als_normal_eq(ctx, side, id, {lambda, reg}, A_out, b_out);
  });
}

int mf_block_update(mf_ctx* ctx, const double* r, const int32_t* uidx, const int32_t* iidx, int64_t len,
                    double* users, const int32_t* uomega, int64_t nu, double* items, const int32_t* iomega,
                    int64_t ni, int k, int iteration, int rating_block_id, int64_t seed, double lr,
                    int lr_method, double lr_arg, double lambda) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    block_update(ctx, r, uidx, iidx, len, users, uomega, nu, items, iomega, ni, k, iteration, rating_block_id, seed,
                 lr, lr_method, lr_arg, lambda);
  });
}

int mf_online_update(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                     int num_partitions, int64_t* touched_users, int64_t* touched_items) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    det_spec_wait(ctx, true);  // new ids change the layouts the builds read
    online_update(ctx, u, i, r, n, flavour, num_partitions, touched_users, touched_items);
  });
}

int mf_online_update_sampled(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                             int32_t negatives, double negative_rating, int64_t seed, int64_t first_event,
                             int32_t* sampled_items_out, int64_t* touched_users, int64_t* touched_items) {
  return guarded([&] {
    const NegSampling neg{negatives, negative_rating, seed, first_event};
    check_negative_sampling(neg);
    MF_REQUIRE(ctx, "null context");
    det_spec_wait(ctx, true);  // new ids change the layouts the builds read
    online_update_sampled(ctx, u, i, r, n, flavour, neg, sampled_items_out, touched_users, touched_items);
  });
}

int mf_negative_draws(int64_t seed, int64_t first_event, int64_t n, int32_t negatives, int64_t pool,
                      const int32_t* pos_row, int32_t* rows_out) {
  return guarded([&] {
    MF_REQUIRE(n >= 0, "negative count");
    MF_REQUIRE(negatives >= 0 && negatives <= kNegMax, "negatives must be in [0, " + std::to_string(kNegMax) + "]");
    MF_REQUIRE(first_event >= 0, "first_event must not be negative");
    MF_REQUIRE(pool >= 1 && pool <= (int64_t{1} << 31), "pool must be in [1, 2^31]");
    if (n == 0 || negatives == 0) return;
    MF_REQUIRE(pos_row && rows_out, "null argument");
    MF_REQUIRE(pool >= 2, "a pool of one row holds no negative");
    for (int64_t j = 0; j < n; ++j) {
      MF_REQUIRE(pos_row[j] >= 0 && pos_row[j] < pool, "pos_row outside the pool");
      for (int32_t s = 0; s < negatives; ++s)
        rows_out[j * negatives + s] = static_cast<int32_t>(
            neg_row(static_cast<uint64_t>(seed), static_cast<uint64_t>(first_event) + static_cast<uint64_t>(j),
                    static_cast<uint32_t>(s), static_cast<uint32_t>(pool), static_cast<uint32_t>(pos_row[j])));
    }
  });
}

int mf_online_update_out(mf_ctx* ctx, const int32_t* u, const int32_t* i, const double* r, int64_t n, int flavour,
                         int num_partitions, int64_t* touched_users, int64_t* touched_items, double* user_out,
                         double* item_out) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    det_spec_wait(ctx, true);  // new ids change the layouts the builds read
    online_update(ctx, u, i, r, n, flavour, num_partitions, touched_users, touched_items, user_out, item_out);
  });
}

int mf_lookup(mf_ctx* ctx, int side, const int32_t* ids, int64_t n, double* vecs_out, uint8_t* found) {
  return guarded([&] {
    MF_REQUIRE(ctx && (n == 0 || (ids && vecs_out && found)), "null argument");
    MF_REQUIRE(side == MF_SIDE_USER || side == MF_SIDE_ITEM, "bad side");
    lookup_factors(ctx, side, ids, n, vecs_out, found);
  });
}

int mf_set_profiling(mf_ctx* ctx, int on) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    sync_all(ctx);
    ctx->profiling = on != 0;
  });
}

int mf_get_stats(mf_ctx* ctx, mf_stats* out) {
  return guarded([&] {
    MF_REQUIRE(ctx && out, "null argument");
    sync_all(ctx);
    ctx->stats.algorithmic_bytes = static_cast<double>(ctx->stats.updates) * bytes_per_update(ctx);
    *out = ctx->stats;
  });
}

int mf_reset_stats(mf_ctx* ctx) {
  return guarded([&] {
    MF_REQUIRE(ctx, "null context");
    sync_all(ctx);
    const int32_t groups = ctx->stats.groups;
    const int64_t pads = ctx->stats.pads;
    ctx->stats = mf_stats{};
    ctx->stats.groups = groups;
    ctx->stats.pads = pads;
  });
}

int mf_jvm_shuffle(int64_t seed, int64_t len, int32_t* out) {
  return guarded([&] {
    MF_REQUIRE(len >= 0 && (len == 0 || out), "bad argument");
    JavaRandom rng(seed);
    scala_shuffle(rng, out, len);
  });
}

int mf_jvm_block_of(int32_t id, int64_t seed, int32_t n_blocks, int32_t* out) {
  return guarded([&] {
    MF_REQUIRE(out && n_blocks >= 1, "bad argument");
    JavaRandom rng(static_cast<int64_t>(id) ^ seed);
    *out = rng.nextInt(n_blocks);
  });
}

int mf_jvm_random_factors(int64_t rng_seed, int32_t k, double* out) {
  return guarded([&] {
    MF_REQUIRE(out && k >= 0, "bad argument");
    JavaRandom rng(rng_seed);
    for (int32_t f = 0; f < k; ++f) out[f] = rng.nextDouble();
  });
}

int mf_debug_levels(const uint32_t* urow, const uint32_t* irow, const int32_t* order, int64_t n, int32_t* level_out) {
  return guarded([&] {
    debug_levels(urow, irow, order, n, level_out);
  });
}

int mf_debug_fast_schedule(const int32_t* u, const int32_t* i, int64_t n, int32_t n_blocks, int64_t seed,
                           int32_t groups, int32_t blocking, int32_t window, int32_t k, int32_t* block_out,
                           int32_t* substep_out, int32_t* group_out, int64_t* pos_out) {
  return mf_debug_fast_split(u, i, n, n_blocks, seed, groups, blocking, window, k, 0, block_out, substep_out, group_out,
                             pos_out, nullptr);
}

int mf_debug_fast_split(const int32_t* u, const int32_t* i, int64_t n, int32_t n_blocks, int64_t seed,
                        int32_t groups, int32_t blocking, int32_t window, int32_t k, int32_t item_split,
                        int32_t* block_out, int32_t* substep_out, int32_t* group_out, int64_t* pos_out,
                        int32_t* replica_out) {
  return mfhip::debug_fast_plan(u, i, n, n_blocks, seed, groups, blocking, window, k, item_split, block_out,
                                substep_out, group_out, pos_out, replica_out);
}

const char* mf_fast_kernel_name(int32_t k) {
  switch (choose_fast_kernel(k)) {
    case FastKernel::kPair: return want_pair_sys() ? "k_sweep_pair_sys" : "k_sweep_pair";
    case FastKernel::kPersistent: return "k_fast_superstep";
    default: return "k_fast_substep";
  }
}

int32_t mf_debug_build_flags(void) { return mfhip::kExperiments ? 1 : 0; }

int mf_debug_device_bytes(int64_t out[2]) {
  if (!out) return MF_ERR_INVALID;
  out[0] = mfhip::dev_bytes_live().load();
  out[1] = mfhip::dev_bytes_peak().load();
  return MF_OK;
}

int mf_debug_plan_digest(mf_ctx* ctx, uint64_t out[2]) {
  return guarded([&] {
    MF_REQUIRE(ctx && out, "null argument");
    plan_digest(ctx, out);
  });
}

int mf_debug_ring_schedule(int32_t rank, int32_t world, int32_t n_blocks, int64_t superstep, int32_t* out_blk,
                           int32_t* in_blk, int32_t* dst, int32_t* src) {
  return guarded([&] {
    MF_REQUIRE(out_blk && in_blk && dst && src, "null argument");
    MF_REQUIRE(world >= 1 && rank >= 0 && rank < world && n_blocks >= 1 && n_blocks % world == 0 && superstep >= 1,
               "bad ring arguments (n_blocks must be a multiple of world, superstep >= 1)");
    const RingStep rs = ring_step(rank, world, n_blocks / world, n_blocks, superstep);
    *out_blk = rs.out_blk;
    *in_blk = rs.in_blk;
    *dst = rs.dst;
    *src = rs.src;
  });
}

int mf_debug_det_slot_table(const int64_t* begin, const int32_t* count, const int32_t* flags, int64_t nw,
                            int64_t max_blocks, int32_t alone, int64_t period, int64_t* begin_out, int32_t* count_out,
                            int32_t* flags_out, int64_t* nslots_out) {
  return guarded([&] {
    MF_REQUIRE(begin_out && count_out && flags_out && nslots_out && (nw == 0 || (begin && count && flags)),
               "null argument");
    MF_REQUIRE(nw >= 0 && nw <= (1 << 24) && max_blocks >= 1 && period >= 1, "bad slot table arguments");
    std::vector<DetWave> waves(static_cast<size_t>(det_slot_room(nw)));
    for (int64_t w = 0; w < nw; ++w) {
      MF_REQUIRE(count[w] >= 0, "negative wave count");
      waves[w] = DetWave{begin[w], count[w], flags[w]};
    }
    const int64_t n = det_slot_table(waves.data(), nw, max_blocks, alone != 0, period);
    for (int64_t x = 0; x < n; ++x) {
      begin_out[x] = waves[x].begin;
      count_out[x] = waves[x].count;
      flags_out[x] = waves[x].flags;
    }
    *nslots_out = n;
  });
}

int mf_debug_sys_placement(const double* load, int64_t nw, int64_t cap, int32_t iso, int32_t* pad_out,
                           int32_t* place_out) {
  return guarded([&] {
    MF_REQUIRE(load && pad_out && place_out, "null argument");
    MF_REQUIRE(nw >= 1 && nw <= cap && cap <= (1 << 24) && iso >= 0 && iso <= 8,
               "bad placement arguments (1 <= nw <= cap, iso in [0, 8])");
    const int32_t pad = iso ? sys_iso_pad(nw, cap, iso) : 0;
    place_by_load(load, nw, pad, place_out);
    check_placement(place_out, nw + 8 * pad, nw);
    *pad_out = pad;
  });
}

int mf_fast_plan_window(int32_t k, int32_t* window_out) {
  return guarded([&] {
    MF_REQUIRE(window_out, "null");
    const FastKernel fk = choose_fast_kernel(k);
    *window_out = fk == FastKernel::kPair ? plan_window(k) : kHazardWindow;
  });
}

int mf_learning_rate(int method, double lr, int32_t iteration, double lambda, double arg, double* out) {
  return guarded([&] {
    MF_REQUIRE(out, "null");
    MF_REQUIRE(method >= MF_LR_DEFAULT && method <= MF_LR_XU, "unknown lr_method");
    *out = learning_rate(method, lr, iteration, lambda, arg);
  });
}

}  // extern "C"
