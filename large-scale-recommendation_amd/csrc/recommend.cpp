// recommend.cpp -- top-N lists (mf_recommend, mf_recommend_seen, mf_similar, mf_recommend_vectors,
// mf_recommend_among; mf_rank_eval and mf_recommend_foldin come in through recommend_scored): a front resolves the
// call's queries and exclusions to rows, one driver scores and selects on the device, on shard 0 like evaluate.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "common.hpp"
#include "context.hpp"
#include "kernels.hpp"
#include "plan.hpp"

namespace mfhip {

void sync_row_ids(mf_ctx* ctx, Shard& s, int side) {
  const SideLayout& L = side_of(ctx, side);
  const size_t bytes = static_cast<size_t>(L.rows()) * 4;
  if (s.rec_id_gen[side] != ctx->layout_gen || s.rec_id[side].bytes() < bytes) {
    s.rec_id[side].alloc(bytes);
    MF_HIP(hipMemcpy(s.rec_id[side].get(), L.row_id.data(), bytes, hipMemcpyHostToDevice));
    s.rec_id_gen[side] = ctx->layout_gen;
  }
}

TopNShape topn_shape(int64_t n, int64_t C, int qtile, int64_t default_batch, const char* batch_knob,
                     const char* split_knob) {
  int64_t batch = default_batch;
  if (const std::string v = test_knob(batch_knob); !v.empty()) batch = std::atoll(v.c_str());
  batch = std::max<int64_t>(1, std::min(batch, n));
  const int64_t qtiles = (batch + qtile - 1) / qtile;
  int64_t S = std::min<int64_t>((512 + qtiles - 1) / qtiles, (C + 127) / 128);
  if (const std::string v = test_knob(split_knob); !v.empty()) S = std::atoll(v.c_str());
  return {batch, std::max<int64_t>(1, std::min<int64_t>({S, 64, C}))};
}

ExclSource::Range ExclSource::batch(hipStream_t st, int64_t b0, int64_t nb, const int32_t* qrows) const {
  if (!sv.any) return {off + b0, off + b0 + 1, rows};
  qbeg->alloc(static_cast<size_t>(nb) * 8);
  qend->alloc(static_cast<size_t>(nb) * 8);
  launch_seen_gather(st, sv.off, qrows, static_cast<int>(nb), qbeg->as<int64_t>(), qend->as<int64_t>());
  return {qbeg->as<int64_t>(), qend->as<int64_t>(), sv.ent};
}

namespace {
const void* slab_of(const Shard& s, int side) { return side == kSideU ? s.uf.get() : s.itf.get(); }
}  // namespace

TopNQueries TopNQueries::of_slab(Shard& s, const void* Q, int64_t n) {
  if (n > 0) {
    s.rec_q.alloc(static_cast<size_t>(n) * 4);
    launch_iota(s.stream, s.rec_q.as<int32_t>(), n);
  }
  return {n, s.rec_q.as<int32_t>(), Q, n};
}

namespace {

// ids / scores (may be null) / counts of the nb lists in s.rec_ids / rec_scores / rec_counts -> the host, after
// a wait for the stream
void download_lists(Shard& s, int64_t nb, int32_t top_n, int32_t* ids, double* scores, int32_t* counts) {
  const size_t slots = static_cast<size_t>(nb) * static_cast<size_t>(top_n);
  MF_HIP(hipStreamSynchronize(s.stream));
  MF_HIP(hipMemcpy(ids, s.rec_ids.get(), slots * 4, hipMemcpyDeviceToHost));
  if (scores) MF_HIP(hipMemcpy(scores, s.rec_scores.get(), slots * 8, hipMemcpyDeviceToHost));
  MF_HIP(hipMemcpy(counts, s.rec_counts.get(), static_cast<size_t>(nb) * 4, hipMemcpyDeviceToHost));
}

// Host vectors: queries [b0, b0 + nb) -> the pinned stage in the context's precision -> rec_qvec, queued behind
// whatever the stream holds (the previous batch's kernels still read rec_qvec)
void stage_vectors(mf_ctx* ctx, Shard& s, const double* vecs, int64_t b0, int64_t nb) {
  const int64_t k = ctx->P.num_factors, n = nb * k;
  const double* src = vecs + b0 * k;
  if (ctx->f64) {
    std::memcpy(s.rec_pin.as<double>(), src, static_cast<size_t>(n) * 8);
  } else {
    float* dst = s.rec_pin.as<float>();
    parallel_for(n, [&](int64_t b, int64_t e, int) {
      for (int64_t x = b; x < e; ++x) dst[x] = static_cast<float>(src[x]);
    });
  }
  MF_HIP(hipMemcpyAsync(s.rec_qvec.get(), s.rec_pin.as<char>(), static_cast<size_t>(n) * ctx->es, hipMemcpyHostToDevice,
                        s.stream));
}

}  // namespace

void recommend_scored(mf_ctx* ctx, Shard& s, const TopNQueries& q, const TopNCandidates& c, int32_t top_n, int metric,
                      const ExclSource& ex, const TopNSink& sink) {
  const int64_t nu = q.n, C = c.n;
  const int k = ctx->P.num_factors;
  const size_t N = static_cast<size_t>(top_n);
  if (nu == 0) return;
  const TopNShape sh = topn_shape(nu, C, recommend_query_tile(top_n, ctx->f64), 8192, "rec_batch", "rec_split");
  const int64_t batch = sh.batch;
  if (C == 0 && !sink.on_batch) {  // every list is empty, and the device is not needed
    std::fill(sink.ids, sink.ids + static_cast<size_t>(nu) * N, 0);
    if (sink.scores) std::fill(sink.scores, sink.scores + static_cast<size_t>(nu) * N, 0.0);
    std::fill(sink.counts, sink.counts + nu, 0);
    return;
  }
  s.rec_ids.alloc(static_cast<size_t>(batch) * N * 4);
  s.rec_counts.alloc(static_cast<size_t>(batch) * 4);
  if (C == 0) {  // ... or on_batch meets empty lists
    MF_HIP(hipMemsetAsync(s.rec_counts.get(), 0, static_cast<size_t>(batch) * 4, s.stream));
    for (int64_t b0 = 0; b0 < nu; b0 += batch) sink.on_batch(b0, std::min(batch, nu - b0));
    return;
  }
  sync_row_ids(ctx, s, c.side);
  s.rec_part.alloc(static_cast<size_t>(batch) * sh.S * N * recommend_key_bytes(ctx->f64));
  if (!sink.on_batch) s.rec_scores.alloc(static_cast<size_t>(batch) * N * 8);

  RecLaunch L;
  L.st = s.stream;
  L.Q = q.Q;
  L.Cf = slab_of(s, c.side);
  L.k = k;
  L.top_n = top_n;
  L.f64 = ctx->f64;
  L.cand_id = s.rec_id[c.side].as<int32_t>();
  L.C = static_cast<int32_t>(C);
  L.S = static_cast<int>(sh.S);
  L.part = s.rec_part.get();
  L.ids = s.rec_ids.as<int32_t>();
  L.scores = sink.on_batch ? nullptr : s.rec_scores.as<double>();
  L.counts = s.rec_counts.as<int32_t>();
  if (c.gathered) {
    s.am_id.alloc(static_cast<size_t>(C) * 4);
    s.am_slab.alloc(static_cast<size_t>(C) * k * ctx->es);
    launch_among_gather(s.stream, L.Cf, s.am_rows.as<int32_t>(), C, k, ctx->f64, L.cand_id, s.am_slab.get(),
                        s.am_id.as<int32_t>());
    MF_HIP(hipGetLastError());
    L.Cf = s.am_slab.get();
    L.cand_id = s.am_id.as<int32_t>();
    L.pos_row = s.am_rows.as<int32_t>();
  }
  // cosine: the inverse norms of this call (never kept: the rows may change before the next one).  Queries
  // that are rows of the candidate slab itself (mf_similar) share its table.
  const bool cosine = metric == MF_METRIC_COSINE;
  if (cosine) {
    s.rec_cinv.alloc(static_cast<size_t>(C) * ctx->es);
    launch_row_inv_norm(s.stream, L.Cf, C, k, ctx->f64, s.rec_cinv.get());
    L.q_inv = L.c_inv = s.rec_cinv.get();
    if (q.staged || q.side != c.side || c.gathered) {
      s.rec_qinv.alloc(static_cast<size_t>(q.staged ? batch : q.q_rows) * ctx->es);
      if (!q.staged) launch_row_inv_norm(s.stream, q.Q, q.q_rows, k, ctx->f64, s.rec_qinv.get());
      L.q_inv = s.rec_qinv.get();
    }
    MF_HIP(hipGetLastError());
  }
  if (q.staged) {
    // the stage is rewritten while a batch runs: only the copying sink's wait makes that safe
    MF_REQUIRE(!sink.on_batch, "recommend_scored: staged queries with a sink that does not wait");
    s.rec_qvec.alloc(static_cast<size_t>(batch) * k * ctx->es);
    s.rec_pin.alloc(static_cast<size_t>(batch) * k * ctx->es);
    stage_vectors(ctx, s, q.vecs, 0, batch);
    MF_HIP(hipStreamSynchronize(s.stream));  // the stage is rewritten while batch 0 runs
    L.Q = s.rec_qvec.get();
  }
  for (int64_t b0 = 0; b0 < nu; b0 += batch) {
    const int64_t nb = std::min(batch, nu - b0);
    // a staged batch is rows 0 .. nb-1 of rec_qvec: the head of the identity list names them
    const int32_t* rows_d = q.rows + (q.staged ? 0 : b0);
    const ExclSource::Range e = ex.batch(s.stream, b0, nb, rows_d);
    L.excl_beg = e.beg;
    L.excl_end = e.end;
    L.excl_rows = e.rows;
    if (q.staged && cosine) launch_row_inv_norm(s.stream, s.rec_qvec.get(), nb, k, ctx->f64, s.rec_qinv.get());
    launch_recommend(L, rows_d, static_cast<int>(nb));
    MF_HIP(hipGetLastError());
    if (q.staged && b0 + batch < nu) {
      // the stage is free: its last copy finished with the previous batch's synchronisation
      stage_vectors(ctx, s, q.vecs, b0 + batch, std::min(batch, nu - b0 - batch));
    }
    if (sink.on_batch)
      sink.on_batch(b0, nb);
    else
      download_lists(s, nb, top_n, sink.ids + static_cast<size_t>(b0) * N,
                     sink.scores ? sink.scores + static_cast<size_t>(b0) * N : nullptr, sink.counts + b0);
  }
}

namespace {

// The call's query rows and exclusion CSR as the host holds them -> s.rec_q and s.rec_eoff / rec_erows
ExclSource upload_call(mf_ctx* ctx, Shard& s, int cside, const std::vector<int32_t>& qrows,
                       const std::vector<int64_t>& eoff, const std::vector<int32_t>& erows) {
  if (side_of(ctx, cside).rows() > 0) {
    s.rec_q.alloc(qrows.size() * 4);
    s.rec_eoff.alloc(eoff.size() * 8);
    s.rec_erows.alloc(std::max<size_t>(erows.size(), 1) * 4);
    MF_HIP(hipMemcpy(s.rec_q.get(), qrows.data(), qrows.size() * 4, hipMemcpyHostToDevice));
    MF_HIP(hipMemcpy(s.rec_eoff.get(), eoff.data(), eoff.size() * 8, hipMemcpyHostToDevice));
    if (!erows.empty()) MF_HIP(hipMemcpy(s.rec_erows.get(), erows.data(), erows.size() * 4, hipMemcpyHostToDevice));
  }
  return ExclSource::csr(s.rec_eoff.as<int64_t>(), s.rec_erows.as<int32_t>());
}

// Exclusion pairs given by id -> (query position << 32 | candidate row) pairs, appended to `pairs`.  pos(e): the
// query position pair e names, or -1; a pair whose candidate id the side does not hold is dropped too.
template <typename Pos>
void exclusion_pairs(const SideLayout& CS, const int32_t* ec, int64_t ne, Pos pos, std::vector<uint64_t>& pairs) {
  std::vector<uint32_t> er_c;
  lookup_rows(CS, ec, ne, er_c);
  pairs.reserve(pairs.size() + static_cast<size_t>(ne));
  for (int64_t e = 0; e < ne; ++e) {
    const int64_t u = pos(e);
    if (u < 0 || er_c[e] == kRowMiss) continue;
    pairs.push_back((static_cast<uint64_t>(u) << 32) | er_c[e]);
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
  if (ne > 0) {
    std::vector<uint32_t> er_q;
    lookup_rows(QS, eq, ne, er_q);
    exclusion_pairs(CS, ec, ne, [&](int64_t e) { return qs.pos(er_q[e]); }, pairs);
  }
  if (no_self)
    for (int64_t u = 0; u < nu; ++u) pairs.push_back((static_cast<uint64_t>(u) << 32) | static_cast<uint32_t>(uniq[u]));
  exclusion_csr(pairs, nu, eoff, erows);
}

// The front of the calls whose queries are ids of side qside, candidates `cand` of the other side (mf_recommend,
// mf_recommend_among's shared list) or of the same side (mf_similar).  Distinct known query rows are scored once;
// every position of queries[] then takes its row's result.  no_self: each query's own row joins its exclusions
// (it is a candidate only when the sides are the same) -- no kernel knows about "self".  seen: the resident set
// stands in for the call's own exclusions.
void recommend_ids(mf_ctx* ctx, int qside, const TopNCandidates& cand, const int32_t* queries, int64_t nq,
                   int32_t top_n, int metric, bool no_self, const int32_t* eq, const int32_t* ec, int64_t ne,
                   int32_t* ids_out, double* scores_out, int32_t* counts_out, bool seen) {
  Shard& s = ctx->shards[0];
  if (seen) ne = 0;
  consolidate(ctx, s);
  sync_all(ctx);  // a run may still be sweeping (mf_dsgd_run returns early)
  const SideLayout& QS = side_of(ctx, qside);
  const SideLayout& CS = side_of(ctx, cand.side);
  const size_t N = static_cast<size_t>(top_n);

  const QuerySet qs(QS, queries, nq);
  const int64_t nu = static_cast<int64_t>(qs.uniq.size());
  std::vector<int64_t> eoff;
  std::vector<int32_t> erows;
  call_exclusions(QS, CS, qs, no_self, eq, ec, ne, eoff, erows);

  std::vector<int32_t> uid(static_cast<size_t>(nu) * N, 0), ucnt(static_cast<size_t>(nu), 0);
  std::vector<double> usc(scores_out ? static_cast<size_t>(nu) * N : 0, 0.0);
  if (nu > 0) {
    DeviceGuard g(s.device);
    ExclSource ex = upload_call(ctx, s, cand.side, qs.uniq, eoff, erows);
    if (seen && cand.n > 0)
      if (const SeenView sv = seen_view(ctx, s, qside); sv.any) ex = ExclSource::seen(sv, s.seen.qbeg, s.seen.qend);
    recommend_scored(ctx, s, TopNQueries::of_side(ctx, s, qside, nu), cand, top_n, metric, ex,
                     TopNSink{uid.data(), scores_out ? usc.data() : nullptr, ucnt.data(), nullptr});
  }
  parallel_for(nq, [&](int64_t b, int64_t e, int) {
    for (int64_t j = b; j < e; ++j) {
      const int64_t u = qs.pos(qs.qr[j]);
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
  const ExclSource seen_ex = ExclSource::seen(sv, s.am_ebeg, s.am_eend);

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
      // the positions' ranges: gathered from the seen set through their query rows, or as cut above
      ExclSource::Range e{s.am_ebeg.as<int64_t>(), s.am_eend.as<int64_t>(), s.rec_erows.as<int32_t>()};
      if (sv.any) {
        e = seen_ex.batch(s.stream, 0, nb, s.am_qrow.as<int32_t>());
      } else {
        MF_HIP(hipMemcpyAsync(s.am_ebeg.get(), ebeg.data(), static_cast<size_t>(nb) * 8, hipMemcpyHostToDevice, s.stream));
        MF_HIP(hipMemcpyAsync(s.am_eend.get(), eend.data(), static_cast<size_t>(nb) * 8, hipMemcpyHostToDevice, s.stream));
      }
      launch_id_lookup_one(s.stream, s.am_in.as<uint32_t>(), nent, mirror.cap ? mirror.slots.get() : nullptr,
                           mirror.cap - 1);
      launch_among(s.stream, slab_of(s, qside), slab_of(s, cside), s.am_tasks.as<AmongTask>(), ntasks,
                   s.am_pbeg.as<int64_t>(), static_cast<int>(nb), s.am_in.as<uint32_t>(), s.am_qrow.as<int32_t>(),
                   s.rec_id[cside].as<int32_t>(), e.beg, e.end, e.rows, k, top_n, ctx->f64, s.rec_part.get(),
                   s.rec_ids.as<int32_t>(), s.rec_scores.as<double>(), s.rec_counts.as<int32_t>());
      MF_HIP(hipGetLastError());
      // (the wait also frees the host vectors, which are rebuilt for the next batch)
      download_lists(s, nb, top_n, ids_out + static_cast<size_t>(j0) * N,
                     scores_out ? scores_out + static_cast<size_t>(j0) * N : nullptr, counts_out + j0);
    }
    j0 = j1;
  }
}

}  // namespace

void recommend(mf_ctx* ctx, int qside, const int32_t* queries, int64_t nq, int32_t top_n, const int32_t* eq,
               const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out, int32_t* counts_out,
               bool seen) {
  recommend_ids(ctx, qside, TopNCandidates::of_side(ctx, 1 - qside), queries, nq, top_n, MF_METRIC_DOT, false, eq, ec,
                ne, ids_out, scores_out, counts_out, seen);
}

// mf_recommend_among.  One shared list (off == null) is resolved to its distinct held rows on the device and
// handed to the driver as its candidates; per-query lists take the gather path above.
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
  recommend_ids(ctx, qside, TopNCandidates::of_rows(1 - qside, held), queries, nq, top_n, MF_METRIC_DOT, false, eq, ec,
                ne, ids_out, scores_out, counts_out, seen);
}

// mf_similar: the nearest rows of the queries' own side.
void similar(mf_ctx* ctx, int side, const int32_t* queries, int64_t nq, int32_t top_n, int metric, bool include_self,
             const int32_t* eq, const int32_t* ec, int64_t ne, int32_t* ids_out, double* scores_out,
             int32_t* counts_out) {
  recommend_ids(ctx, side, TopNCandidates::of_side(ctx, side), queries, nq, top_n, metric, !include_self, eq, ec, ne,
                ids_out, scores_out, counts_out, false);
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
  if (nq == 0) return;
  std::vector<int32_t> rows(static_cast<size_t>(nq));
  std::iota(rows.begin(), rows.end(), 0);
  std::vector<int64_t> eoff(static_cast<size_t>(nq) + 1, 0);
  std::vector<int32_t> erows;
  if (ne > 0 && CS.rows() > 0) {
    std::vector<uint64_t> pairs;
    exclusion_pairs(CS, ec, ne, [&](int64_t e) { return eqi[e] >= 0 && eqi[e] < nq ? eqi[e] : int64_t{-1}; }, pairs);
    exclusion_csr(pairs, nq, eoff, erows);
  }
  DeviceGuard g(s.device);
  const ExclSource ex = upload_call(ctx, s, cside, rows, eoff, erows);
  recommend_scored(ctx, s, TopNQueries::of_vectors(s, vecs, nq), TopNCandidates::of_side(ctx, cside), top_n, metric, ex,
                   TopNSink{ids_out, scores_out, counts_out, nullptr});
}

}  // namespace mfhip
