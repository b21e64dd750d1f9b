// seen.cpp -- the resident seen set (mf_seen_set / mf_seen_add / mf_seen_remove / mf_seen_from_als /
// mf_seen_clear / mf_seen_count): the distinct (user, item) pairs the model's readers hide, built once and kept on the
// device keyed by factor row, so that mf_recommend_seen, mf_rank_eval_seen, mf_pair_ranks_seen and
// mf_online_prequential_seen name it instead of resolving, uploading and sorting the same pairs in every
// call.  Ids are resolved on the host (lookup_rows, as rank_eval.cpp does); everything after that is
// kernels_seen.hip and the sort, run heads and offsets of kernels_rank.hip, on the context's first shard.
//
// Why by row: a factor row never moves while rows are only added (online updates, mf_set_factors,
// mf_load_model, mf_als_append), so the table stays valid through all of them and a reader finds a query's
// entries from the row it scores anyway -- no per-call position table.  mf_dsgd_prepare / mf_dsgd_fit
// rebuild the rows and leave no set (seen_clear), as they invalidate the ALS data.
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
namespace {

constexpr int64_t kMaxKeys = (int64_t{1} << 31) - 1;  // one sort holds fewer keys than this

// Room for rows + 1 offsets and some rows to come: a side that gains rows pads in place (seen_view).
size_t off_bytes(int64_t rows) { return static_cast<size_t>(rows + 1 + std::max<int64_t>(1024, rows / 8)) * 8; }

int64_t read_i64(Shard& s, const int64_t* p) {
  int64_t v = 0;
  MF_HIP(hipMemcpyAsync(&v, p, 8, hipMemcpyDeviceToHost, s.stream));
  MF_HIP(hipStreamSynchronize(s.stream));
  return v;
}

// The user-major table := no pair, over `rows` rows.
void make_empty(Shard& s, int64_t rows) {
  SeenTable& T = s.seen;
  MF_HIP(hipStreamSynchronize(s.stream));  // a reader may still search the old arrays
  T.off[kSideU].alloc(off_bytes(rows));
  MF_HIP(hipMemsetAsync(T.off[kSideU].get(), 0, static_cast<size_t>(rows + 1) * 8, s.stream));
  T.rows[kSideU] = rows;
  T.nnz = 0;
  T.have = true;
  T.item_valid = false;
}

// The user-major table := the distinct kept keys of rank_sc.key[0, n) (positions 0 .. rows - 1).
void build_from_keys(Shard& s, int64_t n, int64_t rows) {
  SeenTable& T = s.seen;
  rank_keys_sort(s.stream, s.rank_sc, n, rows);
  T.off[kSideU].alloc(off_bytes(rows));
  T.ent[kSideU].alloc(static_cast<size_t>(n) * 4);
  rank_keys_csr(s.stream, s.rank_sc, n, rows, false, T.off[kSideU].as<int64_t>(), T.ent[kSideU].as<int32_t>());
  T.rows[kSideU] = rows;
  T.nnz = read_i64(s, T.off[kSideU].as<int64_t>() + rows);
  T.have = true;
  T.item_valid = false;
}

// The sorted batch in rank_sc (after rank_keys_sort) merged into the user-major table, which comes to cover
// `rows` rows.  Fresh arrays by rank; the old ones are freed once the stream has drained.
void merge_sorted_batch(Shard& s, int64_t n, int64_t rows) {
  SeenTable& T = s.seen;
  RankScratch& sc = s.rank_sc;
  T.lb.alloc(static_cast<size_t>(n) * 8);
  T.nov_off.alloc(static_cast<size_t>(rows + 1) * 8);
  T.nov_ent.alloc(static_cast<size_t>(n) * 4);
  launch_seen_novel(s.stream, sc.key2.as<uint64_t>(), sc.head.as<int32_t>(), n, T.off[kSideU].as<int64_t>(),
                    T.rows[kSideU], T.ent[kSideU].as<int32_t>(), T.lb.as<int64_t>());
  rank_keys_csr(s.stream, sc, n, rows, false, T.nov_off.as<int64_t>(), T.nov_ent.as<int32_t>());
  const int64_t m = read_i64(s, T.nov_off.as<int64_t>() + rows);
  if (m == 0) return;  // nothing new: the tables stand (rows gained since are padded on use)
  DevBuf off, ent;
  off.alloc(off_bytes(rows));
  ent.alloc(static_cast<size_t>(T.nnz + m) * 4);
  launch_seen_merge(s.stream, T.off[kSideU].as<int64_t>(), T.rows[kSideU], T.nnz, T.ent[kSideU].as<int32_t>(),
                    T.nov_off.as<int64_t>(), T.nov_ent.as<int32_t>(), rows, sc.key2.as<uint64_t>(), sc.head.as<int32_t>(),
                    sc.wp.as<int32_t>(), T.lb.as<int64_t>(), n, off.as<int64_t>(), ent.as<int32_t>());
  MF_HIP(hipStreamSynchronize(s.stream));
  T.off[kSideU] = std::move(off);
  T.ent[kSideU] = std::move(ent);
  T.rows[kSideU] = rows;
  T.nnz += m;
  T.item_valid = false;
}

}  // namespace

void seen_clear(mf_ctx* ctx) {
  if (ctx->shards.empty()) return;
  SeenTable& T = ctx->shards[0].seen;
  T.have = T.item_valid = false;
  T.nnz = 0;
  T.rows[0] = T.rows[1] = 0;
}

int64_t seen_count(const mf_ctx* ctx) { return ctx->shards[0].seen.have ? ctx->shards[0].seen.nnz : 0; }

void seen_put(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, bool add, int64_t* ignored) {
  Shard& s = ctx->shards[0];
  SeenTable& T = s.seen;
  const int64_t rows = ctx->U.rows();
  std::vector<uint32_t> ur, ir;
  if (n > 0) {
    lookup_rows(ctx->U, u, n, ur);
    lookup_rows(ctx->I, i, n, ir);
  }
  std::atomic<int64_t> dropped{0};
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    int64_t m = 0;
    for (int64_t j = b; j < e; ++j) m += (ur[j] == kRowMiss || ir[j] == kRowMiss) ? 1 : 0;
    dropped += m;
  });
  if (ignored) *ignored = dropped.load();
  DeviceGuard g(s.device);
  const bool merge = add && T.have;
  if (dropped.load() == n) {  // nothing to hold
    if (!merge) make_empty(s, rows);
    return;
  }
  MF_HIP(hipStreamSynchronize(s.stream));  // an earlier build may still read the buffers
  T.in.alloc(static_cast<size_t>(n) * 8);
  MF_HIP(hipMemcpy(T.in.get(), ur.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
  MF_HIP(hipMemcpy(T.in.as<uint32_t>() + n, ir.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
  rank_keys_reserve(s.rank_sc, n);
  launch_seen_pair_keys(s.stream, T.in.as<uint32_t>(), T.in.as<uint32_t>() + n, n, static_cast<uint32_t>(rows),
                        s.rank_sc.key.as<uint64_t>());
  if (merge && T.nnz > 0) {
    rank_keys_sort(s.stream, s.rank_sc, n, rows);
    merge_sorted_batch(s, n, rows);
  } else {
    build_from_keys(s, n, rows);
  }
}

// mf_seen_remove: the user-major table without the pairs given, through the compaction mf_als_remove uses
// (kernels_als_remove.hip, a CSR without values: every held pair a batch key names goes, however often it is
// named).  Fresh arrays; the item-major table is made again on its next use.
void seen_remove(mf_ctx* ctx, const int32_t* u, const int32_t* i, int64_t n, int64_t* removed, int64_t* ignored) {
  Shard& s = ctx->shards[0];
  SeenTable& T = s.seen;
  std::vector<uint32_t> ur, ir;
  if (n > 0) {
    lookup_rows(ctx->U, u, n, ur);
    lookup_rows(ctx->I, i, n, ir);
  }
  const bool held = T.have && T.nnz > 0;
  int64_t dropped = 0;
  std::vector<uint64_t> key;
  for (int64_t j = 0; j < n; ++j) {
    if (ur[j] == kRowMiss || ir[j] == kRowMiss) {
      ++dropped;
    } else if (held && static_cast<int64_t>(ur[j]) < T.rows[kSideU]) {  // (a row gained since holds nothing)
      key.push_back((static_cast<uint64_t>(ur[j]) << 32) | ir[j]);
    }
  }
  if (ignored) *ignored = dropped;
  if (removed) *removed = 0;
  if (key.empty()) return;
  DeviceGuard g(s.device);
  MF_HIP(hipStreamSynchronize(s.stream));  // a reader may still search the arrays
  AlsRemoveScratch& sc = s.als_rem;
  sc.in.alloc(key.size() * 8);
  MF_HIP(hipMemcpy(sc.in.get(), key.data(), key.size() * 8, hipMemcpyHostToDevice));
  const AlsRemoveLaunch L{s.stream, T.off[kSideU].as<int64_t>(), T.rows[kSideU], T.nnz, T.ent[kSideU].as<int32_t>(),
                          nullptr, 0, sc.in.as<uint64_t>(), static_cast<int64_t>(key.size()), nullptr, nullptr};
  const int64_t gone = launch_als_remove_select(L, sc, nullptr, nullptr);
  if (gone == 0) return;  // none of the pairs is held: the tables stand
  DevBuf off, ent;
  off.alloc(off_bytes(T.rows[kSideU]));
  ent.alloc(std::max<size_t>(static_cast<size_t>(T.nnz - gone) * 4, 16));
  launch_als_remove_move(L, sc, off.as<int64_t>(), ent.as<int32_t>(), nullptr);
  MF_HIP(hipStreamSynchronize(s.stream));
  T.off[kSideU] = std::move(off);
  T.ent[kSideU] = std::move(ent);
  T.nnz -= gone;
  T.item_valid = false;
  if (removed) *removed = gone;
}

void seen_from_als(mf_ctx* ctx) {
  als_check(ctx);
  if (!ctx->als_prepared) fail(MF_ERR_STATE, "mf_seen_from_als before mf_als_prepare");
  require_healthy(ctx);
  sync_all(ctx);
  Shard& s = ctx->shards[0];
  const mf_ctx::AlsSide& A = ctx->als[kSideU];
  const int64_t arows = static_cast<int64_t>(A.off.size()) - 1;
  const int64_t nnz = arows > 0 ? A.off.back() : 0;
  MF_REQUIRE(nnz < kMaxKeys, "mf_seen_from_als: the prepared data holds 2^31 - 1 ratings or more");
  const int64_t rows = ctx->U.rows();
  DeviceGuard g(s.device);
  if (nnz == 0) {
    make_empty(s, rows);
    return;
  }
  MF_HIP(hipStreamSynchronize(s.stream));
  rank_keys_reserve(s.rank_sc, nnz);
  launch_seen_csr_keys(s.stream, s.als_off[kSideU].as<int64_t>(), arows, nnz, s.als_cols[kSideU].as<int32_t>(), false,
                       s.rank_sc.key.as<uint64_t>());
  build_from_keys(s, nnz, rows);
}

SeenView seen_view(mf_ctx* ctx, Shard& s, int qside) {
  SeenTable& T = s.seen;
  SeenView v;
  if (!T.have || T.nnz == 0) return v;
  if (qside != kSideU && !T.item_valid) {
    // the other orientation: one sort of the swapped keys of the user-major entries
    MF_REQUIRE(T.nnz < kMaxKeys, "the seen set holds 2^31 - 1 pairs or more: item queries cannot use it");
    const int64_t irows = ctx->I.rows();
    MF_HIP(hipStreamSynchronize(s.stream));
    rank_keys_reserve(s.rank_sc, T.nnz);
    launch_seen_csr_keys(s.stream, T.off[kSideU].as<int64_t>(), T.rows[kSideU], T.nnz, T.ent[kSideU].as<int32_t>(), true,
                         s.rank_sc.key.as<uint64_t>());
    rank_keys_sort(s.stream, s.rank_sc, T.nnz, irows);
    T.off[1].alloc(off_bytes(irows));
    T.ent[1].alloc(static_cast<size_t>(T.nnz) * 4);
    rank_keys_csr(s.stream, s.rank_sc, T.nnz, irows, false, T.off[1].as<int64_t>(), T.ent[1].as<int32_t>());
    T.rows[1] = irows;
    T.item_valid = true;
  }
  const int side = qside == kSideU ? kSideU : 1;
  const int64_t rows = side_of(ctx, qside).rows();
  if (rows > T.rows[side]) {
    // rows gained since the table was built hold nothing: their offsets repeat the last one
    const size_t need = static_cast<size_t>(rows + 1) * 8;
    if (T.off[side].bytes() < need) {
      DevBuf off;
      off.alloc(off_bytes(rows));
      MF_HIP(hipMemcpyAsync(off.get(), T.off[side].get(), static_cast<size_t>(T.rows[side] + 1) * 8,
                            hipMemcpyDeviceToDevice, s.stream));
      MF_HIP(hipStreamSynchronize(s.stream));
      T.off[side] = std::move(off);
    }
    launch_seen_pad(s.stream, T.off[side].as<int64_t>(), T.rows[side], rows);
    T.rows[side] = rows;
  }
  if (T.iota_n < rows + 1) {
    MF_HIP(hipStreamSynchronize(s.stream));
    T.iota_n = rows + 1 + std::max<int64_t>(1024, rows / 8);
    T.iota.alloc(static_cast<size_t>(T.iota_n) * 4);
    launch_iota(s.stream, T.iota.as<int32_t>(), T.iota_n);
  }
  v.off = T.off[side].as<int64_t>();
  v.ent = T.ent[side].as<int32_t>();
  v.iota = T.iota.as<int32_t>();
  v.any = true;
  return v;
}

void seen_debug_csr(mf_ctx* ctx, int side, int32_t* row_ids_out, int64_t* off_out, int32_t* ent_out, int32_t* ent_ids_out,
                    int64_t cap_rows, int64_t cap_nnz, int64_t* rows_out, int64_t* nnz_out) {
  Shard& s = ctx->shards[0];
  const SideLayout& QS = side_of(ctx, side);
  const SideLayout& CS = side_of(ctx, 1 - side);
  const int64_t rows = QS.rows(), nnz = seen_count(ctx);
  *rows_out = rows;
  *nnz_out = nnz;
  if (cap_rows < rows || cap_nnz < nnz) fail(MF_ERR_CAPACITY, "output capacity too small");
  std::copy(QS.row_id.begin(), QS.row_id.begin() + rows, row_ids_out);
  std::fill(off_out, off_out + rows + 1, int64_t{0});
  if (nnz == 0) return;
  DeviceGuard g(s.device);
  const SeenView v = seen_view(ctx, s, side);
  MF_HIP(hipStreamSynchronize(s.stream));
  MF_HIP(hipMemcpy(off_out, v.off, static_cast<size_t>(rows + 1) * 8, hipMemcpyDeviceToHost));
  MF_HIP(hipMemcpy(ent_out, v.ent, static_cast<size_t>(nnz) * 4, hipMemcpyDeviceToHost));
  if (ent_ids_out)
    for (int64_t x = 0; x < nnz; ++x) ent_ids_out[x] = CS.row_id[ent_out[x]];
}

void seen_merge_placement(const uint64_t* old_keys, int64_t n_old, const uint64_t* batch_keys, int64_t n_batch,
                          int64_t* old_pos, int64_t* novel_pos, int64_t* n_novel) {
  for (int64_t p = 1; p < n_old; ++p)
    MF_REQUIRE(old_keys[p - 1] < old_keys[p], "old keys must be distinct and ascending");
  std::vector<uint64_t> novel(batch_keys, batch_keys + n_batch);
  std::sort(novel.begin(), novel.end());
  novel.erase(std::unique(novel.begin(), novel.end()), novel.end());
  const uint64_t* oe = old_keys + n_old;
  novel.erase(std::remove_if(novel.begin(), novel.end(), [&](uint64_t k) { return std::binary_search(old_keys, oe, k); }),
              novel.end());
  for (int64_t p = 0; p < n_old; ++p)
    old_pos[p] = p + (std::lower_bound(novel.begin(), novel.end(), old_keys[p]) - novel.begin());
  for (size_t x = 0; x < novel.size(); ++x)
    novel_pos[x] = static_cast<int64_t>(x) + (std::lower_bound(old_keys, oe, novel[x]) - old_keys);
  *n_novel = static_cast<int64_t>(novel.size());
}

}  // namespace mfhip
