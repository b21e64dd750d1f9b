// ring.cpp -- the item-block ring between shards (the nextRatingBlock rotation,
// DSGDforMF.scala:611-619): which block moves where after a superstep (ring_step, pure: the
// testing hook mf_debug_ring_schedule exposes it), the two protocols that move it -- ring_shift on
// the compute streams, ring_shift_overlapped beside the systolic fast sweep's split launches -- the
// record of which shard holds each item block (item_loc), and consolidate, which reads it.
#include <rccl/rccl.h>

#include "common.hpp"
#include "context.hpp"

namespace mfhip {

// One step of the item-block ring after superstep s (1-based) for shard / rank g of G, n = c*G
// blocks: rating block (p, q) hands its item block to (p-1, q) (nextRatingBlock, :611-619), so
// shard g, which just ran item block (g*c + s-1) mod n in its first user block, sends it to
// shard g-1 and receives ((g+1)*c + s-1) mod n from shard g+1.
RingStep ring_step(int32_t g, int32_t G, int32_t c, int32_t n, int64_t superstep) {
  RingStep r;
  r.out_blk = static_cast<int32_t>((static_cast<int64_t>(g) * c + superstep - 1) % n);
  r.in_blk = static_cast<int32_t>((static_cast<int64_t>((g + 1) % G) * c + superstep - 1) % n);
  r.dst = (g + G - 1) % G;
  r.src = (g + 1) % G;
  return r;
}

namespace {

Shard* local_shard(mf_ctx* ctx, int global) {
  for (auto& s : ctx->shards)
    if (s.index == global) return &s;
  return nullptr;
}

int shard_of_user_block(const mf_ctx* ctx, int32_t p) { return p / ctx->c; }

// The rows of item block blk as a byte range of an item slab.
struct Span {
  size_t off, bytes;
};
Span item_block_span(const mf_ctx* ctx, int32_t blk) {
  const size_t row = static_cast<size_t>(ctx->P.num_factors) * ctx->es;
  const int64_t r0 = ctx->I.block_start[blk], cnt = ctx->I.block_start[blk + 1] - r0;
  return {static_cast<size_t>(r0) * row, static_cast<size_t>(cnt) * row};
}

// Every shard's leaving block is held by its receiver once the ring step after `superstep` ran.
void note_ring_step(mf_ctx* ctx, int64_t superstep) {
  for (int32_t g = 0; g < ctx->G; ++g) {
    const RingStep rs = ring_step(g, ctx->G, ctx->c, ctx->nb, superstep);
    ctx->item_loc[rs.out_blk] = rs.dst;
  }
}

// The ring step with the overlap of fast_superstep's split launches: the block leaving shard g
// is the item block of its local block 0, done when launch A is, so it moves on the comm stream
// behind A while launch B (block c-1) still runs; the arriving block is first needed by the next
// superstep's launch B, which waits for ev_moved.
void ring_shift_overlapped(mf_ctx* ctx, int64_t superstep) {
  const int32_t n = ctx->nb;
  if (ctx->rank_mode) {
    Shard& s = ctx->shards[0];
    DeviceGuard g(s.device);
    const RingStep rs = ring_step(s.index, ctx->G, ctx->c, n, superstep);
    const Span out = item_block_span(ctx, rs.out_blk), in = item_block_span(ctx, rs.in_blk);
    char* base = s.itf.as<char>();
    MF_HIP(hipStreamWaitEvent(s.comm, s.ev_front, 0));
    MF_NCCL(ncclGroupStart());
    if (out.bytes > 0) MF_NCCL(ncclSend(base + out.off, out.bytes / ctx->es, ncclFloat32, rs.dst, ctx->comm, s.comm));
    if (in.bytes > 0) MF_NCCL(ncclRecv(base + in.off, in.bytes / ctx->es, ncclFloat32, rs.src, ctx->comm, s.comm));
    MF_NCCL(ncclGroupEnd());
    MF_HIP(hipEventRecord(s.ev_moved, s.comm));
  } else {
    // the sender copies its leaving block into the receiver's slab on its comm stream once its
    // launch A is done; the receiver's next launch B waits for that copy
    for (auto& src : ctx->shards) {
      const RingStep rs = ring_step(src.index, ctx->G, ctx->c, n, superstep);
      Shard& dst = *local_shard(ctx, rs.dst);
      const Span out = item_block_span(ctx, rs.out_blk);
      DeviceGuard g(src.device);
      MF_HIP(hipStreamWaitEvent(src.comm, src.ev_front, 0));
      if (out.bytes > 0)
        MF_HIP(hipMemcpyPeerAsync(dst.itf.as<char>() + out.off, dst.device, src.itf.as<char>() + out.off, src.device,
                                  out.bytes, src.comm));
      MF_HIP(hipEventRecord(src.done, src.comm));
    }
    for (auto& dst : ctx->shards) {
      Shard& src = *local_shard(ctx, ring_step(dst.index, ctx->G, ctx->c, n, superstep).src);
      DeviceGuard g(dst.device);
      MF_HIP(hipStreamWaitEvent(dst.comm, src.done, 0));
      MF_HIP(hipEventRecord(dst.ev_moved, dst.comm));
    }
  }
  note_ring_step(ctx, superstep);
}

}  // namespace

// nextRatingBlock rotation (:611-619) across shards after superstep s.
void ring_shift(mf_ctx* ctx, int64_t superstep) {
  if (ctx->G <= 1) return;
  if (ctx->ring_overlap) {
    ring_shift_overlapped(ctx, superstep);
    return;
  }
  const int32_t n = ctx->nb;
  if (ctx->rank_mode) {
    Shard& s = ctx->shards[0];
    DeviceGuard g(s.device);
    const RingStep rs = ring_step(s.index, ctx->G, ctx->c, n, superstep);
    const Span out = item_block_span(ctx, rs.out_blk), in = item_block_span(ctx, rs.in_blk);
    const ncclDataType_t type = ctx->f64 ? ncclFloat64 : ncclFloat32;
    char* base = s.itf.as<char>();
    MF_NCCL(ncclGroupStart());
    if (out.bytes > 0) MF_NCCL(ncclSend(base + out.off, out.bytes / ctx->es, type, rs.dst, ctx->comm, s.stream));
    if (in.bytes > 0) MF_NCCL(ncclRecv(base + in.off, in.bytes / ctx->es, type, rs.src, ctx->comm, s.stream));
    MF_NCCL(ncclGroupEnd());
  } else {
    // in-process shards: peer copy on the sender's stream, receiver waits on an event
    for (auto& src : ctx->shards) {
      DeviceGuard g(src.device);
      MF_HIP(hipEventRecord(src.done, src.stream));
    }
    for (auto& src : ctx->shards) {
      const RingStep rs = ring_step(src.index, ctx->G, ctx->c, n, superstep);
      Shard& dst = *local_shard(ctx, rs.dst);
      const Span out = item_block_span(ctx, rs.out_blk);
      if (out.bytes == 0) continue;
      DeviceGuard g(src.device);
      MF_HIP(hipStreamWaitEvent(src.stream, dst.done, 0));  // dst finished superstep s
      MF_HIP(hipMemcpyPeerAsync(dst.itf.as<char>() + out.off, dst.device, src.itf.as<char>() + out.off, src.device,
                                out.bytes, src.stream));
    }
    for (auto& src : ctx->shards) {
      DeviceGuard g(src.device);
      MF_HIP(hipEventRecord(src.done, src.stream));
    }
    for (auto& dst : ctx->shards) {
      Shard& src = *local_shard(ctx, ring_step(dst.index, ctx->G, ctx->c, n, superstep).src);
      DeviceGuard g(dst.device);
      MF_HIP(hipStreamWaitEvent(dst.stream, src.done, 0));
    }
  }
  note_ring_step(ctx, superstep);
}

void reset_item_loc(mf_ctx* ctx) {
  ctx->item_loc.assign(ctx->nb, 0);
  for (int32_t q = 0; q < ctx->nb; ++q) ctx->item_loc[q] = q / ctx->c;
  if (ctx->G > 1)
    for (int64_t s = 1; s <= ctx->superstep_done; ++s) note_ring_step(ctx, s);
}

// Make every row current on shard `dst` (users from their owners, items from their holders).
void consolidate(mf_ctx* ctx, Shard& dst) {
  if (ctx->G <= 1 || ctx->rank_mode || !ctx->prepared) return;
  const size_t k = static_cast<size_t>(ctx->P.num_factors);
  sync_all(ctx);
  for (int32_t b = 0; b < ctx->nb; ++b) {
    for (int side = 0; side < 2; ++side) {
      const SideLayout& S = side_of(ctx, side);
      const int owner = side == kSideU ? shard_of_user_block(ctx, b) : ctx->item_loc[b];
      if (owner == dst.index) continue;
      Shard& src = *local_shard(ctx, owner);
      const int64_t r0 = S.block_start[b], cnt = S.block_start[b + 1] - r0;
      if (cnt == 0) continue;
      const size_t off = static_cast<size_t>(r0) * k * ctx->es, bytes = static_cast<size_t>(cnt) * k * ctx->es;
      DevBuf& sb = side == kSideU ? src.uf : src.itf;
      DevBuf& db = side == kSideU ? dst.uf : dst.itf;
      DeviceGuard g(dst.device);
      MF_HIP(hipMemcpyPeerAsync(db.as<char>() + off, dst.device, sb.as<char>() + off, src.device, bytes, dst.stream));
    }
  }
  DeviceGuard g(dst.device);
  MF_HIP(hipStreamSynchronize(dst.stream));
}

}  // namespace mfhip
