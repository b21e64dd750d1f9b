// kernels_bpr.hip -- one synchronous minibatch step of BPR training (mf_bpr_run, mf_bpr_step_triples; the
// contract is in include/mfhip.h, the draw and the gradient weight in bpr_draw.hpp).  Compiled without FP
// contraction: every product is rounded before it is added, which is what mfhip/bpr.py replays.
//
//  draw      one thread per slot: the positive's entry, its row by row_of, then up to 1 + redraws negatives,
//            each checked against the user's sorted table row (csr_search.hpp).  Or, for caller-given triples,
//            resolve: the looked-up rows with unknown ids and pos == neg made void.
//  keys      per slot one user key (row << 24 | slot) and two item keys (row << 25 | slot << 1 | negative); a
//            void slot takes the row past the side's last, so it sorts behind every segment.
//  gradient  one wave per slot: lane l forms partial l of p_u . (q_i - q_j) over f = l, l + 64, ..., the 64
//            partials are added by the butterfly xor 32 .. 1 (every lane ends with the same sum), and
//            g = 1 / (1 + E(x)) is evaluated in f64 and rounded to T.
//  sorts     two stable radix sorts over the row bits alone (the slot bits ascend already).
//  apply     a wave owns 64 consecutive sorted positions and runs the chunks that begin there: position p
//            begins a chunk when p - (its segment's start) is a multiple of the chunk length C.  A segment of at
//            most C entries is summed and its row finished by that one wave.  A longer one leaves one sum per
//            chunk in a small slab and is finished by the combine launch, which adds them in ascending order.
//            Chunk slots need no count from a scan: an aligned window of C positions holds at most two chunk
//            starts of segments longer than C, one of a segment that began before the window and one of a
//            segment that begins in it, so slot = 2 * (p / C) + (start >= window).
//  commit    user rows are written to a scratch first (the item apply still reads the old ones) and copied
//            into the model last; item rows are written in place: the item apply reads no item row but its
//            own, and the user apply, which reads them, has finished by then.
// No floating-point atomics anywhere; the integer ones only count.
#include <hip/hip_runtime.h>

#include "bpr_draw.hpp"
#include "common.hpp"
#include "csr_search.hpp"
#include "id_index.hpp"
#include "kernels.hpp"
#include "radix_sort_cfg.hpp"

namespace mfhip {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNF = kBprMaxRank / 64;  // factors per lane

__device__ __forceinline__ void count_wave(bool flag, int64_t* counter) {
  const int tot = __popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0 && tot) atomicAdd(reinterpret_cast<unsigned long long*>(counter), static_cast<unsigned long long>(tot));
}

// trip: user rows [B], positive rows [B], negative rows [B]; a void slot has kRowMiss as its user row.
__global__ __launch_bounds__(kThreads) void k_bpr_draw(const int64_t* __restrict__ off, const int32_t* __restrict__ ent,
                                                      int64_t rows, uint64_t pairs, uint32_t pool, uint64_t seed,
                                                      uint64_t step, uint32_t B, uint32_t redraws,
                                                      uint32_t* __restrict__ trip) {
  const uint32_t s = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;
  if (s >= B) return;
  const int64_t e = static_cast<int64_t>(bpr_entry(bpr_draw_bits(seed, step, s, 0), pairs));
  const int64_t u = dev::row_of(off, 0, rows - 1, e);
  const uint32_t i = static_cast<uint32_t>(ent[e]);
  const int64_t b0 = off[u], b1 = off[u + 1];
  uint32_t j = kRowMiss;
  for (uint32_t r = 1; r <= 1 + redraws; ++r) {
    const uint32_t c = neg_pick_row(bpr_draw_bits(seed, step, s, r), pool, i);
    if (!dev::contains(ent, b0, b1, static_cast<int32_t>(c))) {
      j = c;
      break;
    }
  }
  const bool ok = j != kRowMiss;
  trip[s] = ok ? static_cast<uint32_t>(u) : kRowMiss;
  trip[B + s] = i;
  trip[2 * static_cast<size_t>(B) + s] = ok ? j : i;
}

// Caller-given triples after the id lookups: unknown ids and pos == neg make a slot void.
__global__ __launch_bounds__(kThreads) void k_bpr_resolve(uint32_t* __restrict__ trip, uint32_t B) {
  const uint32_t s = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;
  if (s >= B) return;
  const uint32_t u = trip[s], i = trip[B + s], j = trip[2 * static_cast<size_t>(B) + s];
  if (u == kRowMiss || i == kRowMiss || j == kRowMiss || i == j) trip[s] = kRowMiss;
}

__global__ __launch_bounds__(kThreads) void k_bpr_keys(const uint32_t* __restrict__ trip, uint32_t B, uint32_t nU,
                                                      uint32_t nI, uint64_t* __restrict__ ukey,
                                                      uint64_t* __restrict__ ikey, int64_t* __restrict__ stats) {
  const uint32_t s = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;
  bool is_void = false;
  if (s < B) {
    const uint32_t u = trip[s];
    is_void = u == kRowMiss;
    const uint64_t ur = is_void ? nU : u;
    const uint64_t ir = is_void ? nI : trip[B + s], jr = is_void ? nI : trip[2 * static_cast<size_t>(B) + s];
    ukey[s] = (ur << kBprSlotBits) | s;
    ikey[2 * static_cast<size_t>(s)] = (ir << (kBprSlotBits + 1)) | (static_cast<uint64_t>(s) << 1);
    ikey[2 * static_cast<size_t>(s) + 1] = (jr << (kBprSlotBits + 1)) | (static_cast<uint64_t>(s) << 1) | 1u;
  }
  count_wave(is_void, stats + 1);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_bpr_grad(const uint32_t* __restrict__ trip, uint32_t B,
                                                      const T* __restrict__ P, const T* __restrict__ Q, int k,
                                                      T* __restrict__ g) {
  const uint32_t s = blockIdx.x * static_cast<uint32_t>(kWaves) + (threadIdx.x >> 6);
  if (s >= B) return;
  const uint32_t u = trip[s];
  if (u == kRowMiss) return;
  const int lane = threadIdx.x & 63;
  const T* __restrict__ p = P + static_cast<size_t>(u) * k;
  const T* __restrict__ qi = Q + static_cast<size_t>(trip[B + s]) * k;
  const T* __restrict__ qj = Q + static_cast<size_t>(trip[2 * static_cast<size_t>(B) + s]) * k;
  T pv[kNF], av[kNF], bv[kNF];
#pragma unroll
  for (int c = 0; c < kNF; ++c) {
    const int f = lane + 64 * c;
    const bool in = f < k;
    pv[c] = in ? p[f] : T(0);
    av[c] = in ? qi[f] : T(0);
    bv[c] = in ? qj[f] : T(0);
  }
  T x = T(0);
#pragma unroll
  for (int c = 0; c < kNF; ++c) {
    if (lane + 64 * c < k) {
      const T d = av[c] - bv[c];
      const T m = pv[c] * d;
      x = x + m;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, 64);
  if (lane == 0) g[s] = static_cast<T>(bpr_weight(static_cast<double>(x)));
}

// What the apply kernels share.  SHIFT: the key's row shift (kBprSlotBits for users, one more for items).
template <int SHIFT>
__device__ __forceinline__ uint32_t key_row(uint64_t key) { return static_cast<uint32_t>(key >> SHIFT); }

// The first position of row's segment, given that position p belongs to it.
template <int SHIFT>
__device__ __forceinline__ int64_t seg_start(const uint64_t* __restrict__ key, int64_t p, uint32_t row) {
  return dev::lower(key, int64_t{0}, p, static_cast<uint64_t>(row) << SHIFT);
}

__device__ __forceinline__ int64_t chunk_slot(int64_t p, int64_t start, int64_t C) {
  const int64_t w = p / C;
  return 2 * w + (start >= w * C ? 1 : 0);
}

// x' = x + lr * (c * acc - lm * x), each operation rounded.
template <typename T>
__device__ __forceinline__ T finish(T x, T acc, T c, T lm, T lr) {
  const T t1 = c * acc;
  const T t2 = lm * x;
  const T t3 = t1 - t2;
  const T t4 = lr * t3;
  return x + t4;
}

template <typename T>
struct ApplyArgs {
  const uint64_t* key;  // sorted
  int64_t n;            // keys
  uint32_t rows;        // the side's rows (the void row)
  int64_t C;            // chunk length
  const uint32_t* trip;
  uint32_t B;
  const T* g;
  const T* P;  // user rows as the step found them
  const T* Q;  // item rows as the step found them (the item apply writes them)
  T* out;      // users: the scratch; items: Q itself
  int by_row;  // users: the scratch is indexed by row (else by the segment's first position)
  T* csum;     // chunk sums of the long segments
  int k;
  T lr, lambda;
  int mean;
  int64_t* stats;
};

// What an entry names, read by the lane that holds it and handed to the wave by shuffles: its slot's weight
// and the rows it gathers (users: the positive and the negative item row; items: the user row and the sign).
template <typename T>
struct EntryMeta {
  T g;
  uint32_t ra, rb;
};

template <typename T, bool ITEM>
__device__ __forceinline__ EntryMeta<T> entry_meta(const ApplyArgs<T>& A, uint64_t key) {
  EntryMeta<T> m;
  if (!ITEM) {
    const uint32_t s = static_cast<uint32_t>(key) & ((1u << kBprSlotBits) - 1);
    m.g = A.g[s];
    m.ra = A.trip[A.B + s];
    m.rb = A.trip[2 * static_cast<size_t>(A.B) + s];
  } else {
    const uint32_t s = (static_cast<uint32_t>(key) >> 1) & ((1u << kBprSlotBits) - 1);
    m.g = A.g[s];
    m.ra = A.trip[s];
    m.rb = static_cast<uint32_t>(key) & 1u;
  }
  return m;
}

// One contribution: ITEM = false, g * (q_i - q_j) of the slot; ITEM = true, +- g * p_u.
template <typename T, bool ITEM>
__device__ __forceinline__ void add_entry(const ApplyArgs<T>& A, T gs, uint32_t ra, uint32_t rb, int lane,
                                          T (&acc)[kNF]) {
  const int k = A.k;
  if (!ITEM) {
    const T* __restrict__ qi = A.Q + static_cast<size_t>(ra) * k;
    const T* __restrict__ qj = A.Q + static_cast<size_t>(rb) * k;
#pragma unroll
    for (int c = 0; c < kNF; ++c) {
      const int f = lane + 64 * c;
      if (f < k) {
        const T d = qi[f] - qj[f];
        const T m = gs * d;
        acc[c] = acc[c] + m;
      }
    }
  } else {
    const T* __restrict__ p = A.P + static_cast<size_t>(ra) * k;
#pragma unroll
    for (int c = 0; c < kNF; ++c) {
      const int f = lane + 64 * c;
      if (f < k) {
        const T m = gs * p[f];
        acc[c] = rb ? acc[c] - m : acc[c] + m;
      }
    }
  }
}

// The row of a finished segment of n_seg entries: acc holds the chain (or the sum of the chunk sums).
template <typename T, bool ITEM>
__device__ __forceinline__ void finish_row(const ApplyArgs<T>& A, uint32_t row, int64_t start, int64_t n_seg, int lane,
                                           const T (&acc)[kNF]) {
  const int k = A.k;
  const T cnt = static_cast<T>(n_seg);
  const T c = A.mean ? T(1) / cnt : T(1);
  const T lm = A.mean ? A.lambda : A.lambda * cnt;
  const T* __restrict__ x = (ITEM ? A.Q : A.P) + static_cast<size_t>(row) * k;
  T* __restrict__ o = A.out + static_cast<size_t>(ITEM || A.by_row ? static_cast<int64_t>(row) : start) * k;
#pragma unroll
  for (int cc = 0; cc < kNF; ++cc) {
    const int f = lane + 64 * cc;
    if (f < k) o[f] = finish(x[f], acc[cc], c, lm, A.lr);
  }
}

template <typename T, bool ITEM>
__global__ __launch_bounds__(kThreads) void k_bpr_apply(const ApplyArgs<T> A) {
  constexpr int SHIFT = ITEM ? kBprSlotBits + 1 : kBprSlotBits;
  const int lane = threadIdx.x & 63;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6)) * 64;
  if (base >= A.n) return;
  const int64_t p = base + lane;
  // does a chunk begin at p?
  bool lead = false, head = false;
  int64_t start = p;
  uint32_t row = A.rows;
  if (p < A.n) {
    row = key_row<SHIFT>(A.key[p]);
    if (row < A.rows) {
      head = p == 0 || key_row<SHIFT>(A.key[p - 1]) != row;
      if (head) {
        lead = true;
      } else if (p >= A.C && key_row<SHIFT>(A.key[p - A.C]) == row) {  // a long segment: where does it begin?
        start = seg_start<SHIFT>(A.key, p, row);
        lead = (p - start) % A.C == 0;
      }
    }
  }
  count_wave(head, A.stats + (ITEM ? 3 : 2));
  uint64_t todo = __ballot(lead);
  while (todo) {
    const int l = __ffsll(static_cast<long long>(todo)) - 1;
    todo &= todo - 1;
    const int64_t p0 = base + l;
    const uint32_t r0 = static_cast<uint32_t>(__shfl(static_cast<int>(row), l, 64));
    const int64_t s0 = (static_cast<int64_t>(static_cast<uint32_t>(__shfl(static_cast<int>(start >> 32), l, 64))) << 32) |
                       static_cast<uint32_t>(__shfl(static_cast<int>(start), l, 64));
    const int64_t lim = p0 + A.C < A.n ? p0 + A.C : A.n;
    T acc[kNF];
#pragma unroll
    for (int c = 0; c < kNF; ++c) acc[c] = T(0);
    int64_t e = p0;
    for (;;) {  // 64 entries at a time: every lane reads one entry's key and what it names
      const int64_t mine = e + lane;
      bool in = false;
      EntryMeta<T> m{T(0), 0u, 0u};
      if (mine < lim) {
        const uint64_t key = A.key[mine];
        in = key_row<SHIFT>(key) == r0;
        if (in) m = entry_meta<T, ITEM>(A, key);
      }
      const uint64_t out = ~__ballot(in);
      const int cnt = out ? __ffsll(static_cast<long long>(out)) - 1 : 64;  // the segment's entries among them
      const auto one = [&](int t) {
        add_entry<T, ITEM>(A, __shfl(m.g, t, 64), static_cast<uint32_t>(__shfl(static_cast<int>(m.ra), t, 64)),
                           static_cast<uint32_t>(__shfl(static_cast<int>(m.rb), t, 64)), lane, acc);
      };
      int t = 0;
      for (; t + 4 <= cnt; t += 4) {  // four entries' rows in flight; the chain stays in entry order
        one(t);
        one(t + 1);
        one(t + 2);
        one(t + 3);
      }
      for (; t < cnt; ++t) one(t);
      e += cnt;
      if (cnt < 64) break;
    }
    const bool more = e < A.n && key_row<SHIFT>(A.key[e]) == r0;
    if (s0 == p0 && !more) {
      finish_row<T, ITEM>(A, r0, s0, e - p0, lane, acc);
    } else {
      T* __restrict__ cs = A.csum + static_cast<size_t>(chunk_slot(p0, s0, A.C)) * A.k;
#pragma unroll
      for (int c = 0; c < kNF; ++c) {
        const int f = lane + 64 * c;
        if (f < A.k) cs[f] = acc[c];
      }
    }
  }
}

// The segments longer than C: their chunk sums added to 0 in ascending order, then the row.
template <typename T, bool ITEM>
__global__ __launch_bounds__(kThreads) void k_bpr_combine(const ApplyArgs<T> A) {
  constexpr int SHIFT = ITEM ? kBprSlotBits + 1 : kBprSlotBits;
  const int lane = threadIdx.x & 63;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6)) * 64;
  if (base >= A.n) return;
  const int64_t p = base + lane;
  bool lead = false;
  uint32_t row = A.rows;
  if (p + A.C < A.n) {
    row = key_row<SHIFT>(A.key[p]);
    lead = row < A.rows && (p == 0 || key_row<SHIFT>(A.key[p - 1]) != row) && key_row<SHIFT>(A.key[p + A.C]) == row;
  }
  uint64_t todo = __ballot(lead);
  while (todo) {
    const int l = __ffsll(static_cast<long long>(todo)) - 1;
    todo &= todo - 1;
    const int64_t s0 = base + l;
    const uint32_t r0 = static_cast<uint32_t>(__shfl(static_cast<int>(row), l, 64));
    const int64_t end = dev::lower(A.key, s0, A.n, (static_cast<uint64_t>(r0) + 1) << SHIFT);
    T acc[kNF];
#pragma unroll
    for (int c = 0; c < kNF; ++c) acc[c] = T(0);
    for (int64_t q = s0; q < end; q += A.C) {
      const T* __restrict__ cs = A.csum + static_cast<size_t>(chunk_slot(q, s0, A.C)) * A.k;
#pragma unroll
      for (int c = 0; c < kNF; ++c) {
        const int f = lane + 64 * c;
        if (f < A.k) acc[c] = acc[c] + cs[f];
      }
    }
    finish_row<T, ITEM>(A, r0, s0, end - s0, lane, acc);
  }
}

// P[row] = scratch row of every user segment.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_bpr_commit(const uint64_t* __restrict__ key, int64_t n, uint32_t rows,
                                                        const T* __restrict__ scratch, int by_row, T* __restrict__ P,
                                                        int k) {
  const int lane = threadIdx.x & 63;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6)) * 64;
  if (base >= n) return;
  const int64_t p = base + lane;
  bool head = false;
  uint32_t row = rows;
  if (p < n) {
    row = key_row<kBprSlotBits>(key[p]);
    head = row < rows && (p == 0 || key_row<kBprSlotBits>(key[p - 1]) != row);
  }
  uint64_t todo = __ballot(head);
  while (todo) {
    const int l = __ffsll(static_cast<long long>(todo)) - 1;
    todo &= todo - 1;
    const uint32_t r0 = static_cast<uint32_t>(__shfl(static_cast<int>(row), l, 64));
    const T* __restrict__ src = scratch + static_cast<size_t>(by_row ? static_cast<int64_t>(r0) : base + l) * k;
    T* __restrict__ dst = P + static_cast<size_t>(r0) * k;
    for (int f = lane; f < k; f += 64) dst[f] = src[f];
  }
}

unsigned grid_slots(int64_t n, int per_block) { return static_cast<unsigned>((n + per_block - 1) / per_block); }

void sort_rows(hipStream_t st, DevBuf& tmp, const uint64_t* kin, uint64_t* kout, int64_t n, int begin_bit, uint32_t rows) {
  const int end_bit = begin_bit + radix_bits_for(static_cast<uint64_t>(rows) + 1);
  size_t tb = 0;
  MF_HIP(rocprim::radix_sort_keys<SortCfg>(nullptr, tb, kin, kout, static_cast<unsigned int>(n), begin_bit, end_bit, st));
  void* const t = temp_storage(st, tmp, tb);
  MF_HIP(rocprim::radix_sort_keys<SortCfg>(t, tb, kin, kout, static_cast<unsigned int>(n), begin_bit, end_bit, st));
}

template <typename T>
void step_t(const BprStep& L, BprScratch& sc, const BprLap& lap_fn) {
  hipStream_t st = L.st;
  const auto lap = [&](const char* what) {
    if (lap_fn) lap_fn(what);
  };
  const int64_t B = L.batch;
  const uint32_t* trip = sc.trip.as<uint32_t>();
  T* g = sc.g.as<T>();
  T* P = static_cast<T*>(L.P);
  T* Q = static_cast<T*>(L.Q);
  hipLaunchKernelGGL(k_bpr_keys, dim3(grid_slots(B, kThreads)), dim3(kThreads), 0, st, trip, static_cast<uint32_t>(B),
                     L.user_rows, L.item_rows, sc.ukey.as<uint64_t>(), sc.ikey.as<uint64_t>(), sc.stats.as<int64_t>());
  hipLaunchKernelGGL(k_bpr_grad<T>, dim3(grid_slots(B, kWaves)), dim3(kThreads), 0, st, trip, static_cast<uint32_t>(B), P,
                     Q, L.k, g);
  lap("bpr_step: keys + weights");
  sort_rows(st, sc.tmp, sc.ukey.as<uint64_t>(), sc.ukey2.as<uint64_t>(), B, kBprSlotBits, L.user_rows);
  sort_rows(st, sc.tmp, sc.ikey.as<uint64_t>(), sc.ikey2.as<uint64_t>(), 2 * B, kBprSlotBits + 1, L.item_rows);
  lap("bpr_step: sorts");
  ApplyArgs<T> A{};
  A.C = L.chunk;
  A.trip = trip;
  A.B = static_cast<uint32_t>(B);
  A.g = g;
  A.P = P;
  A.Q = Q;
  A.k = L.k;
  A.lr = static_cast<T>(L.lr);
  A.lambda = static_cast<T>(L.lambda);
  A.mean = L.mean ? 1 : 0;
  A.stats = sc.stats.as<int64_t>();
  // users, into the scratch
  A.key = sc.ukey2.as<uint64_t>();
  A.n = B;
  A.rows = L.user_rows;
  A.out = sc.urows.as<T>();
  A.by_row = sc.by_row ? 1 : 0;
  A.csum = sc.csum.as<T>();
  const unsigned gu = grid_slots(B, 64 * kWaves);
  hipLaunchKernelGGL((k_bpr_apply<T, false>), dim3(gu), dim3(kThreads), 0, st, A);
  if (B > L.chunk) hipLaunchKernelGGL((k_bpr_combine<T, false>), dim3(gu), dim3(kThreads), 0, st, A);
  lap("bpr_step: user apply");
  // items, in place
  A.key = sc.ikey2.as<uint64_t>();
  A.n = 2 * B;
  A.rows = L.item_rows;
  A.out = Q;
  A.by_row = 1;
  const unsigned gi = grid_slots(2 * B, 64 * kWaves);
  hipLaunchKernelGGL((k_bpr_apply<T, true>), dim3(gi), dim3(kThreads), 0, st, A);
  if (2 * B > L.chunk) hipLaunchKernelGGL((k_bpr_combine<T, true>), dim3(gi), dim3(kThreads), 0, st, A);
  lap("bpr_step: item apply");
  hipLaunchKernelGGL(k_bpr_commit<T>, dim3(gu), dim3(kThreads), 0, st, sc.ukey2.as<uint64_t>(), B, L.user_rows,
                     sc.urows.as<T>(), sc.by_row ? 1 : 0, P, L.k);
  lap("bpr_step: commit");
  MF_HIP(hipGetLastError());
}

}  // namespace

void bpr_reserve(hipStream_t st, BprScratch& sc, int64_t batch, int64_t user_rows, int k, size_t es, int64_t chunk) {
  MF_HIP(hipStreamSynchronize(st));
  const size_t B = static_cast<size_t>(batch);
  sc.trip.alloc(3 * B * 4);
  sc.g.alloc(B * es);
  sc.ukey.alloc(B * 8);
  sc.ukey2.alloc(B * 8);
  sc.ikey.alloc(2 * B * 8);
  sc.ikey2.alloc(2 * B * 8);
  sc.by_row = user_rows <= batch;
  sc.urows.alloc(static_cast<size_t>(std::min<int64_t>(user_rows, batch)) * k * es);
  // the items' 2 * batch keys need the most windows; the user apply has finished with the slab by then
  sc.csum.alloc(2 * static_cast<size_t>((2 * batch + chunk - 1) / chunk) * k * es);
  sc.stats.alloc(4 * 8);
  // the sorts' storage, sized now so that no step waits for it
  size_t tb = 0, tb2 = 0;
  MF_HIP(rocprim::radix_sort_keys<SortCfg>(nullptr, tb, sc.ukey.as<uint64_t>(), sc.ukey2.as<uint64_t>(),
                                           static_cast<unsigned int>(batch), 0, 64, st));
  MF_HIP(rocprim::radix_sort_keys<SortCfg>(nullptr, tb2, sc.ikey.as<uint64_t>(), sc.ikey2.as<uint64_t>(),
                                           static_cast<unsigned int>(2 * batch), 0, 64, st));
  temp_storage(st, sc.tmp, std::max(tb, tb2));
}

void launch_bpr_draw(const BprStep& L, BprScratch& sc, const int64_t* off, const int32_t* ent, int64_t table_rows,
                     int64_t pairs, int64_t seed, int64_t step, int32_t redraws) {
  hipLaunchKernelGGL(k_bpr_draw, dim3(grid_slots(L.batch, kThreads)), dim3(kThreads), 0, L.st, off, ent, table_rows,
                     static_cast<uint64_t>(pairs), L.item_rows, static_cast<uint64_t>(seed), static_cast<uint64_t>(step),
                     static_cast<uint32_t>(L.batch), static_cast<uint32_t>(redraws), sc.trip.as<uint32_t>());
  MF_HIP(hipGetLastError());
}

void launch_bpr_resolve(const BprStep& L, BprScratch& sc) {
  hipLaunchKernelGGL(k_bpr_resolve, dim3(grid_slots(L.batch, kThreads)), dim3(kThreads), 0, L.st, sc.trip.as<uint32_t>(),
                     static_cast<uint32_t>(L.batch));
  MF_HIP(hipGetLastError());
}

void launch_bpr_step(const BprStep& L, BprScratch& sc, const BprLap& lap) {
  MF_REQUIRE(L.batch >= 1 && L.batch <= kBprMaxBatch && L.k >= 1 && L.k <= kBprMaxRank && L.chunk >= 1,
             "BPR step: bad launch shape");
  if (L.f64) step_t<double>(L, sc, lap);
  else step_t<float>(L, sc, lap);
}

}  // namespace mfhip
