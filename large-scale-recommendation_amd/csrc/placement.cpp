// placement.cpp -- the launch tables of the two persistent sweeps, as pure host functions: the
// deterministic split sweep's slot table (det_slot_table) and the systolic fast sweep's block ->
// wave maps (sys_placement and its parts).  Both decide whether a launch can finish at all -- a
// block past the co-resident limit never starts and the ticket sweep waits for it; a wave missing
// from the block -> wave map stalls its neighbours -- so nothing here touches a device or a
// context: the tables can be checked on a CPU machine before anything is launched
// (mf_debug_det_slot_table, mf_debug_sys_placement; tests/test_placement.py).  Declared in plan.hpp.
#include <algorithm>
#include <array>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "plan.hpp"

namespace mfhip {

// The split sweep's slot table (kernels.hpp launch_det_sweep_split), in place over the nw waves of
// build_det_step (the buffer holds det_slot_room(nw)): each single-item wave with its helper slot,
// longest first (block 0 is the hottest chain), then the other waves two per block; empty waves
// dropped.  The chains within half of the longest (at most kDetAlone) bound the superstep, so they
// get a CU each: the dispatcher deals block b to XCD b % 8 and, inside it, CU (b / 8) % (cus / 8),
// so blocks b + cus m share block b's CU (period = the device's CU count, 256 on MI355X) -- those
// positions stay empty (both waves leave at once) while the table has at most max_blocks blocks
// (the co-resident limit: a block past it would never start and the ticket sweep would hang).
// Returns the slot count (even).
constexpr int64_t kDetAlone = 64;
// H <= period / 2 chains keep their CU, so at most half of the positions are empty: <= 4 nw slots
int64_t det_slot_room(int64_t nw) { return 4 * nw + 4; }
int64_t det_slot_table(DetWave* waves, int64_t nw, int64_t max_blocks, bool alone, int64_t period) {
  period = std::max<int64_t>(period, 8);
  std::vector<DetWave> single, multi;
  for (int64_t w = 0; w < nw; ++w) {
    if (waves[w].count == 0) continue;
    ((waves[w].flags & kDetWaveSingleItem) ? single : multi).push_back(waves[w]);
  }
  std::stable_sort(single.begin(), single.end(), [](const DetWave& a, const DetWave& b) { return a.count > b.count; });
  std::vector<std::array<DetWave, 2>> blocks;
  for (const DetWave& d : single) blocks.push_back({d, DetWave{d.begin, 0, kDetWaveHelper}});
  for (size_t x = 0; x < multi.size(); x += 2)
    blocks.push_back({multi[x], x + 1 < multi.size() ? multi[x + 1] : DetWave{0, 0, 0}});
  if (blocks.empty()) blocks.push_back({DetWave{0, 0, 0}, DetWave{0, 0, 0}});
  int64_t H = 0;  // chains that get a CU each
  if (alone)
    while (H < std::min<int64_t>(kDetAlone, static_cast<int64_t>(single.size())) && 2 * single[H].count >= single[0].count)
      ++H;
  const int64_t nb = static_cast<int64_t>(blocks.size());
  int64_t empties = 0;
  H = std::min(H, period / 2);
  for (int64_t b = period; b < nb + empties; ++b) empties += (b % period) < H;
  if (nb + empties > max_blocks) empties = 0, H = 0;  // no room: the plain order
  MF_REQUIRE(nb <= max_blocks, "det slot table: more blocks than can be resident at once");
  int64_t n = 0, next = 0;
  for (int64_t b = 0; next < nb; ++b) {
    if (b >= period && (b % period) < H) {
      waves[n++] = DetWave{0, 0, 0};
      waves[n++] = DetWave{0, 0, 0};
    } else {
      waves[n++] = blocks[next][0];
      waves[n++] = blocks[next][1];
      ++next;
    }
  }
  return n;
}

// Block -> wave map of one systolic launch.  Measured (profiles/r03_placement_NFLX.txt): the
// dispatcher deals a launch's blocks round-robin over the 8 XCDs (b % 8) and, inside an XCD, over
// its 32 CUs in block order, so the XCD's blocks k, k + 32, k + 64 (k = b / 8) share a CU -- every
// one of 4768 block pairs (b, b + 256) in two traced fits did.  And a wave's pair step slows with
// every other busy wave on its CU (NFLX single-run pairs: 127 ns alone, 173 ns with one other
// wave, 206 ns with two; mixed pairs 214 / 248 ns): the CU's shared vector-memory path, not the
// SIMD (no two waves ever shared one).  So each XCD keeps its contiguous wave range (the hand-offs
// stay in one L2), and inside it the heaviest waves (modelled time) take the CUs that hold the
// fewest waves, with the lightest waves as their partners.  Placement only: results are
// identical (tests compare with the per-sub-step launches bit for bit).  MFHIP_SYS_PLACE=0: the
// plain XCD-contiguous map.  Measured and dropped: per-CU wave counts chosen against a crowding
// factor (1 / 1.3 / 1.52 / 1.8 per waves on the CU), spare slots padded with empty blocks -- NFLX
// 21.6 vs 21.3 ms, ML20M equal (profiles/r03_placement_NFLX.txt).  Kept since round 6: one empty
// block per XCD as the heaviest wave's partner, so each rating block's hot-item wave has a CU to
// itself (NFLX 19.88 -> 19.74 ms, profiles/r06_sys_isolation_ab.txt; single-run pairs now weigh
// 185 ns: at 171 the hot wave sometimes ranked 16th-54th of its XCD).
// The modelled time of wave w of pp.sys_waves.
double sys_wave_load(const PairPlan& pp, int64_t w) {
  const SysWave& sw = pp.sys_waves[w];
  double load = 0.0;
  for (int32_t t = 0; t < sw.G; ++t) {
    const WaveDesc& d = pp.sys[sw.cell0 + t];
    if (d.steps > 0) load += 2000.0 + d.steps * (d.cells == kWaveSingleRun || d.cells == kWaveSingleRunFwd ? 185.0 : 218.0);
  }
  return load;
}

// The map of a launch of nw waves with loads load[0 .. nw): place[b] = the wave of block b.
// pad (>= 0): empty blocks per XCD (place = -1, they exit at once), dealt as the lightest partners:
// the heaviest wave of each XCD then shares its CU with empty blocks only -- alone on it when pad
// covers its CU's other slots (sys_iso_pad).  place gets nw + 8 pad entries.
void place_by_load(const double* load, int64_t nw, int32_t pad, int32_t* place) {
  if (nw <= 0) return;
  const int64_t per = nw / 8, extra = nw % 8;
  for (int64_t x = 0; x < 8; ++x) {
    const int64_t nx = per + (x < extra ? 1 : 0), base = x * per + std::min(x, extra);
    if (nx == 0) continue;
    const int64_t n = nx + pad;  // this XCD's blocks
    std::vector<int64_t> byload(n);  // this XCD's waves, heaviest first, then the empty blocks (-1)
    std::iota(byload.begin(), byload.begin() + nx, base);
    std::fill(byload.begin() + nx, byload.end(), -1);
    std::stable_sort(byload.begin(), byload.begin() + nx, [&](int64_t u, int64_t v) { return load[u] > load[v]; });
    std::vector<int64_t> cus(std::min<int64_t>(n, 32));  // CU slots, fewest waves first
    std::iota(cus.begin(), cus.end(), 0);
    auto members = [&](int64_t c) { return (n - c + 31) / 32; };
    std::stable_sort(cus.begin(), cus.end(), [&](int64_t u, int64_t v) { return members(u) < members(v); });
    int64_t hi = 0, lo = n - 1;
    for (int64_t c : cus)
      for (int64_t kk = c, m = 0; kk < n; kk += 32, ++m)
        place[x + 8 * kk] = static_cast<int32_t>(m == 0 ? byload[hi++] : byload[lo--]);
  }
}

// Empty blocks per XCD that leave the `iso` heaviest waves of every XCD alone on their CUs: iso x
// (the fewest blocks a CU slot holds - 1) once the XCD holds nw / 8 + pad blocks.  0 when the
// launch could not hold them all at once (cap), or when the padding would put one more wave on the
// fullest CUs (YAHOO, 126 waves per XCD: pad 3 makes a five-wave CU, 236.6 -> 270 ms per epoch).
int32_t sys_iso_pad(int64_t nw, int64_t cap, int32_t iso) {
  const int64_t n0 = (nw + 7) / 8;  // the fullest XCD's waves (a smaller XCD needs no more)
  for (int32_t pad = 0; pad <= 3 * iso; ++pad) {
    const int64_t n = n0 + pad;
    const int64_t fewest = n <= 32 ? 1 : n / 32;  // blocks of its emptiest CU slot
    if (iso * (fewest - 1) <= pad)
      return nw + 8 * pad <= cap && (n + 31) / 32 == (n0 + 31) / 32 ? pad : 0;
  }
  return 0;
}

// One launch's map place[0 .. len): every wave 0 .. waves-1 exactly once, the rest empty (a
// missing wave would stall its neighbours).
void check_placement(const int32_t* place, int64_t len, int64_t waves) {
  std::vector<uint8_t> seen(static_cast<size_t>(waves), 0);
  int64_t empty = 0;
  for (int64_t b = 0; b < len; ++b) {
    const int32_t L = place[b];
    if (L < 0) { ++empty; continue; }
    MF_REQUIRE(L < waves && !seen[L], "systolic placement is not a permutation");
    seen[L] = 1;
  }
  MF_REQUIRE(empty == len - waves, "systolic placement: empty blocks miscounted");
}

// The maps of every launch of one shard: the launch of superstep index sm takes place[off[sm] ..
// off[sm + 1]), waves numbered from the launch's first one, with pad[sm] empty blocks per XCD for
// iso > 0 (sys_iso_pad against the sys_cap blocks that can be resident at once).  ring_overlap: a
// superstep is the two launches of fast_superstep, cut at the shard's last local block (of c), each
// with a map of its own behind the other's; they take no empty blocks.  Every launch's map is checked.
void sys_placement(const PairPlan& pp, int32_t nb, int32_t c, bool ring_overlap, int32_t iso, int64_t sys_cap,
                   std::vector<int32_t>& place, std::vector<int64_t>& off, std::vector<int32_t>& pad) {
  MF_REQUIRE(!(ring_overlap && iso), "systolic placement: empty blocks need one launch per superstep");
  off.assign(nb + 1, 0);
  pad.assign(nb, 0);
  for (int32_t sm = 0; sm < nb; ++sm) {
    const int64_t nw = pp.sys_off[sm + 1] - pp.sys_off[sm];
    pad[sm] = iso ? sys_iso_pad(nw, sys_cap, iso) : 0;
    off[sm + 1] = off[sm] + nw + 8 * pad[sm];
  }
  place.assign(static_cast<size_t>(off[nb]), 0);
  std::vector<double> load;
  for (int32_t sm = 0; sm < nb; ++sm) {
    const int64_t w0 = pp.sys_off[sm], nw = pp.sys_off[sm + 1] - w0;
    const int64_t cut = ring_overlap ? pp.sys_block_off[static_cast<size_t>(sm) * (c + 1) + c - 1] : nw;
    const struct { int64_t a, z; int32_t pad; } launches[] = {{0, cut, pad[sm]}, {cut, nw, 0}};
    for (const auto& l : launches) {
      const int64_t n = l.z - l.a;
      load.resize(static_cast<size_t>(n));
      for (int64_t L = 0; L < n; ++L) load[L] = sys_wave_load(pp, w0 + l.a + L);
      int32_t* map = place.data() + off[sm] + l.a;
      place_by_load(load.data(), n, l.pad, map);
      check_placement(map, n + 8 * l.pad, n);
    }
  }
}

}  // namespace mfhip
