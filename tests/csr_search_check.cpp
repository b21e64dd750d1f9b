// CPU check of the table kernels' searches (csrc/csr_search.hpp), built with g++ and run by
// tests/test_csr_search.py: lower / upper / contains against std::lower_bound / std::upper_bound /
// std::binary_search, row_of against a linear scan.  Arrays of length 0, 1, 2, 3 and 2049 (one entry
// past a tile of 2048), runs of equal keys, queries below, inside and above the range, every sub-range
// [b, e) of the short arrays, and offset tables whose first rows, last rows and consecutive middle rows
// are empty, with [lo, hi] narrowed as the tiled kernels narrow it.  Prints "ok" and exits 0 on success.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "csr_search.hpp"

using namespace mfhip::dev;

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); \
      std::_Exit(1);                                                      \
    }                                                                     \
  } while (0)

// lower / upper / contains on a[b, e) for the query x, against the standard library
template <typename K>
static void check_range(const std::vector<K>& a, int64_t b, int64_t e, K x) {
  const K* p = a.data();
  CHECK(lower<K>(p, b, e, x) == std::lower_bound(p + b, p + e, x) - p);
  CHECK(upper<K>(p, b, e, x) == std::upper_bound(p + b, p + e, x) - p);
  CHECK(contains<K>(p, b, e, x) == std::binary_search(p + b, p + e, x));
}

// Every ascending array of length n over the values {base + 2, base + 4, base + 6} (so runs of equal keys of
// every length), every sub-range, and the queries base + 1 .. base + 7: below, equal to, between and above.
template <typename K>
static void check_short(int n, K base) {
  std::vector<K> a(static_cast<size_t>(n));
  std::vector<int> d(static_cast<size_t>(n), 0);
  for (;;) {
    bool ascending = true;
    for (int i = 0; i < n; ++i) {
      a[i] = static_cast<K>(base + 2 + 2 * d[i]);
      if (i > 0 && d[i] < d[i - 1]) ascending = false;
    }
    if (ascending)
      for (int64_t b = 0; b <= n; ++b)
        for (int64_t e = b; e <= n; ++e)
          for (int q = 1; q <= 7; ++q) check_range<K>(a, b, e, static_cast<K>(base + q));
    int i = 0;
    while (i < n && ++d[i] == 3) d[i++] = 0;
    if (i == n) break;
  }
}

// 2049 keys in runs of 1, 2, 3, 1, 2, 3, .. equal keys, two apart
template <typename K>
static void check_long(K base) {
  const int64_t n = 2049;
  std::vector<K> a;
  int run = 0;
  for (K v = base + 2; static_cast<int64_t>(a.size()) < n; v = static_cast<K>(v + 2), ++run)
    for (int r = 0; r < 1 + run % 3 && static_cast<int64_t>(a.size()) < n; ++r) a.push_back(v);
  const K top = a.back();
  for (K x = base; x <= top + 3; ++x) {
    check_range<K>(a, 0, n, x);
    check_range<K>(a, 0, 2048, x);
    check_range<K>(a, 2048, n, x);
    check_range<K>(a, 1, n - 1, x);
    check_range<K>(a, 1000, 1003, x);
  }
}

// The row of entry e by a linear scan: the one row with off[x] <= e < off[x + 1].
static int64_t row_linear(const std::vector<int64_t>& off, int64_t e) {
  for (int64_t x = 0; x + 1 < static_cast<int64_t>(off.size()); ++x)
    if (off[x] <= e && e < off[x + 1]) return x;
  return -1;
}

// row_of over the whole table, and as the tiled kernels call it (csr_device.hpp): per tile of 2048 entries
// the rows of its first and last entry, then 256 lanes that each carry their row forward inside that span.
static void check_rows(const std::vector<int64_t>& count) {
  const int64_t rows = static_cast<int64_t>(count.size());
  std::vector<int64_t> off(static_cast<size_t>(rows) + 1, 0);
  for (int64_t x = 0; x < rows; ++x) off[x + 1] = off[x] + count[x];
  const int64_t nnz = off[rows];
  for (int64_t e = 0; e < nnz; ++e) CHECK(row_of(off.data(), 0, rows - 1, e) == row_linear(off, e));
  for (int64_t t0 = 0; t0 < nnz; t0 += 2048) {
    const int64_t t1 = std::min<int64_t>(t0 + 2048, nnz);
    const int64_t first = row_of(off.data(), 0, rows - 1, t0), last = row_of(off.data(), 0, rows - 1, t1 - 1);
    CHECK(first == row_linear(off, t0) && last == row_linear(off, t1 - 1));
    for (int lane = 0; lane < 256; ++lane) {
      int64_t lo = first;
      for (int64_t e = t0 + lane; e < t1; e += 256) {
        lo = row_of(off.data(), lo, last, e);
        CHECK(lo == row_linear(off, e));
      }
    }
  }
}

// every table of `rows` rows that holds nnz entries in all
static void check_rows_all(int rows, int64_t nnz) {
  std::vector<int64_t> c(static_cast<size_t>(rows), 0);
  for (;;) {
    int64_t sum = 0;
    for (int64_t v : c) sum += v;
    if (sum == nnz) check_rows(c);
    int i = 0;
    while (i < rows && ++c[i] > nnz) c[i++] = 0;
    if (i == rows) break;
  }
}

int main() {
  for (int n = 0; n <= 3; ++n) {
    check_short<int32_t>(n, -4);  // values -2, 0, 2: both signs
    check_short<uint32_t>(n, 0);
    check_short<uint32_t>(n, 0xFFFFFFF0u);
    check_short<int64_t>(n, -4);
    check_short<uint64_t>(n, 0xFFFFFFFF00000000ull);  // the keys (row << 32) | col
  }
  check_long<int32_t>(-700);
  check_long<uint32_t>(0);
  check_long<int64_t>(int64_t{1} << 40);
  check_long<uint64_t>(uint64_t{5} << 32);

  for (int rows = 1; rows <= 6; ++rows)
    for (int64_t nnz = 0; nnz <= 3; ++nnz) check_rows_all(rows, nnz);  // (nnz = 0: nothing to find)
  // 2049 entries: two tiles, the second one entry long
  check_rows({2049});
  check_rows({0, 0, 0, 2049});                          // the first rows empty
  check_rows({2049, 0, 0, 0});                          // the last rows empty
  check_rows({0, 0, 5, 0, 0, 0, 2040, 0, 4, 0, 0});     // consecutive middle rows empty, a row longer than the rest
  check_rows({2047, 0, 0, 1, 0, 1});                    // the tile boundary between rows, empty rows on both sides
  check_rows({2048, 0, 0, 0, 1, 0});                    // a tile that ends with its row; empty rows before the next
  check_rows(std::vector<int64_t>(2049, 1));            // one entry per row
  {
    std::vector<int64_t> c;  // every third row empty, then two empty in a row
    for (int64_t left = 2049, x = 0; left > 0; ++x) {
      const int64_t v = (x % 3 == 2 || x % 7 == 3) ? 0 : std::min<int64_t>(left, 1 + x % 5);
      c.push_back(v);
      left -= v;
    }
    c.push_back(0);
    check_rows(c);
  }
  std::puts("ok");
  return 0;
}
