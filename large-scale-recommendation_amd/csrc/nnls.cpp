// nnls.cpp -- mf_nnls_solve: the non-negative solve of the ALS half-sweeps on the host, the replay of
// als_nnls_device.hpp operation for operation (the rules and the order of every sum are stated in
// mfhip.h).  No GPU needed.  A change here is a change there.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "common.hpp"
#include "context.hpp"

namespace mfhip {
namespace {

template <typename T>
bool finite(T v) {
  return v - v == T(0);
}

// 64 partial sums, partial l an fma chain over f = l, l + 64, ...; then the butterfly xor 32 .. 1
template <typename T>
T dot(const T* a, const T* b, int k) {
#pragma clang fp contract(off)
  T p[64], q[64];
  for (int l = 0; l < 64; ++l) {
    T s = T(0);
    for (int f = l; f < k; f += 64) s = std::fma(a[f], b[f], s);
    p[l] = s;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    for (int l = 0; l < 64; ++l) q[l] = p[l] + p[l ^ m];
    std::copy(q, q + 64, p);
  }
  return p[0];
}

template <typename T>
void matvec(const T* A, const T* v, int k, T* out) {
#pragma clang fp contract(off)
  for (int i = 0; i < k; ++i) {
    T s = T(0);
    for (int j = 0; j < k; ++j) s = std::fma(A[j * k + i], v[j], s);
    out[i] = s;
  }
}

template <typename T>
bool stop(T step, T nd, T thresh) {
  return !finite(step) || !(step > T(0)) || nd <= thresh;
}

template <typename T>
void solve(int k, const double* A64, const double* b64, double* x_out, int32_t* iters_out, int32_t* reason_out) {
#pragma clang fp contract(off)
  const size_t K = static_cast<size_t>(k);
  std::vector<T> A(K * K), b(K), x(K, T(0)), res(K), g(K), dir(K), last(K, T(0)), av(K);
  for (int i = 0; i < k; ++i) {
    b[i] = static_cast<T>(b64[i]);
    for (int j = 0; j <= i; ++j) A[i * k + j] = A[j * k + i] = static_cast<T>(A64[i * k + j]);
  }
  const T bb = dot(b.data(), b.data(), k);
  const T thresh = static_cast<T>(1e-12) * bb;
  const T slack = T(1) - T(64) * std::numeric_limits<T>::epsilon();
  const int cap = std::max(400, 20 * k);
  int it = 0, last_wall = 0, reason = 1;
  T last_norm = T(0);
  if (!finite(bb)) {
    reason = 3;
  } else {
    for (; it < cap; ++it) {
      matvec(A.data(), x.data(), k, res.data());
      for (int i = 0; i < k; ++i) {
        const T r = res[i] - b[i];
        res[i] = r;
        g[i] = (r > T(0) && x[i] == T(0)) ? T(0) : r;
      }
      const T ng = dot(g.data(), g.data(), k);
      const T gr = dot(g.data(), res.data(), k);
      matvec(A.data(), g.data(), k, av.data());
      T step = gr / dot(g.data(), av.data(), k);
      T nd = ng;
      bool conj = false;
      if (it > last_wall + 1) {
        const T beta = ng / last_norm;
        for (int i = 0; i < k; ++i) dir[i] = std::fma(beta, last[i], g[i]);
        matvec(A.data(), dir.data(), k, av.data());
        const T s2 = dot(dir.data(), res.data(), k) / dot(dir.data(), av.data(), k);
        const T n2 = dot(dir.data(), dir.data(), k);
        if (!stop(s2, n2, thresh)) {
          conj = true;
          step = s2;
          nd = n2;
        }
      }
      if (nd <= thresh) {
        reason = 0;
        break;
      }
      if (!finite(step)) {
        reason = 3;
        break;
      }
      if (!(step > T(0))) {
        reason = 2;
        break;
      }
      if (!conj) dir = g;
      for (int i = 0; i < k; ++i)  // do not cross a wall
        if (step * dir[i] > x[i]) step = x[i] / dir[i];
      for (int i = 0; i < k; ++i) {
        const T sd = step * dir[i];
        if (sd > x[i] * slack) {
          x[i] = T(0);
          last_wall = it;
        } else {
          x[i] = x[i] - sd;
        }
      }
      last = dir;
      last_norm = ng;
    }
  }
  for (int i = 0; i < k; ++i)
    x_out[i] = reason == 3 ? std::numeric_limits<double>::quiet_NaN() : static_cast<double>(x[i]);
  if (iters_out) *iters_out = it;
  if (reason_out) *reason_out = reason;
}

}  // namespace

void nnls_solve_host(int32_t k, const double* A, const double* b, bool f64, double* x_out, int32_t* iters_out,
                     int32_t* reason_out) {
  MF_REQUIRE(k >= 1 && k <= 256, "mf_nnls_solve takes a rank in 1 .. 256");
  MF_REQUIRE(A && b && x_out, "null argument");
  if (f64) solve<double>(k, A, b, x_out, iters_out, reason_out);
  else solve<float>(k, A, b, x_out, iters_out, reason_out);
}

}  // namespace mfhip
