// np_sum.h — numpy's own reduction orders on one wavefront (device helpers shared by the
// PFD kernels, the float-row Lyon kernel and the float-profile variants of the 22-score
// kernels).
#pragma once

#include <cmath>

#include "wave.h"

namespace pfe {

#pragma clang fp contract(off)

// ---- numpy pairwise summation ---------------------------------------------------------
// a leaf (n <= 128): r[j] = a[j] + a[j+8] + ... over the largest multiple of 8, combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in order; n < 8: 0 + a0 + a1 ...
__device__ __forceinline__ double np_leaf(const double* a, int n, int lane) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  const int nb = n - (n % 8);
  double r = 0.0;
  if (lane < 8) {
    r = a[lane];
    for (int i = 8 + lane; i < nb; i += 8) r += a[i];
  }
  const double r0 = bcast(r, 0), r1 = bcast(r, 1), r2 = bcast(r, 2), r3 = bcast(r, 3);
  const double r4 = bcast(r, 4), r5 = bcast(r, 5), r6 = bcast(r, 6), r7 = bcast(r, 7);
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (int i = nb; i < n; ++i) res += a[i];
  return res;
}

// np_leaf for 8 <= n <= 128 with every load of a lane issued before its adds (the same
// order of additions, so the same bits)
__device__ __forceinline__ double np_leaf128(const double* a, int n, int lane) {
  const int nb = n - (n % 8);
  double v[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) v[m] = a[min((lane & 7) + 8 * m, n - 1)];
  double r = v[0];
#pragma unroll
  for (int m = 1; m < 16; ++m)
    if (8 * m < nb) r += v[m];
  const double r0 = bcast(r, 0), r1 = bcast(r, 1), r2 = bcast(r, 2), r3 = bcast(r, 3);
  const double r4 = bcast(r, 4), r5 = bcast(r, 5), r6 = bcast(r, 6), r7 = bcast(r, 7);
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (int i = nb; i < n; ++i) res += a[i];
  return res;
}

template <int D>
__device__ __noinline__ double np_pairwise(const double* a, int n, int lane) {
  if (n <= 128) return np_leaf(a, n, lane);
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise<D - 1>(a, n2, lane) + np_pairwise<D - 1>(a + n2, n - n2, lane);
}
template <>
__device__ __noinline__ double np_pairwise<0>(const double* a, int n, int lane) {
  return np_leaf(a, n, lane);
}

// np_pairwise with every level inlined (no call).  numpy splits at floor8(n/2), so the larger
// half n - floor8(n/2) can exceed n/2 (969 -> 489 -> 249 -> 129): D levels reproduce numpy's
// order exactly for n <= np_inl_max(D) = 128, 248, 488, 968, 1928 (D = 0..4), not 128 * 2^D
__host__ __device__ constexpr int np_inl_max(int D) { return D == 0 ? 128 : 2 * (np_inl_max(D - 1) - 4); }
static_assert(np_inl_max(1) == 248 && np_inl_max(3) == 968, "numpy pairwise split bound");
template <int D>
__device__ __forceinline__ double np_pairwise_inl(const double* a, int n, int lane) {
  if (n <= 128 || D == 0) return np_leaf(a, n, lane);
  if constexpr (D > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_inl<D - 1>(a, n2, lane) + np_pairwise_inl<D - 1>(a + n2, n - n2, lane);
  }
  return 0.0;
}

// ---- the same orders for eight rows per wave, the summands formed on the fly -----------
// Row g = lane / 8 lives in lanes 8g..8g+7, t = lane & 7 is a lane's accumulator of a leaf.
// Every row of the wave has the same n, so the splits are wave-uniform and every lane is
// active at the DPP steps.  f(i, v) gives the K summands of element i of the lane's own row
// (x itself; or d^2, d^2 d, (d^2)^2 of d = x - mean): K sums in one pass, each with np_leaf's
// / np_pairwise's additions in their order, the results in every lane of the group.
template <int K>
struct SumK {
  double v[K];
};

template <int K, typename Fn>
__device__ __forceinline__ SumK<K> np_leaf_g8(Fn f, int off, int n, int t) {
  SumK<K> r;
  double v[K];
  if (n < 8) {
#pragma unroll
    for (int k = 0; k < K; ++k) r.v[k] = 0.0;
    for (int i = 0; i < n; ++i) {
      f(off + i, v);
#pragma unroll
      for (int k = 0; k < K; ++k) r.v[k] += v[k];
    }
    return r;
  }
  const int nb = n - (n % 8);
  f(off + t, r.v);
  for (int i = 8 + t; i < nb; i += 8) {
    f(off + i, v);
#pragma unroll
    for (int k = 0; k < K; ++k) r.v[k] += v[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {  // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
    r.v[k] += dpp_f64<DPP_QUAD_XOR1>(r.v[k]);
    r.v[k] += dpp_f64<DPP_QUAD_XOR2>(r.v[k]);
    r.v[k] += dpp_f64<DPP_ROW_HALF_MIRROR>(r.v[k]);
  }
  for (int i = nb; i < n; ++i) {
    f(off + i, v);
#pragma unroll
    for (int k = 0; k < K; ++k) r.v[k] += v[k];
  }
  return r;
}

// D levels of numpy's split at floor8(n / 2): exact for n <= np_inl_max(D).  Inlined (no call
// in the kernel) or one small function per level.
template <int D, int K, typename Fn>
__device__ __forceinline__ SumK<K> np_pairwise_g8_inl(Fn f, int off, int n, int t) {
  if constexpr (D > 0) {
    if (n > 128) {
      int n2 = n / 2;
      n2 -= n2 % 8;
      SumK<K> a = np_pairwise_g8_inl<D - 1, K>(f, off, n2, t);
      const SumK<K> b = np_pairwise_g8_inl<D - 1, K>(f, off + n2, n - n2, t);
#pragma unroll
      for (int k = 0; k < K; ++k) a.v[k] += b.v[k];
      return a;
    }
  }
  return np_leaf_g8<K>(f, off, n, t);
}
template <int D, int K, typename Fn>
__device__ __noinline__ SumK<K> np_pairwise_g8(Fn f, int off, int n, int t) {
  if constexpr (D > 0) {
    if (n > 128) {
      int n2 = n / 2;
      n2 -= n2 % 8;
      SumK<K> a = np_pairwise_g8<D - 1, K>(f, off, n2, t);
      const SumK<K> b = np_pairwise_g8<D - 1, K>(f, off + n2, n - n2, t);
#pragma unroll
      for (int k = 0; k < K; ++k) a.v[k] += b.v[k];
      return a;
    }
  }
  return np_leaf_g8<K>(f, off, n, t);
}

// [mean, std, skew, kurtosis] from numpy's mean and scipy's central moments m2..m4
// (scipy.stats.skew / kurtosis, bias=True, Fisher): NaN when m2 <= (eps * mean)^2
__device__ __forceinline__ void stats4_finish(double mean, double m2, double m3, double m4,
                                              double (&o)[4]) {
  const double eps = 2.220446049250313e-16;
  const double zl = eps * mean;
  const bool zero = m2 <= zl * zl;
  o[0] = mean;
  o[1] = sqrt(m2);
  o[2] = zero ? NAN : m3 / pow(m2, 1.5);
  o[3] = zero ? NAN : m4 / (m2 * m2) - 3.0;
}

constexpr int NP_BUFSIZE = 8192;  // numpy.add.reduce hands its inner loop at most this many values
static_assert(np_inl_max(7) >= NP_BUFSIZE, "levels of a buffer's pairwise tree");

// numpy's sum of a row of any length: the row in buffers of NP_BUFSIZE values, each summed
// pairwise and added, in order, onto 0.  NC: n <= np_inl_max(3), one buffer, every level
// inlined.
template <bool NC, int K, typename Fn>
__device__ __forceinline__ SumK<K> np_sum_g8(Fn f, int n, int t) {
  if constexpr (NC) {
    return np_pairwise_g8_inl<3, K>(f, 0, n, t);
  } else {
    SumK<K> r;
#pragma unroll
    for (int k = 0; k < K; ++k) r.v[k] = 0.0;
    for (int off = 0; off < n; off += NP_BUFSIZE) {
      const SumK<K> c = np_pairwise_g8<7, K>(f, off, min(NP_BUFSIZE, n - off), t);
#pragma unroll
      for (int k = 0; k < K; ++k) r.v[k] += c.v[k];
    }
    return r;
  }
}

// numpy.mean / numpy.std / scipy.stats.skew / scipy.stats.kurtosis of eight float64 rows of
// n values per wave (row lane / 8 at x, in LDS or global memory): the deviations are formed
// from the row and the mean in the pass that sums their powers (d^3 = d^2 d, d^4 = (d^2)^2,
// scipy's _moment), so no scratch row.  T = float: the row is held as float32 and each value
// widened (exactly) at its load, in both passes; every operation is fp64 as for T = double.
template <bool NC, typename T>
__device__ __forceinline__ void stats4_f64_g8(const T* x, int n, int t, double (&o)[4]) {
  auto fx = [x](int i, double (&v)[1]) { v[0] = (double)x[i]; };
  const SumK<1> s = np_sum_g8<NC, 1>(fx, n, t);
  const double mean = s.v[0] / (double)n;
  auto fd = [x, mean](int i, double (&v)[3]) {
    const double d = (double)x[i] - mean;
    const double d2 = d * d;
    v[0] = d2;
    v[1] = d2 * d;
    v[2] = d2 * d2;
  };
  const SumK<3> m = np_sum_g8<NC, 3>(fd, n, t);
  stats4_finish(mean, m.v[0] / (double)n, m.v[1] / (double)n, m.v[2] / (double)n, o);
}

// float32 pairwise sum of a short array (n <= 128), evaluated identically in every lane
__device__ float np_leaf_f32(const float* a, int n) {
  if (n < 8) {
    float r = 0.0f;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  const int nb = n - (n % 8);
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  for (int i = 8; i < nb; i += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (int i = nb; i < n; ++i) res += a[i];
  return res;
}

// Python's builtin min / max over a sequence (first element wins ties and NaN)
__device__ double py_min_seq(const double* a, int n) {
  double m = a[0];
  for (int i = 1; i < n; ++i)
    if (a[i] < m) m = a[i];
  return m;
}
__device__ double py_max_seq(const double* a, int n) {
  double m = a[0];
  for (int i = 1; i < n; ++i)
    if (a[i] > m) m = a[i];
  return m;
}

__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace pfe
