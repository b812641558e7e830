// pfd_kill.hip — killed intervals and sub-bands for the PFD calls on gfx950: the folds' part
// sums in fp64 with every value of a killed part or sub-band replaced by +0.0 at the load.
//
// The float32 path over again (pfd_f32.hip, pfd_be64.hip), for three element types: doubles,
// byte-reversed 8-byte words and floats.  Every PFD kernel reads the n x npart x nsub x proflen
// cube once, to sum the parts of each element in order p = 0 .. npart-1; k_pfd_partsum_kill
// does that one pass on the cube as it lies, with the two masks of the call beside it:
//   v(p) = (parts[c][p] || subs[c][s]) ? +0.0 : (double)X[c][p][s][b]
//   S[c][s][b] = v(0) + v(1) + ... + v(npart-1)
// the adds in that order, starting from the value of part 0 (no 0.0 +, so -0.0 comes out as from
// the f64 kernels' acc = P[src]; acc += ...).  A killed value is replaced, never multiplied: a
// NaN, an inf or 1e308 in a killed row reaches no sum.  The f64 kernels then run on the sums
// with npart = 1 and form the bits they form on np.where(kill, 0.0, x).  Neither the cube nor a
// mask is written and no zapped cube is made.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace pfe {

#pragma clang fp contract(off)

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int KSUM_THREADS = 256;
constexpr int KSUM_BURST = 8;  // part loads a lane keeps in flight

// the three element types: T as loaded, W values to a 16-byte load, val() widens one to double
struct kill_f64 {
  typedef unsigned long long T;
  typedef unsigned long long V __attribute__((ext_vector_type(2)));
  static constexpr int W = 2;
  static __device__ __forceinline__ double val(T w) { return __builtin_bit_cast(double, w); }
};
struct kill_be64 {
  typedef unsigned long long T;
  typedef unsigned long long V __attribute__((ext_vector_type(2)));
  static constexpr int W = 2;
  static __device__ __forceinline__ double val(T w) {
    return __builtin_bit_cast(double, __builtin_bswap64(w));  // the word is reversed, then selected
  }
};
struct kill_f32 {
  typedef float T;
  typedef float V __attribute__((ext_vector_type(4)));
  static constexpr int W = 4;
  static __device__ __forceinline__ double val(T v) { return (double)v; }
};

// the lane's W values of one part.  VEC: consecutive values behind q[0], 16-byte aligned; else W
// element loads, each element behind its own pointer (a lane's elements may span two folds)
template <typename El, bool VEC>
__device__ __forceinline__ typename El::V ksum_load(const typename El::T* const (&q)[El::W],
                                                    int64_t off) {
  if constexpr (VEC) {
    return __builtin_nontemporal_load(reinterpret_cast<const typename El::V*>(q[0] + off));
  } else {
    typename El::V v;
#pragma unroll
    for (int j = 0; j < El::W; ++j) v[j] = __builtin_nontemporal_load(q[j] + off);
    return v;
  }
}

// parts [p, p + K) onto the W sums, all K loads (and the K part bytes of each fold the lane
// touches) issued before the first add; part 0 is the sums' first value, not added to anything.
// kp[j]: the part mask of element j's fold, or null; sd[j]: element j's sub-band is killed
template <typename El, bool VEC, int K>
__device__ __forceinline__ void ksum_add(const typename El::T* const (&q)[El::W],
                                         const uint8_t* const (&kp)[El::W], const bool (&sd)[El::W],
                                         int64_t E, int p, double (&acc)[El::W]) {
  constexpr int W = El::W;
  typename El::V v[K];
  bool pd[K][W];
#pragma unroll
  for (int u = 0; u < K; ++u) {
    if constexpr (VEC) {  // one fold: one byte
      const bool d = kp[0] ? kp[0][p + u] != 0 : false;
#pragma unroll
      for (int j = 0; j < W; ++j) pd[u][j] = d;
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j) pd[u][j] = kp[j] ? kp[j][p + u] != 0 : false;
    }
    v[u] = ksum_load<El, VEC>(q, (int64_t)(p + u) * E);
  }
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const bool first = u == 0 && p == 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double x = (pd[u][j] || sd[j]) ? 0.0 : El::val(v[u][j]);
      acc[j] = first ? x : acc[j] + x;
    }
  }
}

// S[c][e] = v(c,0,e) + ... + v(c,NP-1,e) for the E = nsub x L elements of n folds: X n x NP x E
// values, KP n x NP and KS n x nsub bytes (either null), S n x E doubles, all dense.  A flat grid
// over the n * E sums: lane t of the grid owns sums [W t, W t + W), so a launch fills the chip
// whatever the fold size, and S (256-byte aligned) takes 16-byte stores.  VEC (E % W == 0 and X
// 16-byte aligned): the W sums are of one fold and each part is one 16-byte load; else each sum
// finds its own fold and element.  The sub-band bit is per element on both paths: E can be a
// multiple of W while L is not, and then a lane's elements lie in two sub-bands.  A lane whose
// elements all lie in killed sub-bands loads nothing: its sums are +0.0 (0.0 + 0.0 + ...).
template <typename El, bool VEC>
__global__ __launch_bounds__(KSUM_THREADS) void k_pfd_partsum_kill(
    const typename El::T* __restrict__ X, const uint8_t* __restrict__ KP,
    const uint8_t* __restrict__ KS, double* __restrict__ S, int NP, int nsub, int L, int64_t E,
    int64_t total) {
  constexpr int W = El::W;
  const int64_t f = ((int64_t)blockIdx.x * KSUM_THREADS + threadIdx.x) * W;
  if (f >= total) return;
  int64_t c = f / E;
  int64_t e = f - c * E;
  const typename El::T* q[W];
  const uint8_t* kp[W];
  bool sd[W], ok[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    if (j > 0 && ++e == E) {  // VEC: never (E % W == 0)
      e = 0;
      ++c;
    }
    ok[j] = VEC || f + j < total;
    if (ok[j]) {
      q[j] = X + (c * NP) * E + e;
      kp[j] = KP ? KP + c * NP : nullptr;
      sd[j] = KS ? KS[c * nsub + e / L] != 0 : false;
    } else {  // past the end: a load that is there
      q[j] = q[0];
      kp[j] = kp[0];
      sd[j] = sd[0];
    }
  }
  double acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = 0.0;
  bool live = false;
#pragma unroll
  for (int j = 0; j < W; ++j) live = live || !sd[j];
  if (live) {
    int p = 0;
    for (; p + KSUM_BURST <= NP; p += KSUM_BURST) ksum_add<El, VEC, KSUM_BURST>(q, kp, sd, E, p, acc);
    if (p + 4 <= NP) {
      ksum_add<El, VEC, 4>(q, kp, sd, E, p, acc);
      p += 4;
    }
    if (p + 2 <= NP) {
      ksum_add<El, VEC, 2>(q, kp, sd, E, p, acc);
      p += 2;
    }
    if (p < NP) ksum_add<El, VEC, 1>(q, kp, sd, E, p, acc);
  }
  if (VEC || ok[W - 1]) {
    f64x2* out = reinterpret_cast<f64x2*>(S + f);
#pragma unroll
    for (int j = 0; j < W; j += 2) out[j / 2] = f64x2{acc[j], acc[j + 1]};
  } else {  // the last lane of a launch whose n * E is no multiple of W
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (ok[j]) S[f + j] = acc[j];
  }
}

template <typename El>
static hipError_t launch_partsum_kill(const void* x, const PfdKillSrc& k, double* s, int npart,
                                      int nsub, int L, int64_t n, hipStream_t st) {
  const int64_t E = (int64_t)nsub * L, total = n * E;
  if (total <= 0) return hipSuccess;
  const int64_t lanes = (total + El::W - 1) / El::W;
  const int64_t blocks = (lanes + KSUM_THREADS - 1) / KSUM_THREADS;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(KSUM_THREADS);
  const typename El::T* X = static_cast<const typename El::T*>(x);
  if (E % El::W == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL((k_pfd_partsum_kill<El, true>), grid, block, 0, st, X, k.parts, k.subs, s,
                       npart, nsub, L, E, total);
  else
    hipLaunchKernelGGL((k_pfd_partsum_kill<El, false>), grid, block, 0, st, X, k.parts, k.subs, s,
                       npart, nsub, L, E, total);
  return hipGetLastError();
}

hipError_t launch_pfd_partsum_kill(const void* x, int elem, const PfdKillSrc& k, double* s,
                                   int npart, int nsub, int L, int64_t n, hipStream_t st) {
  switch (elem) {
    case PFD_KILL_F64: return launch_partsum_kill<kill_f64>(x, k, s, npart, nsub, L, n, st);
    case PFD_KILL_BE64: return launch_partsum_kill<kill_be64>(x, k, s, npart, nsub, L, n, st);
    case PFD_KILL_F32: return launch_partsum_kill<kill_f32>(x, k, s, npart, nsub, L, n, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace pfe
