// pfd_f32.hip — float32 fold cubes for the PFD calls on gfx950: the folds' part sums in fp64.
//
// Every PFD kernel reads the n x npart x nsub x proflen cube once, to sum the parts of each
// element in order p = 0 .. npart-1 (pfd.hip, pfd_global.hip).  k_pfd_partsum_f32 does that
// one pass on a float32 cube: each value widened to fp64 (exact), the adds in the same order,
// starting from the value of part 0 (no 0.0 +, so -0.0 and a NaN's payload come out as from
// the f64 kernels' acc = P[src]; acc += ...).  The f64 kernels then run on the sums with
// npart = 1 and form the bits they form on the widened cube.  Nothing is added in float32.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace pfe {

#pragma clang fp contract(off)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int PSUM_THREADS = 256;
constexpr int PSUM_BURST = 8;  // part loads a lane keeps in flight

// the lane's four values of one part.  VEC: consecutive floats behind q[0], 16-byte aligned;
// else four 4-byte loads, each element behind its own pointer (a quad may span two folds)
template <bool VEC>
__device__ __forceinline__ f32x4 psum_load(const float* const (&q)[4], int64_t off) {
  if constexpr (VEC) {
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q[0] + off));
  } else {
    f32x4 v;
    v.x = __builtin_nontemporal_load(q[0] + off);
    v.y = __builtin_nontemporal_load(q[1] + off);
    v.z = __builtin_nontemporal_load(q[2] + off);
    v.w = __builtin_nontemporal_load(q[3] + off);
    return v;
  }
}

// parts [p, p + K) onto the four sums, all K loads issued before the first add; part 0 is
// the sums' first value, not added to anything
template <bool VEC, int K>
__device__ __forceinline__ void psum_add(const float* const (&q)[4], int64_t E, int p,
                                         double (&acc)[4]) {
  f32x4 v[K];
#pragma unroll
  for (int u = 0; u < K; ++u) v[u] = psum_load<VEC>(q, (int64_t)(p + u) * E);
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const bool first = u == 0 && p == 0;
    acc[0] = first ? (double)v[u].x : acc[0] + (double)v[u].x;
    acc[1] = first ? (double)v[u].y : acc[1] + (double)v[u].y;
    acc[2] = first ? (double)v[u].z : acc[2] + (double)v[u].z;
    acc[3] = first ? (double)v[u].w : acc[3] + (double)v[u].w;
  }
}

// S[c][e] = (double)X[c][0][e] + (double)X[c][1][e] + ... + (double)X[c][NP-1][e] for the
// E = nsub x proflen elements of n folds: X n x NP x E floats, S n x E doubles, both dense.
// A flat grid over the n * E sums: lane t of the grid owns sums [4t, 4t + 4), so a launch
// fills the chip whatever the fold size, and S (256-byte aligned) takes 16-byte stores.
// VEC (E % 4 == 0 and X 16-byte aligned): the four sums are of one fold and each part is one
// 16-byte load; else each sum finds its own fold and element.  Same adds, same bits.
template <bool VEC>
__global__ __launch_bounds__(PSUM_THREADS) void k_pfd_partsum_f32(const float* __restrict__ X,
                                                                  double* __restrict__ S, int NP,
                                                                  int64_t E, int64_t total) {
  const int64_t f = ((int64_t)blockIdx.x * PSUM_THREADS + threadIdx.x) * 4;
  if (f >= total) return;
  int64_t c = f / E;
  int64_t e = f - c * E;
  const float* q[4];
  q[0] = X + (c * NP) * E + e;
  bool ok[4] = {true, true, true, true};
  if constexpr (VEC) {
    q[1] = q[2] = q[3] = q[0];
  } else {
#pragma unroll
    for (int u = 1; u < 4; ++u) {
      if (++e == E) {
        e = 0;
        ++c;
      }
      ok[u] = f + u < total;
      q[u] = ok[u] ? X + (c * NP) * E + e : q[0];  // past the end: a load that is there
    }
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int p = 0;
  for (; p + PSUM_BURST <= NP; p += PSUM_BURST) psum_add<VEC, PSUM_BURST>(q, E, p, acc);
  if (p + 4 <= NP) {
    psum_add<VEC, 4>(q, E, p, acc);
    p += 4;
  }
  if (p + 2 <= NP) {
    psum_add<VEC, 2>(q, E, p, acc);
    p += 2;
  }
  if (p < NP) psum_add<VEC, 1>(q, E, p, acc);
  if (VEC || ok[3]) {
    f64x2* out = reinterpret_cast<f64x2*>(S + f);
    out[0] = f64x2{acc[0], acc[1]};
    out[1] = f64x2{acc[2], acc[3]};
  } else {  // the last quad of a launch whose n * E is no multiple of 4
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (ok[u]) S[f + u] = acc[u];
  }
}

hipError_t launch_pfd_partsum_f32(const float* x, double* s, int npart, int nsub, int L, int64_t n,
                                  hipStream_t st) {
  const int64_t E = (int64_t)nsub * L, total = n * E;
  if (total <= 0) return hipSuccess;
  const int64_t quads = (total + 3) / 4;
  const dim3 grid((unsigned)((quads + PSUM_THREADS - 1) / PSUM_THREADS)), block(PSUM_THREADS);
  if (E % 4 == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL((k_pfd_partsum_f32<true>), grid, block, 0, st, x, s, npart, E, total);
  else
    hipLaunchKernelGGL((k_pfd_partsum_f32<false>), grid, block, 0, st, x, s, npart, E, total);
  return hipGetLastError();
}

}  // namespace pfe
