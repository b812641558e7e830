// pfd_be64.hip — fold cubes in the opposite byte order (PFE_FLAG_PFD_BSWAP) on gfx950: the
// folds' part sums in fp64 from the raw 8-byte words of a big-endian .pfd file.
//
// The float32 path over again (pfd_f32.hip): every PFD kernel reads the n x npart x nsub x
// proflen cube once, to sum the parts of each element in order p = 0 .. npart-1.
// k_pfd_partsum_be64 does that one pass on the words as the file holds them: each word's bytes
// reversed in registers (two v_perm_b32), the adds in the same order, starting from the value of
// part 0 (no 0.0 +, so -0.0 and a NaN's payload come out as from the f64 kernels' acc = P[src];
// acc += ...).  The f64 kernels then run on the sums with npart = 1 and form the bits they form
// on the byte-swapped cube.  Nothing in memory is rewritten and no swapped cube is made.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace pfe {

#pragma clang fp contract(off)

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int PSUM_THREADS = 256;
constexpr int PSUM_BURST = 8;  // part loads a lane keeps in flight

__device__ __forceinline__ double be64_value(unsigned long long w) {
  return __builtin_bit_cast(double, __builtin_bswap64(w));
}

// the lane's two words of one part.  VEC: consecutive words behind q[0], 16-byte aligned; else
// two 8-byte loads, each element behind its own pointer (a pair may span two folds)
template <bool VEC>
__device__ __forceinline__ u64x2 psum_load(const unsigned long long* const (&q)[2], int64_t off) {
  if constexpr (VEC) {
    return __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(q[0] + off));
  } else {
    u64x2 v;
    v.x = __builtin_nontemporal_load(q[0] + off);
    v.y = __builtin_nontemporal_load(q[1] + off);
    return v;
  }
}

// parts [p, p + K) onto the two sums, all K loads issued before the first add; part 0 is the
// sums' first value, not added to anything
template <bool VEC, int K>
__device__ __forceinline__ void psum_add(const unsigned long long* const (&q)[2], int64_t E, int p,
                                         double (&acc)[2]) {
  u64x2 v[K];
#pragma unroll
  for (int u = 0; u < K; ++u) v[u] = psum_load<VEC>(q, (int64_t)(p + u) * E);
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const bool first = u == 0 && p == 0;
    const double x = be64_value(v[u].x), y = be64_value(v[u].y);
    acc[0] = first ? x : acc[0] + x;
    acc[1] = first ? y : acc[1] + y;
  }
}

// S[c][e] = X[c][0][e] + X[c][1][e] + ... + X[c][NP-1][e], every X read through the byte
// reversal, for the E = nsub x proflen elements of n folds: X n x NP x E words, S n x E doubles,
// both dense.  A flat grid over the n * E sums: lane t of the grid owns sums [2t, 2t + 2), so a
// launch fills the chip whatever the fold size, and S (256-byte aligned) takes 16-byte stores.
// VEC (E even and X 16-byte aligned): the two sums are of one fold and each part is one 16-byte
// load; else each sum finds its own fold and element.  Same adds, same bits.
template <bool VEC>
__global__ __launch_bounds__(PSUM_THREADS) void k_pfd_partsum_be64(
    const unsigned long long* __restrict__ X, double* __restrict__ S, int NP, int64_t E,
    int64_t total) {
  const int64_t f = ((int64_t)blockIdx.x * PSUM_THREADS + threadIdx.x) * 2;
  if (f >= total) return;
  int64_t c = f / E;
  int64_t e = f - c * E;
  const unsigned long long* q[2];
  q[0] = X + (c * NP) * E + e;
  q[1] = q[0];
  bool pair = true;
  if constexpr (!VEC) {
    if (++e == E) {
      e = 0;
      ++c;
    }
    pair = f + 1 < total;
    if (pair) q[1] = X + (c * NP) * E + e;  // past the end: a load that is there
  }
  double acc[2] = {0.0, 0.0};
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
  if (VEC || pair)
    *reinterpret_cast<f64x2*>(S + f) = f64x2{acc[0], acc[1]};
  else  // the last sum of a launch whose n * E is odd
    S[f] = acc[0];
}

hipError_t launch_pfd_partsum_be64(const double* x, double* s, int npart, int nsub, int L,
                                   int64_t n, hipStream_t st) {
  const int64_t E = (int64_t)nsub * L, total = n * E;
  if (total <= 0) return hipSuccess;
  const int64_t pairs = (total + 1) / 2;
  const int64_t blocks = (pairs + PSUM_THREADS - 1) / PSUM_THREADS;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(PSUM_THREADS);
  const unsigned long long* w = reinterpret_cast<const unsigned long long*>(x);
  if (E % 2 == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL((k_pfd_partsum_be64<true>), grid, block, 0, st, w, s, npart, E, total);
  else
    hipLaunchKernelGGL((k_pfd_partsum_be64<false>), grid, block, 0, st, w, s, npart, E, total);
  return hipGetLastError();
}

}  // namespace pfe
