// pfd_i16.hip — int16 fold cubes for the PFD calls on gfx950: the folds' part sums in fp64 from
// the 2-byte values of a fold-mode archive and their float32 scale, offset and weight.
//
// The float32 path over again (pfd_f32.hip): every PFD kernel reads the n x npart x nsub x
// proflen cube once, to sum the parts of each element in order p = 0 .. npart-1.
// k_pfd_partsum_i16 does that one pass on the values as the archive holds them.  Each is decoded
// where it is loaded,
//   x = (double)d * (double)scl[p][s] + (double)offs[p][s]      one rounding: the product is exact
//   x = x * (double)wts[p][s]                                   with weights: one more rounding
// (16 bits times a 24-bit significand fits fp64 and no float32 exponent leaves its range, so the
// fused multiply-add below rounds where numpy's multiply-then-add does), and the adds run in the
// same order, starting from the value of part 0 (no 0.0 +).  The f64 kernels then run on the
// sums with npart = 1.  PFE_FLAG_PFD_BSWAP: every 2-byte and 4-byte value is byte-reversed in
// registers.  The arrays are read through byte strides (launch.h PfdI16Src), so they may be the
// rows of an uploaded binary table.  Nothing is computed in float32 or in integers.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "pfd_i16_dev.h"

namespace pfe {

#pragma clang fp contract(off)

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int PSUM_THREADS = 256;
constexpr int PSUM_BURST = 8;  // part loads a lane keeps in flight

// S[c][e] = x(c,0,e) + x(c,1,e) + ... + x(c,NP-1,e) for the E = nsub x L elements of n folds, x
// the decoded value; S n x E doubles, dense.  A flat grid over the n * E sums: lane t of the grid
// owns sums [4t, 4t + 4), so a launch fills the chip whatever the fold size, and S (256-byte
// aligned) takes 16-byte stores.  VEC (E % 4 == 0 and data 8-byte aligned at every part): the
// four sums are of one fold and each part is one 8-byte load; else each sum finds its own fold
// and element and is loaded alone.  The parameters of a (fold, part, sub-band) are shared by L
// bins: a lane whose four elements lie in one sub-band -- all but the lanes on a seam -- loads
// them once per part (neighbouring lanes read the same words: one cache line a wave), a lane
// on a seam loads them per element.  Same operations, same bits on every path.
// NS (pfd_i16_dev.h; 0: the cube of the _i16 calls): x the sum of NS polarisations, weighted once
// -- a burst step loads both polarisations of 4 parts, a seam step both of one.  The condition of
// the 8-byte loads is the same: E % 4 == 0 makes the polarisation stride 2 E a multiple of 8.
template <bool VEC, bool BS, bool WT, int NS = 0>
__global__ __launch_bounds__(PSUM_THREADS) void k_pfd_partsum_i16(const PfdI16Src x,
                                                                  double* __restrict__ S, int NP,
                                                                  int L, int64_t E, int64_t total) {
  const int64_t f = ((int64_t)blockIdx.x * PSUM_THREADS + threadIdx.x) * 4;
  if (f >= total) return;
  int64_t c = f / E;
  int e = (int)(f - c * E);  // E = nsub x L < 2^31
  const char* q[4];
  int64_t par[4];
  bool ok[4] = {true, true, true, true};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u > 0 && ++e == (int)E) {  // VEC: never (E % 4 == 0)
      e = 0;
      ++c;
    }
    ok[u] = f + u < total;
    // past the end: loads that are there
    q[u] = ok[u] ? x.data + c * x.dfs + (int64_t)2 * e : q[0];
    par[u] = ok[u] ? c * x.pfs + (int64_t)4 * (e / L) : par[0];
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (NS > 0) {
    // the weights' own strides: the fold and the sub-band of each element once more
    int64_t wpar[4];
    int64_t wc = f / E;
    int we = (int)(f - wc * E);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (u > 0 && ++we == (int)E) {
        we = 0;
        ++wc;
      }
      wpar[u] = ok[u] ? wc * x.wfs + (int64_t)4 * (we / L) : wpar[0];
    }
    if (par[1] == par[0] && par[2] == par[0] && par[3] == par[0])
      psum_pol_run<VEC, BS, WT, NS>(x, q, par[0], wpar[0], NP, acc);
    else
      psum_pol_seam<VEC, BS, WT, NS>(x, q, par, wpar, NP, acc);
  } else if (par[1] == par[0] && par[2] == par[0] && par[3] == par[0]) {
    int p = 0;
    for (; p + PSUM_BURST <= NP; p += PSUM_BURST)
      psum_add<VEC, BS, WT, PSUM_BURST>(x, q, par[0], p, acc);
    if (p + 4 <= NP) {
      psum_add<VEC, BS, WT, 4>(x, q, par[0], p, acc);
      p += 4;
    }
    if (p + 2 <= NP) {
      psum_add<VEC, BS, WT, 2>(x, q, par[0], p, acc);
      p += 2;
    }
    if (p < NP) psum_add<VEC, BS, WT, 1>(x, q, par[0], p, acc);
  } else {  // a seam between sub-bands or folds inside the quad
    for (int p = 0; p < NP; ++p) {
      const u32x2 v = psum_load<VEC>(q, (int64_t)p * x.dps);
      const unsigned h[4] = {v.x, v.x >> 16, v.y, v.y >> 16};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const I16Par r = i16_par<WT>(x, par[u] + (int64_t)p * x.pps);
        const double y = i16_decode<BS, WT>(i16_value<BS>(h[u]), r);
        acc[u] = p == 0 ? y : acc[u] + y;
      }
    }
  }
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

template <bool VEC, bool BS>
static void launch_psum(bool wt, dim3 grid, dim3 block, hipStream_t st, const PfdI16Src& x, double* s,
                        int npart, int L, int64_t E, int64_t total) {
  const int ns = pfd_i16_ns(x);
  if (ns == 2 && wt)
    hipLaunchKernelGGL((k_pfd_partsum_i16<VEC, BS, true, 2>), grid, block, 0, st, x, s, npart, L, E, total);
  else if (ns == 2)
    hipLaunchKernelGGL((k_pfd_partsum_i16<VEC, BS, false, 2>), grid, block, 0, st, x, s, npart, L, E, total);
  else if (ns == 1)  // one polarisation of several, its weights (given) apart from scl's strides
    hipLaunchKernelGGL((k_pfd_partsum_i16<VEC, BS, true, 1>), grid, block, 0, st, x, s, npart, L, E, total);
  else if (wt)
    hipLaunchKernelGGL((k_pfd_partsum_i16<VEC, BS, true>), grid, block, 0, st, x, s, npart, L, E, total);
  else
    hipLaunchKernelGGL((k_pfd_partsum_i16<VEC, BS, false>), grid, block, 0, st, x, s, npart, L, E, total);
}

hipError_t launch_pfd_partsum_i16(const PfdI16Src& x, double* s, int npart, int nsub, int L,
                                  int64_t n, hipStream_t st) {
  const int64_t E = (int64_t)nsub * L, total = n * E;
  if (total <= 0) return hipSuccess;
  const int64_t quads = (total + 3) / 4;
  const int64_t blocks = (quads + PSUM_THREADS - 1) / PSUM_THREADS;
  if (E > 0x7fffffff || blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(PSUM_THREADS);
  const bool vec = E % 4 == 0 && (((uintptr_t)x.data | (uintptr_t)x.dfs | (uintptr_t)x.dps) & 7) == 0;
  const bool wt = x.wts != nullptr;
  if (vec) {
    if (x.bswap)
      launch_psum<true, true>(wt, grid, block, st, x, s, npart, L, E, total);
    else
      launch_psum<true, false>(wt, grid, block, st, x, s, npart, L, E, total);
  } else {
    if (x.bswap)
      launch_psum<false, true>(wt, grid, block, st, x, s, npart, L, E, total);
    else
      launch_psum<false, false>(wt, grid, block, st, x, s, npart, L, E, total);
  }
  return hipGetLastError();
}

}  // namespace pfe
