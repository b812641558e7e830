// pfd_i16_dev.h — the device side of an int16 fold cube, shared by the kernels that read one
// (pfd_i16.hip, pfd_scrunch.hip): a value as loaded -> the double it stands for, and a lane's
// burst of parts over four values of one sub-band.  See pfd_i16.hip for the contract.
#pragma once

#include <hip/hip_runtime.h>

#include "launch.h"

namespace pfe {

#pragma clang fp contract(off)

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// a 2-byte value as loaded (in the low half of w) -> the integer it holds
template <bool BS>
__device__ __forceinline__ int i16_value(unsigned w) {
  const unsigned short h = (unsigned short)w;
  return (int)(short)(BS ? __builtin_bswap16(h) : h);
}
// a 4-byte word as loaded -> the float it holds, widened
template <bool BS>
__device__ __forceinline__ double f32_value(unsigned w) {
  return (double)__builtin_bit_cast(float, BS ? __builtin_bswap32(w) : w);
}
// scale, offset and weight of one (fold, part, sub-band), as loaded
struct I16Par {
  unsigned a, o, w;
};
template <bool WT>
__device__ __forceinline__ I16Par i16_par(const PfdI16Src& x, int64_t at) {
  I16Par r;
  r.a = *reinterpret_cast<const unsigned*>(x.scl + at);
  r.o = *reinterpret_cast<const unsigned*>(x.offs + at);
  r.w = WT ? *reinterpret_cast<const unsigned*>(x.wts + at) : 0u;
  return r;
}
// the decoded value: d * scl + offs rounded once, then, WT, times the weight rounded once
template <bool BS, bool WT>
__device__ __forceinline__ double i16_decode(int d, const I16Par& r) {
  double v = __builtin_fma((double)d, f32_value<BS>(r.a), f32_value<BS>(r.o));
  if constexpr (WT) v = v * f32_value<BS>(r.w);
  return v;
}

// the lane's four values of one part, as two words of two values each.  VEC: consecutive values
// behind q[0], 8-byte aligned; else four 2-byte loads, each element behind its own pointer
template <bool VEC>
__device__ __forceinline__ u32x2 psum_load(const char* const (&q)[4], int64_t off) {
  if constexpr (VEC) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(q[0] + off));
  } else {
    unsigned short h[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      h[u] = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(q[u] + off));
    return u32x2{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
  }
}

// parts [p, p + K) onto the four sums of a lane whose elements share one sub-band: K data loads
// and K parameter loads issued before the first add; part 0 is the sums' first value
template <bool VEC, bool BS, bool WT, int K>
__device__ __forceinline__ void psum_add(const PfdI16Src& x, const char* const (&q)[4], int64_t par,
                                         int p, double (&acc)[4]) {
  u32x2 v[K];
  I16Par r[K];
#pragma unroll
  for (int u = 0; u < K; ++u) {
    v[u] = psum_load<VEC>(q, (int64_t)(p + u) * x.dps);
    r[u] = i16_par<WT>(x, par + (int64_t)(p + u) * x.pps);
  }
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const bool first = u == 0 && p == 0;
    const double y0 = i16_decode<BS, WT>(i16_value<BS>(v[u].x), r[u]);
    const double y1 = i16_decode<BS, WT>(i16_value<BS>(v[u].x >> 16), r[u]);
    const double y2 = i16_decode<BS, WT>(i16_value<BS>(v[u].y), r[u]);
    const double y3 = i16_decode<BS, WT>(i16_value<BS>(v[u].y >> 16), r[u]);
    acc[0] = first ? y0 : acc[0] + y0;
    acc[1] = first ? y1 : acc[1] + y1;
    acc[2] = first ? y2 : acc[2] + y2;
    acc[3] = first ? y3 : acc[3] + y3;
  }
}

}  // namespace pfe
