// pfd_i16_dev.h — the device side of an int16 fold cube, shared by the kernels that read one
// (pfd_i16.hip, pfd_scrunch.hip): a value as loaded -> the double it stands for, and a lane's
// burst of parts over four values of one sub-band.  See pfd_i16.hip for the contract.
//
// NS, the template parameter of everything that reads a cube with a polarisation axis (the
// _i16_pol calls): 0 is the cube of the _i16 calls, whose code and instantiations are what they
// were; 1 and 2 read NS polarisations of every (fold, part), add them (y_0 + y_1, one rounding)
// and weight the sum once, and find the weights, which have no polarisation axis, through
// strides of their own (PfdI16Src wfs, wps).
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

// scale and offset of NS polarisations of one (fold, part, sub-band) and its one weight, as loaded
template <int NS>
struct I16PolPar {
  unsigned a[NS], o[NS], w;
};
// at: the bytes of (fold, part, sub-band) in scl / offs, polarisation 0; wat: in wts
template <bool WT, int NS>
__device__ __forceinline__ I16PolPar<NS> i16_pol_par(const PfdI16Src& x, int64_t at, int64_t wat) {
  I16PolPar<NS> r;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    r.a[k] = *reinterpret_cast<const unsigned*>(x.scl + at + k * x.pks);
    r.o[k] = *reinterpret_cast<const unsigned*>(x.offs + at + k * x.pks);
  }
  r.w = WT ? *reinterpret_cast<const unsigned*>(x.wts + wat) : 0u;
  return r;
}
// the value of the summed polarisations: each decoded with one rounding, y_0 + y_1 rounded once,
// then, WT, the sum times the weight rounded once (not the sum of two weighted values)
template <bool BS, bool WT, int NS>
__device__ __forceinline__ double i16_pol_decode(const int (&d)[NS], const I16PolPar<NS>& r) {
  double v = i16_decode<BS, false>(d[0], I16Par{r.a[0], r.o[0], 0u});
  if constexpr (NS == 2) v = v + i16_decode<BS, false>(d[1], I16Par{r.a[1], r.o[1], 0u});
  if constexpr (WT) v = v * f32_value<BS>(r.w);
  return v;
}

// parts [p, p + K) onto the four sums of a lane whose elements share one sub-band: K data loads
// and K parameter loads issued before the first add; part 0 is the sums' first value.  NS > 0:
// K x NS data loads and the parameters of both polarisations, wpar the bytes of the lane's
// (fold, sub-band) in wts; a part's polarisations are added and weighted before the part joins
// the running sum
template <bool VEC, bool BS, bool WT, int K, int NS = 0>
__device__ __forceinline__ void psum_add(const PfdI16Src& x, const char* const (&q)[4], int64_t par,
                                         int p, double (&acc)[4], int64_t wpar = 0) {
  if constexpr (NS > 0) {
    u32x2 v[K][NS];
    I16PolPar<NS> r[K];
#pragma unroll
    for (int u = 0; u < K; ++u) {
#pragma unroll
      for (int k = 0; k < NS; ++k) v[u][k] = psum_load<VEC>(q, (int64_t)(p + u) * x.dps + k * x.dks);
      r[u] = i16_pol_par<WT, NS>(x, par + (int64_t)(p + u) * x.pps, wpar + (int64_t)(p + u) * x.wps);
    }
#pragma unroll
    for (int u = 0; u < K; ++u) {
      const bool first = u == 0 && p == 0;
      int d[4][NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        d[0][k] = i16_value<BS>(v[u][k].x);
        d[1][k] = i16_value<BS>(v[u][k].x >> 16);
        d[2][k] = i16_value<BS>(v[u][k].y);
        d[3][k] = i16_value<BS>(v[u][k].y >> 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double y = i16_pol_decode<BS, WT, NS>(d[j], r[u]);
        acc[j] = first ? y : acc[j] + y;
      }
    }
  } else {
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
}

// NS > 0: all NP parts of a quad whose elements share one sub-band, in bursts of B parts: by
// default what keeps 8 data loads in flight (8 parts of one polarisation, 4 parts of two)
template <bool VEC, bool BS, bool WT, int NS, int B = 8 / NS>
__device__ __forceinline__ void psum_pol_run(const PfdI16Src& x, const char* const (&q)[4], int64_t par,
                                             int64_t wpar, int NP, double (&acc)[4]) {
  int p = 0;
  for (; p + B <= NP; p += B) psum_add<VEC, BS, WT, B, NS>(x, q, par, p, acc, wpar);
  if constexpr (B > 4) {
    if (p + 4 <= NP) {
      psum_add<VEC, BS, WT, 4, NS>(x, q, par, p, acc, wpar);
      p += 4;
    }
  }
  if constexpr (B > 2) {
    if (p + 2 <= NP) {
      psum_add<VEC, BS, WT, 2, NS>(x, q, par, p, acc, wpar);
      p += 2;
    }
  }
  if (p < NP) psum_add<VEC, BS, WT, 1, NS>(x, q, par, p, acc, wpar);
}
// NS > 0: all NP parts of a quad with a seam inside: each element with parameters of its own
template <bool VEC, bool BS, bool WT, int NS>
__device__ __forceinline__ void psum_pol_seam(const PfdI16Src& x, const char* const (&q)[4],
                                              const int64_t (&par)[4], const int64_t (&wpar)[4], int NP,
                                              double (&acc)[4]) {
  for (int p = 0; p < NP; ++p) {
    unsigned h[4][NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const u32x2 v = psum_load<VEC>(q, (int64_t)p * x.dps + k * x.dks);
      h[0][k] = v.x, h[1][k] = v.x >> 16, h[2][k] = v.y, h[3][k] = v.y >> 16;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const I16PolPar<NS> r =
          i16_pol_par<WT, NS>(x, par[u] + (int64_t)p * x.pps, wpar[u] + (int64_t)p * x.wps);
      int d[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) d[k] = i16_value<BS>(h[u][k]);
      const double y = i16_pol_decode<BS, WT, NS>(d, r);
      acc[u] = p == 0 ? y : acc[u] + y;
    }
  }
}
// one value (its bytes `at` in data, `par` in scl / offs, `wpar` in wts) of part p
template <bool BS, bool WT, int NS>
__device__ __forceinline__ double i16_pol_one(const PfdI16Src& x, const char* q, int64_t par,
                                              int64_t wpar, int p) {
  int d[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k)
    d[k] = i16_value<BS>(__builtin_nontemporal_load(
        reinterpret_cast<const unsigned short*>(q + (int64_t)p * x.dps + k * x.dks)));
  return i16_pol_decode<BS, WT, NS>(
      d, i16_pol_par<WT, NS>(x, par + (int64_t)p * x.pps, wpar + (int64_t)p * x.wps));
}

}  // namespace pfe
