// pfd_avgprof.hip — a fold's average on gfx950: numpy's (profs / proflen).sum() of the cube.
//
// PFDFile.load keeps avgprof = (self.profs / self.proflen).sum() (PFDFile.py:225), and the
// chi^2-vs-DM sweep subtracts it from every bin, so the DM curve wants its exact bits.  numpy
// evaluates the expression as
//   y[e] = (double)x[e] / (double)proflen            the correctly rounded fp64 quotient
//   c[k] = pairwise sum of y[8192 k .. 8192 k + 8191]  (the last chunk shorter)
//   sum  = 0.0 + c[0] + c[1] + c[2] + ...              in order, onto numpy's initial 0.0
// where a pairwise sum splits n > 128 values at floor8(n / 2) and sums a leaf of n <= 128 in
// eight accumulators, r[t] = y[t] + y[t + 8] + ..., ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then
// the n % 8 last values in order (n < 8: 0.0 + y0 + y1 ...).  This is not one pairwise tree
// over the cube: the chunks of 8192 are numpy's reduction buffers.  The initial 0.0 shows in
// one case only: a fold whose values are all -0.0 sums to +0.0, as numpy's does.
//
// k_pfd_avgprof: one wave per (fold, chunk).  Its eight 8-lane groups each take one leaf of
// the chunk's tree at a time, lane t of a group being accumulator t (np_sum.h's layout), so a
// group's load is 8 consecutive values and the 16 loads of a lane walk the leaf's 1 KiB; the
// leaf sums meet in LDS and are added up the tree.  k_pfd_avgprof_fin: one lane per fold adds
// the fold's chunk sums in order.  Two plain kernels on one stream; no atomics.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "launch.h"
#include "np_sum.h"

namespace pfe {

#pragma clang fp contract(off)

static_assert(PFD_AVG_CHUNK == NP_BUFSIZE, "a chunk is one of numpy's reduction buffers");

constexpr int AVG_WPB = 4;        // waves per block (each works alone: no block barrier)
// a node is split only when it holds > 128 values, into floor8(n/2) >= 64 and the rest, so a
// leaf of a split chunk holds >= 64 values: <= 128 leaves, and (np_inl_max(7) >= 8192) every
// leaf at depth <= 7
constexpr int AVG_MAX_LEAVES = PFD_AVG_CHUNK / 64;
constexpr int AVG_STACK = 10;     // depth of the two walks of a chunk's tree (<= 8 needed)

// a node of a chunk's tree: off < 8192 (13 bits), len <= 8192 (14 bits), depth <= 7
__device__ __forceinline__ uint32_t avg_node(int off, int len, int depth) {
  return (uint32_t)off | ((uint32_t)len << 13) | ((uint32_t)depth << 27);
}
__device__ __forceinline__ int avg_off(uint32_t v) { return (int)(v & 8191u); }
__device__ __forceinline__ int avg_len(uint32_t v) { return (int)((v >> 13) & 16383u); }
__device__ __forceinline__ int avg_depth(uint32_t v) { return (int)(v >> 27); }

// an 8-byte value whose bytes are reversed in memory (a big-endian file's double on this
// machine: PFE_FLAG_PFD_BSWAP): loaded as the word it is, widened to double through the reversal
struct be64 {
  unsigned long long w;
  __device__ __forceinline__ explicit operator double() const {
    return __builtin_bit_cast(double, __builtin_bswap64(w));
  }
};
static_assert(sizeof(be64) == 8 && alignof(be64) == 8, "a be64 is one word of the cube");

// A value of an int16 cube (pfd_i16.hip) as loaded with the scale, offset and weight of its
// (part, sub-band): widened to double through the decode, (double)d * scl + offs rounded once
// (the product is exact, so the fused multiply-add rounds where multiply-then-add does), then,
// WT, times the weight rounded once.  BS: every value byte-reversed (PFE_FLAG_PFD_BSWAP)
template <bool BS, bool WT>
struct i16_elem {
  unsigned d, a, o, w;
  static __device__ __forceinline__ double f32(unsigned v) {
    return (double)__builtin_bit_cast(float, BS ? __builtin_bswap32(v) : v);
  }
  __device__ __forceinline__ explicit operator double() const {
    const unsigned short h = (unsigned short)d;
    const double x = __builtin_fma((double)(int)(short)(BS ? __builtin_bswap16(h) : h), f32(a), f32(o));
    if constexpr (WT) return x * f32(w);
    return x;
  }
};
// Where a pointer into a float or double cube stands, for one fold of an int16 cube: values
// [at, ...) of the fold in the order (p, s, b).  at = the chunk's first value as part p0 and
// element r0 of that part, plus what has been added since (a chunk holds <= 8192 values and a
// part E1 = nsub x L < 2^31, so the 32-bit division is by a value that fits)
template <bool BS, bool WT>
struct i16_cursor {
  const char *data, *scl, *offs, *wts;  // of the fold's part p0
  int64_t dps, pps;
  unsigned E1, L, r;
  __device__ __forceinline__ i16_cursor operator+(int k) const {
    i16_cursor c = *this;
    c.r += (unsigned)k;
    return c;
  }
  __device__ __forceinline__ i16_elem<BS, WT> operator[](int k) const {
    const unsigned j = r + (unsigned)k, p = j / E1, e = j - p * E1;
    const int64_t at = (int64_t)p * pps + (int64_t)4 * (e / L);
    i16_elem<BS, WT> v;
    v.d = *reinterpret_cast<const unsigned short*>(data + (int64_t)p * dps + (int64_t)2 * e);
    v.a = *reinterpret_cast<const unsigned*>(scl + at);
    v.o = *reinterpret_cast<const unsigned*>(offs + at);
    v.w = WT ? *reinterpret_cast<const unsigned*>(wts + at) : 0u;
    return v;
  }
};
// the int16 cube of a launch: what a `const T* X` is for the others.  It carries the arrays and
// the four strides these kernels read and nothing of the polarisation fields PfdI16Src has
// beside them, so the kernels' arguments, and with them their code, are what they were
struct i16_arrays {
  const char *data, *scl, *offs, *wts;
  int64_t dfs, dps, pfs, pps;
  bool bswap;
  explicit i16_arrays(const PfdI16Src& q)
      : data(q.data), scl(q.scl), offs(q.offs), wts(q.wts), dfs(q.dfs), dps(q.dps), pfs(q.pfs),
        pps(q.pps), bswap(q.bswap) {}
};
template <bool BS, bool WT>
struct i16_cube {
  i16_arrays x;
  unsigned E1, L;
};

// A value of an int16 cube with a polarisation axis (the _i16_pol calls; NS = 1, 2 as in
// pfd_i16_dev.h) as loaded: the NS polarisations of one (part, sub-band, bin) with their scales and
// offsets and the one weight.  Its value is the polarisation sum: each decoded with one rounding,
// y_0 + y_1 rounded once, then, WT, the sum times the weight rounded once
template <bool BS, bool WT, int NS>
struct i16_pol_elem {
  unsigned d[NS], a[NS], o[NS], w;
  __device__ __forceinline__ explicit operator double() const {
    double x = (double)i16_elem<BS, false>{d[0], a[0], o[0], 0u};
    if constexpr (NS == 2) x = x + (double)i16_elem<BS, false>{d[1], a[1], o[1], 0u};
    if constexpr (WT) return x * i16_elem<BS, false>::f32(w);
    return x;
  }
};
// i16_cursor for such a cube.  The 32-bit part of the walk is as there (r + k < 2^31: j, p and e
// fit); the polarisation strides and the weights' own part stride are added in 64 bits, to
// pointers, so they put no bound of their own on the shape
template <bool BS, bool WT, int NS>
struct i16_pol_cursor {
  const char *data, *scl, *offs, *wts;  // of the fold's part p0, polarisation 0
  int64_t dps, pps, wps, dks, pks;
  unsigned E1, L, r;
  __device__ __forceinline__ i16_pol_cursor operator+(int k) const {
    i16_pol_cursor c = *this;
    c.r += (unsigned)k;
    return c;
  }
  __device__ __forceinline__ i16_pol_elem<BS, WT, NS> operator[](int k) const {
    const unsigned j = r + (unsigned)k, p = j / E1, e = j - p * E1;
    const int64_t sb = (int64_t)4 * (e / L), at = (int64_t)p * pps + sb;
    i16_pol_elem<BS, WT, NS> v;
#pragma unroll
    for (int m = 0; m < NS; ++m) {
      v.d[m] = *reinterpret_cast<const unsigned short*>(data + (int64_t)p * dps + m * dks + (int64_t)2 * e);
      v.a[m] = *reinterpret_cast<const unsigned*>(scl + at + m * pks);
      v.o[m] = *reinterpret_cast<const unsigned*>(offs + at + m * pks);
    }
    v.w = WT ? *reinterpret_cast<const unsigned*>(wts + (int64_t)p * wps + sb) : 0u;
    return v;
  }
};
template <bool BS, bool WT, int NS>
struct i16_pol_cube {
  PfdI16Src x;
  unsigned E1, L;
};

// A value of a masked cube (the _kill calls, pfd_kill.hip) as loaded with the kill bit of its
// (part, sub-band): widened to double through the selection, +0.0 where killed -- replaced,
// never multiplied, so what a killed row holds reaches no sum.  T: double, be64 or float
template <typename T>
struct kill_elem {
  T v;
  bool dead;
  __device__ __forceinline__ explicit operator double() const { return dead ? 0.0 : (double)v; }
};
// Where a pointer into the cube stands, for one fold of a masked cube: values [at, ...) of the
// fold in the order (p, s, b), at = part p0 and element r of that part, as for i16_cursor
template <typename T>
struct kill_cursor {
  const T* x;                   // the fold's part p0
  const uint8_t *parts, *subs;  // the fold's masks, parts from p0 on; either null
  unsigned E1, L, r;
  __device__ __forceinline__ kill_cursor operator+(int k) const {
    kill_cursor c = *this;
    c.r += (unsigned)k;
    return c;
  }
  __device__ __forceinline__ kill_elem<T> operator[](int k) const {
    const unsigned j = r + (unsigned)k, p = j / E1, e = j - p * E1;
    kill_elem<T> v;
    v.v = x[j];
    v.dead = (parts && parts[p] != 0) || (subs && subs[e / L] != 0);
    return v;
  }
};
// the masked cube of a launch: dense, n x NP x E1 values, parts n x NP and subs n x nsub bytes
template <typename T>
struct kill_cube {
  const T* x;
  PfdKillSrc k;
  int NP, nsub;
  unsigned E1, L;
};

// the values of `fold` from its e0-th on: a pointer, or a cursor
template <typename T>
__device__ __forceinline__ const T* avg_at(const T* X, int64_t fold, int64_t E, int64_t e0) {
  return X + fold * E + e0;
}
template <bool BS, bool WT>
__device__ __forceinline__ i16_cursor<BS, WT> avg_at(const i16_cube<BS, WT>& X, int64_t fold, int64_t,
                                                      int64_t e0) {
  const int64_t p0 = e0 / X.E1;
  i16_cursor<BS, WT> c;
  c.data = X.x.data + fold * X.x.dfs + p0 * X.x.dps;
  c.scl = X.x.scl + fold * X.x.pfs + p0 * X.x.pps;
  c.offs = X.x.offs + fold * X.x.pfs + p0 * X.x.pps;
  c.wts = WT ? X.x.wts + fold * X.x.pfs + p0 * X.x.pps : nullptr;
  c.dps = X.x.dps;
  c.pps = X.x.pps;
  c.E1 = X.E1;
  c.L = X.L;
  c.r = (unsigned)(e0 - p0 * X.E1);
  return c;
}

template <bool BS, bool WT, int NS>
__device__ __forceinline__ i16_pol_cursor<BS, WT, NS> avg_at(const i16_pol_cube<BS, WT, NS>& X,
                                                              int64_t fold, int64_t, int64_t e0) {
  const int64_t p0 = e0 / X.E1;
  i16_pol_cursor<BS, WT, NS> c;
  c.data = X.x.data + fold * X.x.dfs + p0 * X.x.dps;
  c.scl = X.x.scl + fold * X.x.pfs + p0 * X.x.pps;
  c.offs = X.x.offs + fold * X.x.pfs + p0 * X.x.pps;
  c.wts = WT ? X.x.wts + fold * X.x.wfs + p0 * X.x.wps : nullptr;
  c.dps = X.x.dps;
  c.pps = X.x.pps;
  c.wps = X.x.wps;
  c.dks = X.x.dks;
  c.pks = X.x.pks;
  c.E1 = X.E1;
  c.L = X.L;
  c.r = (unsigned)(e0 - p0 * X.E1);
  return c;
}

template <typename T>
__device__ __forceinline__ kill_cursor<T> avg_at(const kill_cube<T>& X, int64_t fold, int64_t E,
                                                 int64_t e0) {
  const int64_t p0 = e0 / X.E1;
  kill_cursor<T> c;
  c.x = X.x + fold * E + p0 * X.E1;
  c.parts = X.k.parts ? X.k.parts + fold * X.NP + p0 : nullptr;
  c.subs = X.k.subs ? X.k.subs + fold * X.nsub : nullptr;
  c.E1 = X.E1;
  c.L = X.L;
  c.r = (unsigned)(e0 - p0 * X.E1);
  return c;
}

// x / L.  P2 (L a power of two): x * (1 / L), the same real number rounded once, so the same
// bits (subnormal results included); else the IEEE quotient
template <bool P2>
__device__ __forceinline__ double avg_scale(double x, double dl, double inv) {
  if constexpr (P2) return x * inv;
  return x / dl;
}

// numpy's leaf sum of p[0 .. len), 8 <= len <= 128, scaled: the result in every lane of the
// 8-lane group (t = lane & 7).  Every lane of the wave is here (the DPP steps read within a
// group), groups may hold leaves of different lengths: selects, no divergent branch.
template <typename Cur, bool P2>
__device__ __forceinline__ double avg_leaf(const Cur p, int len, int t, double dl, double inv) {
  const int nb = len & ~7;
  std::remove_cv_t<std::remove_reference_t<decltype(p[0])>> raw[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) raw[m] = p[min(t + 8 * m, len - 1)];
  double r = avg_scale<P2>((double)raw[0], dl, inv);
#pragma unroll
  for (int m = 1; m < 16; ++m) {
    const double y = avg_scale<P2>((double)raw[m], dl, inv);
    r = 8 * m < nb ? r + y : r;
  }
  r += dpp_f64<DPP_QUAD_XOR1>(r);  // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
  r += dpp_f64<DPP_QUAD_XOR2>(r);
  r += dpp_f64<DPP_ROW_HALF_MIRROR>(r);
  for (int k = 0; k < 7; ++k) {  // the len % 8 last values, in order
    const bool more = nb + k < len;
    if (__ballot(more) == 0) break;
    const double y = avg_scale<P2>((double)p[min(nb + k, len - 1)], dl, inv);
    r = more ? r + y : r;
  }
  return r;
}

// csum[fold * nch + chunk] = numpy's pairwise sum of the chunk's scaled values.  X: n folds of
// E values, dense (Src a pointer to them), or the int16 cube of pfd_i16.hip (Src an i16_cube);
// nch = ceil(E / 8192); total = n * nch waves.
template <typename Src, bool P2>
__global__ __launch_bounds__(AVG_WPB * 64) void k_pfd_avgprof(const Src X, int64_t E, int nch,
                                                             int64_t total, double dl, double inv,
                                                             double* __restrict__ csum) {
  __shared__ double s_sum[AVG_WPB][AVG_MAX_LEAVES];
  __shared__ uint32_t s_tab[AVG_WPB][AVG_MAX_LEAVES];
  __shared__ uint32_t s_walk[AVG_WPB][AVG_STACK];
  __shared__ double s_val[AVG_WPB][AVG_STACK];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t wg = (int64_t)blockIdx.x * AVG_WPB + w;
  if (wg >= total) return;  // the whole wave
  const int64_t fold = wg / nch;
  const int ch = (int)(wg - fold * nch);
  const int64_t e0 = (int64_t)ch * PFD_AVG_CHUNK;
  const int n = (int)(E - e0 < PFD_AVG_CHUNK ? E - e0 : PFD_AVG_CHUNK);
  const auto x = avg_at(X, fold, E, e0);

  if (n < 8) {  // 0.0 + y0 + y1 ...
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += avg_scale<P2>((double)x[i], dl, inv);
    if (lane == 0) csum[wg] = r;
    return;
  }

  // the leaves of the chunk's tree, in order: one (n <= 128), 64 of 128 values under six
  // full levels (n = 8192), or what a walk of the tree by lane 0 finds
  const bool full = n == PFD_AVG_CHUNK, one = n <= 128;
  int nleaf = one ? 1 : AVG_MAX_LEAVES / 2;
  if (!full && !one) {
    if (lane == 0) {
      int sp = 1, cnt = 0;
      s_walk[w][0] = avg_node(0, n, 0);
      while (sp > 0) {
        const uint32_t v = s_walk[w][--sp];
        const int off = avg_off(v), len = avg_len(v), d = avg_depth(v);
        if (len <= 128) {
          s_tab[w][cnt++] = v;
        } else {
          int n2 = len / 2;
          n2 -= n2 % 8;
          s_walk[w][sp++] = avg_node(off + n2, len - n2, d + 1);  // the right half waits
          s_walk[w][sp++] = avg_node(off, n2, d + 1);
        }
      }
      s_walk[w][0] = (uint32_t)cnt;
    }
    lds_sync();
    nleaf = uni((int)s_walk[w][0]);
  }

  const int g = lane >> 3, t = lane & 7;
  for (int b = 0; b < nleaf; b += 8) {
    const int j = min(b + g, nleaf - 1);  // a group past the last leaf sums it again, unstored
    int off = 0, len = n;
    if (full) {
      off = 128 * j;
      len = 128;
    } else if (!one) {
      const uint32_t v = s_tab[w][j];
      off = avg_off(v);
      len = avg_len(v);
    }
    const double s = avg_leaf<decltype(x + off), P2>(x + off, len, t, dl, inv);
    if (t == 0 && b + g < nleaf) s_sum[w][b + g] = s;
  }
  lds_sync();

  if (one) {
    if (lane == 0) csum[wg] = s_sum[w][0];
  } else if (full) {
    // six full levels over 64 leaves in order: the xor butterfly (a + b = b + a bit for bit)
    double v = s_sum[w][lane];
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s);
    if (lane == 0) csum[wg] = v;
  } else if (lane == 0) {
    // the leaves in order with their depths: two neighbours of one depth are the halves of a
    // node, left + right
    int sp = 0;
    for (int j = 0; j < nleaf; ++j) {
      double val = s_sum[w][j];
      int d = avg_depth(s_tab[w][j]);
      while (sp > 0 && (int)s_walk[w][sp - 1] == d) {
        val = s_val[w][--sp] + val;
        --d;
      }
      s_val[w][sp] = val;
      s_walk[w][sp++] = (uint32_t)d;
    }
    csum[wg] = s_val[w][0];
  }
}

// out[i * stride] = 0.0 + c[i][0] + c[i][1] + ... + c[i][nch - 1], in order
__global__ __launch_bounds__(256) void k_pfd_avgprof_fin(const double* __restrict__ csum, int nch,
                                                         int64_t n, double* __restrict__ out,
                                                         int64_t stride) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* c = csum + i * nch;
  double r = 0.0;
  for (int k = 0; k < nch; ++k) r += c[k];
  out[i * stride] = r;
}

template <typename Src>
static hipError_t launch_avgprof(const Src x, int64_t E, int L, int64_t n, double* csum, double* out,
                                 int64_t stride, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t nch = pfd_avg_chunks(E), total = n * nch;
  const int64_t blocks = (total + AVG_WPB - 1) / AVG_WPB;
  if (E < 1 || L < 1 || nch > 0x7fffffff || blocks > 0x7fffffff) return hipErrorInvalidValue;
  const bool p2 = (L & (L - 1)) == 0;
  const double dl = (double)L, inv = 1.0 / dl;  // exact for a power of two
  const dim3 grid((unsigned)blocks), block(AVG_WPB * 64);
  if (p2)
    hipLaunchKernelGGL((k_pfd_avgprof<Src, true>), grid, block, 0, st, x, E, (int)nch, total, dl, inv,
                       csum);
  else
    hipLaunchKernelGGL((k_pfd_avgprof<Src, false>), grid, block, 0, st, x, E, (int)nch, total, dl,
                       inv, csum);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pfd_avgprof_fin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, csum,
                     (int)nch, n, out, stride);
  return hipGetLastError();
}

hipError_t launch_pfd_avgprof(const double* x, int64_t E, int L, int64_t n, double* csum,
                              double* out, int64_t stride, hipStream_t st) {
  return launch_avgprof(x, E, L, n, csum, out, stride, st);
}
hipError_t launch_pfd_avgprof_f32(const float* x, int64_t E, int L, int64_t n, double* csum,
                                  double* out, int64_t stride, hipStream_t st) {
  return launch_avgprof(x, E, L, n, csum, out, stride, st);
}
hipError_t launch_pfd_avgprof_be64(const double* x, int64_t E, int L, int64_t n, double* csum,
                                   double* out, int64_t stride, hipStream_t st) {
  return launch_avgprof(reinterpret_cast<const be64*>(x), E, L, n, csum, out, stride, st);
}
template <bool BS>
static hipError_t launch_avgprof_i16(const PfdI16Src& x, unsigned E1, int64_t E, int L, int64_t n,
                                     double* csum, double* out, int64_t stride, hipStream_t st) {
  const int ns = pfd_i16_ns(x);
  if (ns == 2) {
    if (x.wts)
      return launch_avgprof(i16_pol_cube<BS, true, 2>{x, E1, (unsigned)L}, E, L, n, csum, out, stride, st);
    return launch_avgprof(i16_pol_cube<BS, false, 2>{x, E1, (unsigned)L}, E, L, n, csum, out, stride, st);
  }
  if (ns == 1)  // one polarisation of several, its weights (given) apart from scl's strides
    return launch_avgprof(i16_pol_cube<BS, true, 1>{x, E1, (unsigned)L}, E, L, n, csum, out, stride, st);
  const i16_arrays a(x);
  if (x.wts) return launch_avgprof(i16_cube<BS, true>{a, E1, (unsigned)L}, E, L, n, csum, out, stride, st);
  return launch_avgprof(i16_cube<BS, false>{a, E1, (unsigned)L}, E, L, n, csum, out, stride, st);
}
hipError_t launch_pfd_avgprof_i16(const PfdI16Src& x, int npart, int nsub, int L, int64_t n,
                                  double* csum, double* out, int64_t stride, hipStream_t st) {
  const int64_t E1 = (int64_t)nsub * L, E = E1 * npart;
  // i16_cursor's and i16_pol_cursor's 32 bits (the polarisation strides are 64-bit offsets)
  if (E1 < 1 || E1 > 0x7fffffff - PFD_AVG_CHUNK) return hipErrorInvalidValue;
  return x.bswap ? launch_avgprof_i16<true>(x, (unsigned)E1, E, L, n, csum, out, stride, st)
                 : launch_avgprof_i16<false>(x, (unsigned)E1, E, L, n, csum, out, stride, st);
}
template <typename T>
static hipError_t launch_avgprof_kill(const void* x, const PfdKillSrc& k, int npart, int nsub, int L,
                                      int64_t n, double* csum, double* out, int64_t stride,
                                      hipStream_t st) {
  const int64_t E1 = (int64_t)nsub * L, E = E1 * npart;
  if (E1 < 1 || E1 > 0x7fffffff - PFD_AVG_CHUNK) return hipErrorInvalidValue;  // kill_cursor's 32 bits
  return launch_avgprof(kill_cube<T>{static_cast<const T*>(x), k, npart, nsub, (unsigned)E1, (unsigned)L},
                        E, L, n, csum, out, stride, st);
}
hipError_t launch_pfd_avgprof_kill(const void* x, int elem, const PfdKillSrc& k, int npart, int nsub,
                                   int L, int64_t n, double* csum, double* out, int64_t stride,
                                   hipStream_t st) {
  switch (elem) {
    case PFD_KILL_F64: return launch_avgprof_kill<double>(x, k, npart, nsub, L, n, csum, out, stride, st);
    case PFD_KILL_BE64: return launch_avgprof_kill<be64>(x, k, npart, nsub, L, n, csum, out, stride, st);
    case PFD_KILL_F32: return launch_avgprof_kill<float>(x, k, npart, nsub, L, n, csum, out, stride, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace pfe
