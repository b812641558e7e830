// pfd_scrunch.hip — scrunching a fold on gfx950: channels to sub-bands, bins to fewer bins.
//
// A fold-mode archive holds every channel and many bins, and nothing inside a group of channels
// is dedispersed.  k_pfd_scrunch makes the fold the PFD calls score out of it in one pass over
// the cube, for fold i, G = nchan / fscr, K = nbin / bscr, each step in fp64 and in this order:
//   S[c][b] = x[0][c][b] + x[1][c][b] + ... + x[npart-1][c][b]      from part 0's value (no 0.0 +)
//   r_c     = ((rot[i][c] % nbin) + nbin) % nbin                     rot == null: 0
//   R[c][b] = S[c][(b + r_c) % nbin]                                 a left rotation
//   B[c][k] = R[c][k bscr] + R[c][k bscr + 1] + ... + R[c][k bscr + bscr - 1]
//   z[g][k] = B[g fscr][k] + B[g fscr + 1][k] + ... + B[g fscr + fscr - 1][k]
// A float32 value is widened, an int16 value decoded (pfd_i16_dev.h) where it is loaded.  Every
// value is loaded once and z is stored once; nothing is added in float32 or in integers.
//
// k_pfd_scrunch (the LDS route): one block per (fold, group).  The rows of a slab of channels of
// the group are consecutive in a part, so the block part-sums the slab as one flat run of
// values -- lane t owns values [4t, 4t + 4) of it, each part one aligned wide load, 8 + 4 + 2 + 1
// parts in flight, as the part-sum kernels do -- into the LDS.  The rotation would break the
// alignment of a global load; in the LDS it is a wrapped index: output lane k then adds its bscr
// rotated values of each row in order, and the result onto its running sum.
// k_pfd_scrunch_direct (any nbin): one lane per output bin, every value loaded alone at its
// rotated place.  The adds and their order are the same, so are the bits.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "launch.h"
#include "pfd_i16_dev.h"

namespace pfe {

#pragma clang fp contract(off)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int SCR_THREADS = 256;       // the direct route's block
constexpr int SCR_MAX_THREADS = 1024;  // the LDS route's: one lane per quad of a slab, up to this
constexpr int SCR_BURST = 8;           // part loads a lane keeps in flight
// blocks a launch: a batch with more (fold, group[, tile]) blocks is launched in pieces, each
// told the number of its first block, so no shape is refused for the size of its grid
constexpr int64_t SCR_MAX_GRID = (int64_t)1 << 30;

// a dense cube of doubles or floats: value (i, p, e), e = c * nbin + b, at x + i*fs + p*ps + e
template <class T>
struct ScrDense {
  const T* x;
  int64_t ps, fs;  // elements
};
template <class T>
using ScrSrc = std::conditional_t<std::is_same<T, int16_t>::value, PfdI16Src, ScrDense<T>>;

// r_c: any int32 reduced to [0, nbin)
__device__ __forceinline__ int scr_rot(const int32_t* rot, int64_t at, int nbin) {
  if (!rot) return 0;
  const int r = rot[at] % nbin;
  return r < 0 ? r + nbin : r;
}

// ---- dense cubes: the lane's four values of one part ------------------------------------
// VEC: consecutive values behind q[0], 16-byte aligned; else each behind its own pointer
template <class T, bool VEC>
__device__ __forceinline__ void scr_load(const T* const (&q)[4], int64_t off, T (&v)[4]) {
  if constexpr (VEC && sizeof(T) == 4) {
    const f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q[0] + off));
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else if constexpr (VEC) {
    const f64x2 a = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(q[0] + off));
    const f64x2 b = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(q[0] + off) + 1);
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(q[u] + off);
  }
}
// parts [p, p + K) onto the four sums, all K loads issued before the first add
template <class T, bool VEC, int K>
__device__ __forceinline__ void scr_add(const T* const (&q)[4], int64_t ps, int p, double (&acc)[4]) {
  T v[K][4];
#pragma unroll
  for (int u = 0; u < K; ++u) scr_load<T, VEC>(q, (int64_t)(p + u) * ps, v[u]);
#pragma unroll
  for (int u = 0; u < K; ++u) {
    const bool first = u == 0 && p == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = first ? (double)v[u][j] : acc[j] + (double)v[u][j];
  }
}
// the part sums of values [e, e + 4) of the slab that begins at channel chan0 of fold `fold`;
// values at or past `elems` are not there (their loads go to the quad's first value)
template <class T, bool VEC, bool BS, bool WT, int NS>
__device__ __forceinline__ void scr_quad(const ScrDense<T>& x, int64_t fold, int64_t chan0, int e,
                                         int elems, int nbin, int NP, double (&acc)[4]) {
  const T* q[4];
  q[0] = x.x + fold * x.fs + chan0 * nbin + e;
#pragma unroll
  for (int u = 1; u < 4; ++u) q[u] = VEC || e + u < elems ? q[0] + u : q[0];
  int p = 0;
  for (; p + SCR_BURST <= NP; p += SCR_BURST) scr_add<T, VEC, SCR_BURST>(q, x.ps, p, acc);
  if (p + 4 <= NP) {
    scr_add<T, VEC, 4>(q, x.ps, p, acc);
    p += 4;
  }
  if (p + 2 <= NP) {
    scr_add<T, VEC, 2>(q, x.ps, p, acc);
    p += 2;
  }
  if (p < NP) scr_add<T, VEC, 1>(q, x.ps, p, acc);
}
// the part sum of one value: channel `chan`, bin b
template <class T, bool BS, bool WT, int NS>
__device__ __forceinline__ double scr_one(const ScrDense<T>& x, int64_t fold, int64_t chan, int b,
                                          int nbin, int NP) {
  const T* q = x.x + fold * x.fs + chan * nbin + b;
  double acc = 0.0;
  int p = 0;
  for (; p + 4 <= NP; p += 4) {
    T v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(q + (int64_t)(p + u) * x.ps);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = u == 0 && p == 0 ? (double)v[u] : acc + (double)v[u];
  }
  for (; p < NP; ++p) {
    const double y = (double)__builtin_nontemporal_load(q + (int64_t)p * x.ps);
    acc = p == 0 ? y : acc + y;
  }
  return acc;
}

// ---- int16 cubes: the decode and the bursts of pfd_i16_dev.h -------------------------------
// NS (pfd_i16_dev.h; 0: the cube of the _i16 calls): a value is the sum of NS polarisations,
// weighted once; the same helpers on both routes, so the same bits
template <class T, bool VEC, bool BS, bool WT, int NS>
__device__ __forceinline__ void scr_quad(const PfdI16Src& x, int64_t fold, int64_t chan0, int e,
                                         int elems, int nbin, int NP, double (&acc)[4]) {
  const char* q[4];
  int64_t par[4];
  int cc = e / nbin, bb = e - cc * nbin;
  q[0] = x.data + fold * x.dfs + (int64_t)2 * (chan0 * nbin + e);
  par[0] = fold * x.pfs + (int64_t)4 * (chan0 + cc);
#pragma unroll
  for (int u = 1; u < 4; ++u) {
    if (++bb == nbin) {  // VEC: never (nbin % 4 == 0)
      bb = 0;
      ++cc;
    }
    const bool ok = VEC || e + u < elems;
    q[u] = ok ? q[0] + 2 * u : q[0];
    par[u] = ok ? fold * x.pfs + (int64_t)4 * (chan0 + cc) : par[0];
  }
  if constexpr (NS > 0) {
    int64_t wpar[4];  // the weights have strides of their own
#pragma unroll
    for (int u = 0; u < 4; ++u) wpar[u] = par[u] - fold * x.pfs + fold * x.wfs;
    // a block of 1024 lanes has 128 registers a lane: the 2-byte loads of two polarisations
    // (four a part and polarisation) go two parts at a time, 16 loads in flight, to stay in them
    constexpr int B = NS == 2 && !VEC ? 2 : 8 / NS;
    if (par[1] == par[0] && par[2] == par[0] && par[3] == par[0])
      psum_pol_run<VEC, BS, WT, NS, B>(x, q, par[0], wpar[0], NP, acc);
    else
      psum_pol_seam<VEC, BS, WT, NS>(x, q, par, wpar, NP, acc);
  } else if (par[1] == par[0] && par[2] == par[0] && par[3] == par[0]) {
    int p = 0;
    for (; p + SCR_BURST <= NP; p += SCR_BURST) psum_add<VEC, BS, WT, SCR_BURST>(x, q, par[0], p, acc);
    if (p + 4 <= NP) {
      psum_add<VEC, BS, WT, 4>(x, q, par[0], p, acc);
      p += 4;
    }
    if (p + 2 <= NP) {
      psum_add<VEC, BS, WT, 2>(x, q, par[0], p, acc);
      p += 2;
    }
    if (p < NP) psum_add<VEC, BS, WT, 1>(x, q, par[0], p, acc);
  } else {  // a seam between channels inside the quad
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
}
template <class T, bool BS, bool WT, int NS>
__device__ __forceinline__ double scr_one(const PfdI16Src& x, int64_t fold, int64_t chan, int b,
                                          int nbin, int NP) {
  const char* q = x.data + fold * x.dfs + (int64_t)2 * (chan * nbin + b);
  const int64_t par = fold * x.pfs + (int64_t)4 * chan;
  double acc = 0.0;
  int p = 0;
  if constexpr (NS > 0) {
    const int64_t wpar = fold * x.wfs + (int64_t)4 * chan;
    for (; p < NP; ++p) {
      const double y = i16_pol_one<BS, WT, NS>(x, q, par, wpar, p);
      acc = p == 0 ? y : acc + y;
    }
  } else {
    for (; p + 4 <= NP; p += 4) {
      unsigned short v[4];
      I16Par r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = __builtin_nontemporal_load(
            reinterpret_cast<const unsigned short*>(q + (int64_t)(p + u) * x.dps));
        r[u] = i16_par<WT>(x, par + (int64_t)(p + u) * x.pps);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double y = i16_decode<BS, WT>(i16_value<BS>(v[u]), r[u]);
        acc = u == 0 && p == 0 ? y : acc + y;
      }
    }
    for (; p < NP; ++p) {
      const unsigned short v =
          __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(q + (int64_t)p * x.dps));
      const double y = i16_decode<BS, WT>(i16_value<BS>(v), i16_par<WT>(x, par + (int64_t)p * x.pps));
      acc = p == 0 ? y : acc + y;
    }
  }
  return acc;
}

// ---- the LDS route ------------------------------------------------------------------------
// Block (fold, g) of a grid of n x G, of as many lanes as a slab has quads (64 to 1024): a block
// is alone with its group, and what it keeps in flight is its lanes times the burst.  LDS: the
// slab, C rows of nbin doubles (C x nbin rounded up to a multiple of 4), then the K running sums
// of a group that takes more than one slab.  VEC
// (nbin % 4 == 0 and the cube aligned for the wide loads at every part): a quad is one load a
// part and lies in one channel; else every value is loaded alone and a quad may span two
// channels, or end past the slab.  An output lane owns the same k in every slab, so the running
// sums need no barrier of their own; the slab is fenced on both sides.
template <class T, bool VEC, bool BS, bool WT, int NS = 0>
__global__ __launch_bounds__(SCR_MAX_THREADS) void k_pfd_scrunch(const ScrSrc<T> x,
                                                             const int32_t* __restrict__ rot,
                                                             double* __restrict__ Z, int NP, int nchan,
                                                             int nbin, int fscr, int bscr, int C, int G,
                                                             int64_t b0) {
  extern __shared__ double scr_lds[];
  const int64_t fg = b0 + blockIdx.x;  // fold * G + g
  const int64_t fold = fg / G;
  const int g = (int)(fg - fold * G);
  const int K = nbin / bscr, tid = threadIdx.x, lanes = blockDim.x;
  double* slab = scr_lds;
  double* zrun = scr_lds + (((int64_t)C * nbin + 3) & ~(int64_t)3);
  double* zout = Z + fg * K;
  for (int c0 = 0; c0 < fscr; c0 += C) {
    const int cs = fscr - c0 < C ? fscr - c0 : C;
    const int64_t chan0 = (int64_t)g * fscr + c0;
    const int elems = cs * nbin;  // <= max(PFD_SCR_SLAB_DOUBLES, nbin)
    if (c0 > 0) __syncthreads();  // the last slab's readers are done
    for (int e = 4 * tid; e < elems; e += 4 * lanes) {
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      scr_quad<T, VEC, BS, WT, NS>(x, fold, chan0, e, elems, nbin, NP, acc);
      if (VEC || e + 3 < elems) {
        f64x2* o = reinterpret_cast<f64x2*>(slab + e);
        o[0] = f64x2{acc[0], acc[1]};
        o[1] = f64x2{acc[2], acc[3]};
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (e + u < elems) slab[e + u] = acc[u];
      }
    }
    __syncthreads();
    const bool last = c0 + cs == fscr;
    for (int k = tid; k < K; k += lanes) {
      double zk = c0 > 0 ? zrun[k] : 0.0;
      for (int cc = 0; cc < cs; ++cc) {
        const double* row = slab + cc * nbin;
        int b = k * bscr + scr_rot(rot, fold * nchan + chan0 + cc, nbin);  // < 2 nbin <= 16384
        if (b >= nbin) b -= nbin;
        double B = row[b];
        for (int j = 1; j < bscr; ++j) {
          if (++b == nbin) b = 0;
          B = B + row[b];
        }
        zk = c0 == 0 && cc == 0 ? B : zk + B;
      }
      if (last)
        zout[k] = zk;
      else
        zrun[k] = zk;
    }
  }
}

// ---- the direct route ---------------------------------------------------------------------
// A grid of n x G x tiles blocks, tile = SCR_THREADS output bins; lane k walks its fscr channels
// and bscr bins in order and part-sums each value where it lies
template <class T, bool BS, bool WT, int NS = 0>
__global__ __launch_bounds__(SCR_THREADS) void k_pfd_scrunch_direct(const ScrSrc<T> x,
                                                                    const int32_t* __restrict__ rot,
                                                                    double* __restrict__ Z, int NP,
                                                                    int nchan, int nbin, int fscr,
                                                                    int bscr, int tiles, int64_t b0) {
  const int64_t blk = b0 + blockIdx.x;
  const int64_t fg = blk / tiles;  // fold * G + g
  const int K = nbin / bscr, G = nchan / fscr;
  const int k = (int)(blk - fg * tiles) * SCR_THREADS + (int)threadIdx.x;
  if (k >= K) return;
  const int64_t fold = fg / G;
  const int64_t chan0 = (fg - fold * G) * fscr;
  double zk = 0.0;
  for (int cc = 0; cc < fscr; ++cc) {
    int64_t b = (int64_t)k * bscr + scr_rot(rot, fold * nchan + chan0 + cc, nbin);
    if (b >= nbin) b -= nbin;
    double B = 0.0;
    for (int j = 0; j < bscr; ++j) {
      const double s = scr_one<T, BS, WT, NS>(x, fold, chan0 + cc, (int)b, nbin, NP);
      B = j == 0 ? s : B + s;
      if (++b == nbin) b = 0;
    }
    zk = cc == 0 ? B : zk + B;
  }
  Z[fg * K + k] = zk;
}

// ---- launch -------------------------------------------------------------------------------
struct ScrShape {
  int npart, nchan, nbin, fscr, bscr;
  int64_t n;
};

template <class T, bool BS, bool WT, int NS = 0>
static hipError_t scr_launch(const ScrSrc<T>& x, bool vec, const int32_t* rot, double* z,
                             const ScrShape& s, bool direct, hipStream_t st) {
  const int G = s.nchan / s.fscr, K = s.nbin / s.bscr;
  if (direct || !pfd_scrunch_lds(s.nbin, s.bscr)) {
    const dim3 block(SCR_THREADS);
    const int64_t tiles = ((int64_t)K + SCR_THREADS - 1) / SCR_THREADS;
    const int64_t blocks = s.n * G * tiles;
    for (int64_t b0 = 0; b0 < blocks; b0 += SCR_MAX_GRID) {
      const int64_t nb = blocks - b0 < SCR_MAX_GRID ? blocks - b0 : SCR_MAX_GRID;
      hipLaunchKernelGGL((k_pfd_scrunch_direct<T, BS, WT, NS>), dim3((unsigned)nb), block, 0, st, x, rot, z,
                         s.npart, s.nchan, s.nbin, s.fscr, s.bscr, (int)tiles, b0);
    }
    return hipGetLastError();
  }
  const int64_t blocks = s.n * G;
  const int C = pfd_scrunch_slab_chans(s.nbin, s.fscr);
  // the running sums live in the LDS only when a group takes more than one slab
  const size_t lds = ((((size_t)C * s.nbin + 3) & ~(size_t)3) + (C < s.fscr ? K : 0)) * sizeof(double);
  const int64_t quads = ((int64_t)C * s.nbin + 3) / 4;
  const dim3 block(quads >= SCR_MAX_THREADS ? SCR_MAX_THREADS : (unsigned)((quads + 63) & ~63));
  for (int64_t b0 = 0; b0 < blocks; b0 += SCR_MAX_GRID) {
    const dim3 grid((unsigned)(blocks - b0 < SCR_MAX_GRID ? blocks - b0 : SCR_MAX_GRID));
    if (vec)
      hipLaunchKernelGGL((k_pfd_scrunch<T, true, BS, WT, NS>), grid, block, lds, st, x, rot, z, s.npart,
                         s.nchan, s.nbin, s.fscr, s.bscr, C, G, b0);
    else
      hipLaunchKernelGGL((k_pfd_scrunch<T, false, BS, WT, NS>), grid, block, lds, st, x, rot, z, s.npart,
                         s.nchan, s.nbin, s.fscr, s.bscr, C, G, b0);
  }
  return hipGetLastError();
}

hipError_t launch_pfd_scrunch(const PfdScrunchSrc& x, const int32_t* rot, double* z, int npart,
                              int nchan, int nbin, int fscr, int bscr, int64_t n, bool direct,
                              hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const ScrShape s{npart, nchan, nbin, fscr, bscr, n};
  const int64_t E = (int64_t)nchan * nbin;
  if (x.f64) {
    const ScrDense<double> d{x.f64, E, E * npart};
    return scr_launch<double, false, false>(d, nbin % 4 == 0 && ((uintptr_t)x.f64 & 15) == 0, rot, z, s,
                                            direct, st);
  }
  if (x.f32) {
    const ScrDense<float> d{x.f32, E, E * npart};
    return scr_launch<float, false, false>(d, nbin % 4 == 0 && ((uintptr_t)x.f32 & 15) == 0, rot, z, s,
                                           direct, st);
  }
  const PfdI16Src& q = x.i16;
  const bool vec = nbin % 4 == 0 && (((uintptr_t)q.data | (uintptr_t)q.dfs | (uintptr_t)q.dps) & 7) == 0;
  const int ns = pfd_i16_ns(q);
  if (ns == 2) {
    if (q.bswap)
      return q.wts ? scr_launch<int16_t, true, true, 2>(q, vec, rot, z, s, direct, st)
                   : scr_launch<int16_t, true, false, 2>(q, vec, rot, z, s, direct, st);
    return q.wts ? scr_launch<int16_t, false, true, 2>(q, vec, rot, z, s, direct, st)
                 : scr_launch<int16_t, false, false, 2>(q, vec, rot, z, s, direct, st);
  }
  if (ns == 1)  // one polarisation of several, its weights (given) apart from scl's strides
    return q.bswap ? scr_launch<int16_t, true, true, 1>(q, vec, rot, z, s, direct, st)
                   : scr_launch<int16_t, false, true, 1>(q, vec, rot, z, s, direct, st);
  if (q.bswap)
    return q.wts ? scr_launch<int16_t, true, true>(q, vec, rot, z, s, direct, st)
                 : scr_launch<int16_t, true, false>(q, vec, rot, z, s, direct, st);
  return q.wts ? scr_launch<int16_t, false, true>(q, vec, rot, z, s, direct, st)
               : scr_launch<int16_t, false, false>(q, vec, rot, z, s, direct, st);
}

}  // namespace pfe
