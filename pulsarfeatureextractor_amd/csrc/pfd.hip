// pfd.hip — PRESTO-fold (PFD) preprocessing and PFD Lyon features on gfx950.
//
// One 64-lane workgroup per candidate does what a freshly loaded PFDFile does for the
// dmprof path (paths relative to PulsarFeatureExtractor/src/):
//   dedisperse at the best DM                   PFDFile.py:330-374  (integer-bin rotations)
//   getprofile + scale                          PFDFile.py:256-310  ((sumprof-min)/mean -> 0..255)
//   plot_chi2_vs_DM(dms[0], dms[-1], 100)       PFDFile.py:378-423  (rotations accumulate; float32)
//   computeProfileStatScores                    PFDFile.py:522-551  (float64 numpy/scipy stats)
//   computeDMCurveStatScores                    PFDFile.py:553-583  (float32 numpy/scipy stats)
// Every reduction is numpy's own: axis reductions over parts / sub-bands add sequentially,
// contiguous sums use numpy's pairwise summation (8 accumulators per block of <= 128, blocks
// split at n/2 rounded down to a multiple of 8), and the DM-curve statistics run in float32
// as numpy does on a float32 array.  The sub-band profiles of the candidate live in LDS.
#include <cmath>
#include <cstdlib>

#include "pfd_dev.h"

namespace pfe {

#pragma clang fp contract(off)

__global__ __launch_bounds__(64) void k_pfd_dmprof(PfdArgs a) {
  extern __shared__ double lds[];
  const int64_t c = blockIdx.x;
  if (c >= a.n) return;
  const int lane = lane_id();
  const int NP = a.npart, NS = a.nsub, L = a.L;
  double* T = lds;                  // NS x L: sub-band profiles summed over parts, dedispersed
  double* buf = T + (size_t)NS * L;  // L
  double* tmp = buf + L;             // L
  double* dl = tmp + L;              // NS delays
  double* sdb = dl + NS;             // NS subdelays_bins
  double* bv = sdb + NS;             // NS (22-score path: per-band variances)
  int* cum = (int*)(bv + NS);        // NS rotations applied since the dedispersion
  __shared__ float chs[PFE_PFD_NDM], ftmp[PFE_PFD_NDM];
  const double* sc = a.scal + c * PFE_PFD_NSCAL;
  const double bestdm = sc[PFE_PFD_BESTDM], bps = sc[PFE_PFD_BINSPERSEC];
  const double avgprof = sc[PFE_PFD_AVGPROF], varprof = sc[PFE_PFD_VARPROF];
  const double dm_lo = sc[PFE_PFD_DM_LO], dm_hi = sc[PFE_PFD_DM_HI];
  const double numdms = sc[PFE_PFD_NUMDMS];
  const double* fr = a.subfreqs + c * NS;
  const double* P = a.profs + c * (int64_t)NP * NS * L;
  // ---- dedisperse at the best DM (PFDFile.py:346-373, interp = 0)
  for (int j = lane; j < NS; j += 64) dl[j] = delay_from_dm(bestdm, fr[j]);
  lds_sync();
  {
    const double hif = dl[NS - 1];
    for (int j = lane; j < NS; j += 64) {
      const double delaybins = (dl[j] - hif) * bps - 0.0;
      const double nw = floor(delaybins + 0.5);
      sdb[j] = 0.0 + nw;
      cum[j] = pymod((long long)nw, L);  // rotation of the dedispersion itself
    }
  }
  lds_sync();
  // T[j][b] = sum over parts of the rotated sub-integration profiles (profs.sum(0))
  for (int j = 0; j < NS; ++j) {
    const int r = cum[j];
    for (int b = lane; b < L; b += 64) {
      const int src = b + r < L ? b + r : b + r - L;
      double s = P[(int64_t)j * L + src];
      for (int p = 1; p < NP; ++p) s += P[((int64_t)p * NS + j) * L + src];
      T[(size_t)j * L + b] = s;
    }
  }
  lds_sync();
  // sumprof = T.sum(0); the profile (getprofile + scale)
  for (int b = lane; b < L; b += 64) {
    double s = T[b];
    for (int j = 1; j < NS; ++j) s += T[(size_t)j * L + b];
    buf[b] = s;
  }
  lds_sync();
  {
    const double mn = py_ext_wave<false>(buf, L, lane);
    for (int b = lane; b < L; b += 64) buf[b] = buf[b] - mn;  // normprof
    lds_sync();
    const double mean = np_sum_row<false>(buf, L, lane) / (double)L;
    lds_sync();
    for (int b = lane; b < L; b += 64) buf[b] = buf[b] / mean;  // s
    lds_sync();
    const double smin = py_ext_wave<false>(buf, L, lane), smax = py_ext_wave<true>(buf, L, lane);
    lds_sync();
    for (int b = lane; b < L; b += 64) {
      const double t = (buf[b] - smin) / (smax - smin);
      buf[b] = (0.0 * (1.0 - t)) + (255.0 * t);
      if (a.profile) a.profile[c * L + b] = buf[b];
    }
    lds_sync();
  }
  double po[4] = {0.0, 0.0, 0.0, 0.0};
  if (a.lyon8) stats4_f64<false>(buf, tmp, L, lane, po);
  // ---- chi^2 versus DM over span(dms[0], dms[-1], 100) (PFDFile.py:378-423)
  const bool dm_ok = numdms > 1.0;  // numdms == 1: dms is a scalar and dms[0] raises
  if (dm_ok && (a.chis || a.lyon8)) {
    for (int j = lane; j < NS; j += 64) cum[j] = 0;
    lds_sync();
    for (int k = 0; k < PFE_PFD_NDM; ++k) {
      const double dm = dm_lo + ((dm_hi - dm_lo) * (double)k) / (double)(PFE_PFD_NDM - 1);
      for (int j = lane; j < NS; j += 64) dl[j] = delay_from_dm(dm, fr[j]);
      lds_sync();
      const double hif = dl[NS - 1];
      for (int j = lane; j < NS; j += 64) {
        const double delaybins = (dl[j] - hif) * bps - sdb[j];
        const double nw = floor(delaybins + 0.5);
        cum[j] = pymod((long long)cum[j] + (long long)nw, L);
        sdb[j] = sdb[j] + nw;
      }
      lds_sync();
      for (int b = lane; b < L; b += 64) {
        double s = 0.0;
        for (int j = 0; j < NS; ++j) {
          int src = b + cum[j];
          if (src >= L) src -= L;
          const double v = T[(size_t)j * L + src];
          s = (j == 0) ? v : s + v;
        }
        const double d = s - avgprof;
        tmp[b] = (d * d) / varprof;
      }
      lds_sync();
      const double chi = np_pairwise<12>(tmp, L, lane) / ((double)L - 1.0);
      lds_sync();
      if (lane == 0) chs[k] = (float)chi;
      if (a.chis && lane == 0) a.chis[c * PFE_PFD_NDM + k] = (float)chi;
    }
    lds_sync();
  }
  pfd_finish<false>(a, c, T, buf, tmp, dl, sdb, bv, chs, ftmp, po, dm_ok, lane);
}

// The 100-DM chi^2 sweep of k_pfd_dmprof4 for L = 64 / 128 and nsub a multiple of 8 (the
// PRESTO fold shapes): the same additions in the same order as the general loop below, with
// less issue per LDS read.  A trial DM's rotation of sub-band j is wave-uniform, so lanes
// 0-15 read the rotations of two DMs for 8 sub-bands at once and readlane makes them scalar;
// the wrap (b + r) mod L is a mask; and each wave sweeps two DMs at a time (k, k + 4), four
// independent ordered chains per lane.  numpy's pairwise leaf of the two chi^2 rows runs in
// lanes 0-7 (DM k) and 8-15 (DM k + 4) together.
template <int L>
__device__ __forceinline__ void sweep_pow2(const double* T, const uint16_t* rot, int NS, int wv,
                                           int lane, double avgprof, double varprof,
                                           double* xb, float* chs, float* chis) {
  constexpr int B = L / 64;  // bins per lane
  static_assert(B == 1 || B == 2, "L = 64 or 128");
  for (int k0 = wv; k0 < PFE_PFD_NDM; k0 += 8) {
    const bool two = k0 + 4 < PFE_PFD_NDM;  // wave-uniform
    const int k1 = two ? k0 + 4 : k0;
    const uint16_t* ra = rot + k0 * NS;
    const uint16_t* rb = rot + k1 * NS;
    double s[2][B];
    for (int j0 = 0; j0 < NS; j0 += 8) {
      const int rv = lane < 8 ? (int)ra[j0 + lane] : lane < 16 ? (int)rb[j0 + lane - 8] : 0;
      // two halves of 4 sub-bands (the same adds in the same order as one step of 8; half
      // the registers for the row reads in flight)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double v[2][4][B];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r0 = __builtin_amdgcn_readlane(rv, 4 * h + u);
          const int r1 = __builtin_amdgcn_readlane(rv, 8 + 4 * h + u);
          const double* row = T + (size_t)(j0 + 4 * h + u) * L;
#pragma unroll
          for (int q = 0; q < B; ++q) {
            const int b = lane + 64 * q;
            v[0][u][q] = row[(b + r0) & (L - 1)];
            v[1][u][q] = row[(b + r1) & (L - 1)];
          }
        }
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int q = 0; q < B; ++q) {
            double t = (j0 == 0 && h == 0) ? v[d][0][q] : s[d][q] + v[d][0][q];
#pragma unroll
            for (int u = 1; u < 4; ++u) t = t + v[d][u][q];
            s[d][q] = t;
          }
      }
    }
    // chi^2 terms of both DMs, then numpy's leaf: r_i = x[i] + x[i+8] + ... (L multiple of 8)
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int q = 0; q < B; ++q) {
        const double e = s[d][q] - avgprof;
        xb[d * 128 + lane + 64 * q] = (e * e) / varprof;
      }
    lds_sync();
    const double* xr = xb + ((lane >> 3) & 1) * 128;
    double w[L / 8];
#pragma unroll
    for (int m = 0; m < L / 8; ++m) w[m] = xr[(lane & 7) + 8 * m];
    double r = w[0];
#pragma unroll
    for (int m = 1; m < L / 8; ++m) r += w[m];
    const double den = (double)L - 1.0;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int o = 8 * d;
      const double r0 = bcast(r, o), r1 = bcast(r, o + 1), r2 = bcast(r, o + 2), r3 = bcast(r, o + 3);
      const double r4 = bcast(r, o + 4), r5 = bcast(r, o + 5), r6 = bcast(r, o + 6), r7 = bcast(r, o + 7);
      const double chi = (((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))) / den;
      const int k = d ? k1 : k0;
      if (lane == 0 && (d == 0 || two)) {
        chs[k] = (float)chi;
        if (chis) chis[k] = (float)chi;
      }
    }
    lds_sync();
  }
}

// Four-wave form of k_pfd_dmprof for profiles of <= 128 bins (the same arithmetic, bit for
// bit).  The single-wave kernel streamed the fold with one dependent load per lane at a time
// and swept the 100 trial DMs one after another; here
//   * all 256 threads reduce the fold over its parts, 8 elements x 2 parts of loads in
//     flight per thread (each element still sums its parts in order, as numpy);
//   * wave 3 tabulates the accumulated sub-band rotations of all 100 trial DMs while its
//     first loads are in flight;
//   * the sweep runs 4 trial DMs at a time, one per wave: the lanes sum the rotated sub-band
//     rows bin by bin (64 consecutive doubles of a row per read, so the LDS reads are
//     conflict-free) and numpy's pairwise leaf sums the chi^2 terms;
//   * wave 0 builds the profile and finishes the fold (statistics, 22-score parameters) as
//     the single-wave kernel.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_pfd_dmprof4(PfdArgs a) {
  extern __shared__ double lds[];
  const int64_t c = blockIdx.x;
  if (c >= a.n) return;
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int lane = lane_id();
  const int NP = a.npart, NS = a.nsub, L = a.L;
  double* T = lds;                   // NS x L
  double* buf = T + (size_t)NS * L;  // L
  double* tmp = buf + L;             // L
  double* dl = tmp + L;              // NS
  double* sdb = dl + NS;             // NS
  double* bv = sdb + NS;             // NS
  int* cum = (int*)(bv + NS);        // NS
  uint16_t* rot = (uint16_t*)(cum + NS);  // PFE_PFD_NDM x NS accumulated rotations (< L)
  double* xbuf = bv + NS + (4 * NS + 2 * PFE_PFD_NDM * NS + 7) / 8;  // 4 x 256, after cum, rot
  __shared__ float chs[PFE_PFD_NDM], ftmp[PFE_PFD_NDM];
  const double* sc = a.scal + c * PFE_PFD_NSCAL;
  const double bestdm = sc[PFE_PFD_BESTDM], bps = sc[PFE_PFD_BINSPERSEC];
  const double avgprof = sc[PFE_PFD_AVGPROF], varprof = sc[PFE_PFD_VARPROF];
  const double dm_lo = sc[PFE_PFD_DM_LO], dm_hi = sc[PFE_PFD_DM_HI];
  const double numdms = sc[PFE_PFD_NUMDMS];
  const double* fr = a.subfreqs + c * NS;
  const double* P = a.profs + c * (int64_t)NP * NS * L;
  const bool dm_ok = numdms > 1.0;  // numdms == 1: dms is a scalar and dms[0] raises
  const bool sweep = dm_ok && (a.chis || a.lyon8);
  // ---- dedisperse at the best DM (PFDFile.py:346-373, interp = 0)
  if (wv == 0) {
    for (int j = lane; j < NS; j += 64) dl[j] = delay_from_dm(bestdm, fr[j]);
    lds_sync();
    const double hif = dl[NS - 1];
    for (int j = lane; j < NS; j += 64) {
      const double delaybins = (dl[j] - hif) * bps - 0.0;
      const double nw = floor(delaybins + 0.5);
      sdb[j] = 0.0 + nw;
      cum[j] = pymod((long long)nw, L);
    }
  }
  __syncthreads();
  // T[j][b] = sum over parts of the rotated sub-integration profiles (profs.sum(0)): each
  // thread keeps PFD4_E elements and walks the parts, so PFD4_E loads are in flight per
  // thread and step; wave 3 first tabulates the sweep's rotations (below), overlapping them
  // with its first loads.  Split pipeline: T comes from k_pfd_parts (the same sums).
  if (a.tin) {
    const int total = NS * L;
    const double* tg = a.tin + c * (int64_t)total;
    if (wv == 3 && sweep) sweep_rotations(rot, sdb, fr, NS, L, bps, dm_lo, dm_hi, lane);
    for (int e = tid; e < total; e += 256) T[e] = tg[e];
  } else {
    const int total = NS * L;
    const int64_t pstride = (int64_t)NS * L;
    for (int e0 = tid; e0 < total; e0 += 256 * PFD4_E) {
      int src[PFD4_E];
      bool ok[PFD4_E];
      double acc[PFD4_E];
#pragma unroll
      for (int u = 0; u < PFD4_E; ++u) {
        const int e = e0 + 256 * u;
        ok[u] = e < total;
        const int j = ok[u] ? e / L : 0;
        const int b = ok[u] ? e - j * L : 0;
        const int r = cum[j];
        src[u] = j * L + (b + r < L ? b + r : b + r - L);
        acc[u] = ok[u] ? P[src[u]] : 0.0;
      }
      if (wv == 3 && sweep && e0 == tid) sweep_rotations(rot, sdb, fr, NS, L, bps, dm_lo, dm_hi, lane);
#pragma unroll 2
      for (int p = 1; p < NP; ++p) {
        double v[PFD4_E];
#pragma unroll
        for (int u = 0; u < PFD4_E; ++u) v[u] = ok[u] ? P[p * pstride + src[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < PFD4_E; ++u) acc[u] += v[u];
      }
#pragma unroll
      for (int u = 0; u < PFD4_E; ++u)
        if (ok[u]) T[e0 + 256 * u] = acc[u];
    }
    if (wv == 3 && sweep && tid >= total) sweep_rotations(rot, sdb, fr, NS, L, bps, dm_lo, dm_hi, lane);
  }
  __syncthreads();
  // ---- chi^2 versus DM over span(dms[0], dms[-1], 100) (PFDFile.py:378-423): each wave
  // takes every 4th trial DM; its lanes sum the rotated sub-band rows over the bins (a wave
  // reads 64 consecutive doubles of a row at a time), the chi^2 terms go to the wave's LDS
  // row and numpy's pairwise leaf sums them (np_leaf, lanes 0-7)
#if defined(PFE_PFD_PROBE) && PFE_PFD_PROBE == 1  // instrumented build: no sweep
  if (sweep) {
  } else if (false) {
#else
  if (sweep && (L == 128 || L == 64) && NS % 8 == 0) {
#endif
    double* xb = xbuf + wv * 256;
    float* chis = a.chis ? a.chis + c * PFE_PFD_NDM : nullptr;
    if (L == 128)
      sweep_pow2<128>(T, rot, NS, wv, lane, avgprof, varprof, xb, chs, chis);
    else
      sweep_pow2<64>(T, rot, NS, wv, lane, avgprof, varprof, xb, chs, chis);
  } else if (sweep) {
    double* xb = xbuf + wv * 256;
    const int b0 = lane, b1 = lane + 64;
    for (int k = wv; k < PFE_PFD_NDM; k += 4) {
      const uint16_t* rk = rot + k * NS;
      // 8 sub-bands per step: their rotations, then all 16 row reads, then the ordered adds
      // (unconditional reads at clamped indices keep every load of a step in flight)
      double s0 = 0.0, s1 = 0.0;
      const int b0c = b0 < L ? b0 : 0, b1c = b1 < L ? b1 : 0;
      for (int j0 = 0; j0 < NS; j0 += 8) {
        int r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = rk[min(j0 + u, NS - 1)];
        double v0[8], v1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const double* row = T + (size_t)min(j0 + u, NS - 1) * L;
          int i0 = b0c + r[u];
          if (i0 >= L) i0 -= L;
          int i1 = b1c + r[u];
          if (i1 >= L) i1 -= L;
          v0[u] = row[i0];
          v1[u] = row[i1];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (j0 + u < NS) {
            s0 = (j0 + u == 0) ? v0[u] : s0 + v0[u];
            s1 = (j0 + u == 0) ? v1[u] : s1 + v1[u];
          }
      }
      if (b0 < L) {
        const double d = s0 - avgprof;
        xb[b0] = (d * d) / varprof;
      }
      if (b1 < L) {
        const double d = s1 - avgprof;
        xb[b1] = (d * d) / varprof;
      }
      lds_sync();
      const double chi = (L >= 8 ? np_leaf128(xb, L, lane) : np_leaf(xb, L, lane)) / ((double)L - 1.0);
      if (lane == 0) {
        chs[k] = (float)chi;
        if (a.chis) a.chis[c * PFE_PFD_NDM + k] = (float)chi;
      }
      lds_sync();
    }
  }
  __syncthreads();
#if defined(PFE_PFD_PROBE) && PFE_PFD_PROBE == 2  // instrumented build: no wave-0 tail
  return;
#endif
  if (wv != 0) return;
  // (the profile is built after the sweep: it does not feed it, and the wave-0-only calls it
  // makes kept out of the divergent part before the sweep)
  double po[4] = {0.0, 0.0, 0.0, 0.0};
  {
    // sumprof = T.sum(0); the profile (getprofile + scale)
    for (int b = lane; b < L; b += 64) {
      double s = T[b];
      for (int j = 1; j < NS; ++j) s += T[(size_t)j * L + b];
      buf[b] = s;
    }
    lds_sync();
    const double mn = py_ext_wave<false>(buf, L, lane);
    for (int b = lane; b < L; b += 64) buf[b] = buf[b] - mn;  // normprof
    lds_sync();
    const double mean = np_sum_row<true>(buf, L, lane) / (double)L;
    lds_sync();
    for (int b = lane; b < L; b += 64) buf[b] = buf[b] / mean;  // s
    lds_sync();
    const double smin = py_ext_wave<false>(buf, L, lane), smax = py_ext_wave<true>(buf, L, lane);
    lds_sync();
    for (int b = lane; b < L; b += 64) {
      const double t = (buf[b] - smin) / (smax - smin);
      buf[b] = (0.0 * (1.0 - t)) + (255.0 * t);
      if (a.profile) a.profile[c * L + b] = buf[b];
    }
    lds_sync();
    if (a.lyon8) stats4_f64<true>(buf, tmp, L, lane, po);
  }
  pfd_finish<true>(a, c, T, buf, tmp, dl, sdb, bv, chs, ftmp, po, dm_ok, lane);
}

// Split pipeline, stage 1: the fold's part sums T (as k_pfd_dmprof4 reduces them: the
// dedispersion rotations of wave 0, then each element summing its parts in order) streamed
// to global memory.  Little LDS and no sweep state, so many blocks per CU keep enough loads
// in flight to stream the folds at HBM rate while k_pfd_dmprof4 sweeps the previous chunk.
__global__ __launch_bounds__(256) void k_pfd_parts(PfdArgs a, double* __restrict__ tout) {
  extern __shared__ double lds[];
  const int64_t c = blockIdx.x;
  if (c >= a.n) return;
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int NP = a.npart, NS = a.nsub, L = a.L;
  double* dl = lds;               // NS
  int* cum = (int*)(dl + NS);     // NS
  const double* sc = a.scal + c * PFE_PFD_NSCAL;
  const double bestdm = sc[PFE_PFD_BESTDM], bps = sc[PFE_PFD_BINSPERSEC];
  const double* fr = a.subfreqs + c * NS;
  const double* P = a.profs + c * (int64_t)NP * NS * L;
  if ((tid >> 6) == 0) {  // PFDFile.py:346-373 (interp = 0), as k_pfd_dmprof4's wave 0
    for (int j = lane; j < NS; j += 64) dl[j] = delay_from_dm(bestdm, fr[j]);
    lds_sync();
    const double hif = dl[NS - 1];
    for (int j = lane; j < NS; j += 64) {
      const double delaybins = (dl[j] - hif) * bps - 0.0;
      const double nw = floor(delaybins + 0.5);
      cum[j] = pymod((long long)nw, L);
    }
  }
  __syncthreads();
  const int total = NS * L;
  const int64_t pstride = (int64_t)NS * L;
  double* tg = tout + c * (int64_t)total;
  for (int e0 = tid; e0 < total; e0 += 256 * PFD4_E) {
    int src[PFD4_E];
    bool ok[PFD4_E];
    double acc[PFD4_E];
#pragma unroll
    for (int u = 0; u < PFD4_E; ++u) {
      const int e = e0 + 256 * u;
      ok[u] = e < total;
      const int j = ok[u] ? e / L : 0;
      const int b = ok[u] ? e - j * L : 0;
      const int r = cum[j];
      src[u] = j * L + (b + r < L ? b + r : b + r - L);
      acc[u] = ok[u] ? __builtin_nontemporal_load(P + src[u]) : 0.0;
    }
#pragma unroll 2
    for (int p = 1; p < NP; ++p) {
      double v[PFD4_E];
#pragma unroll
      for (int u = 0; u < PFD4_E; ++u)
        v[u] = ok[u] ? __builtin_nontemporal_load(P + p * pstride + src[u]) : 0.0;
#pragma unroll
      for (int u = 0; u < PFD4_E; ++u) acc[u] += v[u];
    }
#pragma unroll
    for (int u = 0; u < PFD4_E; ++u)
      if (ok[u]) tg[e0 + 256 * u] = acc[u];
  }
}

size_t pfd_lds_bytes(int nsub, int L) {
  return ((size_t)nsub * L + 2 * (size_t)L + 3 * (size_t)nsub) * sizeof(double) +
         (size_t)nsub * sizeof(int) + 64;
}

static size_t pfd4_lds_bytes(int nsub, int L) {
  return pfd_lds_bytes(nsub, L) + (size_t)PFE_PFD_NDM * nsub * sizeof(uint16_t) + 8 +
         4 * 256 * sizeof(double);
}

// the four-wave kernel: <= 128 bins, the fold in LDS, and rows of <= 968 values (its
// pairwise sums are inlined three levels deep, np_sum_row<true>)
static bool pfd4_ok(const PfdArgs& a) {
  // nsub: the sub-band sums go through np_pairwise_inl<3>, numpy's order up to np_inl_max(3)
  return a.L <= 128 && a.nsub <= np_inl_max(3) && pfd4_lds_bytes(a.nsub, a.L) <= 64 * 1024 &&
         a.waves == 4;
}

bool pfd_split_ok(const PfdArgs& a) {
  return pfd4_ok(a);
}

// the folds [c0, c0 + cn) of a batch: every per-fold pointer moved to fold c0
static PfdArgs pfd_chunk(const PfdArgs& a, int64_t c0, int64_t cn) {
  PfdArgs b = a;
  b.n = cn;
  b.profs = a.profs + c0 * (int64_t)a.npart * a.nsub * a.L;
  b.subfreqs = a.subfreqs + c0 * a.nsub;
  b.scal = a.scal + c0 * PFE_PFD_NSCAL;
  if (a.profile) b.profile = a.profile + c0 * a.L;
  if (a.chis) b.chis = a.chis + c0 * PFE_PFD_NDM;
  if (a.lyon8) b.lyon8 = a.lyon8 + c0 * 8;
  if (a.status) b.status = a.status + c0;
  if (a.out22) b.out22 = a.out22 + c0 * 22;
  if (a.par22) b.par22 = a.par22 + c0 * 8;
  return b;
}

hipError_t launch_pfd_dmprof_split(const PfdArgs& a, hipStream_t st, hipStream_t side, double* ws,
                                   int64_t chunk, hipEvent_t (&ev)[4]) {
  const size_t lds4 = pfd4_lds_bytes(a.nsub, a.L);
  hipError_t e = ensure_dyn_lds<k_pfd_dmprof4>(lds4);
  if (e != hipSuccess) return e;
  const size_t ldsp = (size_t)a.nsub * (sizeof(double) + sizeof(int)) + 16;
  const int64_t per = (int64_t)a.nsub * a.L;
  // side waits for everything queued on st before the call (the inputs may come from it)
  if ((e = hipEventRecord(ev[2], st)) != hipSuccess) return e;
  if ((e = hipStreamWaitEvent(side, ev[2], 0)) != hipSuccess) return e;
  int k = 0;
  for (int64_t c0 = 0; c0 < a.n; c0 += chunk, ++k) {
    const int64_t cn = a.n - c0 < chunk ? a.n - c0 : chunk;
    const int buf = k & 1;
    double* t = ws + (size_t)buf * chunk * per;
    const PfdArgs b = pfd_chunk(a, c0, cn);
    // buffer reuse: chunk k - 2's sweep (on st) has read this half
    if (k >= 2 && (e = hipStreamWaitEvent(side, ev[2 + buf], 0)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_pfd_parts, dim3((unsigned)cn), dim3(256), ldsp, side, b, t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipEventRecord(ev[buf], side)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(st, ev[buf], 0)) != hipSuccess) return e;
    PfdArgs d = b;
    d.tin = t;
    hipLaunchKernelGGL(k_pfd_dmprof4, dim3((unsigned)cn), dim3(256), lds4, st, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipEventRecord(ev[2 + buf], st)) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_pfd_dmprof(const PfdArgs& a, hipStream_t st) {
  if (a.tg) return launch_pfd_dmprof_g(a, st);  // the caller planned slabs (pfd_global_plan)
  if (pfd4_ok(a)) {
    const size_t lds4 = pfd4_lds_bytes(a.nsub, a.L);
    hipError_t e = ensure_dyn_lds<k_pfd_dmprof4>(lds4);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pfd_dmprof4, dim3((unsigned)a.n), dim3(256), lds4, st, a);
    return hipGetLastError();
  }
  const size_t lds = pfd_lds_bytes(a.nsub, a.L);
  hipError_t e = ensure_dyn_lds<k_pfd_dmprof>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pfd_dmprof, dim3((unsigned)a.n), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace pfe
