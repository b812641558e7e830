// pfd_global.hip — PFD preprocessing for folds of any nsub x proflen on gfx950: the kernel of
// pfd.hip with the fold's sub-band profiles in global scratch instead of LDS.
#include "pfd_dev.h"

namespace pfe {

#pragma clang fp contract(off)

// ---- the fold in global memory: any nsub x proflen ----------------------------------------
// hand-over of slab contents between the waves of a block: every wave's own global stores
// (and loads) retired, then the workgroup barrier with its release / acquire fences.
// lds_sync() orders one wave's accesses only.
__device__ __forceinline__ void slab_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// one wave's share of the 100-DM sweep of k_pfd_dmprof_g (every 4th trial DM): B bins per
// lane and pass, 4 sub-bands of row reads in flight, each bin summing the rotated sub-band
// rows in band order (the slab reads hit L2; a trial DM's rotation is wave-uniform); the
// chi^2 terms go to the wave's LDS row and numpy's pairwise sum adds them
template <int B>
__device__ __forceinline__ void sweep_slab(const double* T, const uint16_t* rot, int NS, int L, int wv,
                                           int lane, double avgprof, double varprof, double* xb,
                                           float* chs, float* chis) {
  for (int k = wv; k < PFE_PFD_NDM; k += 4) {
    const uint16_t* rk = rot + k * NS;
    for (int b0 = 0; b0 < L; b0 += 64 * B) {
      int bc[B];
      double s[B];
#pragma unroll
      for (int q = 0; q < B; ++q) {
        const int b = b0 + lane + 64 * q;
        bc[q] = b < L ? b : 0;  // unconditional reads at a clamped bin
        s[q] = 0.0;
      }
      for (int j0 = 0; j0 < NS; j0 += 4) {
        double v[4][B];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = min(j0 + u, NS - 1);
          const int r = rk[j];
          const double* row = T + (size_t)j * L;
#pragma unroll
          for (int q = 0; q < B; ++q) {
            int i = bc[q] + r;
            if (i >= L) i -= L;
            v[u][q] = row[i];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j0 + u < NS) {
#pragma unroll
            for (int q = 0; q < B; ++q) s[q] = (j0 + u == 0) ? v[u][q] : s[q] + v[u][q];
          }
      }
#pragma unroll
      for (int q = 0; q < B; ++q) {
        const int b = b0 + lane + 64 * q;
        if (b < L) {
          const double d = s[q] - avgprof;
          xb[b] = (d * d) / varprof;
        }
      }
    }
    lds_sync();
    const double chi =
        ((L >= 8 && L <= 128) ? np_leaf128(xb, L, lane) : np_pairwise<12>(xb, L, lane)) / ((double)L - 1.0);
    if (lane == 0) {
      chs[k] = (float)chi;
      if (chis) chis[k] = (float)chi;
    }
    lds_sync();
  }
}

// k_pfd_dmprof for folds of any nsub x proflen (the same arithmetic, bit for bit): the
// sub-band profiles T live in a slab of global scratch that the block owns, not in LDS.
// Persistent 256-thread blocks loop over the folds c = blockIdx.x, += gridDim.x:
//   * all 256 threads reduce the fold over its parts into the slab (each element sums its
//     parts in order, as numpy; coalesced reads) and tabulate the accumulated rotations of
//     the 100 trial DMs, one thread per sub-band (ROT_LDS: the table in LDS, else behind T);
//   * the sweep runs 4 trial DMs at a time, one per wave (sweep_slab);
//   * wave 0 scales the profile and finishes the fold as the single-wave kernel; the
//     sub-band scores overwrite T in place, in the block's own slab.
// slab_sync() hands the slab over: part sums -> sweep, sweep -> wave-0 tail, and wave 0's
// tail of fold c -> the part sums of fold c + gridDim.x (the barrier after wave 0's
// dedispersion of the next fold).
// Two waves per SIMD (256 VGPRs, two blocks per CU): left to itself the kernel is allocated
// 412 VGPRs -- one block per CU, 4 waves' loads in flight -- and streams the folds 20-24 %
// slower, the 146 VGPRs spilled at 256 notwithstanding (profiles/pfd_global_waves_ab.txt).
template <bool ROT_LDS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_pfd_dmprof_g(PfdArgs a) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int lane = lane_id();
  const int NP = a.npart, NS = a.nsub, L = a.L;
  double* T = (double*)((char*)a.tg + (size_t)blockIdx.x * a.gstride);  // NS x L, this block's
  double* buf = lds;              // L
  double* tmp = buf + L;          // L
  double* xbuf = tmp + L;         // 4 x L: the waves' chi^2 rows
  double* dl = xbuf + 4 * (size_t)L;  // NS
  double* sdb = dl + NS;          // NS
  double* bv = sdb + NS;          // NS
  int* cum = (int*)(bv + NS);     // NS
  uint16_t* rot = ROT_LDS ? (uint16_t*)(cum + NS + (NS & 1)) : (uint16_t*)(T + (size_t)NS * L);
  __shared__ float chs[PFE_PFD_NDM], ftmp[PFE_PFD_NDM];
  const int total = NS * L;
  const int64_t pstride = (int64_t)NS * L;
  for (int64_t c = blockIdx.x; c < a.n; c += gridDim.x) {
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
    slab_sync();  // wave 0 has also finished the previous fold: the slab is free
    // T[j][b] = sum over parts of the rotated sub-integration profiles (profs.sum(0)), as
    // k_pfd_dmprof4 reduces them
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
    if (sweep) sweep_rotations(rot, sdb, fr, NS, L, bps, dm_lo, dm_hi, tid, 256);
    slab_sync();  // part sums (and the rotation table) -> every wave
    // sumprof = T.sum(0), the bins over all 256 threads
    for (int b = tid; b < L; b += 256) {
      double s = T[b];
#pragma unroll 8
      for (int j = 1; j < NS; ++j) s += T[(size_t)j * L + b];
      buf[b] = s;
    }
    // ---- chi^2 versus DM over span(dms[0], dms[-1], 100) (PFDFile.py:378-423)
    if (sweep) {
      double* xb = xbuf + (size_t)wv * L;
      float* chis = a.chis ? a.chis + c * PFE_PFD_NDM : nullptr;
      if (L <= 64)
        sweep_slab<1>(T, rot, NS, L, wv, lane, avgprof, varprof, xb, chs, chis);
      else if (L <= 128)
        sweep_slab<2>(T, rot, NS, L, wv, lane, avgprof, varprof, xb, chs, chis);
      else
        sweep_slab<4>(T, rot, NS, L, wv, lane, avgprof, varprof, xb, chs, chis);
    }
    slab_sync();  // sweep (its slab reads, chs, buf) -> wave 0's tail
    if (wv == 0) {
      double po[4] = {0.0, 0.0, 0.0, 0.0};
      // the profile (getprofile + scale)
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
      if (a.lyon8) stats4_f64<false>(buf, tmp, L, lane, po);
      pfd_finish<false>(a, c, T, buf, tmp, dl, sdb, bv, chs, ftmp, po, dm_ok, lane);
    }
  }
}

static size_t pfd_g_lds_bytes(int nsub, int L, bool rot_lds) {
  return (6 * (size_t)L + 3 * (size_t)nsub) * sizeof(double) +
         ((size_t)nsub + (nsub & 1)) * sizeof(int) +
         (rot_lds ? (size_t)PFE_PFD_NDM * nsub * sizeof(uint16_t) : 0) + 64;  // dynamic
}
// with the kernel's static chs / ftmp
static size_t pfd_g_lds_total(int nsub, int L, bool rot_lds) {
  return pfd_g_lds_bytes(nsub, L, rot_lds) + 2 * PFE_PFD_NDM * sizeof(float) + 224;
}

static int pfd_device_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      cus = v;
    else
      (void)hipGetLastError();
  }
  return cus;
}

PfdGlobalPlan pfd_global_plan(int nsub, int L, int64_t n) {
  PfdGlobalPlan p;
  // the rotation table on chip while two blocks still fit a CU, else behind the fold
  p.rot_lds = pfd_g_lds_total(nsub, L, true) <= PFD_LDS_LIMIT / 2;
  p.lds = pfd_g_lds_bytes(nsub, L, p.rot_lds);
  p.ok = L <= PFD_G_MAX_L && pfd_g_lds_total(nsub, L, p.rot_lds) <= PFD_LDS_LIMIT;
  if (!p.ok) return p;
  const size_t fold = (size_t)nsub * L * sizeof(double);
  const size_t rot = p.rot_lds ? 0 : (size_t)PFE_PFD_NDM * nsub * sizeof(uint16_t);
  p.stride = (fold + rot + 255) & ~(size_t)255;
  int64_t blocks = 2 * (int64_t)pfd_device_cus();
  const int64_t budget = (int64_t)(((size_t)1 << 30) / p.stride);
  if (blocks > budget) blocks = budget;
  if (blocks > n) blocks = n;
  if (blocks < 1) blocks = 1;
  p.blocks = (int)blocks;
  return p;
}

// a.tg: a.gblocks slabs of a.gstride bytes, as pfd_global_plan(a.nsub, a.L, a.n) sized them
hipError_t launch_pfd_dmprof_g(const PfdArgs& a, hipStream_t st) {
  const PfdGlobalPlan p = pfd_global_plan(a.nsub, a.L, a.n);
  if (!p.ok || !a.tg || a.tin || a.gblocks < 1 || a.gblocks > p.blocks || a.gstride != p.stride)
    return hipErrorInvalidValue;
  hipError_t e = p.rot_lds ? ensure_dyn_lds<k_pfd_dmprof_g<true>>(p.lds)
                           : ensure_dyn_lds<k_pfd_dmprof_g<false>>(p.lds);
  if (e != hipSuccess) return e;
  if (p.rot_lds)
    hipLaunchKernelGGL(k_pfd_dmprof_g<true>, dim3((unsigned)a.gblocks), dim3(256), p.lds, st, a);
  else
    hipLaunchKernelGGL(k_pfd_dmprof_g<false>, dim3((unsigned)a.gblocks), dim3(256), p.lds, st, a);
  return hipGetLastError();
}

}  // namespace pfe
