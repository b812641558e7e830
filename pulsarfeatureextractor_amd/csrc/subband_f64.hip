// subband_f64.hip — scores 20-22 of candidates held as float arrays (pfe_subband3_f64), and
// the float 22-score call composed from the five groups (pfe_bates22_f64).
//
// Reference: PHCXOperations.getSubbandParameters (PHCXOperations.py:305-349) on float
// sub-bands -- ProfileOperations.getSubband_scores (ProfileOperations.py:1585-1686) and
// getProfileCorr (PHCXOperations.py:387-415).  The arithmetic is pfd_subband_scores
// (pfd_dev.h), the device function the fold kernels run on a fold's own dedispersed
// sub-bands; this kernel runs it on caller-supplied arrays.
//
// One wave scores one candidate; waves are persistent and loop over the candidates.
// pfd_subband_scores overwrites T (boxcar sums in place), so a wave works on its own copy of
// the candidate's nsub x lsb doubles and the caller's array is only read:
//   * on chip: the copy in the wave's partition of the block's LDS, with the per-candidate
//     vectors behind it; a block holds as many waves as the 160 KiB admit (8 at 16 x 128,
//     4 at 32 x 128);
//   * global: the copy in the wave's slab of the handle's scratch (every shape whose copy does
//     not fit, and every shape under PFE_OPT_SUBF64_GLOBAL), only the vectors on chip.  The
//     wave alone reads and writes its slab, so its own program order is all it needs, as for
//     the tail of k_pfd_dmprof_g.
// The same device function, the same order of operations: the two paths give the same bits.
#include "launch.h"
#include "pfd_dev.h"

namespace pfe {

#pragma clang fp contract(off)

struct SubF64Args {
  const double* prof;  // n x lp
  int lp;
  const double* sub;   // n x nsub x lsb
  int nsub, lsb;
  const double* scal;  // n x PFE_NSCAL (width at PFE_SCAL_WIDTH)
  int64_t n;
  double* out;         // scores 20-22 of candidate c at out[c * ldo + 0..2]
  int ldo;
  uint32_t* status;
  int chain;           // 1: OR the failure bit, leave a failed row's scores alone
  unsigned char* slabs;  // global path: one slab per wave
  size_t slab;           // bytes per slab
  unsigned wave_lds;     // LDS bytes per wave
  unsigned t_lds;        // of which T (on chip)
};

typedef double f64x2 __attribute__((ext_vector_type(2)));

// total doubles src -> dst (LDS or the wave's slab), 16 bytes per lane and load, four loads
// in flight; src is 8-byte aligned, so an odd first or last double goes alone
__device__ __forceinline__ void copy_doubles(double* dst, const double* src, int total, int lane) {
  const int head = (int)(((uintptr_t)src >> 3) & 1);  // wave-uniform
  if (head && lane == 0) dst[0] = src[0];
  const int pairs = (total - head) >> 1;
  if (pairs > 0) {
    const f64x2* s2 = reinterpret_cast<const f64x2*>(src + head);
    double* d = dst + head;
    for (int p0 = 0; p0 < pairs; p0 += 256) {
      f64x2 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = s2[min(p0 + 64 * u + lane, pairs - 1)];  // clamped, unconditional
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + 64 * u + lane;
        if (p < pairs) {
          d[2 * p] = v[u].x;
          d[2 * p + 1] = v[u].y;
        }
      }
    }
  }
  if (((total - head) & 1) && lane == 0) dst[total - 1] = src[total - 1];
}

// NC: every row sum inlined (rows of <= np_inl_max(3) values: lsb and nsub <= 968), as the
// four-wave fold kernel; else numpy's pairwise sum by calls, as k_pfd_dmprof_g.  GLOBAL: T in
// the wave's slab.
template <bool NC, bool GLOBAL>
__global__ __launch_bounds__(64 * SUBF64_MAX_WPB) void k_subband_f64(SubF64Args a) {
  extern __shared__ __align__(16) unsigned char sf_lds[];
  const int lane = lane_id();
  const int w = uni((int)(threadIdx.x >> 6));
  const int wpb = (int)(blockDim.x >> 6);
  const int NS = a.nsub, L = a.lsb;
  unsigned char* part = sf_lds + (size_t)w * a.wave_lds;
  double* T = GLOBAL ? reinterpret_cast<double*>(a.slabs + ((size_t)blockIdx.x * wpb + w) * a.slab)
                     : reinterpret_cast<double*>(part);
  double* prof = reinterpret_cast<double*>(part + (GLOBAL ? 0u : a.t_lds));  // L
  double* tmp = prof + L;                                                     // L
  double* mb = tmp + L;                                                       // NS
  double* bmean = mb + NS;                                                    // NS
  double* bvar = bmean + NS;                                                  // NS
  const int total = NS * L;
  for (int64_t c = (int64_t)blockIdx.x * wpb + w; c < a.n; c += (int64_t)gridDim.x * wpb) {
    const double width = a.scal[c * PFE_NSCAL + PFE_SCAL_WIDTH];
    const double wbd = ceil(width * (double)L);                          // :1603
    double o[3] = {0.0, 0.0, 0.0};
    // wb <= 0: rms = stdev / 0 or no valid pair; wb > lsb: no window, max_bin unbound; NaN or
    // infinite width: int() raises; lp != lsb: corrcoef of different lengths raises (:403)
    bool ok = wbd >= 1.0 && wbd <= (double)L && a.lp == L;
    if (ok) {
      lds_sync();  // the previous candidate's reads precede this one's stores
      const double* pr = a.prof + c * (int64_t)a.lp;
      for (int b = lane; b < L; b += 64) prof[b] = pr[b];
      copy_doubles(T, a.sub + c * (int64_t)total, total, lane);
      lds_sync();
      ok = pfd_subband_scores<NC>(T, prof, tmp, mb, bmean, bvar, NS, L, lane, width, o);
    }
    if (lane == 0) {
      if (a.chain) {
        if (!ok) atomicOr(&a.status[c], PFE_ST_SUBBAND_FAIL);
      } else {
        a.status[c] = ok ? 0u : PFE_ST_SUBBAND_FAIL;
      }
      if (ok || !a.chain) {
        double* q = a.out + c * (int64_t)a.ldo;
        q[0] = ok ? o[0] : 0.0;
        q[1] = ok ? o[1] : 0.0;
        q[2] = ok ? o[2] : 0.0;
      }
    }
  }
}

template <bool NC, bool GLOBAL>
static hipError_t launch_k(const SubF64Args& a, const SubF64Plan& p, hipStream_t st) {
  const size_t lds = p.wave_lds * (size_t)p.wpb;
  hipError_t e = ensure_dyn_lds<k_subband_f64<NC, GLOBAL>>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_subband_f64<NC, GLOBAL>), dim3((unsigned)p.blocks), dim3(64u * p.wpb), lds,
                     st, a);
  return hipGetLastError();
}

hipError_t launch_subband_f64(const pfe_bates_f64_in* in, double* out, int ldo, uint32_t* status,
                              bool chain, const SubF64Plan& p, void* slabs, hipStream_t st) {
  if (in->n <= 0) return hipSuccess;
  // the plan is the caller's (it sized the slabs): check it against the shape before a launch
  if (!p.ok || p.wpb < 1 || p.wpb > SUBF64_MAX_WPB || p.blocks < 1 ||
      p.wave_lds * (size_t)p.wpb > SUBF64_LDS_LIMIT ||
      p.wave_lds != p.t_lds + subf64_vec_bytes(in->nsub, in->lsb) ||
      (p.global ? (!slabs || p.t_lds != 0 || p.slab < (size_t)in->nsub * in->lsb * sizeof(double))
                : p.t_lds < (size_t)in->nsub * in->lsb * sizeof(double)))
    return hipErrorInvalidValue;
  SubF64Args a{in->prof, in->lp, in->sub, in->nsub, in->lsb, in->scal, in->n, out, ldo, status,
               chain ? 1 : 0, (unsigned char*)slabs, p.slab, (unsigned)p.wave_lds,
               (unsigned)p.t_lds};
  if (p.global) return launch_k<false, true>(a, p, st);
  if (in->lsb <= np_inl_max(3) && in->nsub <= np_inl_max(3)) return launch_k<true, false>(a, p, st);
  return launch_k<false, false>(a, p, st);
}

// The float 22-score call: the schedule of launch_bates_groups (bates22.hip) with the float-
// profile kernels (a.fprof) and the float sub-band kernel -- sine fits on the caller's stream,
// the Gaussian chain on one side stream, the DM fit and the sub-bands on the other.
hipError_t launch_bates22_f64(const pfe_bates_f64_in* in, double* out, uint32_t* status,
                              const BatesArgs& work, const SubF64Plan& p, void* slabs,
                              hipStream_t st, const Fork* fk, const Options& o) {
  BatesArgs a = work;
  bates_setup(a, in->n, in->lp, o);
  a.prof = nullptr;
  a.fprof = in->prof;
  a.sub = nullptr;
  a.nsub = 0;
  a.lsb = 0;
  a.dmcurve = in->dmcurve;
  a.ndm = in->ndm;
  a.scal = in->scal;
  a.out = out;
  a.status = status;
  hipError_t e = hipMemsetAsync(status, 0, (size_t)in->n * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(out, 0, (size_t)in->n * 22 * sizeof(double), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.counters, 0, BATES_NCOUNTERS * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  const bool forked = fork_begin(fk, st);
  const hipStream_t sg = forked ? fk->side[0] : st, sd = forked ? fk->side[1] : st;
  if (forked) {
    if ((e = launch_gauss(a, sg)) != hipSuccess) return e;
    if ((e = launch_dmfit(a, sd)) != hipSuccess) return e;
    if ((e = launch_subband_f64(in, out + 19, 22, status, true, p, slabs, sd)) != hipSuccess) return e;
    if ((e = launch_sine(a, st)) != hipSuccess) return e;
    if ((e = fork_end(fk, st)) != hipSuccess) return e;
  } else {
    if ((e = launch_sine(a, st)) != hipSuccess) return e;
    if ((e = launch_gauss(a, st)) != hipSuccess) return e;
    if ((e = launch_dmfit(a, st)) != hipSuccess) return e;
    if ((e = launch_subband_f64(in, out + 19, 22, status, true, p, slabs, st)) != hipSuccess) return e;
  }
  launch_clear_internal(status, in->n, st);
  return hipGetLastError();
}

}  // namespace pfe
