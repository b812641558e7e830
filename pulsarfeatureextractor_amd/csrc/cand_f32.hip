// cand_f32.hip — candidates held as float32 arrays: the sub-band scores (pfe_subband3_f32), the
// widening of the small per-candidate arrays the fits read (pfe_sinusoid4_f32, pfe_gauss7_f32)
// and the float32 22-score call composed from them (pfe_bates22_f32).
//
// Nothing is computed in float32.  The large array -- n x nsub x lsb sub-bands -- is read as
// the floats it is and widened in registers on its way into the copy k_subband_f64
// (subband_f64.hip) makes of a candidate anyway: the wave's LDS partition or scratch slab holds
// the same doubles as in the f64 call on the widened array, and pfd_subband_scores (pfd_dev.h)
// runs on them unchanged.  The profiles and DM curves, which the LM kernels read many times
// and in many places, get a widened copy in the handle's scratch (k_widen_f32) and those
// kernels run on the copy as they are.  (double)x is exact, so every value every kernel sees
// is the value the f64 call sees: the same bits out.
//
// k_subband_f32 restates k_subband_f64 with its two loads widened rather than sharing a
// template with it, so that subband_f64.hip compiles to the code object it always has.
#include "launch.h"
#include "pfd_dev.h"

namespace pfe {

#pragma clang fp contract(off)

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- profiles and DM curves: one widened copy ---------------------------------------------
__global__ __launch_bounds__(256) void k_widen_f32(const float* __restrict__ a,
                                                   double* __restrict__ da, int64_t na,
                                                   const float* __restrict__ b,
                                                   double* __restrict__ db, int64_t nb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < na)
    da[i] = (double)a[i];
  else if (i - na < nb)
    db[i - na] = (double)b[i - na];
}

hipError_t launch_widen_f32(const float* a, double* da, int64_t na, const float* b, double* db,
                            int64_t nb, hipStream_t st) {
  if (na + nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_widen_f32, dim3((unsigned)((na + nb + 255) / 256)), dim3(256), 0, st, a, da,
                     na, b, db, nb);
  return hipGetLastError();
}

// ---- sub-bands ------------------------------------------------------------------------------
struct SubF32Args {
  const float* prof;   // n x lp
  int lp;
  const float* sub;    // n x nsub x lsb
  int nsub, lsb;
  const double* scal;  // n x PFE_NSCAL (width at PFE_SCAL_WIDTH)
  int64_t n;
  double* out;         // scores 20-22 of candidate c at out[c * ldo + 0..2]
  int ldo;
  uint32_t* status;
  int chain;             // 1: OR the failure bit, leave a failed row's scores alone
  unsigned char* slabs;  // global path: one slab per wave
  size_t slab;           // bytes per slab
  unsigned wave_lds;     // LDS bytes per wave
  unsigned t_lds;        // of which T (on chip)
};

// total floats src -> total doubles dst (LDS or the wave's slab), 16 bytes per lane and load,
// four loads in flight; src is 4-byte aligned, so up to three floats in front of the first
// 16-byte boundary and up to three behind the last whole quad go singly (as copy_doubles of
// subband_f64.hip treats an odd double).  Every load lies within [src, src + total).
__device__ __forceinline__ void copy_widen(double* dst, const float* src, int total, int lane) {
  const int head = min(total, (int)((4u - (unsigned)(((uintptr_t)src >> 2) & 3u)) & 3u));  // wave-uniform
  if (lane < head) dst[lane] = (double)src[lane];
  const int quads = (total - head) >> 2;
  if (quads > 0) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src + head);
    double* d = dst + head;
    for (int q0 = 0; q0 < quads; q0 += 256) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = s4[min(q0 + 64 * u + lane, quads - 1)];  // clamped, unconditional
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = q0 + 64 * u + lane;
        if (q < quads) {
          d[4 * q] = (double)v[u].x;
          d[4 * q + 1] = (double)v[u].y;
          d[4 * q + 2] = (double)v[u].z;
          d[4 * q + 3] = (double)v[u].w;
        }
      }
    }
  }
  const int done = head + 4 * quads;
  if (lane < total - done) dst[done + lane] = (double)src[done + lane];
}

// k_subband_f64 (subband_f64.hip) on float32 arrays: the same partitions, the same slabs, the
// same device function on the same doubles.  NC / GLOBAL as there.
template <bool NC, bool GLOBAL>
__global__ __launch_bounds__(64 * SUBF64_MAX_WPB) void k_subband_f32(SubF32Args a) {
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
    const double wbd = ceil(width * (double)L);
    double o[3] = {0.0, 0.0, 0.0};
    bool ok = wbd >= 1.0 && wbd <= (double)L && a.lp == L;  // the rows k_subband_f64 fails
    if (ok) {
      lds_sync();  // the previous candidate's reads precede this one's stores
      const float* pr = a.prof + c * (int64_t)a.lp;
      for (int b = lane; b < L; b += 64) prof[b] = (double)pr[b];
      copy_widen(T, a.sub + c * (int64_t)total, total, lane);
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
static hipError_t launch_k(const SubF32Args& a, const SubF64Plan& p, hipStream_t st) {
  const size_t lds = p.wave_lds * (size_t)p.wpb;
  hipError_t e = ensure_dyn_lds<k_subband_f32<NC, GLOBAL>>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_subband_f32<NC, GLOBAL>), dim3((unsigned)p.blocks), dim3(64u * p.wpb), lds,
                     st, a);
  return hipGetLastError();
}

hipError_t launch_subband_f32(const pfe_bates_f32_in* in, double* out, int ldo, uint32_t* status,
                              bool chain, const SubF64Plan& p, void* slabs, hipStream_t st) {
  if (in->n <= 0) return hipSuccess;
  // the plan is the caller's (it sized the slabs): check it against the shape before a launch;
  // the copy is doubles, so the checks are launch_subband_f64's
  if (!p.ok || p.wpb < 1 || p.wpb > SUBF64_MAX_WPB || p.blocks < 1 ||
      p.wave_lds * (size_t)p.wpb > SUBF64_LDS_LIMIT ||
      p.wave_lds != p.t_lds + subf64_vec_bytes(in->nsub, in->lsb) ||
      (p.global ? (!slabs || p.t_lds != 0 || p.slab < (size_t)in->nsub * in->lsb * sizeof(double))
                : p.t_lds < (size_t)in->nsub * in->lsb * sizeof(double)))
    return hipErrorInvalidValue;
  SubF32Args a{in->prof, in->lp, in->sub, in->nsub, in->lsb, in->scal, in->n, out, ldo, status,
               chain ? 1 : 0, (unsigned char*)slabs, p.slab, (unsigned)p.wave_lds,
               (unsigned)p.t_lds};
  if (p.global) return launch_k<false, true>(a, p, st);
  if (in->lsb <= np_inl_max(3) && in->nsub <= np_inl_max(3)) return launch_k<true, false>(a, p, st);
  return launch_k<false, false>(a, p, st);
}

// The float32 22-score call: the widened profiles and DM curves first, on the caller's stream
// and so before the fork; then the schedule of launch_bates22_f64 -- sine fits on the caller's
// stream, the Gaussian chain on one side stream, the DM fit and the sub-bands on the other.
hipError_t launch_bates22_f32(const pfe_bates_f32_in* in, double* fprof, double* fdm, double* out,
                              uint32_t* status, const BatesArgs& work, const SubF64Plan& p,
                              void* slabs, hipStream_t st, const Fork* fk, const Options& o) {
  BatesArgs a = work;
  bates_setup(a, in->n, in->lp, o);
  a.prof = nullptr;
  a.fprof = fprof;
  a.sub = nullptr;
  a.nsub = 0;
  a.lsb = 0;
  a.dmcurve = fdm;
  a.ndm = in->ndm;
  a.scal = in->scal;
  a.out = out;
  a.status = status;
  hipError_t e = launch_widen_f32(in->prof, fprof, in->n * in->lp, in->dmcurve, fdm,
                                  in->n * in->ndm, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(status, 0, (size_t)in->n * sizeof(uint32_t), st);
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
    if ((e = launch_subband_f32(in, out + 19, 22, status, true, p, slabs, sd)) != hipSuccess) return e;
    if ((e = launch_sine(a, st)) != hipSuccess) return e;
    if ((e = fork_end(fk, st)) != hipSuccess) return e;
  } else {
    if ((e = launch_sine(a, st)) != hipSuccess) return e;
    if ((e = launch_gauss(a, st)) != hipSuccess) return e;
    if ((e = launch_dmfit(a, st)) != hipSuccess) return e;
    if ((e = launch_subband_f32(in, out + 19, 22, status, true, p, slabs, st)) != hipSuccess) return e;
  }
  launch_clear_internal(status, in->n, st);
  return hipGetLastError();
}

}  // namespace pfe
