// bates22.hip — host launcher of the 22-score pipeline (PHCXFile.compute, PHCXFile.py:383-409).
//
// Score groups run as separate kernels on the caller's stream, in the reference's group
// order; each writes its own output columns and ORs its failure bit into status[c]:
//   k_sine (s1-s4) -> k_ghist (+ k_ghist<BIG> for wide histograms) -> k_gt1 (s8,s9)
//   -> k_gdg (s10,s11) -> k_dmfit (s12-s19) -> k_subband (s20-s22)
#include <cmath>

#include "launch.h"

namespace pfe {

int device_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      cus = v;
  }
  return cus;
}

// Fit slots per wave of the pooled kernels (lm_group.h): a wave works its slots in groups of
// 4 and runs lmpar one slot per lane, so it wants many; but n / slots waves should still
// cover the chip's wave slots (CUs x 8) -- the handle option PFE_OPT_GSLOTS overrides
static int glm_slots(int64_t n, int cus, int fixed) {
  if (fixed > 0) return fixed > GLM_FPW ? GLM_FPW : fixed;
  const int64_t f = n / ((int64_t)cus * 8);
  return (int)(f < 4 ? 4 : f > GLM_FPW ? GLM_FPW : f);
}

__global__ void k_clear_internal(uint32_t* status, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) status[i] &= 0xFFFFu;
}

void launch_clear_internal(uint32_t* status, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_clear_internal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     status, n);
}

void bates_setup(BatesArgs& a, int64_t n, int lp, const Options& o) {
  a.raw_dm = 0;
  a.fpw = blm_fits_per_wave(n, a.cus);
  a.gslots = glm_slots(n, a.cus, o.gslots);
  a.solver = o.solver;
  a.lp = lp;
  a.n = n;
  // Python evaluates pow(len(data), -0.3333333) with the C library; so does this host code
  a.c_lp = std::pow((double)lp, -0.3333333);
  a.c_lp1 = std::pow((double)(lp - 1), -0.3333333);
}

// fork the three independent score groups onto the handle's side streams (false: serial,
// when the handle has none or its PFE_OPT_SERIAL option is set)
bool fork_begin(const Fork* fk, hipStream_t st) {
  if (!fk || !fk->side[0] || fk->serial) return false;
  if (hipEventRecord(fk->ev[0], st) != hipSuccess) return false;
  return hipStreamWaitEvent(fk->side[0], fk->ev[0], 0) == hipSuccess &&
         hipStreamWaitEvent(fk->side[1], fk->ev[0], 0) == hipSuccess;
}
hipError_t fork_end(const Fork* fk, hipStream_t st) {
  hipError_t e;
  if ((e = hipEventRecord(fk->ev[1], fk->side[0])) != hipSuccess) return e;
  if ((e = hipEventRecord(fk->ev[2], fk->side[1])) != hipSuccess) return e;
  if ((e = hipStreamWaitEvent(st, fk->ev[1], 0)) != hipSuccess) return e;
  return hipStreamWaitEvent(st, fk->ev[2], 0);
}

hipError_t launch_bates_groups(const pfe_bates_in* in, double* out, uint32_t* status,
                               const BatesArgs& work, hipStream_t st, const Fork* fk,
                               const Options& o, unsigned groups, bool raw_dm,
                               const double* fprof) {
  BatesArgs a = work;
  bates_setup(a, in->n, in->lp, o);
  a.raw_dm = raw_dm ? 1 : 0;
  a.prof = fprof ? nullptr : in->prof;
  a.fprof = fprof;
  a.lp = in->lp;
  a.sub = in->sub;
  a.nsub = in->nsub;
  a.lsb = in->lsb;
  a.dmcurve = in->dmcurve;
  a.ndm = in->ndm;
  a.scal = in->scal;
  a.n = in->n;
  a.out = out;
  a.status = status;
  hipError_t e = hipMemsetAsync(status, 0, (size_t)in->n * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(out, 0, (size_t)in->n * 22 * sizeof(double), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.counters, 0, BATES_NCOUNTERS * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  if (groups == BG_ALL && fork_begin(fk, st)) {
    if ((e = launch_gauss(a, fk->side[0])) != hipSuccess) return e;
    if ((e = launch_dmfit(a, fk->side[1])) != hipSuccess) return e;
    if ((e = launch_subband(a, fk->side[1])) != hipSuccess) return e;
    if ((e = launch_sine(a, st)) != hipSuccess) return e;
    if ((e = fork_end(fk, st)) != hipSuccess) return e;
  } else {
    if ((groups & BG_SINE) && (e = launch_sine(a, st)) != hipSuccess) return e;
    if ((groups & BG_GAUSS) && (e = launch_gauss(a, st)) != hipSuccess) return e;
    if ((groups & BG_DM) && (e = launch_dmfit(a, st)) != hipSuccess) return e;
    if ((groups & BG_SUB) && (e = launch_subband(a, st)) != hipSuccess) return e;
  }
  launch_clear_internal(status, in->n, st);
  return hipGetLastError();
}

hipError_t launch_bates22(const pfe_bates_in* in, double* out, uint32_t* status,
                          const BatesArgs& work, hipStream_t st, const Fork* fk,
                          const Options& o) {
  return launch_bates_groups(in, out, status, work, st, fk, o, BG_ALL, false, nullptr);
}

}  // namespace pfe
