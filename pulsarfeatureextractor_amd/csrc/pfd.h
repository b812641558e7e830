// pfd.h — arguments of the PFD kernel (pfd.hip) shared with the C-ABI layer (capi.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/pfe.h"
#include "options.h"

namespace pfe {

// score groups of the 22-score path that a PFD launch serves (PfdArgs::groups): the candidate
// parameters (s12-s15, which the other two read), the DM-curve fit (s16-s19) and the
// sub-band scores (s20-s22)
enum : unsigned { PFD_G_PARAMS = 1u, PFD_G_DM = 2u, PFD_G_SUB = 4u, PFD_G_ALL = 7u };

struct PfdArgs {
  const double* profs;     // n x npart x nsub x L
  const double* subfreqs;  // n x nsub
  const double* scal;      // n x PFE_PFD_NSCAL
  int npart, nsub, L;
  int64_t n;
  double* profile;  // n x L or null
  float* chis;      // n x PFE_PFD_NDM or null
  double* lyon8;    // n x 8 or null
  uint32_t* status;
  // the 22-score path (pfd22.hip): scores 12-15 and 20-22 into out22 (n x 22), and the
  // DM-fit inputs [period, snr, dm, width, dm_start, dm_end] into par22 (n x 8); both or none
  double* out22 = nullptr;
  double* par22 = nullptr;
  // the groups the caller wants of out22 (pfe_pfd_params4 / _dmfit4 / _subband3 ask for one):
  // without PFD_G_SUB the sub-band scores are not computed (columns 19-21 are 0), without
  // PFD_G_DM a fold with numdms == 1 is not marked (nothing reads its DM curve)
  unsigned groups = PFD_G_ALL;
  int waves = 4;  // handle option PFE_OPT_PFD_WAVES: the four-wave kernel (<= 128 bins) or one wave
  // the folds' part sums T (n x nsub x L, k_pfd_parts) read from global memory instead of
  // reduced in the kernel (split pipeline), or null (fused)
  const double* tin = nullptr;
  // k_pfd_dmprof_g: gblocks private slabs of gstride bytes each (pfd_global_plan) in device
  // scratch, or null (the fold lives in LDS)
  void* tg = nullptr;
  int gblocks = 0;
  size_t gstride = 0;
};

// split pipeline of pfe_pfd_dmprof: k_pfd_parts streams chunks of `chunk` folds' part sums
// into the two halves of ws (2 x chunk x nsub x L doubles) on `side` while k_pfd_dmprof4
// sweeps the previous chunk on `st`; ev: four events (two per buffer).  False when the
// shape takes the fused kernels (> 128 bins or the four-wave LDS limit).
bool pfd_split_ok(const PfdArgs& a);
hipError_t launch_pfd_dmprof_split(const PfdArgs& a, hipStream_t st, hipStream_t side, double* ws,
                                   int64_t chunk, hipEvent_t (&ev)[4]);

size_t pfd_lds_bytes(int nsub, int L);
constexpr size_t PFD_LDS_LIMIT = 160 * 1024;  // the LDS one workgroup can hold (gfx950)
constexpr int PFD_G_MAX_L = 65535;            // k_pfd_dmprof_g keeps its rotations as uint16_t
// k_pfd_dmprof_g keeps the fold in a slab of global scratch, so it takes every shape whose
// per-fold vectors (lds bytes) fit on chip.  A launch over n folds runs `blocks` persistent
// workgroups -- min(n, 2 x CUs, 1 GiB of slabs), at least one -- on blocks x stride bytes.
struct PfdGlobalPlan {
  size_t lds = 0;        // dynamic LDS of the kernel
  size_t stride = 0;     // bytes per slab (a multiple of 256)
  int blocks = 0;
  bool rot_lds = false;  // the 100 x nsub rotation table in LDS (else behind the fold in the slab)
  bool ok = false;       // false: proflen > PFD_G_MAX_L or lds > PFD_LDS_LIMIT
  size_t bytes() const { return stride * (size_t)blocks; }
};
PfdGlobalPlan pfd_global_plan(int nsub, int L, int64_t n);
hipError_t launch_pfd_dmprof_g(const PfdArgs& a, hipStream_t st);  // pfd_global.hip
hipError_t launch_pfd_dmprof(const PfdArgs& a, hipStream_t st);
// the 22-score chain (pfd22.hip): launch_pfd22 and its workspace are in launch.h

}  // namespace pfe
