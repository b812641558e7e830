// launch.h — what crosses translation units below the C-ABI: the launchers, and the layout of
// every piece of device scratch they and the C-ABI calls (capi.hip) work on.  Each layout is
// one walk over an Arena (arena.h): measured, then placed once the handle's scratch is large
// enough.  The layouts make no HIP call (tests/native/layout_driver.cpp runs them on a CPU).
#pragma once

#include "arena.h"
#include "bates_common.h"
#include "pfd.h"

namespace pfe {

// ---- launchers -------------------------------------------------------------------------
hipError_t launch_lyon8_u8(const uint8_t* prof, int64_t ps, int lp, const uint8_t* dm,
                           int64_t ds, int ld, int64_t n, double* out, hipStream_t st,
                           const Options& o);
hipError_t launch_lyon8_f64(const double* prof, int64_t ps, int lp, const double* dm,
                            int64_t ds, int ld, int64_t n, double* out, hipStream_t st,
                            const Options& o);
// float32 rows (pfe_lyon8_f32): the kernels of launch_lyon8_f64 loading floats, widened at the load
hipError_t launch_lyon8_f32(const float* prof, int64_t ps, int lp, const float* dm, int64_t ds,
                            int ld, int64_t n, double* out, hipStream_t st, const Options& o);
hipError_t launch_sine(const BatesArgs& a, hipStream_t st);
hipError_t launch_gauss(const BatesArgs& a, hipStream_t st);
hipError_t launch_dmfit(const BatesArgs& a, hipStream_t st);
hipError_t launch_subband(const BatesArgs& a, hipStream_t st);
// pfe_subband3: out n x 3; work: subband_work_bytes(n, nsub, lsb) bytes, or null when 0
hipError_t launch_subband3(const pfe_bates_in* in, double* out, uint32_t* status, void* work,
                           hipStream_t st);
const char* subband_shape_error(int nsub, int lsb);
size_t subband_work_bytes(int64_t n, int nsub, int lsb);
void launch_clear_internal(uint32_t* status, int64_t n, hipStream_t st);
bool fork_begin(const Fork* fk, hipStream_t st);
hipError_t fork_end(const Fork* fk, hipStream_t st);
int device_cus();  // compute units of the current device (the `cus` of the layouts)

// ---- the 22-score chain's workspace ----------------------------------------------------
// Fits per wave of the batched kernels: as many as fit the LDS state (32), but few enough
// that the grid holds ~4 waves for every one of (CUs x 16) wave slots -- each wave runs its
// fits one after another, so a batch of fewer waves than slots finishes with its slowest wave
inline int blm_fits_per_wave(int64_t n, int cus) {
  const int64_t f = n / ((int64_t)cus * 64);
  return (int)(f < 4 ? 4 : f > BLM_FPW ? BLM_FPW : f);
}

// persistent waves of the batched and pooled kernels: enough to fill every CU (8 waves
// each), never more than there are batches
inline int persistent_waves(int64_t n, int cus) {
  const int fpw = blm_fits_per_wave(n, cus);
  const int64_t batches = (n + fpw - 1) / fpw;
  const int64_t w = (int64_t)cus * 8;
  return (int)(batches < w ? (batches > 0 ? batches : 1) : w);
}

// hand-over regions (lm_group.h HandOver) of the three chains: waves x slots x K x group
// lanes (16; 32 for the profile fits of > 128 bins); the Gaussian chain runs a.pwaves waves,
// the DM and sine kernels pool_grid(a, 3)
inline int64_t hand_waves(int64_t n, int region, int cus) {
  const int64_t cap = (int64_t)cus * (region == HAND_GAUSS ? 8 : 12);
  return n < 1 ? 1 : n < cap ? n : cap;
}
inline size_t hand_doubles(int64_t n, int region, int lp, int cus) {
  const int k = region == HAND_GAUSS ? HAND_K_GAUSS : region == HAND_DM ? HAND_K_DM : HAND_K_SINE;
  const int slots = region == HAND_GAUSS ? GDG8_FPW : GLM_FPW;  // the Gaussian chain's widest pool
  return (size_t)hand_waves(n, region, cus) * slots * k * glm_group_lanes(lp);
}

// waves of k_ghist_wide (each with a WIDE_SLAB_BYTES = 720 KB scratch slab): one per 64
// candidates up to 256, so a small batch does not carry 184 MB of slabs for a queue that is
// usually empty, and a large one still drains a big queue (low-noise data) in parallel
inline int wide_waves(int64_t n) {
  const int64_t w = n / 64;
  return (int)(w < 1 ? 1 : w > 256 ? 256 : w);
}

// The workspace fields of `a` for a chain over n candidates of lp bins on a device of `cus`
// compute units: [GaussWS x n][counters][hand-over regions][wide queue][wide slabs][per-wave
// scratch], then sub_bytes (subband_work_bytes: not 0 for the sub-band shapes the LDS
// kernels do not hold) of the any-shape sub-band kernel's slabs
inline void bates_layout(Arena& A, BatesArgs& a, int64_t n, int lp, size_t sub_bytes, int cus,
                         const Options& o) {
  static const char* const hand_name[3] = {"hand_gauss", "hand_dm", "hand_sine"};
  a.cus = cus;
  a.ws = A.take<GaussWS>((size_t)n, "gauss_ws");
  a.counters = A.take<unsigned>(BATES_NCOUNTERS, "counters");
  for (int r = 0; r < 3; ++r) {
    double* hb = A.take<double>(hand_doubles(n, r, lp, cus), hand_name[r]);
    a.hand[r] = o.handover ? hb : nullptr;
  }
  a.wide_list = A.take<int>((size_t)n, "wide_list");
  a.wide_waves = wide_waves(n);
  a.wide_scr = (double*)A.take<char>((size_t)a.wide_waves * WIDE_SLAB_BYTES, "wide_slabs");
  a.pwaves = persistent_waves(n, cus);
  a.wscr = A.take<double>((size_t)a.pwaves * gdg_wave_scratch_doubles(lp), "wave_scratch");
  a.sub_work = nullptr;
  if (sub_bytes) a.sub_work = A.take<char>(sub_bytes, "sub_work");
}

// The score groups `groups` (BG_*) of the chain, each into its own columns of out (n x 22);
// status gets the failure bits of those groups only.  work: the fields bates_layout fills.
// raw_dm: getDMFittings' signed shift in column 17 (the per-group entry point pfe_dmfit4)
// instead of the 22-score vector's |shift|.  fprof: the profiles as n x lp doubles (a PFD's
// float profile: the F = true kernels that launch_pfd22 runs) instead of in->prof, or null.
hipError_t launch_bates_groups(const pfe_bates_in* in, double* out, uint32_t* status,
                               const BatesArgs& work, hipStream_t st, const Fork* fk,
                               const Options& o, unsigned groups, bool raw_dm,
                               const double* fprof);
hipError_t launch_bates22(const pfe_bates_in* in, double* out, uint32_t* status,
                          const BatesArgs& work, hipStream_t st, const Fork* fk,
                          const Options& o);
// batching parameters and the Freedman-Diaconis constants of a chain over n candidates of lp
// bins, on the workspace bates_layout placed in `a`
void bates_setup(BatesArgs& a, int64_t n, int lp, const Options& o);

// ---- the PFD 22-score chain's workspace (pfd22.hip) --------------------------------------
struct Pfd22Work {
  double* profile = nullptr;  // n x L: the whole chain only (no group call fits the profile)
  float* chis = nullptr;      // n x PFE_PFD_NDM: with PFD_G_DM (the sweep runs for the fit only)
  double* par22 = nullptr;    // n x 8, the DM-fit inputs [period, snr, dm, width, ...], unfiltered
  BatesArgs bates;            // with PFD_G_DM
};
inline Pfd22Work pfd22_layout(Arena& A, int64_t n, int L, unsigned groups, int cus,
                              const Options& o) {
  Pfd22Work w{};
  if (groups == PFD_G_ALL) w.profile = A.take<double>((size_t)n * L, "profile");
  if (groups & PFD_G_DM) w.chis = A.take<float>((size_t)n * PFE_PFD_NDM, "chis");
  w.par22 = A.take<double>((size_t)n * 8, "par22");
  if (groups & PFD_G_DM) bates_layout(A, w.bates, n, L, 0, cus, o);
  return w;
}
// pa: the PFD inputs (profs, subfreqs, scal, shape, n); out n x 22, status n (device).
// groups != PFD_G_ALL: only those groups' kernels run and only their columns of out and their
// status bits are set; raw_dm: getDMFittings' signed shift in column 17
hipError_t launch_pfd22(PfdArgs pa, double* out, uint32_t* status, const Pfd22Work& w,
                        hipStream_t st, const Fork* fk, const Options& o,
                        unsigned groups = PFD_G_ALL, bool raw_dm = false);

// ---- the scratch of one C-ABI call -------------------------------------------------------
// Host-pointer calls (host = true) stage their inputs, outputs and status first; the
// launcher's workspace follows.  Device-pointer calls take the workspace only.

// pfe_bates22 (chain: nout = 22, the DM curve, bates_layout) / pfe_subband3 (nout = 3)
struct ScoreStage {
  uint8_t *prof = nullptr, *sub = nullptr;
  double *dmcurve = nullptr, *scal = nullptr, *out = nullptr;
  uint32_t* status = nullptr;
  void* sub_work = nullptr;  // pfe_subband3
  BatesArgs bates;           // pfe_bates22
};
inline ScoreStage score_layout(Arena& A, const pfe_bates_in& in, bool host, bool chain,
                               size_t sub_bytes, int cus, const Options& o) {
  ScoreStage s{};
  const size_t n = (size_t)in.n;
  if (host) {
    s.prof = A.take<uint8_t>(n * in.lp, "prof");
    s.sub = A.take<uint8_t>(n * in.nsub * in.lsb, "sub");
    if (chain) s.dmcurve = A.take<double>(n * in.ndm, "dmcurve");
    s.scal = A.take<double>(n * PFE_NSCAL, "scal");
    s.out = A.take<double>(n * (chain ? 22 : 3), "out");
    s.status = A.take<uint32_t>(n, "status");
  }
  if (chain)
    bates_layout(A, s.bates, in.n, in.lp, sub_bytes, cus, o);
  else if (sub_bytes)
    s.sub_work = A.take<char>(sub_bytes, "sub_work");
  return s;
}

// ---- float sub-bands: pfe_subband3_f64 / pfe_bates22_f64 (subband_f64.hip) ---------------
// One wave scores one candidate: its nsub x lsb doubles T and the per-candidate vectors (the
// profile, the centred profile / boxcar row, three nsub-vectors) in the wave's partition of the
// LDS, or -- when that does not fit, or under PFE_OPT_SUBF64_GLOBAL -- T in the wave's slab of
// global scratch and only the vectors on chip.  Pure arithmetic on the shape (no HIP call).
constexpr size_t SUBF64_LDS_LIMIT = 160 * 1024;  // the LDS one workgroup can hold (gfx950)
constexpr int SUBF64_MAX_WPB = 8;                // waves per block
constexpr size_t SUBF64_SLAB_BUDGET = (size_t)1 << 30;
struct SubF64Plan {
  bool ok = false;      // false: the per-candidate vectors alone exceed the LDS
  bool global = false;  // T in global scratch
  size_t wave_lds = 0;  // LDS bytes per wave (a multiple of 16)
  size_t t_lds = 0;     // of which T, in front (0: global)
  size_t slab = 0;      // bytes per wave's slab (a multiple of 256; 0: on chip)
  int wpb = 0;          // waves per block
  int blocks = 0;       // persistent blocks
  size_t slab_bytes() const { return slab * (size_t)wpb * (size_t)blocks; }
};
inline size_t subf64_vec_bytes(int nsub, int lsb) {
  return ((2 * (size_t)lsb + 3 * (size_t)nsub) * sizeof(double) + 15) & ~(size_t)15;
}
inline SubF64Plan subf64_plan(int nsub, int lsb, int64_t n, int cus, bool force_global) {
  SubF64Plan p;
  if (nsub < 1 || lsb < 1) return p;
  const size_t vec = subf64_vec_bytes(nsub, lsb);
  if (vec > SUBF64_LDS_LIMIT) return p;
  p.ok = true;
  const size_t t = ((size_t)nsub * lsb * sizeof(double) + 15) & ~(size_t)15;
  p.global = force_global || t + vec > SUBF64_LDS_LIMIT;
  p.t_lds = p.global ? 0 : t;
  p.wave_lds = p.t_lds + vec;
  int64_t wpb = (int64_t)(SUBF64_LDS_LIMIT / p.wave_lds);
  if (wpb > SUBF64_MAX_WPB) wpb = SUBF64_MAX_WPB;
  // as many blocks per CU as the LDS holds, up to 32 waves
  int64_t per_cu = (int64_t)(SUBF64_LDS_LIMIT / ((size_t)wpb * p.wave_lds));
  if (per_cu > 32 / wpb) per_cu = 32 / wpb;
  int64_t blocks = (int64_t)(cus > 0 ? cus : 1) * per_cu;
  if (blocks > (n + wpb - 1) / wpb) blocks = (n + wpb - 1) / wpb;
  if (p.global) {
    p.slab = ((size_t)nsub * lsb * sizeof(double) + 255) & ~(size_t)255;
    const int64_t budget = (int64_t)(SUBF64_SLAB_BUDGET / p.slab);  // >= 1 for every ok shape
    if (wpb > budget) wpb = budget > 0 ? budget : 1;
    if (blocks * wpb > budget) blocks = budget / wpb;
  }
  p.wpb = (int)wpb;
  p.blocks = (int)(blocks < 1 ? 1 : blocks);
  return p;
}
// scores 20-22 of n candidates into out[c * ldo + 0..2].  chain: a failed row ORs
// PFE_ST_SUBBAND_FAIL into status and leaves out alone (the 22-score call zeroed both); else
// every row's status and scores are stored (0.0 where it failed).  slabs: p.slab_bytes() bytes
hipError_t launch_subband_f64(const pfe_bates_f64_in* in, double* out, int ldo, uint32_t* status,
                              bool chain, const SubF64Plan& p, void* slabs, hipStream_t st);
// pfe_bates22_f64: the four fitted / copied groups by the float-profile kernels of the chain
// and launch_subband_f64, forked over the side streams as launch_bates22 forks its groups
hipError_t launch_bates22_f64(const pfe_bates_f64_in* in, double* out, uint32_t* status,
                              const BatesArgs& work, const SubF64Plan& p, void* slabs,
                              hipStream_t st, const Fork* fk, const Options& o);

// pfe_subband3_f64 (chain = false: nout = 3) / pfe_bates22_f64 (chain: nout = 22, the DM curve,
// bates_layout): the staged host arrays, then the per-wave slabs of the global path
struct SubF64Stage {
  double *prof = nullptr, *sub = nullptr, *dmcurve = nullptr, *scal = nullptr, *out = nullptr;
  uint32_t* status = nullptr;
  BatesArgs bates;  // pfe_bates22_f64
  void* slabs = nullptr;
};
inline SubF64Stage subband_f64_layout(Arena& A, const pfe_bates_f64_in& in, bool host, bool chain,
                                      size_t slab_bytes, int cus, const Options& o) {
  SubF64Stage s{};
  const size_t n = (size_t)in.n;
  if (host) {
    s.prof = A.take<double>(n * in.lp, "prof");
    s.sub = A.take<double>(n * in.nsub * in.lsb, "sub");
    if (chain) s.dmcurve = A.take<double>(n * in.ndm, "dmcurve");
    s.scal = A.take<double>(n * PFE_NSCAL, "scal");
    s.out = A.take<double>(n * (chain ? 22 : 3), "out");
    s.status = A.take<uint32_t>(n, "status");
  }
  if (chain) bates_layout(A, s.bates, in.n, in.lp, 0, cus, o);
  if (slab_bytes) s.slabs = A.take<char>(slab_bytes, "slabs");
  return s;
}

// ---- float32 candidates: the _f32 forms of the float-array calls (cand_f32.hip) -----------
// da[i] = (double)a[i], i < na, and db[i] = (double)b[i], i < nb (nb = 0: a alone): the small
// per-candidate arrays the fit kernels read many times (profiles, DM curves), widened once
hipError_t launch_widen_f32(const float* a, double* da, int64_t na, const float* b, double* db,
                            int64_t nb, hipStream_t st);
// launch_subband_f64 on float32 arrays: the copy of a candidate's sub-bands and its profile row
// are widened on their way into the LDS or the slab; plan, slabs and arithmetic are the f64 call's
hipError_t launch_subband_f32(const pfe_bates_f32_in* in, double* out, int ldo, uint32_t* status,
                              bool chain, const SubF64Plan& p, void* slabs, hipStream_t st);
// pfe_bates22_f32: launch_widen_f32 of the profiles into fprof (n x lp) and the DM curves into
// fdm (n x ndm) on st, then the schedule of launch_bates22_f64 with launch_subband_f32
hipError_t launch_bates22_f32(const pfe_bates_f32_in* in, double* fprof, double* fdm, double* out,
                              uint32_t* status, const BatesArgs& work, const SubF64Plan& p,
                              void* slabs, hipStream_t st, const Fork* fk, const Options& o);

// pfe_subband3_f32 / pfe_bates22_f32: subband_f64_layout with the staged float arrays as the
// floats they are, and (chain, host pointers or device) the widened profiles and DM curves
// behind them.  The sub-bands are never widened in memory.
struct SubF32Stage {
  float *prof = nullptr, *sub = nullptr, *dmcurve = nullptr;
  double *scal = nullptr, *out = nullptr;
  uint32_t* status = nullptr;
  double *fprof = nullptr, *fdm = nullptr;  // pfe_bates22_f32
  BatesArgs bates;                          // pfe_bates22_f32
  void* slabs = nullptr;
};
inline SubF32Stage subband_f32_layout(Arena& A, const pfe_bates_f32_in& in, bool host, bool chain,
                                      size_t slab_bytes, int cus, const Options& o) {
  SubF32Stage s{};
  const size_t n = (size_t)in.n;
  if (host) {
    s.prof = A.take<float>(n * in.lp, "prof");
    s.sub = A.take<float>(n * in.nsub * in.lsb, "sub");
    if (chain) s.dmcurve = A.take<float>(n * in.ndm, "dmcurve");
    s.scal = A.take<double>(n * PFE_NSCAL, "scal");
    s.out = A.take<double>(n * (chain ? 22 : 3), "out");
    s.status = A.take<uint32_t>(n, "status");
  }
  if (chain) {
    s.fprof = A.take<double>(n * in.lp, "fprof");
    s.fdm = A.take<double>(n * in.ndm, "fdm");
    bates_layout(A, s.bates, in.n, in.lp, 0, cus, o);
  }
  if (slab_bytes) s.slabs = A.take<char>(slab_bytes, "slabs");
  return s;
}

// one score group of n candidates (groups: BG_SINE / BG_GAUSS / BG_DM; 0: pfe_params4, which
// fits nothing).  A fit scores into a 22-column scratch d22 and hands out its k columns.
// Inputs: the DM curves (BG_DM: lp = 0), the float profiles (f64) or the byte profiles, and
// the scalars of every call but the f64 ones.  The float32 forms (f32, with f64): the profiles
// staged as the floats they are (prof32), and fprof -- host pointers or device -- for
// launch_widen_f32 to fill; the fit kernels read fprof as in the f64 call.
struct GroupStage {
  uint8_t* prof = nullptr;
  float* prof32 = nullptr;
  double *fprof = nullptr, *dmcurve = nullptr, *scal = nullptr, *d22 = nullptr, *out = nullptr;
  uint32_t* status = nullptr;
  BatesArgs bates;
};
inline GroupStage group_layout(Arena& A, int64_t n_, int lp, int ndm, unsigned groups, bool f64,
                               int k, bool host, int cus, const Options& o, bool f32 = false) {
  GroupStage s{};
  const size_t n = (size_t)n_;
  if (host) {
    if (groups == BG_DM)
      s.dmcurve = A.take<double>(n * ndm, "dmcurve");
    else if (f32)
      s.prof32 = A.take<float>(n * lp, "prof32");
    else if (f64)
      s.fprof = A.take<double>(n * lp, "fprof");
    else if (groups)
      s.prof = A.take<uint8_t>(n * lp, "prof");
    if (!f64) s.scal = A.take<double>(n * PFE_NSCAL, "scal");
  }
  if (f32) s.fprof = A.take<double>(n * lp, "fprof");
  if (groups) s.d22 = A.take<double>(n * 22, "d22");
  if (host) {
    s.out = A.take<double>(n * k, "out");
    s.status = A.take<uint32_t>(n, "status");
  }
  if (groups) bates_layout(A, s.bates, n_, lp, 0, cus, o);
  return s;
}

// ---- float32 fold cubes: the pfe_pfd_*_f32 calls (pfd_f32.hip) ---------------------------
// A float32 call runs in passes of `chunk` folds: k_pfd_partsum_f32 sums the parts of the
// pass's folds into psum (chunk x nsub x proflen doubles), and the f64 kernels run on psum
// with npart = 1.  chunk: as many folds as keep psum within 1 GiB (at least one), fewer when
// PFE_OPT_PFD_F32_CHUNK (opt > 0) asks for fewer, never more than n.
constexpr size_t PFD_F32_PSUM_BUDGET = (size_t)1 << 30;
inline int64_t pfd_f32_chunk(int nsub, int L, int64_t n, int64_t opt) {
  int64_t c = (int64_t)(PFD_F32_PSUM_BUDGET / ((size_t)nsub * (size_t)L * sizeof(double)));
  if (c < 1) c = 1;
  if (opt > 0 && opt < c) c = opt;
  return c < n ? c : n;
}
// s[c][e] = (double)x[c][0][e] + ... + (double)x[c][npart-1][e], e over nsub x L, c over n folds
hipError_t launch_pfd_partsum_f32(const float* x, double* s, int npart, int nsub, int L, int64_t n,
                                  hipStream_t st);

// ---- cubes in the opposite byte order: PFE_FLAG_PFD_BSWAP (pfd_be64.hip) ------------------
// A flagged f64 call is the float32 call with 8-byte words: passes of pfd_f32_chunk folds
// (PFE_OPT_PFD_F32_CHUNK governs both), k_pfd_partsum_be64 summing the parts of the pass's
// folds -- every word read through the byte reversal -- into psum, the f64 kernels on psum
// with npart = 1.  The scratch of a flagged call (be64 = true in the layouts below), in order:
//   host pointers: [profs: the n x npart x nsub x proflen words as they are][subfreqs][scal]
//                  [the outputs the call stages][status]
//   then, host pointers or device:
//                  [psum: chunk x nsub x proflen doubles]
//                  [PFE_FLAG_PFD_AVGPROF: avg_csum of chunk folds (and avg_scal, device pointers)]
//                  [the scratch of the f64 call on the folds of one pass]
// that is the float32 layout with profs (8 bytes a value) where that has profs32.
// s[c][e] = v(x[c][0][e]) + ... + v(x[c][npart-1][e]), v the value of the byte-reversed word
hipError_t launch_pfd_partsum_be64(const double* x, double* s, int npart, int nsub, int L,
                                   int64_t n, hipStream_t st);

// ---- int16 fold cubes: the pfe_pfd_*_i16 calls (pfd_i16.hip) -----------------------------
// An int16 call is the float32 call with 2-byte values and their float32 scale, offset and
// weight per (fold, part, sub-band): passes of pfd_f32_chunk folds (PFE_OPT_PFD_F32_CHUNK
// governs this path too), k_pfd_partsum_i16 decoding and summing the parts of the pass's folds
// into psum, the f64 kernels on psum with npart = 1.  The scratch of an int16 call (i16 != 0 in
// the layouts below), in order:
//   host pointers: [data16: the n x npart x nsub x proflen values][scl16][offs16][wts16, when
//                  weights are given: n x npart x nsub floats each][subfreqs][scal]
//                  [the outputs the call stages][status]
//   then, host pointers or device:
//                  [psum: chunk x nsub x proflen doubles]
//                  [PFE_FLAG_PFD_AVGPROF: avg_csum of chunk folds (and avg_scal, device pointers)]
//                  [the scratch of the f64 call on the folds of one pass]
enum PfdI16 { PFD_I16_NONE = 0, PFD_I16_PLAIN = 1, PFD_I16_WEIGHTS = 2 };
// the four arrays of an int16 call as the kernels read them: value (c, p, s, b) of data at
// data + c*dfs + p*dps + 2*(s*L + b), value (c, p, s) of scl (offs, wts) at scl + c*pfs +
// p*pps + 4*s.  Dense arrays have the strides of their shapes; table rows share one pair
//
// A cube with a polarisation axis (the _i16_pol calls: npol stored per (fold, part), dense between
// part and sub-band in data, scl and offs; wts has none): polarisation k of a value lies dks (of
// its scl and offs: pks) bytes further, the leading nsum of them are summed, and value (c, p, s)
// of wts is at wts + c*wfs + p*wps + 4*s.  Table rows still share one pair of strides; dense
// arrays of npol > 1 do not (wfs != pfs).  pfd_i16_ns() says which kernels read the cube
struct PfdI16Src {
  const char *data = nullptr, *scl = nullptr, *offs = nullptr, *wts = nullptr;  // wts may be null
  int64_t dfs = 0, dps = 0, pfs = 0, pps = 0;  // bytes
  bool bswap = false;                          // PFE_FLAG_PFD_BSWAP: every value byte-reversed
  int nsum = 1;                                // polarisations summed: 1 or 2
  int64_t dks = 0, pks = 0;                    // bytes between polarisations: data, scl / offs
  int64_t wfs = 0, wps = 0;                    // bytes between folds and parts of wts
  PfdI16Src from(int64_t c0) const {           // folds c0 ..
    PfdI16Src r = *this;
    r.data += c0 * dfs;
    r.scl += c0 * pfs;
    r.offs += c0 * pfs;
    if (wts) r.wts += c0 * wfs;
    return r;
  }
};
// npol polarisations stored, the leading nsum summed (1, 1: the cube of the _i16 calls)
inline PfdI16Src pfd_i16_src(const pfe_pfd_i16_in& in, bool bswap, int npol = 1, int nsum = 1) {
  PfdI16Src q;
  q.data = reinterpret_cast<const char*>(in.data);
  q.scl = reinterpret_cast<const char*>(in.scl);
  q.offs = reinterpret_cast<const char*>(in.offs);
  q.wts = reinterpret_cast<const char*>(in.wts);
  q.dks = (int64_t)2 * in.nsub * in.proflen;
  q.pks = (int64_t)4 * in.nsub;
  if (in.fold_stride) {
    q.dfs = q.pfs = q.wfs = in.fold_stride;
    q.dps = q.pps = q.wps = in.part_stride;
  } else {
    q.dps = q.dks * npol;
    q.dfs = q.dps * in.npart;
    q.pps = q.pks * npol;
    q.pfs = q.pps * in.npart;
    q.wps = q.pks;
    q.wfs = q.wps * in.npart;
  }
  q.nsum = nsum;
  q.bswap = bswap;
  return q;
}
// the NS of the kernels that read x (pfd_i16_dev.h): 0, the kernels of the _i16 calls, whenever
// one polarisation is read and the weights lie where those kernels look for them (none given, or
// the strides of scl: table rows, and dense arrays of npol = 1); else the polarisations read
inline int pfd_i16_ns(const PfdI16Src& x) {
  if (x.nsum == 2) return 2;
  return x.wts && (x.wfs != x.pfs || x.wps != x.pps) ? 1 : 0;
}
// s[c][e] = x(c,0,e) + ... + x(c,npart-1,e), x the decoded value ((double)d * scl + offs, then
// * wts when given), e over nsub x L, c over n folds; s dense
hipError_t launch_pfd_partsum_i16(const PfdI16Src& x, double* s, int npart, int nsub, int L,
                                  int64_t n, hipStream_t st);

// ---- kill masks: the pfe_pfd_*_kill calls (pfd_kill.hip) ---------------------------------
// A masked call, f64 included, is the float32 call with a selection at the load: passes of
// pfd_f32_chunk folds (PFE_OPT_PFD_F32_CHUNK governs this path too), k_pfd_partsum_kill summing
// the selected values of the pass's folds -- +0.0 where the part or the sub-band of the value is
// killed -- into psum, the f64 kernels on psum with npart = 1.  The scratch of a masked call
// (kill != 0 in the layouts below: PFD_KILL_PARTS | PFD_KILL_SUBS, each mask that is given), in
// order:
//   host pointers: [profs (8 bytes a value; be64 = true in the layouts, reversed or not) or
//                  profs32][subfreqs][scal][kill_parts: n x npart bytes][kill_subs: n x nsub
//                  bytes][the outputs the call stages][status]
//   then, host pointers or device:
//                  [psum: chunk x nsub x proflen doubles]
//                  [PFE_FLAG_PFD_AVGPROF: avg_csum of chunk folds (and avg_scal, device pointers)]
//                  [the scratch of the f64 call on the folds of one pass]
enum PfdKillMask { PFD_KILL_NONE = 0, PFD_KILL_PARTS = 1, PFD_KILL_SUBS = 2 };
enum PfdKillElem { PFD_KILL_F64 = 0, PFD_KILL_BE64 = 1, PFD_KILL_F32 = 2 };
// the masks of a launch on the device: parts n x npart, subs n x nsub bytes, non-zero = killed,
// either null (none killed)
struct PfdKillSrc {
  const uint8_t *parts = nullptr, *subs = nullptr;
  PfdKillSrc from(int64_t c0, int npart, int nsub) const {  // folds c0 ..
    PfdKillSrc r;
    r.parts = parts ? parts + c0 * npart : nullptr;
    r.subs = subs ? subs + c0 * nsub : nullptr;
    return r;
  }
  int mask() const { return (parts ? PFD_KILL_PARTS : 0) | (subs ? PFD_KILL_SUBS : 0); }
};
// s[c][e] = v(c,0,e) + ... + v(c,npart-1,e), v the value of x (elem: doubles, byte-reversed
// doubles, floats) or +0.0 where k kills its part or its sub-band; e over nsub x L, c over n folds
hipError_t launch_pfd_partsum_kill(const void* x, int elem, const PfdKillSrc& k, double* s,
                                   int npart, int nsub, int L, int64_t n, hipStream_t st);

// ---- scrunching a fold: pfe_pfd_scrunch and its _f32 / _i16 forms (pfd_scrunch.hip) ------
// z[i][g][k], G = nchan / fscr groups of channels by K = nbin / bscr bins: the parts of every
// element summed in order, each channel's row rotated left by rot[i][c] mod nbin, bscr bins
// summed in order, fscr channels summed in order; all in fp64 (include/pfe.h states the steps).
// Two routes, the same adds in the same order on both:
//   LDS    (pfd_scrunch_lds: a row and the K running sums fit 64 KB of LDS) one block per (fold,
//          group): slabs of `pfd_scrunch_slab_chans` channel rows are part-summed into the LDS with
//          aligned wide loads, then K lanes add their bscr rotated values of every row in order;
//   direct (any nbin) one lane per output bin, each value loaded alone at its rotated place.
constexpr int PFD_SCR_LDS_DOUBLES = 8192;   // 64 KB: a row and the running sums of one block
constexpr int PFD_SCR_SLAB_DOUBLES = 4096;  // 32 KB: the channel rows a block sums at a time
inline bool pfd_scrunch_lds(int nbin, int bscr) {
  return (((int64_t)nbin + 3) & ~(int64_t)3) + nbin / bscr <= PFD_SCR_LDS_DOUBLES;
}
inline int pfd_scrunch_slab_chans(int nbin, int fscr) {
  const int c = PFD_SCR_SLAB_DOUBLES / nbin;
  return c < 1 ? 1 : c > fscr ? fscr : c;
}
// the cube of a scrunch call: exactly one of f64, f32 and i16 (its data non-null) is set
struct PfdScrunchSrc {
  const double* f64 = nullptr;
  const float* f32 = nullptr;
  PfdI16Src i16;
};
// rot: n x nchan, or null; z: n x (nchan / fscr) x (nbin / bscr), dense.  direct: the direct
// route whatever the shape (measurements and tests; a shape the LDS does not hold takes it anyway)
hipError_t launch_pfd_scrunch(const PfdScrunchSrc& x, const int32_t* rot, double* z, int npart,
                              int nchan, int nbin, int fscr, int bscr, int64_t n, bool direct,
                              hipStream_t st);

// pfe_pfd_scrunch / _f32 / _i16: a host-pointer call stages the cube as the values it holds (an
// int16 cube with scl, offs and, when given, wts behind it: ES = npart x nchan floats a fold
// each), then rot (n x nchan, when given), then out (n x GK doubles, GK = G x K).  A
// device-pointer call takes no scratch.  pol (a _i16_pol call: the polarisations it sums): the
// cube, scl and offs staged compacted, pol times their size, the axis between part and channel
struct PfdScrunchStage {
  double* profs = nullptr;
  float* profs32 = nullptr;
  int16_t* data16 = nullptr;
  float *scl16 = nullptr, *offs16 = nullptr, *wts16 = nullptr;
  int32_t* rot = nullptr;
  double* out = nullptr;
};
inline PfdScrunchStage pfd_scrunch_layout(Arena& A, int64_t E, int64_t ES, int nchan, int64_t GK,
                                          int64_t n, bool host, bool f32, int i16, bool rot,
                                          int pol = 1) {
  PfdScrunchStage s;
  if (!host) return s;
  if (i16) {
    s.data16 = A.take<int16_t>((size_t)n * E * pol, "data16");
    s.scl16 = A.take<float>((size_t)n * ES * pol, "scl16");
    s.offs16 = A.take<float>((size_t)n * ES * pol, "offs16");
    if (i16 == PFD_I16_WEIGHTS) s.wts16 = A.take<float>((size_t)n * ES, "wts16");
  } else if (f32)
    s.profs32 = A.take<float>((size_t)n * E, "profs32");
  else
    s.profs = A.take<double>((size_t)n * E, "profs");
  if (rot) s.rot = A.take<int32_t>((size_t)n * nchan, "rot");
  s.out = A.take<double>((size_t)n * GK, "out");
  return s;
}

// ---- a fold's average: pfe_pfd_avgprof and PFE_FLAG_PFD_AVGPROF (pfd_avgprof.hip) --------
// numpy's (profs / proflen).sum() of each fold: k_pfd_avgprof sums every chunk of
// PFD_AVG_CHUNK values (numpy's reduction buffer) of a fold's E = npart x nsub x proflen into
// csum (n x pfd_avg_chunks(E) doubles), k_pfd_avgprof_fin adds a fold's chunk sums in order
// into out[i * stride]
constexpr int PFD_AVG_CHUNK = 8192;
inline int64_t pfd_avg_chunks(int64_t E) { return (E + PFD_AVG_CHUNK - 1) / PFD_AVG_CHUNK; }
hipError_t launch_pfd_avgprof(const double* x, int64_t E, int L, int64_t n, double* csum,
                              double* out, int64_t stride, hipStream_t st);
hipError_t launch_pfd_avgprof_f32(const float* x, int64_t E, int L, int64_t n, double* csum,
                                  double* out, int64_t stride, hipStream_t st);
// PFE_FLAG_PFD_BSWAP: x holds byte-reversed doubles, each widened through the reversal
hipError_t launch_pfd_avgprof_be64(const double* x, int64_t E, int L, int64_t n, double* csum,
                                   double* out, int64_t stride, hipStream_t st);
// an int16 cube: each value decoded where it is loaded, the n folds' E = npart x nsub x L values
// in the order (p, s, b)
hipError_t launch_pfd_avgprof_i16(const PfdI16Src& x, int npart, int nsub, int L, int64_t n,
                                  double* csum, double* out, int64_t stride, hipStream_t st);
// a masked cube (x and elem as for launch_pfd_partsum_kill): each value selected where it is
// loaded, +0.0 where killed, the n folds' E = npart x nsub x L values in the order (p, s, b)
hipError_t launch_pfd_avgprof_kill(const void* x, int elem, const PfdKillSrc& k, int npart, int nsub,
                                   int L, int64_t n, double* csum, double* out, int64_t stride,
                                   hipStream_t st);

// pfe_pfd_avgprof / pfe_pfd_avgprof_f32: a host-pointer call stages the cube (as the values it
// holds) and its n results; the chunk sums follow.  A masked call (kill: PfdKillMask bits, with
// the fold's npart and nsub) stages its masks directly behind the cube, parts then subs.  pol (a
// _i16_pol call: the polarisations it sums): data16, scl16 and offs16 pol times their size; E
// stays the npart x nsub x proflen summed values of a fold
struct PfdAvgStage {
  double* profs = nullptr;
  float* profs32 = nullptr;
  int16_t* data16 = nullptr;  // pfe_pfd_avgprof_i16: the cube and its parameters (ES = npart x nsub)
  float *scl16 = nullptr, *offs16 = nullptr, *wts16 = nullptr;
  uint8_t *kparts = nullptr, *ksubs = nullptr;
  double *out = nullptr, *csum = nullptr;
};
inline PfdAvgStage pfd_avgprof_layout(Arena& A, int64_t E, int64_t n, bool host, bool f32,
                                      int i16 = PFD_I16_NONE, int64_t ES = 0, int kill = 0,
                                      int npart = 0, int nsub = 0, int pol = 1) {
  PfdAvgStage s;
  if (host) {
    if (i16) {
      s.data16 = A.take<int16_t>((size_t)n * E * pol, "data16");
      s.scl16 = A.take<float>((size_t)n * ES * pol, "scl16");
      s.offs16 = A.take<float>((size_t)n * ES * pol, "offs16");
      if (i16 == PFD_I16_WEIGHTS) s.wts16 = A.take<float>((size_t)n * ES, "wts16");
    } else if (f32)
      s.profs32 = A.take<float>((size_t)n * E, "profs32");
    else
      s.profs = A.take<double>((size_t)n * E, "profs");
    if (kill & PFD_KILL_PARTS) s.kparts = A.take<uint8_t>((size_t)n * npart, "kill_parts");
    if (kill & PFD_KILL_SUBS) s.ksubs = A.take<uint8_t>((size_t)n * nsub, "kill_subs");
    s.out = A.take<double>((size_t)n, "out");
  }
  s.csum = A.take<double>((size_t)n * pfd_avg_chunks(E), "avg_csum");
  return s;
}

// PFE_FLAG_PFD_AVGPROF on a PFD call: the chunk sums of the `folds` folds one pass derives
// (all n of an f64 call), and -- device pointers, whose scal is the caller's and is never
// written -- a copy of scal for the derived values (a host-pointer call writes into its
// staged scal)
struct PfdAvgWork {
  double *csum = nullptr, *scal = nullptr;
};
inline PfdAvgWork pfd_avg_work_layout(Arena& A, const pfe_pfd_in& in, bool host, int64_t folds) {
  PfdAvgWork w;
  const int64_t E = (int64_t)in.npart * in.nsub * in.proflen;
  w.csum = A.take<double>((size_t)folds * pfd_avg_chunks(E), "avg_csum");
  if (!host) w.scal = A.take<double>((size_t)in.n * PFE_PFD_NSCAL, "avg_scal");
  return w;
}

// the three inputs every PFD call stages.  A float32 call (f32_chunk > 0: its folds per pass)
// stages the cube as the floats it is (profs32, no profs), and -- host pointers or device --
// takes psum behind its staged arrays.  A masked call (kill: PfdKillMask bits) stages its masks
// directly behind scal, parts then subs, each only when given.  pol (a _i16_pol call: the
// polarisations it sums, staged compacted): data16, scl16 and offs16 pol times their size; wts16
// has no polarisation axis
struct PfdInputs {
  double *profs = nullptr, *subfreqs = nullptr, *scal = nullptr;
  float* profs32 = nullptr;
  int16_t* data16 = nullptr;  // an int16 call: the cube and its parameters
  float *scl16 = nullptr, *offs16 = nullptr, *wts16 = nullptr;
  uint8_t *kparts = nullptr, *ksubs = nullptr;
  double* psum = nullptr;
};
inline PfdInputs pfd_inputs_layout(Arena& A, const pfe_pfd_in& in, bool f32 = false,
                                   int i16 = PFD_I16_NONE, int kill = 0, int pol = 1) {
  PfdInputs s;
  const size_t n = (size_t)in.n, cube = n * in.npart * in.nsub * in.proflen;
  if (i16) {
    const size_t par = n * in.npart * in.nsub;
    s.data16 = A.take<int16_t>(cube * pol, "data16");
    s.scl16 = A.take<float>(par * pol, "scl16");
    s.offs16 = A.take<float>(par * pol, "offs16");
    if (i16 == PFD_I16_WEIGHTS) s.wts16 = A.take<float>(par, "wts16");
  } else if (f32)
    s.profs32 = A.take<float>(cube, "profs32");
  else
    s.profs = A.take<double>(cube, "profs");
  s.subfreqs = A.take<double>(n * in.nsub, "subfreqs");
  s.scal = A.take<double>(n * PFE_PFD_NSCAL, "scal");
  if (kill & PFD_KILL_PARTS) s.kparts = A.take<uint8_t>(n * in.npart, "kill_parts");
  if (kill & PFD_KILL_SUBS) s.ksubs = A.take<uint8_t>(n * in.nsub, "kill_subs");
  return s;
}
inline double* pfd_psum_layout(Arena& A, const pfe_pfd_in& in, int64_t f32_chunk) {
  return A.take<double>((size_t)f32_chunk * in.nsub * in.proflen, "psum");
}

// pfe_pfd_dmprof: the outputs the caller asked for, then ws_bytes for the two part-sum
// buffers of the split pipeline or the slabs of the global-memory kernel (PfdGlobalPlan).
// pfe_pfd_dmprof_f32 (f32_chunk > 0): the same with the float cube and psum; ws_bytes is
// then what one pass needs.  avgprof (PFE_FLAG_PFD_AVGPROF): pfd_avg_work_layout behind psum.
// be64 (PFE_FLAG_PFD_BSWAP, with f32_chunk > 0): the same passes on the cube staged as the
// 8-byte words it holds (profs).  i16 (an int16 call, with f32_chunk > 0; be64 false, whatever
// the flag): the same passes on the cube staged as int16 with its parameters.  kill (a masked
// call, with f32_chunk > 0; be64 true for an f64 cube, reversed or not): the masks behind scal
struct PfdDmprofStage {
  PfdInputs in;
  PfdAvgWork avg;
  double* profile = nullptr;
  float* chis = nullptr;
  double* lyon8 = nullptr;
  uint32_t* status = nullptr;
  void* ws = nullptr;
};
inline PfdDmprofStage pfd_dmprof_layout(Arena& A, const pfe_pfd_in& in, bool host, bool profile,
                                        bool chis, bool lyon8, size_t ws_bytes,
                                        int64_t f32_chunk = 0, bool avgprof = false,
                                        bool be64 = false, int i16 = PFD_I16_NONE,
                                        int kill = 0, int pol = 1) {
  PfdDmprofStage s;
  const size_t n = (size_t)in.n;
  if (host) {
    s.in = pfd_inputs_layout(A, in, f32_chunk > 0 && !be64, i16, kill, pol);
    if (profile) s.profile = A.take<double>(n * in.proflen, "profile");
    if (chis) s.chis = A.take<float>(n * PFE_PFD_NDM, "chis");
    if (lyon8) s.lyon8 = A.take<double>(n * 8, "lyon8");
    s.status = A.take<uint32_t>(n, "status");
  }
  if (f32_chunk > 0) s.in.psum = pfd_psum_layout(A, in, f32_chunk);
  if (avgprof) s.avg = pfd_avg_work_layout(A, in, host, f32_chunk > 0 ? f32_chunk : in.n);
  if (ws_bytes) s.ws = A.take<char>(ws_bytes, "ws");
  return s;
}

// pfe_pfd_bates22 (groups = PFD_G_ALL, k = 22) and the PFD group calls, which score into a
// 22-column scratch d22 of their own and hand out k columns; g_bytes: the slabs of the
// global-memory kernel (0: the fold lives in LDS).  The float32 forms (f32_chunk > 0): the
// float cube and psum, and d22, the chain's workspace and g_bytes for the `pass` folds of one
// pass (a pass's chain then works on what the f64 call on that many folds lays out); the
// staged arrays and psum come first, so they stay put from one pass to the next.  avgprof
// (PFE_FLAG_PFD_AVGPROF on a call that reads the average): pfd_avg_work_layout behind psum,
// sized by f32_chunk, so it stays put as well.  be64 (PFE_FLAG_PFD_BSWAP, with f32_chunk > 0):
// the float32 layout with the cube staged as the 8-byte words it holds (profs).  i16 (an int16
// call, with f32_chunk > 0; be64 false): the float32 layout with the int16 cube and its parameters.
// kill (a masked call, with f32_chunk > 0; be64 true for an f64 cube): the masks behind scal
struct PfdScoresStage {
  PfdInputs in;
  PfdAvgWork avg;
  double *out = nullptr, *d22 = nullptr;
  uint32_t* status = nullptr;
  Pfd22Work work;
  void* tg = nullptr;
};
inline PfdScoresStage pfd_scores_layout(Arena& A, const pfe_pfd_in& in, bool host,
                                        unsigned groups, int k, size_t g_bytes, int cus,
                                        const Options& o, int64_t f32_chunk = 0,
                                        int64_t pass = 0, bool avgprof = false,
                                        bool be64 = false, int i16 = PFD_I16_NONE,
                                        int kill = 0, int pol = 1) {
  PfdScoresStage s;
  const size_t n = (size_t)in.n;
  const int64_t wn = f32_chunk > 0 ? pass : in.n;
  if (host) {
    s.in = pfd_inputs_layout(A, in, f32_chunk > 0 && !be64, i16, kill, pol);
    s.out = A.take<double>(n * k, "out");
    s.status = A.take<uint32_t>(n, "status");
  }
  if (f32_chunk > 0) s.in.psum = pfd_psum_layout(A, in, f32_chunk);
  if (avgprof) s.avg = pfd_avg_work_layout(A, in, host, f32_chunk > 0 ? f32_chunk : in.n);
  if (groups != PFD_G_ALL) s.d22 = A.take<double>((size_t)wn * 22, "d22");
  s.work = pfd22_layout(A, wn, in.proflen, groups, cus, o);
  if (g_bytes) s.tg = A.take<char>(g_bytes, "tg");
  return s;
}

// one slot of the chunked Lyon-8 host pipeline: `chunk` rows in, their features out (the
// device slots and the pinned staging ring share the layout)
template <typename T>
struct Lyon8Slot {
  T *prof = nullptr, *dm = nullptr;
  double* out = nullptr;
};
template <typename T>
inline Lyon8Slot<T> lyon8_slot_layout(Arena& A, int64_t chunk, int lp, int ld) {
  Lyon8Slot<T> s;
  s.prof = A.take<T>((size_t)chunk * lp, "prof");
  s.dm = A.take<T>((size_t)chunk * ld, "dm");
  s.out = A.take<double>((size_t)chunk * 8, "out");
  return s;
}

}  // namespace pfe
