/*
 * pfe.h — C-ABI of libpfe.so, the MI355X (gfx950) batched pulsar-candidate feature engine.
 *
 * This is the drop-in boundary for the per-candidate score path of
 * scienceguyrob/PulsarFeatureExtractor (ScoreGenerator.py).  The reference computes one
 * candidate at a time in Python; every entry point here is the BATCHED equivalent of one
 * reference interface, taking row-major candidate arrays (plain pointers + sizes, no
 * framework types) and writing one row of fp64 scores per candidate.
 *
 * Interfaces replaced (reference paths relative to PulsarFeatureExtractor/src/):
 *   pfe_lyon8_u8   <- PHCXFile.computeProfileStatScores          PHCXFile.py:320-349
 *                     + PHCXFile.computeDMCurveStatScores         PHCXFile.py:351-379
 *                     (concatenated as in DataProcessor.dmprof    DataProcessor.py:884-886;
 *                      SUPERBPHCXFile.py has identical bodies at the same lines)
 *   pfe_lyon8_f64  <- the same two functions on float profiles (PFDFile.py:522-583)
 *   pfe_bates22    <- PHCXFile.compute                            PHCXFile.py:383-409
 *                     (score groups 1-4 :413, 5-11 :475, 12-15 :547, 16-19 :589, 20-22 :633)
 *   Every call that takes float arrays has an _f64 form (doubles) and an _f32 form (floats read
 *   where they lie, the bits of the _f64 form on the widened values): see the end of this file.
 *
 * Conventions
 *   - One handle per (device, stream).  Calls on one handle are serialised by the caller;
 *     different handles may be used concurrently from different threads.
 *   - Caller owns all input/output buffers.  With PFE_FLAG_DEVICE_PTRS the pointers are
 *     device (HBM) pointers and the call is asynchronous on the handle's stream (no host
 *     sync); without it they are host pointers and the library stages them through
 *     per-handle device scratch, returning when the outputs are back on the host.
 *   - The 22-score calls run their independent score groups on two side streams the handle
 *     owns; they start after the work already queued on the handle's stream and are joined
 *     back into it (events) before the call returns, so callers only ever see one stream.
 *   - Raw IEEE values are returned (NaN/inf included).  NaN/inf -> "0" replacement is the
 *     writer's job, as in DataProcessor.storeScore (DataProcessor.py:321-325).
 *   - Return value: 0 = OK, otherwise a PFE_E* code; the text is in pfe_last_error().
 *   - There is NO CPU backend: pfe_create(-1, ...) fails.  The CPU restatement used for
 *     parity testing lives in oracle/ and is not part of this library.
 */
#ifndef PFE_H_
#define PFE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFE_ABI_VERSION 1

/* return codes */
#define PFE_OK 0
#define PFE_EINVAL 1   /* bad argument (null pointer, negative size, unsupported layout) */
#define PFE_EDEVICE 2  /* HIP runtime failure (allocation, launch, copy) */
#define PFE_ENODEV 3   /* no such device / no GPU present */

/* flags */
#define PFE_FLAG_DEVICE_PTRS 0x1u /* all array arguments are device pointers */
/* PFE_FLAG_PFD_AVGPROF 0x2u: the PFD calls only; defined with pfe_pfd_avgprof below */
/* PFE_FLAG_PFD_BSWAP 0x4u: the f64 and _i16 PFD calls only; defined with pfe_pfd_avgprof below */

/* Per-candidate status bits (pfe_bates22).  A non-zero status means the reference would
 * have raised inside Candidate.calculateScores and DataProcessor would have logged the
 * candidate to CandidateErrorLog.txt and dropped its row (DataProcessor.py:517-523). */
#define PFE_ST_SINE_FAIL      0x001u /* scores 1-4 raised            (PHCXFile.py:467-470) */
#define PFE_ST_GAUSS_FAIL     0x002u /* scores 5-11 raised           (PHCXFile.py:540-543) */
#define PFE_ST_DMFIT_FAIL     0x004u /* scores 16-19 raised          (PHCXFile.py:626-629) */
#define PFE_ST_SUBBAND_FAIL   0x008u /* scores 20-22 raised          (PHCXFile.py:665-668) */
#define PFE_ST_UNSUPPORTED    0x010u /* outside the shapes this build scores (a histogram with
                                        more than 16384 Freedman-Diaconis bins).  Unreachable
                                        for byte (PHCX) profiles of up to 32768 bins: their
                                        non-zero IQR is a multiple of 0.25, so the bin count
                                        is at most 510 n^(1/3); or, in pfe_bates22, a
                                        sub-band shape beyond nsub 65536 x nBins 16384 --
                                        the other groups' scores are still computed).  The
                                        row is not scored.  pfe_bates22 refuses the whole
                                        call (PFE_EINVAL) when nsub * nBins > 2^24 bytes
                                        per candidate, so the per-row mark is reached by
                                        nsub > 65536 with nBins < 256 or nBins > 16384
                                        with nsub < 1024 */
#define PFE_ST_DGF_INDEXERROR 0x100u /* informational: double-Gaussian IndexError path taken,
                                        s10=s11=1e6 (ProfileOperations.py:762-764) */
#define PFE_ST_FAIL_MASK      0x0FFu

typedef struct pfe_handle pfe_handle;

/* Query the ABI version compiled into the library. */
int pfe_abi_version(void);

/* Number of visible GPUs (0 when none); never fails. */
int pfe_device_count(void);

/* Create a handle bound to GPU `device` (>= 0) and its own non-blocking stream. */
int pfe_create(int device, pfe_handle** out);
void pfe_destroy(pfe_handle* h);

/* Text of the last error on this handle (or of the last failed pfe_create when h is NULL). */
const char* pfe_last_error(const pfe_handle* h);

/* Launch subsequent work on `hip_stream` (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL selects the HIP default (null) stream.  A new handle starts on its own non-blocking
 * stream.  The library never destroys a stream it did not create. */
int pfe_set_stream(pfe_handle* h, void* hip_stream);
/* Block until all work queued on the handle's stream has finished. */
int pfe_synchronize(pfe_handle* h);

/* ---------------------------------------------------------------------------------------
 * Handle options (A/B and verification switches).  The defaults are the product
 * configuration; the library never reads the process environment, so only an explicit
 * pfe_set_option changes what a handle computes.  Options marked (bits) change the last
 * bits of the LM-fitted scores (the m-sums are ordered differently); all others give
 * identical results and only change the schedule.
 *   PFE_OPT_SOLVER       (bits) LM solver of the 22-score kernels: PFE_SOLVER_POOLED
 *                        (default; pooled group engine for <= 256 bins -- 16-lane groups up
 *                        to 128 bins, 32-lane groups above -- batched beyond),
 *                        PFE_SOLVER_BATCHED (one wave owns 32 fits), or
 *                        PFE_SOLVER_WAVE (one wave per fit; bit-identical to BATCHED)
 *   PFE_OPT_SERIAL       1: the independent score groups run in order on the handle's
 *                        stream instead of on its two side streams (default 0)
 *   PFE_OPT_HANDOVER     0: re-evaluate the residuals after an accepted LM step instead of
 *                        handing the trial's residuals over (default 1)
 *   PFE_OPT_GSLOTS       fit slots per pooled wave, 1..32 (0 = sized from n; default 0)
 *   PFE_OPT_LYON8_BLOCKS grid cap of the Lyon-8 kernels (default 131072)
 *   PFE_OPT_LYON8_BURST  candidate groups per wave step of the Lyon-8 kernel: 1, 2 or 4
 *                        (default 2)
 *   PFE_OPT_PFD_WAVES    waves per fold of the PFD preprocessing kernel: 4 (default) or 1
 *   PFE_OPT_LYON8_DM     Lyon-8 kernel for DataBlock-length DM rows (PHCX nDM x 128 bytes):
 *                        0 = lyon8_u8_dm, skew / kurt from fp64 d^3 / d^4 sums (default);
 *                        1 = the round-3 kernels; 2 = lyon8_u8_dm with exact integer power
 *                        sums.  Mean and std are numpy's bits with every option; skew / kurt
 *                        may differ in the last bits
 *   PFE_OPT_PFD_SPLIT    PFD preprocessing: 1 = the folds' part sums streamed by their own kernel
 *                        on a side stream while the sweep kernel works on the previous chunk,
 *                        0 = one fused kernel (default; same bits)
 *   PFE_OPT_LYON8_DM_SPLIT  1 (default): the last numpy chunk of a DataBlock row with <= 32
 *                        leaves is summed by 2, 4 or 8 lanes per leaf, each taking some of the
 *                        leaf's 8 chains (the tri form's 128-byte leaves over the idle lane of
 *                        their quad), and one-chunk rows of 17-32 leaves are taken two per
 *                        wave; 2: the chain splits only; 0: one lane per leaf.  Mean and std
 *                        the same bits with every value, skew / kurt within 1e-12
 *   PFE_OPT_PFD_GLOBAL   PFD preprocessing: 0 (default) = folds whose sub-band profiles fit the
 *                        LDS stay on chip and every other shape goes through global scratch of
 *                        the handle; 1 = every shape through global scratch (same bits)
 *   PFE_OPT_SUBF64_GLOBAL  pfe_subband3_f64 / pfe_bates22_f64: 0 (default) = candidates whose
 *                        sub-bands fit the LDS stay on chip and every other shape goes through
 *                        per-wave slabs of the handle's scratch; 1 = every shape through the
 *                        slabs (same bits)
 *   PFE_OPT_PFD_F32_CHUNK  the pfe_pfd_*_f32 calls, and the f64 PFD calls under
 *                        PFE_FLAG_PFD_BSWAP: folds per pass, >= 0.  0 (default) = as many
 *                        folds as keep a pass's part sums (nsub x proflen doubles a fold)
 *                        within 1 GiB; a larger value is cut to that, and to n (same bits)
 *   PFE_OPT_PFD_SCRUNCH_DIRECT  the pfe_pfd_scrunch calls: 0 (default) = folds whose rows fit the
 *                        LDS are summed there and every other shape takes one lane per output
 *                        bin; 1 = every shape one lane per output bin (same bits)
 * Returns PFE_EINVAL for an unknown option or an out-of-range value.
 * --------------------------------------------------------------------------------------- */
#define PFE_OPT_SOLVER 1
#define PFE_OPT_SERIAL 2
#define PFE_OPT_HANDOVER 3
#define PFE_OPT_GSLOTS 4
#define PFE_OPT_LYON8_BLOCKS 5
#define PFE_OPT_LYON8_BURST 6
#define PFE_OPT_PFD_WAVES 7
#define PFE_OPT_LYON8_DM 8
#define PFE_OPT_PFD_SPLIT 9
#define PFE_OPT_LYON8_DM_SPLIT 10
#define PFE_OPT_PFD_GLOBAL 11
#define PFE_OPT_SUBF64_GLOBAL 12
#define PFE_OPT_PFD_F32_CHUNK 13
#define PFE_OPT_PFD_SCRUNCH_DIRECT 14
#define PFE_SOLVER_POOLED 0
#define PFE_SOLVER_BATCHED 1
#define PFE_SOLVER_WAVE 2
int pfe_set_option(pfe_handle* h, int32_t option, int64_t value);
int pfe_get_option(const pfe_handle* h, int32_t option, int64_t* value);

/* Pinned (page-locked) host memory.  Host-pointer calls DMA pinned caller buffers in place
 * (chunked, with the copies of one chunk overlapping the kernel of another); pageable
 * buffers are staged through the handle's own pinned ring by the calling thread.  A
 * producer that writes candidate rows straight into pfe_host_alloc memory (e.g.
 * pfe_phcx_pack) therefore skips that staging copy.  Not tied to a handle. */
int pfe_host_alloc(size_t bytes, void** out);
void pfe_host_free(void* p);

/* ---------------------------------------------------------------------------------------
 * 8 Lyon features.
 *   prof : n rows of lp uint8 bins (PHCX 02X-decoded profile), row r at prof + r*prof_stride
 *   dm   : n rows of ld uint8 values (PHCX DataBlock of section 0), row r at dm + r*dm_stride
 *   out  : n x 8 fp64, row-major, per candidate
 *          [prof_mean, prof_std, prof_skew, prof_kurt, dm_mean, dm_std, dm_skew, dm_kurt]
 *          std is ddof=0; skew is the biased g1 and kurt the biased Fisher g2 of
 *          scipy.stats; both are NaN when the row has zero variance (scipy >= 1.9).
 *   status : may be NULL; set to 0 for every row (the 8-feature path has no failure mode).
 * Requires lp >= 1, ld >= 1, strides >= row lengths.
 * --------------------------------------------------------------------------------------- */
int pfe_lyon8_u8(pfe_handle* h, const uint8_t* prof, int64_t prof_stride, int32_t lp,
                 const uint8_t* dm, int64_t dm_stride, int32_t ld, int64_t n, double* out,
                 uint32_t* status, uint32_t flags);

/* Same with fp64 rows (PFD profiles are float; PFDFile.py:522-583).  Two-pass fp64 moments
 * summed in numpy's own order (8-accumulator leaves of <= 128 values, pairwise splits at
 * floor8(n/2), rows longer than 8192 values in buffers of 8192), so for rows of any length,
 * stride and 8-byte alignment:
 *   mean, std, kurt (columns 0, 1, 3, 4, 5, 7) : the bits of numpy.mean, numpy.std and
 *          scipy.stats.kurtosis evaluated as m4 / (m2 * m2) - 3, infinities included;
 *   skew (columns 2, 6) : m3 / pow(m2, 1.5) with the device's pow, within 1e-13 relative of
 *          scipy.stats.skew;
 *   NaN exactly where scipy gives NaN: non-finite rows, and zero variance by scipy's rule
 *          m2 <= (eps * mean)^2 -- a constant row of a value whose sum rounds is not always
 *          one (numpy's mean may land an ulp off the value; scipy then returns skew = +-1,
 *          kurt = -2, and so does this call). */
int pfe_lyon8_f64(pfe_handle* h, const double* prof, int64_t prof_stride, int32_t lp,
                  const double* dm, int64_t dm_stride, int32_t ld, int64_t n, double* out,
                  uint32_t* status, uint32_t flags);

/* ---------------------------------------------------------------------------------------
 * 22 Bates scores (PHCX / SUPERB PHCX).
 *   prof    : n x lp uint8 profile (Profile of the scored section)
 *   sub     : n x nsub x lsb uint8 sub-bands (SubBands of the scored section)
 *   dmcurve : n x ndm fp64 reduced DM curve (PHCXOperations.dm_curve of that section's
 *             DataBlock: max over the first 127 of every 128 values); point k sits at
 *             DM = dm_start + (128k - 1) * |dm_start - dm_end| / length_all  (:196)
 *   scal    : n x PFE_NSCAL fp64 per-candidate scalars (layout below)
 *   out     : n x 22 fp64 in reference score order (score 1 in column 0)
 *   status  : n x uint32 PFE_ST_* bits (required)
 * Strides are in elements and equal the row length (dense rows).
 * --------------------------------------------------------------------------------------- */
#define PFE_NSCAL 8
#define PFE_SCAL_PERIOD_MS 0 /* BaryPeriod * 1000            (PHCXOperations.py:109) */
#define PFE_SCAL_SNR 1       /* Snr                            (:107) */
#define PFE_SCAL_DM 2        /* Dm                             (:108) */
#define PFE_SCAL_WIDTH 3     /* Width                          (:110) */
#define PFE_SCAL_DM_START 4  /* float(DmIndex token[1])        (:172-182) */
#define PFE_SCAL_DM_END 5    /* float(DmIndex last token)      (:182) */
#define PFE_SCAL_LENGTH_ALL 6 /* len(decoded DataBlock)        (:168) */
#define PFE_SCAL_RESERVED 7

typedef struct pfe_bates_in {
  const uint8_t* prof;  /* n x lp */
  int32_t lp;
  const uint8_t* sub;   /* n x nsub x lsb */
  int32_t nsub;
  int32_t lsb;
  const double* dmcurve; /* n x ndm */
  int32_t ndm;
  const double* scal;   /* n x PFE_NSCAL */
  int64_t n;
} pfe_bates_in;

int pfe_bates22(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                uint32_t flags);

/* Sub-band scores alone (scores 20-22):
 *   pfe_subband3 <- PHCXOperations.getSubbandParameters          PHCXOperations.py:305-349
 *                   (getSubband_scores ProfileOperations.py:1585-1686, getProfileCorr
 *                    PHCXOperations.py:387-415)
 * Reads prof, sub and scal[PFE_SCAL_WIDTH] of `in` (dmcurve/ndm are ignored and may be
 * NULL/0); out = n x 3 fp64 [RMS of sub-band peak positions, mean pairwise correlation,
 * sum of profile correlations > 0.0055]; status bits PFE_ST_SUBBAND_FAIL where the
 * reference raises (boxcar width <= 0 or > nBins, every pair NaN, lp != lsb).
 * Any nsub in [1, 65536] and lsb in [1, 16384] (lp up to 16384 here): nsub 2-256 with
 * nsub * (lsb + 1) <= 32768 on chip, every other shape through global scratch of the handle. */
int pfe_subband3(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                 uint32_t flags);

/* One score group of the chain alone: the batched form of one method of the reference's
 * second plug-in class, ProfileOperationsInterface (ProfileOperationsInterface.py:69-130),
 * as PHCXOperations implements it.  `in` as for pfe_bates22, but only the arrays a group
 * reads are used (the others may be NULL / 0); the same kernels, so every value is the bits
 * the group's columns of pfe_bates22 hold; status carries that group's failure bit only.
 *   pfe_sinusoid4 <- getSinusoidFittings(profile)        ProfileOperations.py:190-376
 *                    reads prof; out n x 4 = s1-s4 (pfe_bates22 columns 0-3)
 *   pfe_gauss7    <- getGaussianFittings(profile)        ProfileOperations.py:595-770
 *                    reads prof; out n x 7 = s5-s11 (columns 4-10)
 *   pfe_params4   <- getCandidateParameters(data, sec)   PHCXOperations.py:81-112
 *                    reads scal; out n x 4 = [period_ms, snr, dm, width] as the method
 *                    returns them (PHCXFile applies filterScore(13/14) for s13/s14)
 *   pfe_dmfit4    <- getDMFittings(data, sec)            PHCXOperations.py:121-233
 *                    reads dmcurve, scal; out n x 4 = [peak, |1 - Prop|, Shift, chi_theo]:
 *                    the method's signed Shift (s18 = filterScore(18, Shift) = |Shift|) */
int pfe_sinusoid4(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                  uint32_t flags);
int pfe_gauss7(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
               uint32_t flags);
int pfe_params4(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                uint32_t flags);
int pfe_dmfit4(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
               uint32_t flags);

/* The two profile groups on float profiles: the batched form of getSinusoidFittings /
 * getGaussianFittings on the 0..255 float profile PFDFile hands them (PFDFile.py:658, :725).
 *   prof : n dense rows of lp fp64 bins (8 <= lp <= 1024), host or device as the flags say
 *   out  : n x 4 = s1-s4 (pfe_sinusoid4_f64) / n x 7 = s5-s11 (pfe_gauss7_f64)
 * The kernels are those pfe_pfd_bates22 runs on its profile, so with `prof` the profile
 * pfe_pfd_dmprof returns for a fold the values are the bits of columns 0-3 / 4-10 of
 * pfe_pfd_bates22.  Status, pointers and scratch as pfe_sinusoid4 / pfe_gauss7. */
int pfe_sinusoid4_f64(pfe_handle* h, const double* prof, int32_t lp, int64_t n, double* out,
                      uint32_t* status, uint32_t flags);
int pfe_gauss7_f64(pfe_handle* h, const double* prof, int32_t lp, int64_t n, double* out,
                   uint32_t* status, uint32_t flags);

/* A folded candidate held as float arrays (another fold format, normalised or baseline-
 * subtracted PHCX data, the dedispersed sub-bands of a fold): the sub-band scores and the
 * whole 22-score vector.
 *   prof    : n x lp fp64 profile
 *   sub     : n x nsub x lsb fp64 sub-bands
 *   dmcurve : n x ndm fp64 reduced DM curve, as for pfe_bates22
 *   scal    : n x PFE_NSCAL fp64, as for pfe_bates22
 * Dense rows, 8-byte aligned; host or device pointers as the flags say.  `sub` is never
 * written: a candidate is scored on a copy (its own LDS partition or scratch slab).
 *
 *   pfe_subband3_f64 <- PHCXOperations.getSubbandParameters        PHCXOperations.py:305-349
 *                       (getSubband_scores ProfileOperations.py:1585-1686, getProfileCorr
 *                        PHCXOperations.py:387-415) on float arrays, with the arithmetic of
 *                       PFDOperations.getSubbandParameters (PFDOperations.py:401-466)
 * Reads prof, sub and scal[PFE_SCAL_WIDTH] (dmcurve / ndm are ignored and may be NULL / 0);
 * out = n x 3 fp64 [s20, s21, s22]: boxcar sums of wb = ceil(width * lsb) bins added left to
 * right from 0 (:1608-1617), each band's first strict maximum above -10000.0 with max_bin
 * carried across the bands (:1619-1628), the RMS rule (:1629-1651), the mean of the pair
 * correlations that are not NaN (:1653-1677) and the sum of |corrcoef(band, profile)| >
 * 0.0055.  s20 holds the reference's bits, s21 and s22 are within 1e-12 relative (numpy's dots
 * run in BLAS order).  status = PFE_ST_SUBBAND_FAIL, and out = 0, where the reference raises:
 * no window (wb > lsb), wb <= 0, a NaN or infinite width, no valid pair, nsub == 1,
 * lp != lsb.
 * Shapes: nsub >= 1, lsb >= 1 and lp >= 1 with the per-candidate vectors
 *   (2 * lsb + 3 * nsub) * 8 bytes, rounded up to 16,  <=  163840 bytes (160 KiB of LDS),
 * so every nsub <= 1024 with lsb <= 2048; beyond that PFE_EINVAL.  A candidate whose
 * nsub * lsb doubles (rounded up to 16 bytes) fit the LDS beside those vectors is scored on
 * chip, several waves to a block; every other shape, and every shape under
 * PFE_OPT_SUBF64_GLOBAL = 1, in a per-wave slab of the handle's scratch (at most 1 GiB of
 * slabs), with the same bits.
 *
 *   pfe_bates22_f64  <- PHCXFile.compute                           PHCXFile.py:383-409
 * out = n x 22: columns 0-3 the bits of pfe_sinusoid4_f64(prof), 4-10 of pfe_gauss7_f64(prof),
 * 11-14 pfe_params4 with filterScore(13/14) applied as pfe_bates22 applies it, 15-18
 * pfe_dmfit4 with s18 = |Shift|, 19-21 the bits of pfe_subband3_f64; status the OR of the
 * groups' bits.  8 <= lp <= 1024 and 3 <= ndm <= 1024 (the fits), the sub-band shapes above.
 * The groups run on the handle's side streams (PFE_OPT_SERIAL, PFE_OPT_SOLVER as for
 * pfe_bates22) and are joined before the call returns. */
typedef struct pfe_bates_f64_in {
  const double* prof;    /* n x lp */
  int32_t lp;
  const double* sub;     /* n x nsub x lsb */
  int32_t nsub;
  int32_t lsb;
  const double* dmcurve; /* n x ndm */
  int32_t ndm;
  const double* scal;    /* n x PFE_NSCAL */
  int64_t n;
} pfe_bates_f64_in;

int pfe_subband3_f64(pfe_handle* h, const pfe_bates_f64_in* in, double* out, uint32_t* status,
                     uint32_t flags);
int pfe_bates22_f64(pfe_handle* h, const pfe_bates_f64_in* in, double* out, uint32_t* status,
                    uint32_t flags);

/* ---- PFD (PRESTO fold) files: preprocessing + Lyon features -------------------------
 * pfe_pfd_dmprof <- what a freshly loaded PFDFile computes for the dmprof path
 *   dedisperse (PFDFile.py:330-374) at the best DM, getprofile + scale (:256-310),
 *   plot_chi2_vs_DM(dms[0], dms[-1]) (:378-423, 100 DMs, float32),
 *   computeProfileStatScores (:522-551) and computeDMCurveStatScores (:553-583).
 * Inputs per candidate: the fold's sub-integration profiles profs[npart][nsub][proflen],
 * the sub-band centre frequencies (PFDFile.py:222-226) and the scalars below (from the
 * file header: best DM, fold_p1 * proflen, (profs/proflen).sum() of the file as read,
 * the summed prof_var foldstats, dms[0], dms[-1] and numdms).
 * Outputs (each may be NULL): profile[n][proflen] (0..255 fp64, also the --profile bins of
 * PFDFile.computeProfileScores :479-492), chis[n][PFE_PFD_NDM] (the float32 DM curve),
 * lyon8[n][8] = [profile mean, std, skew, kurt, DM-curve mean, std, skew, kurt].
 * status[i] = PFE_ST_PFD_DMCURVE_FAIL when numdms == 1 (the reference raises on dms[0]).
 * Any npart >= 1, nsub >= 1 and proflen >= 2 with 6 * proflen + 3.5 * nsub doubles of per-fold
 * vectors within the 160 KiB of LDS (so every nsub <= 1024 with proflen <= 2048): a fold
 * whose nsub x proflen sub-band profiles fit the LDS as well (about nsub * proflen <= 20000)
 * is kept on chip, every other shape in global scratch of the handle (up to 1 GiB).  Beyond
 * that, and for proflen > 65535, PFE_EINVAL. */
#define PFE_PFD_NSCAL 8
#define PFE_PFD_BESTDM 0
#define PFE_PFD_BINSPERSEC 1
#define PFE_PFD_AVGPROF 2
#define PFE_PFD_VARPROF 3
#define PFE_PFD_DM_LO 4
#define PFE_PFD_DM_HI 5
#define PFE_PFD_NUMDMS 6
#define PFE_PFD_BARY_P1 7 /* bary_p1 (s; the 22-score path: period = bary_p1 * 1000) */
#define PFE_PFD_NDM 100
#define PFE_ST_PFD_DMCURVE_FAIL 0x020u

typedef struct pfe_pfd_in {
  const double* profs;    /* n x npart x nsub x proflen */
  const double* subfreqs; /* n x nsub */
  const double* scal;     /* n x PFE_PFD_NSCAL */
  int32_t npart, nsub, proflen;
  int64_t n;
} pfe_pfd_in;

int pfe_pfd_dmprof(pfe_handle* h, const pfe_pfd_in* in, double* profile, float* chis,
                   double* lyon8, uint32_t* status, uint32_t flags);

/* pfe_pfd_bates22 <- PFDFile.compute (PFDFile.py:587-613): the 22 scores of each fold in the
 * reference's order -- ProfileOperations' sinusoid and Gaussian fits on the 0..255 float
 * profile (s1-s11), PFDOperations.getCandidateParameters (s12-s15, PFDOperations.py:93-233),
 * getDMFittings (s16-s19, the clamped 4-parameter fit to the chi^2-vs-DM curve, :274-393) and
 * getSubbandParameters over the dedispersed sub-band profiles (s20-s22, :401-466).
 * Same inputs as pfe_pfd_dmprof (scal[PFE_PFD_BARY_P1] is used); out[n][22]; status bits as
 * pfe_bates22 (PFE_ST_DMFIT_FAIL when numdms == 1).  nsub >= 2 and 8 <= proflen <= 1024 (the
 * fits); within those, the shapes of pfe_pfd_dmprof (so every nsub <= 1024). */
int pfe_pfd_bates22(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                    uint32_t flags);

/* One score group of a fold alone: the batched form of one method of PFDOperations.  Inputs,
 * shape limits and PFE_EINVAL texts as pfe_pfd_bates22; the same kernels doing only the
 * group's work, so every value is the bits of the group's columns of pfe_pfd_bates22, and
 * status carries that group's failure bit only.
 *   pfe_pfd_params4  <- getCandidateParameters(data)      PFDOperations.py:93-233
 *                       out n x 4 = [period_ms, snr, dm, width] as the method returns them
 *                       (PFDFile applies filterScore(13/14) for s13/s14); status 0.  No
 *                       chi^2 sweep, no sub-band scores.
 *   pfe_pfd_dmfit4   <- getDMFittings(data)               PFDOperations.py:274-393
 *                       out n x 4 = [s16, s17, Shift, s19]: the method's signed Shift
 *                       (s18 = |Shift|); PFE_ST_DMFIT_FAIL.  The sweep, the parameters the
 *                       fit reads and the fit of PFE_OPT_SOLVER; no sub-band scores, no
 *                       sine or Gaussian fit.
 *   pfe_pfd_subband3 <- getSubbandParameters(data)        PFDOperations.py:401-466
 *                       out n x 3 = s20-s22 (with the fold's own width);
 *                       PFE_ST_SUBBAND_FAIL.  No sweep. */
int pfe_pfd_params4(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                    uint32_t flags);
int pfe_pfd_dmfit4(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                   uint32_t flags);
int pfe_pfd_subband3(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                     uint32_t flags);

/* ---- float32 folds: the five PFD calls on a cube of floats ----------------------------
 * A fold that never was a .pfd file (PRESTO writes doubles) -- the output of a GPU folder, a
 * float32 tensor -- is scored where it is: the cube is read once, as the 4-byte values it
 * holds, and never widened in memory, on the host or on the device.
 *
 * Contract: the result of an _f32 call is, bit for bit, the result of the f64 call of the
 * same name on the same cube widened value by value ((double)x, exact), with the same
 * subfreqs and scal.  Nothing is accumulated in float32: every fold's parts are summed in
 * fp64, S[e] = (double)X[0][e] + (double)X[1][e] + ... + (double)X[npart-1][e], in that order
 * from the value of part 0 -- the order the f64 kernels sum the parts of an element in --
 * and the f64 kernels run on S as folds of one part.  This is NOT numpy.sum of a float32
 * array, which accumulates in float32: compare with profs.astype(numpy.float64) scored by the
 * f64 call, or summed in fp64.  The header scalars (PFE_PFD_AVGPROF, PFE_PFD_VARPROF and the
 * others) stay fp64 and stay the caller's to supply -- but for PFE_PFD_AVGPROF, which
 * PFE_FLAG_PFD_AVGPROF (below) derives from the floats on the device.
 *
 * Shape limits, PFE_EINVAL texts, status bits, stream behaviour, PFE_FLAG_DEVICE_PTRS and
 * the routing options (PFE_OPT_PFD_WAVES, _SPLIT, _GLOBAL) are those of the f64 call of the
 * same name; profs must be 4-byte aligned (16-byte aligned with nsub x proflen a multiple
 * of 4 takes the 16-byte loads; same bits either way).
 * Scratch: a call runs in passes of `chunk` folds -- chunk = min(n, max(1, 2^30 / (8 x nsub x
 * proflen))), or PFE_OPT_PFD_F32_CHUNK when that is smaller -- and takes, behind the arrays a
 * host-pointer call stages (the cube as n x npart x nsub x proflen floats: half the bytes of
 * the f64 call over the bus), chunk x nsub x proflen doubles of part sums, then the scratch of
 * the f64 call on `chunk` folds. */
typedef struct pfe_pfd_f32_in {
  const float* profs;     /* n x npart x nsub x proflen, dense, 4-byte aligned */
  const double* subfreqs; /* n x nsub */
  const double* scal;     /* n x PFE_PFD_NSCAL */
  int32_t npart, nsub, proflen;
  int64_t n;
} pfe_pfd_f32_in;

int pfe_pfd_dmprof_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* profile, float* chis,
                       double* lyon8, uint32_t* status, uint32_t flags);
int pfe_pfd_bates22_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                        uint32_t flags);
int pfe_pfd_params4_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                        uint32_t flags);
int pfe_pfd_dmfit4_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                       uint32_t flags);
int pfe_pfd_subband3_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                         uint32_t flags);

/* ---- a fold's average, derived where the cube is ---------------------------------------
 * scal[PFE_PFD_AVGPROF] is the one per-fold input that is a function of the cube alone:
 * PFDFile.load's self.avgprof = (self.profs / self.proflen).sum() (PFDFile.py:225), which the
 * chi^2-vs-DM sweep subtracts from every bin (calc_redchi2, :427-438).  A fold that is already
 * on the device -- or a cube the caller does not want to pass over twice on the host -- gets
 * it here, with numpy's bits.
 *
 * Contract: out[i * out_stride] is, bit for bit, numpy's (x / proflen).sum() of fold i's
 * E = npart x nsub x proflen values x in memory order (float64; a float32 cube widened value
 * by value first, profs.astype(numpy.float64): nothing is divided or added in float32):
 *   y[e] = (double)x[e] / (double)proflen, the correctly rounded fp64 quotient (a power-of-two
 *          proflen scales by its exact reciprocal: the same bits);
 *   c[k] = numpy's pairwise sum of y[8192 k .. 8192 k + 8191] (the last chunk shorter): n < 8
 *          values 0.0 + y0 + y1 ..., n <= 128 in eight accumulators r[t] = y[t] + y[t + 8] +
 *          ... combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 last in order,
 *          more than 128 split at floor8(n / 2);
 *   out  = 0.0 + c[0] + c[1] + c[2] + ..., in order onto numpy's initial 0.0 (which shows in
 *          one case: a fold whose values are all -0.0 gives +0.0, whatever its size).
 * This is NOT one pairwise tree over the cube, and not torch.sum.  inf, NaN, subnormal
 * quotients and overflow come out as numpy's.
 *
 * Any npart >= 1, nsub >= 1 and proflen >= 2: the call only streams the cube, so it has no LDS
 * shape limit.  out_stride >= 1, in doubles: with out = &scal[PFE_PFD_AVGPROF] and out_stride =
 * PFE_PFD_NSCAL the values land in the scal array of a PFD call and nothing else of it is
 * written.  PFE_EINVAL for a null array, a negative size, out_stride < 1 or a float cube that
 * is not 4-byte aligned.  Stream behaviour and PFE_FLAG_DEVICE_PTRS as the PFD calls; a
 * host-pointer call stages the cube in the handle's scratch.  Scratch: n x ceil(E / 8192)
 * doubles of chunk sums behind what a host-pointer call stages.
 *
 * PFE_FLAG_PFD_AVGPROF, on any of the ten PFD calls (f64 and _f32): scal[i][PFE_PFD_AVGPROF]
 * is not read; the call uses what pfe_pfd_avgprof gives for the cube as the call holds it on
 * the device -- a host-pointer call derives it from the copy it staged (the cube crosses the
 * bus once), a float32 call pass by pass (PFE_OPT_PFD_F32_CHUNK) from the floats -- written
 * into a scratch copy of scal that the kernels then read.  The caller's scal is never written
 * (a device-pointer call takes n x PFE_PFD_NSCAL doubles of scratch for the copy).  Every
 * output is the bits of the unflagged call given that value.  pfe_pfd_params4, pfe_pfd_subband3
 * and their _f32 forms do not read the average: they accept the flag and do no extra work.
 * Without the flag every call does what it did before. */
#define PFE_FLAG_PFD_AVGPROF 0x2u /* PFD calls: derive scal[PFE_PFD_AVGPROF] from the cube */

/* ---- cubes in the opposite byte order ----------------------------------------------------
 * A .pfd file written on a big-endian machine holds every double of its cube byte-reversed.
 * PFE_FLAG_PFD_BSWAP, on the five f64 PFD calls (pfe_pfd_dmprof, _bates22, _params4, _dmfit4,
 * _subband3) and on pfe_pfd_avgprof: profs holds 8-byte values whose bytes are reversed, as
 * such a file holds them; the file's cube bytes go to the device untouched (pfe_pfd_pack,
 * pfe_io.h) and the byte order is dealt with where each value is loaded.  subfreqs, scal and
 * every output stay native.
 *
 * Contract: every output of a flagged call is, bit for bit, the output of the unflagged call on
 * the cube with every 8-byte value byte-reversed (numpy's cube.byteswap()), with the same
 * subfreqs, scal, options and other flags.  NaN payloads, signed zeros, infinities and
 * subnormals are carried through.  Nothing in memory is rewritten: the caller's cube is never
 * written to, and no swapped copy of the whole cube is made.  One case is outside it: where
 * two NaNs of different payloads meet in the sum of one element's parts, the payload of the
 * earlier part survives here, while the unflagged call keeps the one its kernel's add holds in
 * its first operand (the later part's on the four-wave route, the earlier one's on the split
 * pipeline: the f64 routes do not agree among themselves).  The result is a NaN either way.
 *
 * How: the float32 path with 8-byte words.  A part-sum kernel reads the raw words, reverses
 * them in registers and forms S[e] = X[0][e] + X[1][e] + ... + X[npart-1][e] in fp64, from the
 * value of part 0, in the order the f64 kernels sum the parts of an element in; the f64 kernels
 * run on S as folds of one part.  16-byte loads when nsub x proflen is even and profs is
 * 16-byte aligned, 8-byte loads otherwise (profs 8-byte aligned as ever); same bits.  The
 * average (pfe_pfd_avgprof, and PFE_FLAG_PFD_AVGPROF together with this flag, pass by pass) is
 * taken by the same kernels with each word widened to double through the reversal.
 * Scratch: passes of `chunk` folds by the rule of the float32 calls -- chunk = min(n, max(1,
 * 2^30 / (8 x nsub x proflen))), or PFE_OPT_PFD_F32_CHUNK when that is smaller (the option
 * governs both paths) -- and, behind the arrays a host-pointer call stages (the cube as the
 * words it holds), chunk x nsub x proflen doubles of part sums, then the scratch of the f64
 * call on `chunk` folds.
 * The _f32 calls refuse the flag with PFE_EINVAL.  Without the flag nothing changes. */
#define PFE_FLAG_PFD_BSWAP 0x4u /* f64 PFD calls: profs holds byte-reversed 8-byte values */

int pfe_pfd_avgprof(pfe_handle* h, const double* profs, int32_t npart, int32_t nsub,
                    int32_t proflen, int64_t n, double* out, int64_t out_stride, uint32_t flags);
int pfe_pfd_avgprof_f32(pfe_handle* h, const float* profs, int32_t npart, int32_t nsub,
                        int32_t proflen, int64_t n, double* out, int64_t out_stride,
                        uint32_t flags);

/* ---- int16 folds: the five PFD calls on scaled 16-bit values ----------------------------
 * The most common fold that never was a .pfd file is a fold-mode archive: PSRFITS (dspsr,
 * PulsarX, every psrchive-based pipeline) keeps a fold as 16-bit integers d with, per
 * sub-integration x channel, a float32 scale, offset and weight -- a bin's value is d * scl +
 * offs, a channel of weight 0 is a zapped one -- big-endian, one row of a binary table per
 * sub-integration.  The _i16 calls score such a fold where it is: the cube is read once, as the
 * 2-byte values it holds, decoded in registers and never widened in memory, and the inputs may
 * be the raw rows of an uploaded table, read through two byte strides.
 *
 * Contract: every output and the status of an _i16 call is, bit for bit, that of the f64 call
 * of the same name on the cube
 *   x[p][s][b] = ((double)d[p][s][b] * (double)scl[p][s] + (double)offs[p][s])   [ * (double)wts[p][s] ]
 * evaluated in fp64, with the same subfreqs, scal, options and other flags.  The product
 * (double)d * (double)scl is exact (16 bits times a 24-bit significand, and no float32 exponent
 * over- or underflows fp64), so the decode rounds once, at + offs (a fused multiply-add gives
 * the same bits); the multiply by the weight rounds once more, before the value is added to
 * anything.  wts == NULL: no multiply at all (not a multiply by 1.0).  In
 * numpy: d.astype(f8) * scl.astype(f8)[..., None] + offs.astype(f8)[..., None], then
 * * wts.astype(f8)[..., None].  The parts of an element are summed in fp64, S[s][b] = x[0][s][b]
 * + x[1][s][b] + ... + x[npart-1][s][b], in that order from the value of part 0, and the f64
 * kernels run on S as folds of one part (the float32 path).  A NaN is a NaN; which payload
 * survives is unspecified.  Nothing is computed in float32 or in integers, and the inputs are
 * never written.
 *
 * Strides, in bytes.  Both 0: the four arrays are dense, data n x npart x nsub x proflen and
 * scl, offs, wts n x npart x nsub.  Both non-zero: the four arrays lie in the same rows, one
 * table row per sub-integration, and share the two strides: value (i,p,s,b) of data is at
 * (char*)data + i*fold_stride + p*part_stride + 2*(s*proflen + b), value (i,p,s) of scl (offs,
 * wts) at (char*)scl + i*fold_stride + p*part_stride + 4*s.  For a PSRFITS SUBINT table
 * part_stride = NAXIS1 and the four pointers are the columns' addresses in row 0.  Required:
 * part_stride >= 2 x nsub x proflen and a multiple of 4; fold_stride a multiple of 4 and >=
 * npart x part_stride; data 2-byte aligned; scl, offs and wts 4-byte aligned.  Exactly one
 * stride non-zero, or any violation, is PFE_EINVAL with a text naming the rule.  Strided input
 * is for device pointers, where the table's bytes were uploaded as they are: non-zero strides
 * without PFE_FLAG_DEVICE_PTRS is PFE_EINVAL.  A host-pointer call takes dense arrays and stages
 * the cube as int16 (a quarter of the f64 call's bytes over the bus) and the parameters as
 * floats.  8-byte loads (four values) when nsub x proflen is a multiple of 4 and data is 8-byte
 * aligned at every part, 2-byte loads otherwise; same bits.
 *
 * PFE_FLAG_PFD_BSWAP on an _i16 call: data holds 2-byte values and scl, offs, wts 4-byte values
 * with their bytes reversed (the table as the file holds it); subfreqs, scal and every output
 * stay native.  Each value is reversed in registers where it is loaded; no swapped copy is made.
 *
 * pfe_pfd_avgprof_i16 (it reads the four arrays, the strides and the shape only) and
 * PFE_FLAG_PFD_AVGPROF on an _i16 call, pass by pass: numpy's (x / proflen).sum() of the decoded
 * cube x in memory order (p, s, b), by the rule of pfe_pfd_avgprof.
 *
 * Everything else -- shape limits, status bits, stream behaviour, the routing options -- is that
 * of the f64 call of the same name; PFE_EINVAL texts go under the _i16 name.
 * Scratch: passes of `chunk` folds by the rule of the float32 calls (PFE_OPT_PFD_F32_CHUNK
 * governs this path too): the arrays a host-pointer call stages (data as int16, then scl, offs
 * and, when given, wts as floats, then subfreqs, scal and the outputs), then chunk x nsub x
 * proflen doubles of part sums, then the scratch of the f64 call on `chunk` folds. */
typedef struct pfe_pfd_i16_in {
  const int16_t* data;    /* value (i,p,s,b) at (char*)data + i*fold_stride + p*part_stride + 2*(s*proflen + b) */
  const float* scl;       /* (i,p,s) at (char*)scl + i*fold_stride + p*part_stride + 4*s */
  const float* offs;      /* as scl */
  const float* wts;       /* as scl; NULL: no weights, no multiply */
  int64_t fold_stride;    /* bytes; 0 with part_stride 0 = every array dense */
  int64_t part_stride;    /* bytes */
  const double* subfreqs; /* n x nsub */
  const double* scal;     /* n x PFE_PFD_NSCAL */
  int32_t npart, nsub, proflen;
  int64_t n;
} pfe_pfd_i16_in;

int pfe_pfd_dmprof_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* profile, float* chis,
                       double* lyon8, uint32_t* status, uint32_t flags);
int pfe_pfd_bates22_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                        uint32_t flags);
int pfe_pfd_params4_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                        uint32_t flags);
int pfe_pfd_dmfit4_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                       uint32_t flags);
int pfe_pfd_subband3_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                         uint32_t flags);
int pfe_pfd_avgprof_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, int64_t out_stride,
                        uint32_t flags);

/* ---- kill masks: killed intervals and sub-bands of a fold --------------------------------
 * PRESTO's pfd class re-scores a fold after RFI excision with kill_intervals() and
 * kill_subbands() (show_pfd -killparts ... -killsubs ...): the rows of the cube are zeroed and
 * sumprof, avgprof and varprof recomputed.  The _kill calls score such a fold where it lies: the
 * cube is read once, as the values it holds, and a value of a killed part (sub-integration) or
 * sub-band is selected away where it is loaded.  No zapped copy of the cube is made.
 *
 * Contract: every output and the status of a _kill call is, bit for bit, that of the plain call
 * of the same name on the cube z, with the same subfreqs, scal, options and other flags.
 *   z[i][p][s][b] = (parts[i][p] || subs[i][s]) ? +0.0 : x[i][p][s][b]
 * is numpy's np.where(kill, 0.0, x).  A float32 cube is widened first.
 *
 * A killed value is replaced, never multiplied: a NaN, +-inf or a huge value in a killed row
 * reaches no sum.  This differs from PRESTO's `*= 0.0` only for non-finite values (NaN * 0 and
 * inf * 0 are NaN there) and for the sign of zero (a negative value times 0.0 is -0.0 there, +0.0
 * here).  The caller's cube and masks are never written.  A NaN that is not killed is a NaN;
 * which payload survives is unspecified, as for PFE_FLAG_PFD_BSWAP.  scal[PFE_PFD_AVGPROF] and
 * scal[PFE_PFD_VARPROF] stay the caller's: they must be those of the zapped fold.  With
 * PFE_FLAG_PFD_AVGPROF the average is derived from z: numpy's (z / proflen).sum() in memory
 * order, by the rule of pfe_pfd_avgprof -- the zeros sit where the killed values were, inside
 * the 8192-value chunks and the pairwise leaves.  pfe_pfd_avgprof_kill gives that value alone.
 *
 * Masks: parts n x npart and subs n x nsub bytes, dense, non-zero = killed; host or device
 * pointers as PFE_FLAG_DEVICE_PTRS says for every array.  kill == NULL, or both members NULL:
 * the call is the plain call -- the same kernels, the same scratch, the same bits.  One member
 * NULL: nothing of that kind is killed.  The f64 forms accept PFE_FLAG_PFD_BSWAP: the word is
 * reversed, then selected.  All forms accept PFE_FLAG_PFD_AVGPROF.  The parts of an element are
 * summed in fp64, S[s][b] = z[0][s][b] + z[1][s][b] + ... + z[npart-1][s][b], in that order from
 * the value of part 0, and the f64 kernels run on S as folds of one part (the float32 path).
 * A fold with every part or every sub-band killed is the zero cube.
 *
 * Everything else -- shape limits, status bits, stream behaviour, the routing options -- is that
 * of the plain call of the same name; PFE_EINVAL texts go under the _kill name.
 * Scratch: a masked call, f64 included, runs in passes of `chunk` folds by the rule of the
 * float32 calls (PFE_OPT_PFD_F32_CHUNK governs this path too): the arrays a host-pointer call
 * stages (the cube as the values it holds, subfreqs, scal, then directly behind scal parts and
 * subs, each only when given, then the outputs; pfe_pfd_avgprof_kill: the cube, parts, subs, the
 * n results), then chunk x nsub x proflen doubles of part sums, then the scratch of the f64 call
 * on `chunk` folds.
 *
 * There are no _i16 forms: an int16 cube carries a weight per (part, sub-band), and a weight of
 * 0 is the kill.  Not offered: per-element masks, and weights for float cubes. */
typedef struct pfe_pfd_kill {
  const uint8_t* parts; /* n x npart, non-zero = killed; NULL = none */
  const uint8_t* subs;  /* n x nsub,  non-zero = killed; NULL = none */
} pfe_pfd_kill;

int pfe_pfd_dmprof_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill,
                        double* profile, float* chis, double* lyon8, uint32_t* status,
                        uint32_t flags);
int pfe_pfd_bates22_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                         uint32_t* status, uint32_t flags);
int pfe_pfd_params4_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                         uint32_t* status, uint32_t flags);
int pfe_pfd_dmfit4_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                        uint32_t* status, uint32_t flags);
int pfe_pfd_subband3_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                          uint32_t* status, uint32_t flags);
int pfe_pfd_avgprof_kill(pfe_handle* h, const double* profs, int32_t npart, int32_t nsub,
                         int32_t proflen, int64_t n, const pfe_pfd_kill* kill, double* out,
                         int64_t out_stride, uint32_t flags);
int pfe_pfd_dmprof_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                            double* profile, float* chis, double* lyon8, uint32_t* status,
                            uint32_t flags);
int pfe_pfd_bates22_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                             double* out, uint32_t* status, uint32_t flags);
int pfe_pfd_params4_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                             double* out, uint32_t* status, uint32_t flags);
int pfe_pfd_dmfit4_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                            double* out, uint32_t* status, uint32_t flags);
int pfe_pfd_subband3_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                              double* out, uint32_t* status, uint32_t flags);
int pfe_pfd_avgprof_kill_f32(pfe_handle* h, const float* profs, int32_t npart, int32_t nsub,
                             int32_t proflen, int64_t n, const pfe_pfd_kill* kill, double* out,
                             int64_t out_stride, uint32_t flags);

/* ---- scrunching a fold: channels to sub-bands, bins to fewer bins -------------------------
 * prepfold writes 16-128 sub-bands of 64-256 bins, dedispersed at the fold DM inside each
 * sub-band.  A fold-mode archive holds every channel (512-4096), often 512-2048 bins, and
 * nothing inside a group of channels is dedispersed: pfe_pfd_bates22 refuses its proflen, the
 * sub-band scores would correlate millions of pairs of noise rows.  The scrunch calls make the
 * fold the PFD calls score out of such a cube where it lies, in one pass: every value is loaded
 * once, as the value it is, and the result is stored once.
 *
 * Inputs for fold i: the cube x[i][p][c][b], npart x nchan x nbin; an optional rotation per
 * channel rot[i][c], any int32; two factors, fscr dividing nchan and bscr dividing nbin.
 * G = nchan / fscr, K = nbin / bscr.  Contract: out is z, n x G x K doubles, dense, with
 *   S[c][b] = x[0][c][b] + x[1][c][b] + ... + x[npart-1][c][b]       from part 0's value (no 0.0 +)
 *   r_c     = ((rot[i][c] % nbin) + nbin) % nbin                      rot == NULL: 0
 *   R[c][b] = S[c][(b + r_c) % nbin]                                  a left rotation: np.roll(S[c], -r_c)
 *   B[c][k] = R[c][k*bscr] + R[c][k*bscr+1] + ... + R[c][k*bscr+bscr-1]   from the first value
 *   z[g][k] = B[g*fscr][k] + B[g*fscr+1][k] + ... + B[g*fscr+fscr-1][k]   from the first value
 * each step in fp64, each sum in exactly this order.  A float32 cube is widened value by value
 * first.  An int16 cube is decoded first, exactly as the _i16 contract above says: d * scl +
 * offs, then * wts when given; a channel of weight 0 therefore adds +0.0.  Nothing is computed
 * in float32 or in integers, and the inputs are never written.  A NaN is a NaN; which payload
 * survives is unspecified.  With fscr = bscr = 1 and no rotation z is the part sums S the PFD
 * kernels form.  No result depends on the route the shape takes (below).
 *
 * z is an ordinary fold of one part: pass it to the f64 PFD calls with npart = 1, nsub = G,
 * proflen = K and PFE_FLAG_PFD_AVGPROF, so that the average is derived from it.  prepfold builds
 * its sub-bands the same way -- channels aligned at the fold DM inside a sub-band, sub-bands left
 * unaligned for the DM search -- with rot[c] the delay of channel c against the centre of its
 * group, in bins.
 *
 * pfe_pfd_scrunch_i16 reads data, scl, offs, wts, the two strides, npart, nsub (= nchan), proflen
 * (= nbin) and n of its struct; subfreqs and scal are ignored and may be NULL.  The alignment and
 * stride rules are those of the _i16 calls, with the same texts under this name: strided table
 * rows are for device pointers.  It honours PFE_FLAG_PFD_BSWAP.  The f64 and f32 forms refuse
 * PFE_FLAG_PFD_BSWAP, and all forms refuse PFE_FLAG_PFD_AVGPROF (no call here reads scal), with
 * PFE_EINVAL.  PFE_EINVAL, with a text naming the rule, also for: a null array; a factor below 1;
 * a factor that does not divide its dimension; a cube that is not aligned to its values (8, 4,
 * 2 bytes), rot not 4-byte, out not 8-byte aligned.  There is no shape limit: any npart, nchan,
 * nbin >= 1, with 64-bit offsets throughout.  Stream behaviour and PFE_FLAG_DEVICE_PTRS are as in
 * the PFD calls.
 *
 * How: rows with nbin (rounded up to a multiple of 4) + K <= 8192 doubles, 64 KB of LDS, take one
 * block per (fold, group): slabs of up to 4096 values of consecutive channel rows are part-summed
 * into the LDS -- 16-byte loads (8-byte for int16) when nbin is a multiple of 4 and the cube is
 * aligned for them at every part, loads of single values otherwise -- and K lanes add their bscr
 * rotated values of each row in order.  Longer rows, and every shape under
 * PFE_OPT_PFD_SCRUNCH_DIRECT, take one lane per output bin, each value loaded alone at its
 * rotated place.  Same adds, same order, same bits.
 * Scratch: a host-pointer call stages the cube as the values it holds (an int16 cube as data,
 * then scl, offs and, when given, wts as floats), then rot (when given), then out; nothing else.
 * A device-pointer call takes no scratch. */
typedef struct pfe_pfd_scrunch_how {
  const int32_t* rot; /* n x nchan, any int32 (reduced mod nbin on the device); NULL = none */
  int32_t fscr, bscr; /* >= 1; fscr divides nchan, bscr divides nbin */
} pfe_pfd_scrunch_how;

int pfe_pfd_scrunch(pfe_handle* h, const double* profs, int32_t npart, int32_t nchan, int32_t nbin,
                    int64_t n, const pfe_pfd_scrunch_how* how, double* out, uint32_t flags);
int pfe_pfd_scrunch_f32(pfe_handle* h, const float* profs, int32_t npart, int32_t nchan,
                        int32_t nbin, int64_t n, const pfe_pfd_scrunch_how* how, double* out,
                        uint32_t flags);
int pfe_pfd_scrunch_i16(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_scrunch_how* how,
                        double* out, uint32_t flags);

/* ---- total intensity of int16 folds: polarisations summed where they are loaded ------------
 * A fold-mode archive usually stores four polarisations per sub-integration (AABBCRCI) or two
 * (AABB): its DATA cell is [npol][nchan][nbin] int16, DAT_SCL / DAT_OFFS are [npol][nchan]
 * float32, DAT_WTS is [nchan] with no polarisation axis, and total intensity is AA + BB.  The
 * _i16_pol forms of the seven calls that take pfe_pfd_i16_in score that sum, formed where the
 * values are loaded; `pol` stands directly behind `in`, as `kill` does in the _kill forms.
 *
 * Layout.  The polarisation axis lies between part and sub-band, dense, for data and for scl /
 * offs; wts has none:
 *   value (i,p,k,s,b) of data        (char*)data + i*fold_stride + p*part_stride
 *                                                + k*2*nsub*proflen + 2*(s*proflen + b)
 *   value (i,p,k,s) of scl / offs    (char*)scl + i*fold_stride + p*part_stride + k*4*nsub + 4*s
 *   value (i,p,s) of wts             as in the _i16 calls
 * Both strides 0: dense arrays -- data n x npart x npol x nsub x proflen, scl and offs n x npart
 * x npol x nsub, wts n x npart x nsub.  For a SUBINT table the four pointers are still the
 * columns' addresses in row 0 and part_stride = NAXIS1.  The stride rule is part_stride >= 2 x
 * npol x nsub x proflen; the other rules of the _i16 calls hold, their texts under the _i16_pol
 * names.  PFE_EINVAL, the text naming the rule: npol outside 1..4, nsum outside 1..2, nsum > npol.
 *
 * Values.  Every output and the status is, bit for bit, that of the f64 call of the same name
 * (pfe_pfd_scrunch for the scrunch) on the cube
 *   y_k[p][s][b] = (double)d[p][k][s][b] * (double)scl[p][k][s] + (double)offs[p][k][s]   one rounding
 *   x[p][s][b]   = y_0                  nsum = 1
 *                = y_0 + y_1            nsum = 2: one more rounding
 *   x[p][s][b]   = x * (double)wts[p][s]          wts given: one more rounding, on the sum
 * In numpy: dec = d.astype(f8) * scl.astype(f8)[..., None] + offs.astype(f8)[..., None];
 * x = dec[:, :, 0] + dec[:, :, 1]; x = x * wts.astype(f8)[..., None].  The weight multiplies the
 * sum: one multiply per element.  That is not the sum of two weighted polarisations, y_0 w + y_1 w,
 * which rounds twice more and differently.  From there on the _i16 contract holds: parts summed
 * from part 0's value in order, the f64 kernels on the sums as folds of one part,
 * PFE_FLAG_PFD_BSWAP reversing every 2- and 4-byte value in registers, PFE_FLAG_PFD_AVGPROF and
 * pfe_pfd_avgprof_i16_pol giving numpy's (x / proflen).sum() of x in memory order (p, s, b); a NaN
 * is a NaN, nothing is computed in float32 or integers, the inputs are never written.
 * Polarisations nsum .. npol-1 are never read.  pol == NULL or {1, 1} is the _i16 call: the same
 * kernels, the same scratch, the same bits.  nsum = 1 with npol > 1 runs those kernels too (only
 * the strides know of npol), except on dense device arrays with weights, whose wts strides are
 * not those of scl: there, and for nsum = 2, the polarisation forms of the kernels run.
 * Scratch: a host-pointer call stages only what is read, compacted so the kernels see npol = nsum:
 * data n x npart x nsum x nsub x proflen int16, scl and offs n x npart x nsum x nsub floats, wts
 * as in the _i16 call; everything behind them is as for the _i16 call. */
typedef struct pfe_pfd_i16_pol {
  int32_t npol; /* polarisations stored per (fold, part): 1..4 */
  int32_t nsum; /* leading polarisations summed: 1 or 2, <= npol */
} pfe_pfd_i16_pol;

int pfe_pfd_dmprof_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                           double* profile, float* chis, double* lyon8, uint32_t* status,
                           uint32_t flags);
int pfe_pfd_bates22_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                            double* out, uint32_t* status, uint32_t flags);
int pfe_pfd_params4_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                            double* out, uint32_t* status, uint32_t flags);
int pfe_pfd_dmfit4_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                           double* out, uint32_t* status, uint32_t flags);
int pfe_pfd_subband3_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                             double* out, uint32_t* status, uint32_t flags);
int pfe_pfd_avgprof_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                            double* out, int64_t out_stride, uint32_t flags);
int pfe_pfd_scrunch_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                            const pfe_pfd_scrunch_how* how, double* out, uint32_t flags);

/* ---- float32 candidates: the float-array calls on arrays of floats ----------------------
 * A candidate that never was a .pfd or .phcx file -- a float32 tensor from a GPU folder or a
 * normalising step, the arrays an ML pipeline keeps, the float32 DM curve pfe_pfd_dmprof
 * returns in `chis` -- is scored where it is: every float array the f64 calls take as doubles
 * is taken here as 4-byte floats and read as such.
 *
 * Contract: the result of an _f32 call is, bit for bit, the result of the _f64 call of the same
 * name on the same arrays widened value by value ((double)x, exact; float32 subnormals, signed
 * zeros, infinities and NaNs are carried), in every column it returns (skew included: the same
 * device pow on the same value), in the placement of NaNs and in the status bits.  Nothing is
 * computed in float32: each value is widened at its load and every operation is the fp64
 * operation of the f64 call, in its order.  This is NOT numpy on a float32 array, which
 * accumulates in float32 (numpy.mean, numpy.sum, numpy.corrcoef of float32 rows): compare with
 * the f64 call on x.astype(numpy.float64).
 *
 * Shape limits, PFE_EINVAL texts (under the _f32 name), status bits, stream behaviour,
 * PFE_FLAG_DEVICE_PTRS and the options (PFE_OPT_SOLVER, _SERIAL, _HANDOVER, _GSLOTS,
 * _SUBF64_GLOBAL, PFE_OPT_LYON8_BLOCKS) are those of the f64 call of the same name.  Float
 * arrays must be 4-byte aligned (any such alignment gives the same bits; a sub-band array whose
 * candidates start on 16-byte boundaries takes 16-byte loads throughout); scal and out keep the
 * 8 bytes of the f64 calls.  Dense rows, except pfe_lyon8_f32, which takes any row strides that
 * are at least the row lengths, in floats.  Inputs are never written.
 *
 *   pfe_lyon8_f32      the kernels of pfe_lyon8_f64 loading floats: both passes (the sum, then
 *                      the powers of x - mean) add in numpy's float64 order.  Host rows cross
 *                      the bus as floats, chunked and overlapped as for pfe_lyon8_f64.
 *   pfe_sinusoid4_f32, pfe_gauss7_f32
 *                      the profiles are widened once into the handle's scratch and the fit
 *                      kernels of the f64 calls run on that copy.
 *   pfe_subband3_f32   a candidate's nsub x lsb floats are widened on their way into the copy
 *                      the f64 call makes of them (LDS partition or scratch slab, still
 *                      doubles: the LDS budget and the on-chip / slab routing are unchanged),
 *                      and its profile row likewise.
 *   pfe_bates22_f32    the profiles and the DM curves are widened into the scratch on the
 *                      handle's stream, then the groups run as in pfe_bates22_f64 (side
 *                      streams, joined before the call returns) with the sub-band kernel of
 *                      pfe_subband3_f32.  dmcurve may be the `chis` of pfe_pfd_dmprof.
 * Scratch: that of the f64 call of the same name, plus n x lp doubles (pfe_sinusoid4_f32,
 * pfe_gauss7_f32, pfe_bates22_f32) and n x ndm doubles (pfe_bates22_f32) for the widened
 * copies; on the host path the staged arrays are floats instead of doubles (half the bytes
 * over the bus).  The sub-bands are never widened in memory; pfe_subband3_f32 and
 * pfe_lyon8_f32 take no scratch beyond the f64 call's. */
int pfe_lyon8_f32(pfe_handle* h, const float* prof, int64_t prof_stride, int32_t lp,
                  const float* dm, int64_t dm_stride, int32_t ld, int64_t n, double* out,
                  uint32_t* status, uint32_t flags);
int pfe_sinusoid4_f32(pfe_handle* h, const float* prof, int32_t lp, int64_t n, double* out,
                      uint32_t* status, uint32_t flags);
int pfe_gauss7_f32(pfe_handle* h, const float* prof, int32_t lp, int64_t n, double* out,
                   uint32_t* status, uint32_t flags);

typedef struct pfe_bates_f32_in {
  const float* prof;     /* n x lp */
  int32_t lp;
  const float* sub;      /* n x nsub x lsb */
  int32_t nsub;
  int32_t lsb;
  const float* dmcurve;  /* n x ndm */
  int32_t ndm;
  const double* scal;    /* n x PFE_NSCAL, fp64 as everywhere */
  int64_t n;
} pfe_bates_f32_in;

int pfe_subband3_f32(pfe_handle* h, const pfe_bates_f32_in* in, double* out, uint32_t* status,
                     uint32_t flags);
int pfe_bates22_f32(pfe_handle* h, const pfe_bates_f32_in* in, double* out, uint32_t* status,
                    uint32_t flags);

#ifdef __cplusplus
}
#endif

#endif /* PFE_H_ */
