// capi.hip — extern "C" boundary of libpfe.so (declared in include/pfe.h).
//
// Owns: the per-handle HIP streams, device scratch, the pinned staging ring of the chunked
// host-pointer path, the handle options and the argument validation that mirrors the
// reference's failure behaviour.  No CPU fallback: every compute entry point launches a
// gfx950 kernel or returns an error.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pfe.h"
#include "launch.h"
#include "options.h"

// chunked host path: device/staging slots in flight (H2D of k+1 | kernel k | D2H of k-1)
constexpr int PIPE_SLOTS = 3;
constexpr size_t PIPE_CHUNK_BYTES = 64u << 20;  // input bytes per chunk

struct pfe_handle {
  int device = -1;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  pfe::Fork fork;  // side streams of the 22-score chains (bates_common.h)
  pfe::Options opt;
  // device scratch: staging of the one-shot host paths, the 22-score workspace and the
  // device slots of the chunked host path
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  // completion of the last call, on the stream it ran on: a call on another stream first
  // waits for it, so work on the shared scratch never overlaps
  hipEvent_t done = nullptr;
  hipStream_t last = nullptr;
  bool done_recorded = false;
  // chunked host path: copy streams, per-slot events and the pinned staging ring
  hipStream_t h2d = nullptr, d2h = nullptr;
  hipEvent_t ev_in[PIPE_SLOTS] = {}, ev_k[PIPE_SLOTS] = {}, ev_out[PIPE_SLOTS] = {};
  void* pin = nullptr;
  size_t pin_bytes = 0;
  size_t scratch_bytes_peak = 0;  // the largest scratch allocated (growth policy)
  // split PFD pipeline (pfe_pfd_dmprof): two events per part-sum buffer, made on first use
  hipEvent_t pev[4] = {};
  std::string err;
};

static thread_local std::string g_create_err;

static int set_err(pfe_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h)
    h->err = buf;
  else
    g_create_err = buf;
  return code;
}

#define PFE_HIP(h, expr)                                                                   \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return set_err((h), PFE_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

// every compute call: bind the device and order after the previous call of this handle
static int call_begin(pfe_handle* h) {
  PFE_HIP(h, hipSetDevice(h->device));
  if (h->done_recorded && h->last != h->stream) PFE_HIP(h, hipStreamWaitEvent(h->stream, h->done, 0));
  return PFE_OK;
}
static int call_end(pfe_handle* h) {
  PFE_HIP(h, hipEventRecord(h->done, h->stream));
  h->done_recorded = true;
  h->last = h->stream;
  return PFE_OK;
}

static int ensure_scratch(pfe_handle* h, size_t bytes) {
  if (bytes <= h->scratch_bytes) return PFE_OK;
  if (h->scratch) {
    // every earlier call's work on the old scratch has finished before it is freed
    if (h->done_recorded) PFE_HIP(h, hipEventSynchronize(h->done));
    PFE_HIP(h, hipStreamSynchronize(h->stream));
    PFE_HIP(h, hipFree(h->scratch));
    h->scratch = nullptr;
    h->scratch_bytes = 0;
  }
  // grow geometrically (4x the previous peak, below 1 GiB): a run whose batches grow (a
  // ramped start) reallocates (device-wide synchronising free) once or twice, not at every
  // size -- but never beyond twice what this call asked for, so a handle does not keep
  // several GiB for moderate batches
  const size_t old = h->scratch_bytes_peak;
  size_t want = bytes + (bytes >> 3) + 4096;
  size_t geo = old * 4 < ((size_t)1 << 30) ? old * 4 : ((size_t)1 << 30);
  if (geo > 2 * bytes) geo = 2 * bytes;
  if (geo > want) want = geo;
  PFE_HIP(h, hipMalloc(&h->scratch, want));
  h->scratch_bytes_peak = want;
  h->scratch_bytes = want;
  // the one alignment every layout (arena.h) relies on
  if ((uintptr_t)h->scratch & 255)
    return set_err(h, PFE_EDEVICE, "hipMalloc: block not 256-byte aligned");
  return PFE_OK;
}

// A call's scratch: the walk (a layout of launch.h) measures, the scratch grows to that,
// and the same walk places the pointers -- only then, because growing moves the scratch
template <class S, class F>
static int lay_out(pfe_handle* h, S& s, F walk) {
  pfe::Arena measure;
  walk(measure);
  int rc = ensure_scratch(h, measure.bytes());
  if (rc) return rc;
  pfe::Arena place{(uintptr_t)h->scratch};
  s = walk(place);
  return PFE_OK;
}

// The checks every call on a batch starts with: PFE_OK and n > 0 when there is work to do.
// args: the caller's pointer arguments besides `in` are all there
template <class In>
static int call_check(pfe_handle* h, const char* fn, const In* in, bool args, int64_t& n) {
  n = 0;
  if (!h) return PFE_EINVAL;
  h->err.clear();
  if (!in || !args) return set_err(h, PFE_EINVAL, "%s: null argument", fn);
  if (in->n < 0) return set_err(h, PFE_EINVAL, "%s: n < 0", fn);
  n = in->n;
  return PFE_OK;
}

// host -> a region the layout took, on the call's stream
template <class T>
static int stage_in(pfe_handle* h, T* dst, const void* src, size_t count) {
  PFE_HIP(h, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return PFE_OK;
}
template <class T>
static int fetch(pfe_handle* h, T* dst, const T* src, size_t count) {
  PFE_HIP(h, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  return PFE_OK;
}
// the end of a host-pointer call: out (n x k, or null), status, and the results are there
static int fetch_out(pfe_handle* h, double* out, const double* dout, int k, uint32_t* status,
                     const uint32_t* dstat, int64_t n) {
  int rc = out ? fetch(h, out, dout, (size_t)n * k) : PFE_OK;
  if (!rc) rc = fetch(h, status, dstat, (size_t)n);
  if (rc) return rc;
  PFE_HIP(h, hipStreamSynchronize(h->stream));
  return PFE_OK;
}

static int ensure_pinned(pfe_handle* h, size_t bytes) {
  if (bytes <= h->pin_bytes) return PFE_OK;
  if (h->pin) {
    PFE_HIP(h, hipHostFree(h->pin));
    h->pin = nullptr;
    h->pin_bytes = 0;
  }
  PFE_HIP(h, hipHostMalloc(&h->pin, bytes, hipHostMallocDefault));
  h->pin_bytes = bytes;
  return PFE_OK;
}

// host memory the DMA engines can read directly (hipHostMalloc / hipHostRegister)
static bool is_pinned(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

extern "C" {

int pfe_abi_version(void) { return PFE_ABI_VERSION; }

int pfe_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pfe_create(int device, pfe_handle** out) {
  if (!out) return set_err(nullptr, PFE_EINVAL, "pfe_create: out is NULL");
  *out = nullptr;
  if (device < 0)
    return set_err(nullptr, PFE_ENODEV,
                   "pfe_create: device %d: libpfe has no CPU backend; a gfx950 GPU is required",
                   device);
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return set_err(nullptr, PFE_ENODEV, "pfe_create: no HIP device visible (%s)",
                   hipGetErrorString(e));
  if (device >= n)
    return set_err(nullptr, PFE_ENODEV, "pfe_create: device %d out of range (%d visible)",
                   device, n);
  pfe_handle* h = new (std::nothrow) pfe_handle();
  if (!h) return set_err(nullptr, PFE_EDEVICE, "pfe_create: out of host memory");
  h->device = device;
  if ((e = hipSetDevice(device)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking)) != hipSuccess) {
    delete h;
    return set_err(nullptr, PFE_EDEVICE, "pfe_create: %s", hipGetErrorString(e));
  }
  h->stream = h->own;
  for (int i = 0; i < 2 && e == hipSuccess; ++i)
    e = hipStreamCreateWithFlags(&h->fork.side[i], hipStreamNonBlocking);
  for (int i = 0; i < 3 && e == hipSuccess; ++i)
    e = hipEventCreateWithFlags(&h->fork.ev[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    pfe_destroy(h);
    return set_err(nullptr, PFE_EDEVICE, "pfe_create: %s", hipGetErrorString(e));
  }
  *out = h;
  return PFE_OK;
}

void pfe_destroy(pfe_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->done_recorded) (void)hipEventSynchronize(h->done);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->h2d) (void)hipStreamSynchronize(h->h2d);
  if (h->d2h) (void)hipStreamSynchronize(h->d2h);
  if (h->scratch) (void)hipFree(h->scratch);
  if (h->pin) (void)hipHostFree(h->pin);
  for (hipStream_t& s : h->fork.side)
    if (s) (void)hipStreamDestroy(s);
  for (hipEvent_t& v : h->fork.ev)
    if (v) (void)hipEventDestroy(v);
  for (hipEvent_t& v : h->pev)
    if (v) (void)hipEventDestroy(v);
  for (int i = 0; i < PIPE_SLOTS; ++i) {
    if (h->ev_in[i]) (void)hipEventDestroy(h->ev_in[i]);
    if (h->ev_k[i]) (void)hipEventDestroy(h->ev_k[i]);
    if (h->ev_out[i]) (void)hipEventDestroy(h->ev_out[i]);
  }
  if (h->h2d) (void)hipStreamDestroy(h->h2d);
  if (h->d2h) (void)hipStreamDestroy(h->d2h);
  if (h->done) (void)hipEventDestroy(h->done);
  if (h->own) (void)hipStreamDestroy(h->own);
  delete h;
}

const char* pfe_last_error(const pfe_handle* h) {
  return h ? h->err.c_str() : g_create_err.c_str();
}

int pfe_set_stream(pfe_handle* h, void* s) {
  if (!h) return PFE_EINVAL;
  h->stream = (hipStream_t)s;  // NULL selects the HIP default (null) stream
  return PFE_OK;
}

int pfe_synchronize(pfe_handle* h) {
  if (!h) return PFE_EINVAL;
  PFE_HIP(h, hipSetDevice(h->device));
  PFE_HIP(h, hipStreamSynchronize(h->stream));
  return PFE_OK;
}

int pfe_set_option(pfe_handle* h, int32_t option, int64_t v) {
  if (!h) return PFE_EINVAL;
  h->err.clear();
  pfe::Options& o = h->opt;
  switch (option) {
    case PFE_OPT_SOLVER:
      if (v != PFE_SOLVER_POOLED && v != PFE_SOLVER_BATCHED && v != PFE_SOLVER_WAVE) break;
      o.solver = (int)v;
      return PFE_OK;
    case PFE_OPT_SERIAL:
      if (v != 0 && v != 1) break;
      o.serial = (int)v;
      h->fork.serial = (int)v;
      return PFE_OK;
    case PFE_OPT_HANDOVER:
      if (v != 0 && v != 1) break;
      o.handover = (int)v;
      return PFE_OK;
    case PFE_OPT_GSLOTS:
      if (v < 0 || v > pfe::GLM_FPW) break;
      o.gslots = (int)v;
      return PFE_OK;
    case PFE_OPT_LYON8_BLOCKS:
      if (v < 1 || v > (1 << 24)) break;
      o.lyon8_blocks = (int)v;
      return PFE_OK;
    case PFE_OPT_LYON8_BURST:
      if (v != 1 && v != 2 && v != 4) break;
      o.lyon8_burst = (int)v;
      return PFE_OK;
    case PFE_OPT_PFD_WAVES:
      if (v != 1 && v != 4) break;
      o.pfd_waves = (int)v;
      return PFE_OK;
    case PFE_OPT_LYON8_DM:
      if (v < 0 || v > 2) break;
      o.lyon8_dm = (int)v;
      return PFE_OK;
    case PFE_OPT_PFD_SPLIT:
      if (v != 0 && v != 1) break;
      o.pfd_split = (int)v;
      return PFE_OK;
    case PFE_OPT_LYON8_DM_SPLIT:
      if (v < 0 || v > 2) break;
      o.lyon8_dm_split = (int)v;
      return PFE_OK;
    case PFE_OPT_PFD_GLOBAL:
      if (v != 0 && v != 1) break;
      o.pfd_global = (int)v;
      return PFE_OK;
    case PFE_OPT_SUBF64_GLOBAL:
      if (v != 0 && v != 1) break;
      o.subf64_global = (int)v;
      return PFE_OK;
    case PFE_OPT_PFD_F32_CHUNK:
      if (v < 0) break;
      o.pfd_f32_chunk = v;
      return PFE_OK;
    case PFE_OPT_PFD_SCRUNCH_DIRECT:
      if (v != 0 && v != 1) break;
      o.pfd_scrunch_direct = (int)v;
      return PFE_OK;
    default:
      return set_err(h, PFE_EINVAL, "pfe_set_option: unknown option %d", option);
  }
  return set_err(h, PFE_EINVAL, "pfe_set_option: value %lld out of range for option %d",
                 (long long)v, option);
}

int pfe_get_option(const pfe_handle* h, int32_t option, int64_t* v) {
  if (!h || !v) return PFE_EINVAL;
  const pfe::Options& o = h->opt;
  switch (option) {
    case PFE_OPT_SOLVER: *v = o.solver; return PFE_OK;
    case PFE_OPT_SERIAL: *v = o.serial; return PFE_OK;
    case PFE_OPT_HANDOVER: *v = o.handover; return PFE_OK;
    case PFE_OPT_GSLOTS: *v = o.gslots; return PFE_OK;
    case PFE_OPT_LYON8_BLOCKS: *v = o.lyon8_blocks; return PFE_OK;
    case PFE_OPT_LYON8_BURST: *v = o.lyon8_burst; return PFE_OK;
    case PFE_OPT_PFD_WAVES: *v = o.pfd_waves; return PFE_OK;
    case PFE_OPT_LYON8_DM: *v = o.lyon8_dm; return PFE_OK;
    case PFE_OPT_PFD_SPLIT: *v = o.pfd_split; return PFE_OK;
    case PFE_OPT_LYON8_DM_SPLIT: *v = o.lyon8_dm_split; return PFE_OK;
    case PFE_OPT_PFD_GLOBAL: *v = o.pfd_global; return PFE_OK;
    case PFE_OPT_SUBF64_GLOBAL: *v = o.subf64_global; return PFE_OK;
    case PFE_OPT_PFD_F32_CHUNK: *v = o.pfd_f32_chunk; return PFE_OK;
    case PFE_OPT_PFD_SCRUNCH_DIRECT: *v = o.pfd_scrunch_direct; return PFE_OK;
    default: return PFE_EINVAL;
  }
}

int pfe_host_alloc(size_t bytes, void** out) {
  if (!out) return PFE_EINVAL;
  *out = nullptr;
  if (bytes == 0) bytes = 1;
  if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return PFE_EDEVICE;
  }
  return PFE_OK;
}

void pfe_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

}  // extern "C"

// ---- 8 Lyon features ------------------------------------------------------------------
template <typename T>
static hipError_t launch_lyon8(const T* prof, int64_t ps, int lp, const T* dm, int64_t ds, int ld,
                               int64_t n, double* out, hipStream_t st, const pfe::Options& o) {
  if constexpr (sizeof(T) == 1)
    return pfe::launch_lyon8_u8((const uint8_t*)prof, ps, lp, (const uint8_t*)dm, ds, ld, n, out,
                                st, o);
  else if constexpr (sizeof(T) == 4)
    return pfe::launch_lyon8_f32((const float*)prof, ps, lp, (const float*)dm, ds, ld, n, out, st,
                                 o);
  else
    return pfe::launch_lyon8_f64((const double*)prof, ps, lp, (const double*)dm, ds, ld, n, out,
                                 st, o);
}

// rows [r0, r0 + rows) of a strided host array into a dense buffer
template <typename T>
static void pack_rows(T* dst, const T* src, int64_t stride, int len, int64_t r0, int64_t rows) {
  if (stride == len) {
    memcpy(dst, src + r0 * stride, (size_t)rows * len * sizeof(T));
    return;
  }
  for (int64_t r = 0; r < rows; ++r)
    memcpy(dst + r * len, src + (r0 + r) * stride, (size_t)len * sizeof(T));
}

// The host-pointer path, chunked and pipelined: chunk k's rows go host -> HBM on the h2d
// stream while chunk k-1's kernel runs on the handle's stream and chunk k-2's features go
// back on the d2h stream.  Pinned caller buffers (pfe_host_alloc) are DMA'd in place;
// pageable ones are packed into (or unpacked from) the handle's pinned staging ring by the
// calling thread, overlapped with the DMA of the other slots.
template <typename T>
static int lyon8_host(pfe_handle* h, const T* prof, int64_t ps, int32_t lp, const T* dm,
                      int64_t ds, int32_t ld, int64_t n, double* out) {
  const size_t row_in = (size_t)(lp + ld) * sizeof(T);
  int64_t chunk = (int64_t)(PIPE_CHUNK_BYTES / row_in);
  chunk = std::max<int64_t>(1024, chunk & ~(int64_t)63);
  if (chunk > n) chunk = n;
  // every slot has one layout, in the device scratch and in the pinned staging ring
  pfe::Arena one;
  pfe::lyon8_slot_layout<T>(one, chunk, lp, ld);
  const size_t slot = one.bytes();
  auto slot_at = [&](void* ring, int s) {
    pfe::Arena a{(uintptr_t)ring, s * slot};
    return pfe::lyon8_slot_layout<T>(a, chunk, lp, ld);
  };
  int rc = ensure_scratch(h, PIPE_SLOTS * slot);
  if (rc) return rc;
  const bool pin_p = is_pinned(prof), pin_d = is_pinned(dm), pin_o = is_pinned(out);
  if (!(pin_p && pin_d && pin_o)) {
    rc = ensure_pinned(h, PIPE_SLOTS * slot);
    if (rc) return rc;
  }
  if (!h->h2d) {
    PFE_HIP(h, hipStreamCreateWithFlags(&h->h2d, hipStreamNonBlocking));
    PFE_HIP(h, hipStreamCreateWithFlags(&h->d2h, hipStreamNonBlocking));
    for (int i = 0; i < PIPE_SLOTS; ++i) {
      PFE_HIP(h, hipEventCreateWithFlags(&h->ev_in[i], hipEventDisableTiming));
      PFE_HIP(h, hipEventCreateWithFlags(&h->ev_k[i], hipEventDisableTiming));
      PFE_HIP(h, hipEventCreateWithFlags(&h->ev_out[i], hipEventDisableTiming));
    }
  }
  // the copy streams start after the work already queued on the handle's stream
  PFE_HIP(h, hipEventRecord(h->done, h->stream));
  PFE_HIP(h, hipStreamWaitEvent(h->h2d, h->done, 0));
  PFE_HIP(h, hipStreamWaitEvent(h->d2h, h->done, 0));
  const int64_t K = (n + chunk - 1) / chunk;
  auto rows_of = [&](int64_t k) { return std::min<int64_t>(chunk, n - k * chunk); };
  auto unstage_out = [&](int64_t k) -> int {  // pageable out: staging -> caller, after D2H k
    const int s = (int)(k % PIPE_SLOTS);
    PFE_HIP(h, hipEventSynchronize(h->ev_out[s]));
    if (!pin_o)
      memcpy(out + k * chunk * 8, slot_at(h->pin, s).out, (size_t)rows_of(k) * 8 * sizeof(double));
    return PFE_OK;
  };
  for (int64_t k = 0; k < K; ++k) {
    const int s = (int)(k % PIPE_SLOTS);
    const int64_t r0 = k * chunk, rows = rows_of(k);
    const pfe::Lyon8Slot<T> d = slot_at(h->scratch, s);
    const pfe::Lyon8Slot<T> hs = slot_at(h->pin, s);  // staging of a caller's pageable arrays
    T *dprof = d.prof, *ddm = d.dm;
    double* dout = d.out;
    if (k >= PIPE_SLOTS) {
      // slot reuse: chunk k-3's staged output is drained (and with it its H2D and kernel)
      rc = unstage_out(k - PIPE_SLOTS);
      if (rc) return rc;
    }
    if (!pin_p) pack_rows(hs.prof, prof, ps, lp, r0, rows);
    if (!pin_d) pack_rows(hs.dm, dm, ds, ld, r0, rows);
    if (pin_p && ps == lp)
      PFE_HIP(h, hipMemcpyAsync(dprof, prof + r0 * ps, (size_t)rows * lp * sizeof(T),
                                hipMemcpyHostToDevice, h->h2d));
    else if (pin_p)
      PFE_HIP(h, hipMemcpy2DAsync(dprof, lp * sizeof(T), prof + r0 * ps, ps * sizeof(T),
                                  lp * sizeof(T), rows, hipMemcpyHostToDevice, h->h2d));
    else
      PFE_HIP(h, hipMemcpyAsync(dprof, hs.prof, (size_t)rows * lp * sizeof(T),
                                hipMemcpyHostToDevice, h->h2d));
    if (pin_d && ds == ld)
      PFE_HIP(h, hipMemcpyAsync(ddm, dm + r0 * ds, (size_t)rows * ld * sizeof(T),
                                hipMemcpyHostToDevice, h->h2d));
    else if (pin_d)
      PFE_HIP(h, hipMemcpy2DAsync(ddm, ld * sizeof(T), dm + r0 * ds, ds * sizeof(T),
                                  ld * sizeof(T), rows, hipMemcpyHostToDevice, h->h2d));
    else
      PFE_HIP(h, hipMemcpyAsync(ddm, hs.dm, (size_t)rows * ld * sizeof(T),
                                hipMemcpyHostToDevice, h->h2d));
    PFE_HIP(h, hipEventRecord(h->ev_in[s], h->h2d));
    PFE_HIP(h, hipStreamWaitEvent(h->stream, h->ev_in[s], 0));
    hipError_t e = launch_lyon8<T>(dprof, lp, lp, ddm, ld, ld, rows, dout, h->stream, h->opt);
    if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "lyon8 launch: %s", hipGetErrorString(e));
    PFE_HIP(h, hipEventRecord(h->ev_k[s], h->stream));
    PFE_HIP(h, hipStreamWaitEvent(h->d2h, h->ev_k[s], 0));
    PFE_HIP(h, hipMemcpyAsync(pin_o ? out + r0 * 8 : hs.out, dout,
                              (size_t)rows * 8 * sizeof(double), hipMemcpyDeviceToHost, h->d2h));
    PFE_HIP(h, hipEventRecord(h->ev_out[s], h->d2h));
  }
  for (int64_t k = std::max<int64_t>(0, K - PIPE_SLOTS); k < K; ++k) {
    rc = unstage_out(k);
    if (rc) return rc;
  }
  return PFE_OK;
}

template <typename T>
static int lyon8_impl(pfe_handle* h, const T* prof, int64_t ps, int32_t lp, const T* dm,
                      int64_t ds, int32_t ld, int64_t n, double* out, uint32_t* status,
                      uint32_t flags, bool is_u8) {
  if (!h) return PFE_EINVAL;
  h->err.clear();
  if (n < 0) return set_err(h, PFE_EINVAL, "lyon8: n=%lld < 0", (long long)n);
  if (lp < 1 || ld < 1) return set_err(h, PFE_EINVAL, "lyon8: lp=%d ld=%d must be >= 1", lp, ld);
  if (ps < lp || ds < ld)
    return set_err(h, PFE_EINVAL, "lyon8: strides (%lld,%lld) shorter than rows (%d,%d)",
                   (long long)ps, (long long)ds, lp, ld);
  if (n == 0) return PFE_OK;
  if (!prof || !dm || !out) return set_err(h, PFE_EINVAL, "lyon8: null buffer");
  if (sizeof(T) == 4 && (((uintptr_t)prof | (uintptr_t)dm) & 3))
    return set_err(h, PFE_EINVAL, "lyon8_f32: rows not 4-byte aligned");
  if (!is_u8 && (lp > (1 << 30) || ld > (1 << 30)))
    return set_err(h, PFE_EINVAL, "lyon8: row too long");
  if (is_u8 && (lp >= (1 << 24) || ld >= (1 << 24)))
    return set_err(h, PFE_EINVAL, "lyon8_u8: rows must be shorter than 2^24 bins");
  int rc = call_begin(h);
  if (rc) return rc;
  if (flags & PFE_FLAG_DEVICE_PTRS) {
    hipError_t e = launch_lyon8<T>(prof, ps, lp, dm, ds, ld, n, out, h->stream, h->opt);
    if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "lyon8 launch: %s", hipGetErrorString(e));
    if (status) PFE_HIP(h, hipMemsetAsync(status, 0, (size_t)n * sizeof(uint32_t), h->stream));
    return call_end(h);
  }
  rc = lyon8_host<T>(h, prof, ps, lp, dm, ds, ld, n, out);
  if (rc) return rc;
  if (status) memset(status, 0, (size_t)n * sizeof(uint32_t));
  return call_end(h);
}

extern "C" {

int pfe_lyon8_u8(pfe_handle* h, const uint8_t* prof, int64_t ps, int32_t lp, const uint8_t* dm,
                 int64_t ds, int32_t ld, int64_t n, double* out, uint32_t* status,
                 uint32_t flags) {
  return lyon8_impl<uint8_t>(h, prof, ps, lp, dm, ds, ld, n, out, status, flags, true);
}

int pfe_lyon8_f64(pfe_handle* h, const double* prof, int64_t ps, int32_t lp, const double* dm,
                  int64_t ds, int32_t ld, int64_t n, double* out, uint32_t* status,
                  uint32_t flags) {
  return lyon8_impl<double>(h, prof, ps, lp, dm, ds, ld, n, out, status, flags, false);
}

int pfe_lyon8_f32(pfe_handle* h, const float* prof, int64_t ps, int32_t lp, const float* dm,
                  int64_t ds, int32_t ld, int64_t n, double* out, uint32_t* status,
                  uint32_t flags) {
  return lyon8_impl<float>(h, prof, ps, lp, dm, ds, ld, n, out, status, flags, false);
}

}  // extern "C"

// ---- 22 Bates scores / sub-band scores -------------------------------------------------
static int check_bates_in(pfe_handle* h, const pfe_bates_in* in, const char* fn, bool need_dm) {
  if (!in->prof || !in->sub || !in->scal || (need_dm && !in->dmcurve))
    return set_err(h, PFE_EINVAL, "%s: null input array", fn);
  // the 22-score chain's profile kernels take 8-1024 bins; the sub-band scores alone only
  // compare the profile with the sub-bands (any nBins the any-shape kernel holds)
  if (need_dm ? (in->lp < 8 || in->lp > 1024) : (in->lp < 1 || in->lp > 16384))
    return set_err(h, PFE_EINVAL, "%s: lp=%d outside [%d,%d]", fn, in->lp, need_dm ? 8 : 1,
                   need_dm ? 1024 : 16384);
  // pfe_subband3 computes nothing else, so an unsupported sub-band shape fails the call; in
  // pfe_bates22 it only fails the rows' sub-band group (PFE_ST_UNSUPPORTED per row), within
  // the per-candidate bound of 2^24 sub-band bytes that pfe_bates22 itself checks (pfe.h
  // PFE_ST_UNSUPPORTED)
  if (!need_dm) {
    if (const char* why = pfe::subband_shape_error(in->nsub, in->lsb))
      return set_err(h, PFE_EINVAL, "%s: sub-band shape %dx%d: %s", fn, in->nsub, in->lsb, why);
  } else if (in->nsub < 1 || in->lsb < 1 || (int64_t)in->nsub * in->lsb > (1 << 24)) {
    return set_err(h, PFE_EINVAL, "%s: sub-band shape %dx%d", fn, in->nsub, in->lsb);
  }
  if (need_dm && (in->ndm < 3 || in->ndm > 1024))
    return set_err(h, PFE_EINVAL, "%s: ndm=%d outside [3,1024]", fn, in->ndm);
  return PFE_OK;
}

// pfe_bates22 (chain: the 22 scores) and pfe_subband3: on the host path the inputs go to the
// scratch and the results come back; the launcher works behind them
static int score_call(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                      uint32_t flags, const char* fn, bool chain) {
  int64_t n;
  int rc = call_check(h, fn, in, out && status, n);
  if (rc || n == 0) return rc;
  if ((rc = check_bates_in(h, in, fn, chain)) || (rc = call_begin(h))) return rc;
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  const size_t sub_bytes = pfe::subband_work_bytes(n, in->nsub, in->lsb);
  const int cus = chain ? pfe::device_cus() : 0;
  pfe::ScoreStage s;
  rc = lay_out(h, s, [&](pfe::Arena& A) {
    return pfe::score_layout(A, *in, host, chain, sub_bytes, cus, h->opt);
  });
  if (rc) return rc;
  pfe_bates_in din = *in;
  if (host) {
    const size_t m = (size_t)n;
    if ((rc = stage_in(h, s.prof, in->prof, m * in->lp)) ||
        (rc = stage_in(h, s.sub, in->sub, m * in->nsub * in->lsb)) ||
        (chain && (rc = stage_in(h, s.dmcurve, in->dmcurve, m * in->ndm))) ||
        (rc = stage_in(h, s.scal, in->scal, m * PFE_NSCAL)))
      return rc;
    din.prof = s.prof;
    din.sub = s.sub;
    if (chain) din.dmcurve = s.dmcurve;
    din.scal = s.scal;
  }
  double* dout = host ? s.out : out;
  uint32_t* dstat = host ? s.status : status;
  hipStream_t st = h->stream;
  hipError_t e = chain ? pfe::launch_bates22(&din, dout, dstat, s.bates, st, &h->fork, h->opt)
                       : pfe::launch_subband3(&din, dout, dstat, s.sub_work, st);
  if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  if (host && (rc = fetch_out(h, out, dout, chain ? 22 : 3, status, dstat, n))) return rc;
  return call_end(h);
}

extern "C" {

int pfe_bates22(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                uint32_t flags) {
  return score_call(h, in, out, status, flags, "bates22", true);
}

int pfe_subband3(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                 uint32_t flags) {
  return score_call(h, in, out, status, flags, "subband3", false);
}

}  // extern "C"

// ---- one score group of the chain (ProfileOperationsInterface.py:69-130) ----------------
// columns [c0, c0 + k) of the rows of src (n x ld: the 22-score vector, or the 8 DM-fit
// inputs of the PFD path) -> dst (n x k)
__global__ void k_take_cols(const double* src, int ld, int c0, int k, int64_t n, double* dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * k) dst[i] = src[(i / k) * ld + c0 + i % k];
}

// getCandidateParameters: (period, snr, dm, width) of each candidate, unfiltered
__global__ void k_params4(const double* scal, int64_t n, double* out, uint32_t* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* sc = scal + i * PFE_NSCAL;
  out[i * 4 + 0] = sc[PFE_SCAL_PERIOD_MS];
  out[i * 4 + 1] = sc[PFE_SCAL_SNR];
  out[i * 4 + 2] = sc[PFE_SCAL_DM];
  out[i * 4 + 3] = sc[PFE_SCAL_WIDTH];
  status[i] = 0;
}

// groups: pfe::BG_SINE (cols 0-3) / BG_GAUSS (4-10) / BG_DM (15-18, raw shift).  f64: the
// profile rows are in->n x in->lp doubles at fprof (the float profile of a PFD), in->prof and
// in->scal are not read.  prof32 (with f64, fprof null): the rows as floats, which
// launch_widen_f32 widens into the layout's fprof for the same kernels
static int bates_group_call(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                            uint32_t flags, const char* fn, unsigned groups, int c0, int k,
                            bool f64 = false, const double* fprof = nullptr,
                            const float* prof32 = nullptr, bool f32 = false) {
  int64_t n;
  int rc = call_check(h, fn, in, out && status, n);
  if (rc || n == 0) return rc;
  const bool dm = groups == pfe::BG_DM;
  if (f64 ? (f32 ? !prof32 : !fprof) : (!in->scal || (dm ? !in->dmcurve : !in->prof)))
    return set_err(h, PFE_EINVAL, "%s: null input array", fn);
  if (f32 && ((uintptr_t)prof32 & 3))
    return set_err(h, PFE_EINVAL, "%s: prof not 4-byte aligned", fn);
  if (!dm && (in->lp < 8 || in->lp > 1024))
    return set_err(h, PFE_EINVAL, "%s: lp=%d outside [8,1024]", fn, in->lp);
  if (dm && (in->ndm < 3 || in->ndm > 1024))
    return set_err(h, PFE_EINVAL, "%s: ndm=%d outside [3,1024]", fn, in->ndm);
  if ((rc = call_begin(h))) return rc;
  hipStream_t st = h->stream;
  // only the arrays the group reads; no sub-band work
  pfe_bates_in g = *in;
  g.sub = nullptr;
  g.nsub = g.lsb = 0;
  if (f64) g.prof = nullptr;
  if (dm) {
    g.prof = nullptr;
    g.lp = 0;
  } else {
    g.dmcurve = nullptr;
    g.ndm = 0;
  }
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  const int cus = pfe::device_cus();
  pfe::GroupStage s;
  rc = lay_out(h, s, [&](pfe::Arena& A) {
    return pfe::group_layout(A, n, g.lp, g.ndm, groups, f64, k, host, cus, h->opt, f32);
  });
  if (rc) return rc;
  if (host) {
    const size_t m = (size_t)n;
    if (dm) {
      rc = stage_in(h, s.dmcurve, in->dmcurve, m * g.ndm);
      g.dmcurve = s.dmcurve;
    } else if (f32) {
      rc = stage_in(h, s.prof32, prof32, m * g.lp);
      prof32 = s.prof32;
    } else if (f64) {
      rc = stage_in(h, s.fprof, fprof, m * g.lp);
      fprof = s.fprof;
    } else {
      rc = stage_in(h, s.prof, in->prof, m * g.lp);
      g.prof = s.prof;
    }
    if (!rc && !f64) {
      rc = stage_in(h, s.scal, in->scal, m * PFE_NSCAL);
      g.scal = s.scal;
    }
    if (rc) return rc;
  }
  double* dk = host ? s.out : out;
  uint32_t* dst = host ? s.status : status;
  hipError_t e = hipSuccess;
  if (f32) {
    e = pfe::launch_widen_f32(prof32, s.fprof, n * g.lp, nullptr, nullptr, 0, st);
    fprof = s.fprof;
  }
  if (e == hipSuccess)
    e = pfe::launch_bates_groups(&g, s.d22, dst, s.bates, st, &h->fork, h->opt, groups, dm,
                                 f64 ? fprof : nullptr);
  if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(k_take_cols, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, st, s.d22,
                     22, c0, k, n, dk);
  PFE_HIP(h, hipGetLastError());
  if (host && (rc = fetch_out(h, out, dk, k, status, dst, n))) return rc;
  return call_end(h);
}

extern "C" {

int pfe_sinusoid4(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                  uint32_t flags) {
  return bates_group_call(h, in, out, status, flags, "sinusoid4", pfe::BG_SINE, 0, 4);
}

int pfe_gauss7(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
               uint32_t flags) {
  return bates_group_call(h, in, out, status, flags, "gauss7", pfe::BG_GAUSS, 4, 7);
}

int pfe_dmfit4(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
               uint32_t flags) {
  return bates_group_call(h, in, out, status, flags, "dmfit4", pfe::BG_DM, 15, 4);
}

// the float profile of a PFD (pfe_pfd_dmprof's `profile`) through the same kernels
static int bates_group_call_f64(pfe_handle* h, const double* prof, int32_t lp, int64_t n,
                                double* out, uint32_t* status, uint32_t flags, const char* fn,
                                unsigned groups, int c0, int k) {
  pfe_bates_in in{};
  in.lp = lp;
  in.n = n;
  return bates_group_call(h, &in, out, status, flags, fn, groups, c0, k, true, prof);
}

int pfe_sinusoid4_f64(pfe_handle* h, const double* prof, int32_t lp, int64_t n, double* out,
                      uint32_t* status, uint32_t flags) {
  return bates_group_call_f64(h, prof, lp, n, out, status, flags, "sinusoid4_f64", pfe::BG_SINE,
                              0, 4);
}

int pfe_gauss7_f64(pfe_handle* h, const double* prof, int32_t lp, int64_t n, double* out,
                   uint32_t* status, uint32_t flags) {
  return bates_group_call_f64(h, prof, lp, n, out, status, flags, "gauss7_f64", pfe::BG_GAUSS, 4,
                              7);
}

// the same on float32 profiles: widened once into the scratch, then the kernels of the f64 call
static int bates_group_call_f32(pfe_handle* h, const float* prof, int32_t lp, int64_t n,
                                double* out, uint32_t* status, uint32_t flags, const char* fn,
                                unsigned groups, int c0, int k) {
  pfe_bates_in in{};
  in.lp = lp;
  in.n = n;
  return bates_group_call(h, &in, out, status, flags, fn, groups, c0, k, true, nullptr, prof, true);
}

int pfe_sinusoid4_f32(pfe_handle* h, const float* prof, int32_t lp, int64_t n, double* out,
                      uint32_t* status, uint32_t flags) {
  return bates_group_call_f32(h, prof, lp, n, out, status, flags, "sinusoid4_f32", pfe::BG_SINE,
                              0, 4);
}

int pfe_gauss7_f32(pfe_handle* h, const float* prof, int32_t lp, int64_t n, double* out,
                   uint32_t* status, uint32_t flags) {
  return bates_group_call_f32(h, prof, lp, n, out, status, flags, "gauss7_f32", pfe::BG_GAUSS, 4,
                              7);
}

int pfe_params4(pfe_handle* h, const pfe_bates_in* in, double* out, uint32_t* status,
                uint32_t flags) {
  int64_t n;
  int rc = call_check(h, "params4", in, out && status && !(in && in->n > 0 && !in->scal), n);
  if (rc || n == 0) return rc;
  if ((rc = call_begin(h))) return rc;
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  pfe::GroupStage s;  // the host path's scal, out and status: no fit, no workspace
  rc = lay_out(h, s, [&](pfe::Arena& A) {
    return pfe::group_layout(A, n, 0, 0, 0, false, 4, host, 0, h->opt);
  });
  if (rc || (host && (rc = stage_in(h, s.scal, in->scal, (size_t)n * PFE_NSCAL)))) return rc;
  double* dout = host ? s.out : out;
  uint32_t* dstat = host ? s.status : status;
  hipLaunchKernelGGL(k_params4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                     host ? s.scal : in->scal, n, dout, dstat);
  PFE_HIP(h, hipGetLastError());
  if (host && (rc = fetch_out(h, out, dout, 4, status, dstat, n))) return rc;
  return call_end(h);
}

}  // extern "C"

// ---- float sub-bands and the float 22-score call ------------------------------------------
// pfe_subband3_f64 (chain = false: out n x 3) and pfe_bates22_f64 (chain: the 22 scores): on
// the host path the inputs go to the scratch and the results come back; the launchers of
// subband_f64.hip work behind them.  In = pfe_bates_f32_in: the _f32 calls, with the float
// arrays held (and staged) as floats and the launchers of cand_f32.hip
template <class In>
static int score_float_call(pfe_handle* h, const In* in, double* out, uint32_t* status,
                            uint32_t flags, const char* fn, bool chain) {
  constexpr bool F32 = std::is_same<In, pfe_bates_f32_in>::value;
  constexpr uintptr_t amask = F32 ? 3 : 7;  // of the float arrays
  int64_t n;
  int rc = call_check(h, fn, in, out && status, n);
  if (rc || n == 0) return rc;
  if (!in->prof || !in->sub || !in->scal || (chain && !in->dmcurve))
    return set_err(h, PFE_EINVAL, "%s: null input array", fn);
  if ((((uintptr_t)in->scal | (uintptr_t)out) & 7) ||
      (((uintptr_t)in->prof | (uintptr_t)in->sub) & amask) ||
      (chain && ((uintptr_t)in->dmcurve & amask)))
    return set_err(h, PFE_EINVAL,
                   F32 ? "%s: array not aligned (4 bytes: prof, sub, dmcurve; 8: scal, out)"
                       : "%s: array not 8-byte aligned",
                   fn);
  if (chain ? (in->lp < 8 || in->lp > 1024) : in->lp < 1)
    return set_err(h, PFE_EINVAL, "%s: lp=%d outside [%d,%d]", fn, in->lp, chain ? 8 : 1,
                   chain ? 1024 : INT32_MAX);
  if (chain && (in->ndm < 3 || in->ndm > 1024))
    return set_err(h, PFE_EINVAL, "%s: ndm=%d outside [3,1024]", fn, in->ndm);
  if (in->nsub < 1 || in->lsb < 1)
    return set_err(h, PFE_EINVAL, "%s: sub-band shape %dx%d", fn, in->nsub, in->lsb);
  if (!pfe::subf64_plan(in->nsub, in->lsb, n, 1, false).ok)
    return set_err(h, PFE_EINVAL,
                   "%s: sub-band shape %dx%d unsupported: the per-candidate vectors "
                   "((2*lsb + 3*nsub) doubles = %zu bytes) exceed %zu bytes of LDS",
                   fn, in->nsub, in->lsb, pfe::subf64_vec_bytes(in->nsub, in->lsb),
                   pfe::SUBF64_LDS_LIMIT);
  if ((rc = call_begin(h))) return rc;
  const int cus = pfe::device_cus();
  const pfe::SubF64Plan p = pfe::subf64_plan(in->nsub, in->lsb, n, cus, h->opt.subf64_global != 0);
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  typename std::conditional<F32, pfe::SubF32Stage, pfe::SubF64Stage>::type s;
  rc = lay_out(h, s, [&](pfe::Arena& A) {
    if constexpr (F32)
      return pfe::subband_f32_layout(A, *in, host, chain, p.slab_bytes(), cus, h->opt);
    else
      return pfe::subband_f64_layout(A, *in, host, chain, p.slab_bytes(), cus, h->opt);
  });
  if (rc) return rc;
  In din = *in;
  if (host) {
    const size_t m = (size_t)n;
    if ((rc = stage_in(h, s.prof, in->prof, m * in->lp)) ||
        (rc = stage_in(h, s.sub, in->sub, m * in->nsub * in->lsb)) ||
        (chain && (rc = stage_in(h, s.dmcurve, in->dmcurve, m * in->ndm))) ||
        (rc = stage_in(h, s.scal, in->scal, m * PFE_NSCAL)))
      return rc;
    din.prof = s.prof;
    din.sub = s.sub;
    if (chain) din.dmcurve = s.dmcurve;
    din.scal = s.scal;
  }
  double* dout = host ? s.out : out;
  uint32_t* dstat = host ? s.status : status;
  hipStream_t st = h->stream;
  hipError_t e;
  if constexpr (F32)
    e = chain ? pfe::launch_bates22_f32(&din, s.fprof, s.fdm, dout, dstat, s.bates, p, s.slabs, st,
                                        &h->fork, h->opt)
              : pfe::launch_subband_f32(&din, dout, 3, dstat, false, p, s.slabs, st);
  else
    e = chain ? pfe::launch_bates22_f64(&din, dout, dstat, s.bates, p, s.slabs, st, &h->fork,
                                        h->opt)
              : pfe::launch_subband_f64(&din, dout, 3, dstat, false, p, s.slabs, st);
  if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  if (host && (rc = fetch_out(h, out, dout, chain ? 22 : 3, status, dstat, n))) return rc;
  return call_end(h);
}

extern "C" {

int pfe_subband3_f64(pfe_handle* h, const pfe_bates_f64_in* in, double* out, uint32_t* status,
                     uint32_t flags) {
  return score_float_call(h, in, out, status, flags, "subband3_f64", false);
}

int pfe_bates22_f64(pfe_handle* h, const pfe_bates_f64_in* in, double* out, uint32_t* status,
                    uint32_t flags) {
  return score_float_call(h, in, out, status, flags, "bates22_f64", true);
}

int pfe_subband3_f32(pfe_handle* h, const pfe_bates_f32_in* in, double* out, uint32_t* status,
                     uint32_t flags) {
  return score_float_call(h, in, out, status, flags, "subband3_f32", false);
}

int pfe_bates22_f32(pfe_handle* h, const pfe_bates_f32_in* in, double* out, uint32_t* status,
                    uint32_t flags) {
  return score_float_call(h, in, out, status, flags, "bates22_f32", true);
}

// ---- PFD -------------------------------------------------------------------------------
// folds that fit the LDS keep the LDS-resident kernels; every other shape (and every shape
// under PFE_OPT_PFD_GLOBAL = 1) takes k_pfd_dmprof_g on slabs of the handle's scratch
static bool pfd_use_global(const pfe_handle* h, const pfe_pfd_in* in) {
  return h->opt.pfd_global || pfe::pfd_lds_bytes(in->nsub, in->proflen) > pfe::PFD_LDS_LIMIT;
}
static int pfd_shape_err(pfe_handle* h, const char* fn, const pfe_pfd_in* in) {
  const pfe::PfdGlobalPlan p = pfe::pfd_global_plan(in->nsub, in->proflen, 1);
  return set_err(h, PFE_EINVAL,
                 "%s: nsub=%d proflen=%d unsupported: proflen <= %d and the per-fold vectors "
                 "(6*proflen + 3.5*nsub doubles = %zu bytes) <= %zu bytes of LDS",
                 fn, in->nsub, in->proflen, pfe::PFD_G_MAX_L, p.lds, pfe::PFD_LDS_LIMIT);
}
// the shape and the caller's arrays of a PFD call
static pfe::PfdArgs pfd_args(const pfe_handle* h, const pfe_pfd_in* in) {
  pfe::PfdArgs a;
  a.profs = in->profs;
  a.subfreqs = in->subfreqs;
  a.scal = in->scal;
  a.npart = in->npart;
  a.nsub = in->nsub;
  a.L = in->proflen;
  a.n = in->n;
  a.waves = h->opt.pfd_waves;
  return a;
}
// host path of every int16 call: the dense arrays of q (n folds of npart parts of npol
// polarisations of nsub x L values) into their regions, and q reads them there.  Only the q.nsum
// leading polarisations, the ones that are read, are staged, compacted -- one pitched copy an
// array when npol > nsum -- so the kernels see a dense cube of npol = nsum; wts has no such axis
static int stage_i16(pfe_handle* h, pfe::PfdI16Src& q, int16_t* data16, float* scl16, float* offs16,
                     float* wts16, int64_t n, int npart, int nsub, int L, int npol) {
  const size_t rows = (size_t)n * npart, ns = (size_t)q.nsum;
  const size_t drow = (size_t)nsub * L * sizeof(int16_t), prow = (size_t)nsub * sizeof(float);
  int rc;
  if (npol == q.nsum) {
    if ((rc = stage_in(h, data16, q.data, rows * ns * nsub * L)) ||
        (rc = stage_in(h, scl16, q.scl, rows * ns * nsub)) ||
        (rc = stage_in(h, offs16, q.offs, rows * ns * nsub)))
      return rc;
  } else {
    PFE_HIP(h, hipMemcpy2DAsync(data16, ns * drow, q.data, npol * drow, ns * drow, rows,
                                hipMemcpyHostToDevice, h->stream));
    PFE_HIP(h, hipMemcpy2DAsync(scl16, ns * prow, q.scl, npol * prow, ns * prow, rows,
                                hipMemcpyHostToDevice, h->stream));
    PFE_HIP(h, hipMemcpy2DAsync(offs16, ns * prow, q.offs, npol * prow, ns * prow, rows,
                                hipMemcpyHostToDevice, h->stream));
  }
  if (q.wts && (rc = stage_in(h, wts16, q.wts, rows * nsub))) return rc;
  q.data = reinterpret_cast<const char*>(data16);
  q.scl = reinterpret_cast<const char*>(scl16);
  q.offs = reinterpret_cast<const char*>(offs16);
  if (q.wts) q.wts = reinterpret_cast<const char*>(wts16);
  q.dps = q.dks * (int64_t)ns;
  q.dfs = q.dps * npart;
  q.pps = q.pks * (int64_t)ns;
  q.pfs = q.pps * npart;
  return PFE_OK;
}
// host path: the three inputs into their regions `d`, and `a` reads them there (x32: the
// float cube of an _f32 call, copied as the floats it is; q: the dense int16 cube of an _i16
// call and its parameters, copied as they are, npol polarisations a part of which stage_i16
// takes those that are read; each pass points a.profs at its sums)
static int stage_pfd(pfe_handle* h, const pfe_pfd_in* in, const float*& x32, pfe::PfdI16Src* q,
                     const pfe::PfdInputs& d, pfe::PfdArgs& a, int npol = 1) {
  const size_t n = (size_t)in->n, cube = n * in->npart * in->nsub * in->proflen;
  int rc;
  if (q) {
    if ((rc = stage_i16(h, *q, d.data16, d.scl16, d.offs16, d.wts16, in->n, in->npart, in->nsub,
                        in->proflen, npol)))
      return rc;
  } else if ((rc = x32 ? stage_in(h, d.profs32, x32, cube) : stage_in(h, d.profs, in->profs, cube))) {
    return rc;
  }
  if ((rc = stage_in(h, d.subfreqs, in->subfreqs, n * in->nsub)) ||
      (rc = stage_in(h, d.scal, in->scal, n * PFE_PFD_NSCAL)))
    return rc;
  if (x32)
    x32 = d.profs32;
  else if (!q)
    a.profs = d.profs;
  a.subfreqs = d.subfreqs;
  a.scal = d.scal;
  return PFE_OK;
}

// The pfe_pfd_*_f32 calls go through the bodies of the f64 calls: `in` without its cube, the
// float cube beside it
struct PfdF32View {
  pfe_pfd_in in{};
  const float* x32 = nullptr;
  const pfe_pfd_in* view = nullptr;  // null as the caller's `in` was
  explicit PfdF32View(const pfe_pfd_f32_in* f) {
    if (!f) return;
    in.subfreqs = f->subfreqs;
    in.scal = f->scal;
    in.npart = f->npart;
    in.nsub = f->nsub;
    in.proflen = f->proflen;
    in.n = f->n;
    x32 = f->profs;
    view = &in;
  }
};
// The pfe_pfd_*_i16 calls go through the bodies of the f64 calls as well: `in` without its
// cube, the four arrays and their strides beside it (q: null as the caller's `in` was)
// The polarisations of an _i16_pol call: NULL is {1, 1}, the _i16 call
static int pfd_npol(const pfe_pfd_i16_pol* pol) { return pol ? pol->npol : 1; }
static int pfd_nsum(const pfe_pfd_i16_pol* pol) { return pol ? pol->nsum : 1; }
struct PfdI16View {
  pfe_pfd_in in{};
  pfe::PfdI16Src src;
  const pfe_pfd_in* view = nullptr;
  pfe::PfdI16Src* q = nullptr;
  PfdI16View(const pfe_pfd_i16_in* f, uint32_t flags, const pfe_pfd_i16_pol* pol = nullptr) {
    if (!f) return;
    in.subfreqs = f->subfreqs;
    in.scal = f->scal;
    in.npart = f->npart;
    in.nsub = f->nsub;
    in.proflen = f->proflen;
    in.n = f->n;
    src = pfe::pfd_i16_src(*f, flags & PFE_FLAG_PFD_BSWAP, pfd_npol(pol), pfd_nsum(pol));
    view = &in;
    q = &src;
  }
};
// the four arrays and the strides of an _i16 call, each rule of include/pfe.h by its name
// (the shape is positive: the caller's shape check has run); pol: the polarisations of an
// _i16_pol call (null: one), whose rules come first
static int pfd_i16_check(pfe_handle* h, const char* fn, const pfe_pfd_i16_in* f, uint32_t flags,
                         bool arrays, const pfe_pfd_i16_pol* pol = nullptr) {
  if (pol) {
    if (pol->npol < 1 || pol->npol > 4)
      return set_err(h, PFE_EINVAL, "%s: npol %d: polarisations stored per (fold, part) must be 1..4", fn,
                     pol->npol);
    if (pol->nsum < 1 || pol->nsum > 2)
      return set_err(h, PFE_EINVAL, "%s: nsum %d: polarisations summed must be 1 or 2", fn, pol->nsum);
    if (pol->nsum > pol->npol)
      return set_err(h, PFE_EINVAL, "%s: nsum %d must be <= npol %d", fn, pol->nsum, pol->npol);
  }
  const int npol = pfd_npol(pol);
  if (!f->data || !f->scl || !f->offs || (arrays && (!f->subfreqs || !f->scal)))
    return set_err(h, PFE_EINVAL, "%s: null input array", fn);
  if ((uintptr_t)f->data & 1) return set_err(h, PFE_EINVAL, "%s: data not 2-byte aligned", fn);
  if (((uintptr_t)f->scl | (uintptr_t)f->offs | (uintptr_t)f->wts) & 3)
    return set_err(h, PFE_EINVAL, "%s: scl, offs and wts must be 4-byte aligned", fn);
  const int64_t fs = f->fold_stride, ps = f->part_stride;
  if (!fs && !ps) return PFE_OK;
  if (!fs || !ps)
    return set_err(h, PFE_EINVAL,
                   "%s: fold_stride %lld and part_stride %lld: both 0 (dense arrays) or both non-zero",
                   fn, (long long)fs, (long long)ps);
  if (!(flags & PFE_FLAG_DEVICE_PTRS))
    return set_err(h, PFE_EINVAL,
                   "%s: strided input is for device pointers (PFE_FLAG_DEVICE_PTRS); a host-pointer "
                   "call takes dense arrays (both strides 0)", fn);
  const int64_t row = (int64_t)2 * npol * f->nsub * f->proflen;
  if (ps < row || ps % 4)
    return set_err(h, PFE_EINVAL, "%s: part_stride %lld must be >= 2 x %snsub x proflen = %lld and a multiple of 4",
                   fn, (long long)ps, pol ? "npol x " : "", (long long)row);
  if (fs % 4 || fs / ps < f->npart)
    return set_err(h, PFE_EINVAL,
                   "%s: fold_stride %lld must be >= npart x part_stride = %d x %lld and a multiple of 4",
                   fn, (long long)fs, f->npart, (long long)ps);
  return PFE_OK;
}
// The masks of a _kill call.  kill == NULL, or both members NULL: the call is the plain call
static bool pfd_killed(const pfe_pfd_kill* kill) { return kill && (kill->parts || kill->subs); }
static pfe::PfdKillSrc pfd_kill_src(const pfe_pfd_kill* kill) {
  pfe::PfdKillSrc k;
  k.parts = kill->parts;
  k.subs = kill->subs;
  return k;
}
// host path: the masks into their regions behind scal, and `k` reads them there
static int stage_kill(pfe_handle* h, pfe::PfdKillSrc& k, uint8_t* dparts, uint8_t* dsubs, int64_t n,
                      int npart, int nsub) {
  int rc;
  if (k.parts) {
    if ((rc = stage_in(h, dparts, k.parts, (size_t)n * npart))) return rc;
    k.parts = dparts;
  }
  if (k.subs) {
    if ((rc = stage_in(h, dsubs, k.subs, (size_t)n * nsub))) return rc;
    k.subs = dsubs;
  }
  return PFE_OK;
}
// the cube of a masked pass from its value `at` on, and the form of its values
static const void* pfd_kill_cube(const pfe::PfdArgs& a, const float* x32, int64_t at) {
  return x32 ? static_cast<const void*>(x32 + at) : static_cast<const void*>(a.profs + at);
}
static int pfd_kill_elem(const float* x32, bool be) {
  return x32 ? pfe::PFD_KILL_F32 : be ? pfe::PFD_KILL_BE64 : pfe::PFD_KILL_F64;
}
// a null or misaligned cube, in the words of the f64 call
static int pfd_cube_check(pfe_handle* h, const char* fn, const pfe_pfd_in* in, bool f32,
                          const float* x32, uint32_t flags) {
  if (f32 && (flags & PFE_FLAG_PFD_BSWAP))
    return set_err(h, PFE_EINVAL, "%s: PFE_FLAG_PFD_BSWAP is for the f64 calls (8-byte values)", fn);
  if ((f32 ? !x32 : !in->profs) || !in->subfreqs || !in->scal)
    return set_err(h, PFE_EINVAL, "%s: null input array", fn);
  if (f32 && ((uintptr_t)x32 & 3))
    return set_err(h, PFE_EINVAL, "%s: profs not 4-byte aligned", fn);
  return PFE_OK;
}
// Folds [c0, c0 + cn) of the batch `a`: the whole batch of an f64 call; one pass of a float32
// call, whose part sums k_pfd_partsum_f32 forms in psum first, for the f64 kernels to read as
// folds of one part; one pass of a PFE_FLAG_PFD_BSWAP call (be: a.profs holds the words),
// whose part sums k_pfd_partsum_be64 forms; one pass of an _i16 call (q: its arrays on the
// device), whose values k_pfd_partsum_i16 decodes and sums; one pass of a _kill call (km: its
// masks on the device, the cube in x32 or a.profs), whose selected values k_pfd_partsum_kill
// sums, with the masks of the pass's first fold.  Outputs are moved by the caller.
static int pfd_pass(pfe_handle* h, const char* fn, const pfe::PfdArgs& a, const float* x32, bool be,
                    const pfe::PfdI16Src* q, double* psum, int64_t c0, int64_t cn, pfe::PfdArgs& b,
                    const pfe::PfdKillSrc* km = nullptr) {
  b = a;
  b.n = cn;
  b.subfreqs = a.subfreqs + c0 * a.nsub;
  b.scal = a.scal + c0 * PFE_PFD_NSCAL;
  if (!x32 && !be && !q && !km) return PFE_OK;  // c0 = 0, cn = n
  const int64_t at = c0 * a.npart * (int64_t)a.nsub * a.L;
  hipError_t e =
      km   ? pfe::launch_pfd_partsum_kill(pfd_kill_cube(a, x32, at), pfd_kill_elem(x32, be),
                                          km->from(c0, a.npart, a.nsub), psum, a.npart, a.nsub, a.L,
                                          cn, h->stream)
      : q  ? pfe::launch_pfd_partsum_i16(q->from(c0), psum, a.npart, a.nsub, a.L, cn, h->stream)
      : be ? pfe::launch_pfd_partsum_be64(a.profs + at, psum, a.npart, a.nsub, a.L, cn, h->stream)
           : pfe::launch_pfd_partsum_f32(x32 + at, psum, a.npart, a.nsub, a.L, cn, h->stream);
  if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  b.profs = psum;
  b.npart = 1;
  return PFE_OK;
}

// PFE_FLAG_PFD_AVGPROF: where the derived averages go -- the scal a host-pointer call staged
// (`staged`), or, device pointers (null), a copy of the caller's scal in scratch -- and `a`
// reads its scalars there
static int pfd_avg_begin(pfe_handle* h, const pfe_pfd_in* in, double* staged,
                         const pfe::PfdAvgWork& w, pfe::PfdArgs& a, double*& wscal) {
  wscal = staged;
  if (!staged) {
    PFE_HIP(h, hipMemcpyAsync(w.scal, in->scal, (size_t)in->n * PFE_PFD_NSCAL * sizeof(double),
                              hipMemcpyDeviceToDevice, h->stream));
    wscal = w.scal;
  }
  a.scal = wscal;
  return PFE_OK;
}
// the averages of folds [c0, c0 + cn) of the batch `a` into their rows of wscal, from the cube
// as the call holds it on the device (x32: the floats of an _f32 call; be: the byte-reversed
// words of a PFE_FLAG_PFD_BSWAP call; q: the arrays of an _i16 call; km: the masks of a _kill
// call, whose average is that of the zapped cube)
static int pfd_avg_pass(pfe_handle* h, const char* fn, const pfe::PfdArgs& a, const float* x32,
                        bool be, const pfe::PfdI16Src* q, int64_t c0, int64_t cn, double* csum,
                        double* wscal, const pfe::PfdKillSrc* km = nullptr) {
  const int64_t E = (int64_t)a.npart * a.nsub * a.L;
  double* out = wscal + c0 * PFE_PFD_NSCAL + PFE_PFD_AVGPROF;
  const hipError_t e =
      km   ? pfe::launch_pfd_avgprof_kill(pfd_kill_cube(a, x32, c0 * E), pfd_kill_elem(x32, be),
                                          km->from(c0, a.npart, a.nsub), a.npart, a.nsub, a.L, cn,
                                          csum, out, PFE_PFD_NSCAL, h->stream)
      : q  ? pfe::launch_pfd_avgprof_i16(q->from(c0), a.npart, a.nsub, a.L, cn, csum, out, PFE_PFD_NSCAL,
                                         h->stream)
      : x32 ? pfe::launch_pfd_avgprof_f32(x32 + c0 * E, E, a.L, cn, csum, out, PFE_PFD_NSCAL, h->stream)
      : be ? pfe::launch_pfd_avgprof_be64(a.profs + c0 * E, E, a.L, cn, csum, out, PFE_PFD_NSCAL,
                                          h->stream)
           : pfe::launch_pfd_avgprof(a.profs + c0 * E, E, a.L, cn, csum, out, PFE_PFD_NSCAL, h->stream);
  if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  return PFE_OK;
}

// pfe_pfd_dmprof, pfe_pfd_dmprof_f32 (f32: the cube is x32, in->profs is not read) and
// pfe_pfd_dmprof_i16 (i16: the caller's struct; q: its arrays, in->profs is not read), and the
// _kill forms of the first two (kcall; kill: the caller's masks, or null)
static int pfd_dmprof_call(pfe_handle* h, const pfe_pfd_in* in, bool f32, const float* x32,
                           double* profile, float* chis, double* lyon8, uint32_t* status,
                           uint32_t flags, const pfe_pfd_i16_in* i16 = nullptr,
                           pfe::PfdI16Src* q = nullptr, bool kcall = false,
                           const pfe_pfd_kill* kill = nullptr, bool polcall = false,
                           const pfe_pfd_i16_pol* pol = nullptr) {
  const char* fn = polcall ? "pfd_dmprof_i16_pol"
                   : q     ? "pfd_dmprof_i16"
                   : kcall ? "pfd_dmprof_kill"
                           : "pfd_dmprof";
  int64_t n;
  int rc = call_check(h, fn, in, status != nullptr, n);
  if (rc || n == 0) return rc;
  if (!q && (rc = pfd_cube_check(h, fn, in, f32, x32, flags))) return rc;
  if (in->npart < 1 || in->nsub < 1 || in->proflen < 2)
    return set_err(h, PFE_EINVAL, "%s: shape %dx%dx%d", fn, in->npart, in->nsub, in->proflen);
  if (q && (rc = pfd_i16_check(h, fn, i16, flags, true, pol))) return rc;
  const bool useg = pfd_use_global(h, in);
  if (useg && !pfe::pfd_global_plan(in->nsub, in->proflen, n).ok)
    return pfd_shape_err(h, fn, in);
  if ((rc = call_begin(h))) return rc;
  // folds per pass: all of them, or what the part sums of a float32, byte-reversed or int16
  // cube allow (an int16 call deals with the byte order in its own kernels)
  const bool be = !q && (flags & PFE_FLAG_PFD_BSWAP), killed = pfd_killed(kill);
  const bool sums = f32 || be || q || killed;
  pfe::PfdKillSrc kmask;
  if (killed) kmask = pfd_kill_src(kill);
  const pfe::PfdKillSrc* km = killed ? &kmask : nullptr;
  const int ki = !q ? pfe::PFD_I16_NONE : q->wts ? pfe::PFD_I16_WEIGHTS : pfe::PFD_I16_PLAIN;
  const int64_t pass =
      sums ? pfe::pfd_f32_chunk(in->nsub, in->proflen, n, h->opt.pfd_f32_chunk) : n;
  const pfe::PfdGlobalPlan gp = useg ? pfe::pfd_global_plan(in->nsub, in->proflen, pass) : pfe::PfdGlobalPlan();
  hipStream_t st = h->stream;
  pfe::PfdArgs a = pfd_args(h, in);
  // split pipeline: two buffers of part sums, chunks of up to 4096 folds
  // (2 x 4096 x nsub x L doubles: 268 MB at 32 x 128)
  const bool split = !useg && h->opt.pfd_split && h->fork.side[0] && pfe::pfd_split_ok(a);
  const int64_t chunk = pass < 4096 ? pass : 4096;
  // (or the slabs of the global-memory kernel)
  const size_t ws_bytes =
      split ? 2 * (size_t)chunk * in->nsub * in->proflen * sizeof(double) : gp.bytes();
  if (split) {
    for (hipEvent_t& v : h->pev)
      if (!v) PFE_HIP(h, hipEventCreateWithFlags(&v, hipEventDisableTiming));
  }
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  const bool derive = flags & PFE_FLAG_PFD_AVGPROF;
  pfe::PfdDmprofStage s;
  rc = lay_out(h, s, [&](pfe::Arena& A) {
    return pfe::pfd_dmprof_layout(A, *in, host, profile, chis, lyon8, ws_bytes, sums ? pass : 0,
                                  derive, be || (killed && !f32), ki, kmask.mask(), pfd_nsum(pol));
  });
  if (rc || (host && (rc = stage_pfd(h, in, x32, q, s.in, a, pfd_npol(pol))))) return rc;
  if (host && killed && (rc = stage_kill(h, kmask, s.in.kparts, s.in.ksubs, n, in->npart, in->nsub)))
    return rc;
  double* wscal = nullptr;
  if (derive && (rc = pfd_avg_begin(h, in, host ? s.in.scal : nullptr, s.avg, a, wscal))) return rc;
  a.profile = host ? s.profile : profile;
  a.chis = host ? s.chis : chis;
  a.lyon8 = host ? s.lyon8 : lyon8;
  a.status = host ? s.status : status;
  for (int64_t c0 = 0; c0 < n; c0 += pass) {
    const int64_t cn = n - c0 < pass ? n - c0 : pass;
    pfe::PfdArgs b;
    if (derive && (rc = pfd_avg_pass(h, fn, a, x32, be, q, c0, cn, s.avg.csum, wscal, km))) return rc;
    if ((rc = pfd_pass(h, fn, a, x32, be, q, s.in.psum, c0, cn, b, km))) return rc;
    if (a.profile) b.profile = a.profile + c0 * a.L;
    if (a.chis) b.chis = a.chis + c0 * PFE_PFD_NDM;
    if (a.lyon8) b.lyon8 = a.lyon8 + c0 * 8;
    b.status = a.status + c0;
    if (useg) {
      b.tg = s.ws;
      b.gblocks = cn == pass ? gp.blocks : pfe::pfd_global_plan(in->nsub, in->proflen, cn).blocks;
      b.gstride = gp.stride;
    }
    hipError_t e = split ? pfe::launch_pfd_dmprof_split(b, st, h->fork.side[0], (double*)s.ws,
                                                        chunk, h->pev)
                         : pfe::launch_pfd_dmprof(b, st);
    if (e != hipSuccess)
      return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  }
  if (host) {
    if ((profile && (rc = fetch(h, profile, a.profile, (size_t)n * in->proflen))) ||
        (chis && (rc = fetch(h, chis, a.chis, (size_t)n * PFE_PFD_NDM))) ||
        (rc = fetch_out(h, lyon8, a.lyon8, 8, status, a.status, n)))
      return rc;
  }
  return call_end(h);
}

// pfe_pfd_avgprof (xd) / pfe_pfd_avgprof_f32 (xf): the other cube is null; their _kill forms
// (fn: the name the texts go under; kill: the caller's masks, or null)
static int pfd_avgprof_call(pfe_handle* h, const double* xd, const float* xf, bool f32, int npart,
                            int nsub, int proflen, int64_t n, double* out, int64_t out_stride,
                            uint32_t flags, const char* fn = "pfd_avgprof",
                            const pfe_pfd_kill* kill = nullptr) {
  if (!h) return PFE_EINVAL;
  h->err.clear();
  if ((f32 ? !xf : !xd) || !out) return set_err(h, PFE_EINVAL, "%s: null argument", fn);
  if (n < 0) return set_err(h, PFE_EINVAL, "%s: n < 0", fn);
  if (npart < 1 || nsub < 1 || proflen < 2)
    return set_err(h, PFE_EINVAL, "%s: shape %dx%dx%d", fn, npart, nsub, proflen);
  if (out_stride < 1) return set_err(h, PFE_EINVAL, "%s: out_stride < 1", fn);
  if (f32 && ((uintptr_t)xf & 3))
    return set_err(h, PFE_EINVAL, "%s: profs not 4-byte aligned", fn);
  const bool be = flags & PFE_FLAG_PFD_BSWAP;
  if (f32 && be)
    return set_err(h, PFE_EINVAL, "%s: PFE_FLAG_PFD_BSWAP is for the f64 call (8-byte values)", fn);
  if (n == 0) return PFE_OK;
  int rc = call_begin(h);
  if (rc) return rc;
  const int64_t E = (int64_t)npart * nsub * proflen;
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  const bool killed = pfd_killed(kill);
  pfe::PfdKillSrc kmask;
  if (killed) kmask = pfd_kill_src(kill);
  pfe::PfdAvgStage s;
  rc = lay_out(h, s, [&](pfe::Arena& A) {
    return pfe::pfd_avgprof_layout(A, E, n, host, f32, pfe::PFD_I16_NONE, 0, kmask.mask(), npart, nsub);
  });
  if (rc) return rc;
  if (host) {
    if ((rc = f32 ? stage_in(h, s.profs32, xf, (size_t)n * E) : stage_in(h, s.profs, xd, (size_t)n * E)))
      return rc;
    xf = s.profs32;
    xd = s.profs;
    if (killed && (rc = stage_kill(h, kmask, s.kparts, s.ksubs, n, npart, nsub))) return rc;
  }
  double* dout = host ? s.out : out;
  const int64_t dstride = host ? 1 : out_stride;
  const hipError_t e =
      killed ? pfe::launch_pfd_avgprof_kill(f32 ? (const void*)xf : (const void*)xd,
                                            f32  ? pfe::PFD_KILL_F32
                                            : be ? pfe::PFD_KILL_BE64
                                                 : pfe::PFD_KILL_F64,
                                            kmask, npart, nsub, proflen, n, s.csum, dout, dstride,
                                            h->stream)
      : f32 ? pfe::launch_pfd_avgprof_f32(xf, E, proflen, n, s.csum, dout, dstride, h->stream)
      : be ? pfe::launch_pfd_avgprof_be64(xd, E, proflen, n, s.csum, dout, dstride, h->stream)
           : pfe::launch_pfd_avgprof(xd, E, proflen, n, s.csum, dout, dstride, h->stream);
  if (e != hipSuccess)
    return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  if (host) {
    // the n values as one block, then to their places among the caller's doubles
    std::vector<double> dense;
    double* dst = out;
    if (out_stride > 1) {
      dense.resize((size_t)n);
      dst = dense.data();
    }
    if ((rc = fetch(h, dst, dout, (size_t)n))) return rc;
    PFE_HIP(h, hipStreamSynchronize(h->stream));
    if (out_stride > 1)
      for (int64_t i = 0; i < n; ++i) out[i * out_stride] = dense[(size_t)i];
  }
  return call_end(h);
}

int pfe_pfd_avgprof(pfe_handle* h, const double* profs, int32_t npart, int32_t nsub,
                    int32_t proflen, int64_t n, double* out, int64_t out_stride, uint32_t flags) {
  return pfd_avgprof_call(h, profs, nullptr, false, npart, nsub, proflen, n, out, out_stride, flags);
}

int pfe_pfd_avgprof_f32(pfe_handle* h, const float* profs, int32_t npart, int32_t nsub,
                        int32_t proflen, int64_t n, double* out, int64_t out_stride,
                        uint32_t flags) {
  return pfd_avgprof_call(h, nullptr, profs, true, npart, nsub, proflen, n, out, out_stride, flags);
}

int pfe_pfd_avgprof_kill(pfe_handle* h, const double* profs, int32_t npart, int32_t nsub,
                         int32_t proflen, int64_t n, const pfe_pfd_kill* kill, double* out,
                         int64_t out_stride, uint32_t flags) {
  return pfd_avgprof_call(h, profs, nullptr, false, npart, nsub, proflen, n, out, out_stride, flags,
                          "pfd_avgprof_kill", kill);
}

int pfe_pfd_avgprof_kill_f32(pfe_handle* h, const float* profs, int32_t npart, int32_t nsub,
                             int32_t proflen, int64_t n, const pfe_pfd_kill* kill, double* out,
                             int64_t out_stride, uint32_t flags) {
  return pfd_avgprof_call(h, nullptr, profs, true, npart, nsub, proflen, n, out, out_stride, flags,
                          "pfd_avgprof_kill", kill);
}

// pfe_pfd_avgprof_i16: the four arrays, the strides and the shape of `in` only
// and pfe_pfd_avgprof_i16_pol (polcall; pol: the caller's polarisations, or null)
static int pfd_avgprof_i16_call(pfe_handle* h, const pfe_pfd_i16_in* in, double* out,
                                int64_t out_stride, uint32_t flags, bool polcall = false,
                                const pfe_pfd_i16_pol* pol = nullptr) {
  const char* fn = polcall ? "pfd_avgprof_i16_pol" : "pfd_avgprof_i16";
  if (!h) return PFE_EINVAL;
  h->err.clear();
  if (!in || !out) return set_err(h, PFE_EINVAL, "%s: null argument", fn);
  const int64_t n = in->n;
  if (n < 0) return set_err(h, PFE_EINVAL, "%s: n < 0", fn);
  if (in->npart < 1 || in->nsub < 1 || in->proflen < 2)
    return set_err(h, PFE_EINVAL, "%s: shape %dx%dx%d", fn, in->npart, in->nsub, in->proflen);
  if (out_stride < 1) return set_err(h, PFE_EINVAL, "%s: out_stride < 1", fn);
  int rc = pfd_i16_check(h, fn, in, flags, false, pol);
  if (rc || n == 0) return rc;
  if ((rc = call_begin(h))) return rc;
  const int64_t ES = (int64_t)in->npart * in->nsub, E = ES * in->proflen;
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  pfe::PfdI16Src q = pfe::pfd_i16_src(*in, flags & PFE_FLAG_PFD_BSWAP, pfd_npol(pol), pfd_nsum(pol));
  pfe::PfdAvgStage s;
  rc = lay_out(h, s, [&](pfe::Arena& A) {
    return pfe::pfd_avgprof_layout(A, E, n, host, false,
                                   in->wts ? pfe::PFD_I16_WEIGHTS : pfe::PFD_I16_PLAIN, ES, 0, 0, 0,
                                   pfd_nsum(pol));
  });
  if (rc) return rc;
  if (host && (rc = stage_i16(h, q, s.data16, s.scl16, s.offs16, s.wts16, n, in->npart, in->nsub,
                              in->proflen, pfd_npol(pol))))
    return rc;
  double* dout = host ? s.out : out;
  const int64_t dstride = host ? 1 : out_stride;
  const hipError_t e = pfe::launch_pfd_avgprof_i16(q, in->npart, in->nsub, in->proflen, n, s.csum,
                                                   dout, dstride, h->stream);
  if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  if (host) {
    // the n values as one block, then to their places among the caller's doubles
    std::vector<double> dense;
    double* dst = out;
    if (out_stride > 1) {
      dense.resize((size_t)n);
      dst = dense.data();
    }
    if ((rc = fetch(h, dst, dout, (size_t)n))) return rc;
    PFE_HIP(h, hipStreamSynchronize(h->stream));
    if (out_stride > 1)
      for (int64_t i = 0; i < n; ++i) out[i * out_stride] = dense[(size_t)i];
  }
  return call_end(h);
}

int pfe_pfd_avgprof_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, int64_t out_stride,
                        uint32_t flags) {
  return pfd_avgprof_i16_call(h, in, out, out_stride, flags);
}

int pfe_pfd_avgprof_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                            double* out, int64_t out_stride, uint32_t flags) {
  return pfd_avgprof_i16_call(h, in, out, out_stride, flags, true, pol);
}

// pfe_pfd_scrunch (xd), pfe_pfd_scrunch_f32 (xf) and pfe_pfd_scrunch_i16 (i16: the four arrays,
// the strides and the shape of the caller's struct; the shape arguments are then its own)
static int pfd_scrunch_call(pfe_handle* h, const char* fn, const double* xd, const float* xf,
                            bool f32, const pfe_pfd_i16_in* i16, int npart, int nchan, int nbin, int64_t n,
                            const pfe_pfd_scrunch_how* how, double* out, uint32_t flags,
                            const pfe_pfd_i16_pol* pol = nullptr) {
  if (!h) return PFE_EINVAL;
  h->err.clear();
  if (!how || !out) return set_err(h, PFE_EINVAL, "%s: null argument", fn);
  if (n < 0) return set_err(h, PFE_EINVAL, "%s: n < 0", fn);
  if (npart < 1 || nchan < 1 || nbin < 1)
    return set_err(h, PFE_EINVAL, "%s: shape %dx%dx%d", fn, npart, nchan, nbin);
  if (flags & PFE_FLAG_PFD_AVGPROF)
    return set_err(h, PFE_EINVAL, "%s: PFE_FLAG_PFD_AVGPROF is for the calls that read scal", fn);
  if (!i16 && (flags & PFE_FLAG_PFD_BSWAP))
    return set_err(h, PFE_EINVAL, "%s: PFE_FLAG_PFD_BSWAP is for the _i16 form", fn);
  if (how->fscr < 1 || how->bscr < 1)
    return set_err(h, PFE_EINVAL, "%s: fscr %d and bscr %d must be >= 1", fn, how->fscr, how->bscr);
  if (nchan % how->fscr)
    return set_err(h, PFE_EINVAL, "%s: fscr %d does not divide nchan %d", fn, how->fscr, nchan);
  if (nbin % how->bscr)
    return set_err(h, PFE_EINVAL, "%s: bscr %d does not divide nbin %d", fn, how->bscr, nbin);
  int rc;
  if (i16) {
    if ((rc = pfd_i16_check(h, fn, i16, flags, false, pol))) return rc;
  } else {
    if (f32 ? !xf : !xd) return set_err(h, PFE_EINVAL, "%s: null input array", fn);
    if (f32 ? ((uintptr_t)xf & 3) : ((uintptr_t)xd & 7))
      return set_err(h, PFE_EINVAL, "%s: profs not %d-byte aligned", fn, f32 ? 4 : 8);
  }
  if ((uintptr_t)how->rot & 3) return set_err(h, PFE_EINVAL, "%s: rot not 4-byte aligned", fn);
  if ((uintptr_t)out & 7) return set_err(h, PFE_EINVAL, "%s: out not 8-byte aligned", fn);
  if (n == 0) return PFE_OK;
  if ((rc = call_begin(h))) return rc;
  const int64_t ES = (int64_t)npart * nchan, E = ES * nbin;
  const int64_t GK = (int64_t)(nchan / how->fscr) * (nbin / how->bscr);
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  pfe::PfdScrunchSrc x;
  x.f64 = xd;
  x.f32 = xf;
  if (i16) x.i16 = pfe::pfd_i16_src(*i16, flags & PFE_FLAG_PFD_BSWAP, pfd_npol(pol), pfd_nsum(pol));
  const int32_t* rot = how->rot;
  double* z = out;
  if (host) {
    pfe::PfdScrunchStage s;
    rc = lay_out(h, s, [&](pfe::Arena& A) {
      return pfe::pfd_scrunch_layout(
          A, E, ES, nchan, GK, n, true, f32,
          !i16 ? pfe::PFD_I16_NONE : i16->wts ? pfe::PFD_I16_WEIGHTS : pfe::PFD_I16_PLAIN,
          rot != nullptr, pfd_nsum(pol));
    });
    if (rc) return rc;
    if (i16) {
      if ((rc = stage_i16(h, x.i16, s.data16, s.scl16, s.offs16, s.wts16, n, npart, nchan, nbin,
                          pfd_npol(pol))))
        return rc;
    } else if (f32) {
      if ((rc = stage_in(h, s.profs32, xf, (size_t)n * E))) return rc;
      x.f32 = s.profs32;
    } else {
      if ((rc = stage_in(h, s.profs, xd, (size_t)n * E))) return rc;
      x.f64 = s.profs;
    }
    if (rot) {
      if ((rc = stage_in(h, s.rot, rot, (size_t)n * nchan))) return rc;
      rot = s.rot;
    }
    z = s.out;
  }
  const hipError_t e = pfe::launch_pfd_scrunch(x, rot, z, npart, nchan, nbin, how->fscr, how->bscr, n,
                                               h->opt.pfd_scrunch_direct != 0, h->stream);
  if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
  if (host) {
    if ((rc = fetch(h, out, z, (size_t)n * GK))) return rc;
    PFE_HIP(h, hipStreamSynchronize(h->stream));
  }
  return call_end(h);
}

int pfe_pfd_scrunch(pfe_handle* h, const double* profs, int32_t npart, int32_t nchan, int32_t nbin,
                    int64_t n, const pfe_pfd_scrunch_how* how, double* out, uint32_t flags) {
  return pfd_scrunch_call(h, "pfd_scrunch", profs, nullptr, false, nullptr, npart, nchan, nbin, n, how, out,
                          flags);
}

int pfe_pfd_scrunch_f32(pfe_handle* h, const float* profs, int32_t npart, int32_t nchan,
                        int32_t nbin, int64_t n, const pfe_pfd_scrunch_how* how, double* out,
                        uint32_t flags) {
  return pfd_scrunch_call(h, "pfd_scrunch_f32", nullptr, profs, true, nullptr, npart, nchan, nbin, n, how,
                          out, flags);
}

int pfe_pfd_scrunch_i16(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_scrunch_how* how,
                        double* out, uint32_t flags) {
  if (h && !in) {
    h->err.clear();
    return set_err(h, PFE_EINVAL, "pfd_scrunch_i16: null argument");
  }
  if (!h) return PFE_EINVAL;
  return pfd_scrunch_call(h, "pfd_scrunch_i16", nullptr, nullptr, false, in, in->npart, in->nsub, in->proflen,
                          in->n, how, out, flags);
}

int pfe_pfd_scrunch_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                            const pfe_pfd_scrunch_how* how, double* out, uint32_t flags) {
  if (h && !in) {
    h->err.clear();
    return set_err(h, PFE_EINVAL, "pfd_scrunch_i16_pol: null argument");
  }
  if (!h) return PFE_EINVAL;
  return pfd_scrunch_call(h, "pfd_scrunch_i16_pol", nullptr, nullptr, false, in, in->npart, in->nsub,
                          in->proflen, in->n, how, out, flags, pol);
}

int pfe_pfd_dmprof_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* profile, float* chis,
                       double* lyon8, uint32_t* status, uint32_t flags) {
  if (h && !in) {
    h->err.clear();
    return set_err(h, PFE_EINVAL, "pfd_dmprof_i16: null argument");
  }
  PfdI16View v(in, flags);
  return pfd_dmprof_call(h, v.view, false, nullptr, profile, chis, lyon8, status, flags, in, v.q);
}

int pfe_pfd_dmprof_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                           double* profile, float* chis, double* lyon8, uint32_t* status,
                           uint32_t flags) {
  if (h && !in) {
    h->err.clear();
    return set_err(h, PFE_EINVAL, "pfd_dmprof_i16_pol: null argument");
  }
  PfdI16View v(in, flags, pol);
  return pfd_dmprof_call(h, v.view, false, nullptr, profile, chis, lyon8, status, flags, in, v.q, false,
                         nullptr, true, pol);
}

int pfe_pfd_dmprof(pfe_handle* h, const pfe_pfd_in* in, double* profile, float* chis,
                   double* lyon8, uint32_t* status, uint32_t flags) {
  return pfd_dmprof_call(h, in, false, nullptr, profile, chis, lyon8, status, flags);
}

int pfe_pfd_dmprof_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* profile, float* chis,
                       double* lyon8, uint32_t* status, uint32_t flags) {
  const PfdF32View v(in);
  return pfd_dmprof_call(h, v.view, true, v.x32, profile, chis, lyon8, status, flags);
}

int pfe_pfd_dmprof_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill,
                        double* profile, float* chis, double* lyon8, uint32_t* status,
                        uint32_t flags) {
  return pfd_dmprof_call(h, in, false, nullptr, profile, chis, lyon8, status, flags, nullptr, nullptr,
                         true, kill);
}

int pfe_pfd_dmprof_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                            double* profile, float* chis, double* lyon8, uint32_t* status,
                            uint32_t flags) {
  const PfdF32View v(in);
  return pfd_dmprof_call(h, v.view, true, v.x32, profile, chis, lyon8, status, flags, nullptr,
                         nullptr, true, kill);
}

}  // extern "C"

// pfe_pfd_bates22 (groups = PFD_G_ALL: out n x 22) and the PFD group calls (one group: its k
// columns from column c0 of the 22-score vector, or of the DM-fit inputs par22 when c0 < 0),
// and their float32 forms (f32: the cube is x32, in->profs is not read)
static int pfd_scores_call(pfe_handle* h, const pfe_pfd_in* in, bool f32, const float* x32,
                           double* out, uint32_t* status, uint32_t flags, const char* fn,
                           unsigned groups, int c0, int k, const pfe_pfd_i16_in* i16 = nullptr,
                           pfe::PfdI16Src* q = nullptr, const pfe_pfd_kill* kill = nullptr,
                           const pfe_pfd_i16_pol* pol = nullptr) {
  int64_t n;
  int rc = call_check(h, fn, in, out && status, n);
  if (rc || n == 0) return rc;
  if (!q && (rc = pfd_cube_check(h, fn, in, f32, x32, flags))) return rc;
  if (in->npart < 1 || in->nsub < 2 || in->proflen < 8 || in->proflen > 1024)
    return set_err(h, PFE_EINVAL, "%s: shape %dx%dx%d unsupported", fn, in->npart, in->nsub,
                   in->proflen);
  if (q && (rc = pfd_i16_check(h, fn, i16, flags, true, pol))) return rc;
  const bool useg = pfd_use_global(h, in);
  if (useg && !pfe::pfd_global_plan(in->nsub, in->proflen, n).ok)
    return pfd_shape_err(h, fn, in);
  if ((rc = call_begin(h))) return rc;
  // folds per pass: all of them, or what the part sums of a float32, byte-reversed or int16
  // cube allow
  const bool be = !q && (flags & PFE_FLAG_PFD_BSWAP), killed = pfd_killed(kill);
  const bool sums = f32 || be || q || killed;
  pfe::PfdKillSrc kmask;
  if (killed) kmask = pfd_kill_src(kill);
  const pfe::PfdKillSrc* km = killed ? &kmask : nullptr;
  const int ki = !q ? pfe::PFD_I16_NONE : q->wts ? pfe::PFD_I16_WEIGHTS : pfe::PFD_I16_PLAIN;
  const int64_t pass =
      sums ? pfe::pfd_f32_chunk(in->nsub, in->proflen, n, h->opt.pfd_f32_chunk) : n;
  auto plan = [&](int64_t cn) {
    return useg ? pfe::pfd_global_plan(in->nsub, in->proflen, cn) : pfe::PfdGlobalPlan();
  };
  hipStream_t st = h->stream;
  pfe::PfdArgs a = pfd_args(h, in);
  const bool all = groups == pfe::PFD_G_ALL;
  const bool host = !(flags & PFE_FLAG_DEVICE_PTRS);
  // only the chi^2 sweep reads the average: a call without it has nothing to derive
  const bool derive = (flags & PFE_FLAG_PFD_AVGPROF) && (groups & pfe::PFD_G_DM);
  const int cus = pfe::device_cus();
  // the scratch with the chain's workspace laid out for a pass of cn folds
  auto walk = [&](int64_t cn) {
    return [&, cn](pfe::Arena& A) {
      return pfe::pfd_scores_layout(A, *in, host, groups, k, plan(cn).bytes(), cus, h->opt,
                                    sums ? pass : 0, cn, derive, be || (killed && !f32), ki,
                                    kmask.mask(), pfd_nsum(pol));
    };
  };
  if (n % pass) {  // a shorter last pass: its layout fits as well
    pfe::Arena last;
    walk(n % pass)(last);
    if ((rc = ensure_scratch(h, last.bytes()))) return rc;
  }
  pfe::PfdScoresStage s;
  rc = lay_out(h, s, walk(pass));
  if (rc || (host && (rc = stage_pfd(h, in, x32, q, s.in, a, pfd_npol(pol))))) return rc;
  if (host && killed && (rc = stage_kill(h, kmask, s.in.kparts, s.in.ksubs, n, in->npart, in->nsub)))
    return rc;
  double* wscal = nullptr;
  if (derive && (rc = pfd_avg_begin(h, in, host ? s.in.scal : nullptr, s.avg, a, wscal))) return rc;
  double* dout = host ? s.out : out;
  uint32_t* dstat = host ? s.status : status;
  for (int64_t f0 = 0; f0 < n; f0 += pass) {
    const int64_t cn = n - f0 < pass ? n - f0 : pass;
    if (cn != pass) {
      pfe::Arena place{(uintptr_t)h->scratch};
      s = walk(cn)(place);
    }
    pfe::PfdArgs b;
    if (derive && (rc = pfd_avg_pass(h, fn, a, x32, be, q, f0, cn, s.avg.csum, wscal, km))) return rc;
    if ((rc = pfd_pass(h, fn, a, x32, be, q, s.in.psum, f0, cn, b, km))) return rc;
    // a group call scores into a 22-column scratch of its own
    double* d22 = all ? dout + f0 * 22 : s.d22;
    if (useg) {
      const pfe::PfdGlobalPlan gp = plan(cn);
      b.tg = s.tg;
      b.gblocks = gp.blocks;
      b.gstride = gp.stride;
    }
    hipError_t e =
        pfe::launch_pfd22(b, d22, dstat + f0, s.work, st, &h->fork, h->opt, groups, !all);
    if (e != hipSuccess) return set_err(h, PFE_EDEVICE, "%s launch: %s", fn, hipGetErrorString(e));
    if (!all) {
      hipLaunchKernelGGL(k_take_cols, dim3((unsigned)((cn * k + 255) / 256)), dim3(256), 0, st,
                         c0 < 0 ? s.work.par22 : d22, c0 < 0 ? 8 : 22, c0 < 0 ? 0 : c0, k, cn,
                         dout + f0 * k);
      PFE_HIP(h, hipGetLastError());
    }
  }
  if (host && (rc = fetch_out(h, out, dout, k, status, dstat, n))) return rc;
  return call_end(h);
}

// what each of the four score calls asks of pfd_scores_call
struct PfdScores {
  const char* fn;
  unsigned groups;
  int c0, k;
};
static constexpr PfdScores PFD_BATES22{"pfd_bates22", pfe::PFD_G_ALL, 0, 22};
// [period_ms, snr, dm, width] as getCandidateParameters returns them: par22's first columns
static constexpr PfdScores PFD_PARAMS4{"pfd_params4", pfe::PFD_G_PARAMS, -1, 4};
static constexpr PfdScores PFD_DMFIT4{"pfd_dmfit4", pfe::PFD_G_PARAMS | pfe::PFD_G_DM, 15, 4};
static constexpr PfdScores PFD_SUBBAND3{"pfd_subband3", pfe::PFD_G_PARAMS | pfe::PFD_G_SUB, 19, 3};

static int pfd_scores_f64(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                          uint32_t flags, const PfdScores& c) {
  return pfd_scores_call(h, in, false, nullptr, out, status, flags, c.fn, c.groups, c.c0, c.k);
}
static int pfd_scores_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                          uint32_t flags, const PfdScores& c) {
  const PfdF32View v(in);
  return pfd_scores_call(h, v.view, true, v.x32, out, status, flags, c.fn, c.groups, c.c0, c.k);
}

// the _kill forms: the texts under the _kill name, the masks beside `in`
static int pfd_scores_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                           uint32_t* status, uint32_t flags, const PfdScores& c) {
  const std::string fn = std::string(c.fn) + "_kill";
  return pfd_scores_call(h, in, false, nullptr, out, status, flags, fn.c_str(), c.groups, c.c0, c.k,
                         nullptr, nullptr, kill);
}
static int pfd_scores_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                               double* out, uint32_t* status, uint32_t flags, const PfdScores& c) {
  const PfdF32View v(in);
  const std::string fn = std::string(c.fn) + "_kill";
  return pfd_scores_call(h, v.view, true, v.x32, out, status, flags, fn.c_str(), c.groups, c.c0,
                         c.k, nullptr, nullptr, kill);
}

static int pfd_scores_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                          uint32_t flags, const PfdScores& c) {
  PfdI16View v(in, flags);
  const std::string fn = std::string(c.fn) + "_i16";
  return pfd_scores_call(h, v.view, false, nullptr, out, status, flags, fn.c_str(), c.groups, c.c0,
                         c.k, in, v.q);
}
// the _i16_pol forms: the texts under the _i16_pol name, the polarisations beside `in`
static int pfd_scores_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                              double* out, uint32_t* status, uint32_t flags, const PfdScores& c) {
  PfdI16View v(in, flags, pol);
  const std::string fn = std::string(c.fn) + "_i16_pol";
  return pfd_scores_call(h, v.view, false, nullptr, out, status, flags, fn.c_str(), c.groups, c.c0,
                         c.k, in, v.q, nullptr, pol);
}

extern "C" {

int pfe_pfd_bates22_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                            double* out, uint32_t* status, uint32_t flags) {
  return pfd_scores_i16_pol(h, in, pol, out, status, flags, PFD_BATES22);
}
int pfe_pfd_params4_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                            double* out, uint32_t* status, uint32_t flags) {
  return pfd_scores_i16_pol(h, in, pol, out, status, flags, PFD_PARAMS4);
}
int pfe_pfd_dmfit4_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                           double* out, uint32_t* status, uint32_t flags) {
  return pfd_scores_i16_pol(h, in, pol, out, status, flags, PFD_DMFIT4);
}
int pfe_pfd_subband3_i16_pol(pfe_handle* h, const pfe_pfd_i16_in* in, const pfe_pfd_i16_pol* pol,
                             double* out, uint32_t* status, uint32_t flags) {
  return pfd_scores_i16_pol(h, in, pol, out, status, flags, PFD_SUBBAND3);
}

int pfe_pfd_bates22_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                        uint32_t flags) {
  return pfd_scores_i16(h, in, out, status, flags, PFD_BATES22);
}
int pfe_pfd_params4_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                        uint32_t flags) {
  return pfd_scores_i16(h, in, out, status, flags, PFD_PARAMS4);
}
int pfe_pfd_dmfit4_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                       uint32_t flags) {
  return pfd_scores_i16(h, in, out, status, flags, PFD_DMFIT4);
}
int pfe_pfd_subband3_i16(pfe_handle* h, const pfe_pfd_i16_in* in, double* out, uint32_t* status,
                         uint32_t flags) {
  return pfd_scores_i16(h, in, out, status, flags, PFD_SUBBAND3);
}

int pfe_pfd_bates22(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                    uint32_t flags) {
  return pfd_scores_f64(h, in, out, status, flags, PFD_BATES22);
}
int pfe_pfd_params4(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                    uint32_t flags) {
  return pfd_scores_f64(h, in, out, status, flags, PFD_PARAMS4);
}
int pfe_pfd_dmfit4(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                   uint32_t flags) {
  return pfd_scores_f64(h, in, out, status, flags, PFD_DMFIT4);
}
int pfe_pfd_subband3(pfe_handle* h, const pfe_pfd_in* in, double* out, uint32_t* status,
                     uint32_t flags) {
  return pfd_scores_f64(h, in, out, status, flags, PFD_SUBBAND3);
}

int pfe_pfd_bates22_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                        uint32_t flags) {
  return pfd_scores_f32(h, in, out, status, flags, PFD_BATES22);
}
int pfe_pfd_params4_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                        uint32_t flags) {
  return pfd_scores_f32(h, in, out, status, flags, PFD_PARAMS4);
}
int pfe_pfd_dmfit4_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                       uint32_t flags) {
  return pfd_scores_f32(h, in, out, status, flags, PFD_DMFIT4);
}
int pfe_pfd_subband3_f32(pfe_handle* h, const pfe_pfd_f32_in* in, double* out, uint32_t* status,
                         uint32_t flags) {
  return pfd_scores_f32(h, in, out, status, flags, PFD_SUBBAND3);
}

int pfe_pfd_bates22_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                        uint32_t* status, uint32_t flags) {
  return pfd_scores_kill(h, in, kill, out, status, flags, PFD_BATES22);
}

int pfe_pfd_params4_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                        uint32_t* status, uint32_t flags) {
  return pfd_scores_kill(h, in, kill, out, status, flags, PFD_PARAMS4);
}

int pfe_pfd_dmfit4_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                       uint32_t* status, uint32_t flags) {
  return pfd_scores_kill(h, in, kill, out, status, flags, PFD_DMFIT4);
}

int pfe_pfd_subband3_kill(pfe_handle* h, const pfe_pfd_in* in, const pfe_pfd_kill* kill, double* out,
                         uint32_t* status, uint32_t flags) {
  return pfd_scores_kill(h, in, kill, out, status, flags, PFD_SUBBAND3);
}

int pfe_pfd_bates22_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                            double* out, uint32_t* status, uint32_t flags) {
  return pfd_scores_kill_f32(h, in, kill, out, status, flags, PFD_BATES22);
}

int pfe_pfd_params4_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                            double* out, uint32_t* status, uint32_t flags) {
  return pfd_scores_kill_f32(h, in, kill, out, status, flags, PFD_PARAMS4);
}

int pfe_pfd_dmfit4_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                           double* out, uint32_t* status, uint32_t flags) {
  return pfd_scores_kill_f32(h, in, kill, out, status, flags, PFD_DMFIT4);
}

int pfe_pfd_subband3_kill_f32(pfe_handle* h, const pfe_pfd_f32_in* in, const pfe_pfd_kill* kill,
                             double* out, uint32_t* status, uint32_t flags) {
  return pfd_scores_kill_f32(h, in, kill, out, status, flags, PFD_SUBBAND3);
}

}  // extern "C"
