"""ctypes binding of libpfe.so (the C-ABI declared in include/pfe.h).

This is the reference-side binding a maintainer would add to PulsarFeatureExtractor: a thin
ctypes layer over the extern "C" entry points.  It never falls back to a CPU
implementation: if the library is missing or no GPU is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PFE_LIBRARY", os.path.join(_HERE, "lib", "libpfe.so"))

PFE_OK = 0
PFE_FLAG_DEVICE_PTRS = 0x1
PFE_NSCAL = 8
PFE_ST_FAIL_MASK = 0x0FF
PFE_ST_SINE_FAIL = 0x001
PFE_ST_GAUSS_FAIL = 0x002
PFE_ST_DMFIT_FAIL = 0x004
PFE_ST_SUBBAND_FAIL = 0x008
PFE_ST_UNSUPPORTED = 0x010
PFE_ST_DGF_INDEXERROR = 0x100

# every symbol include/pfe.h declares (checked by tests/test_capi_symbols.py)
EXPORTED_SYMBOLS = (
    "pfe_abi_version",
    "pfe_device_count",
    "pfe_create",
    "pfe_destroy",
    "pfe_last_error",
    "pfe_set_stream",
    "pfe_synchronize",
    "pfe_set_option",
    "pfe_get_option",
    "pfe_host_alloc",
    "pfe_host_free",
    "pfe_lyon8_u8",
    "pfe_lyon8_f64",
    "pfe_bates22",
    "pfe_subband3",
    "pfe_sinusoid4",
    "pfe_gauss7",
    "pfe_params4",
    "pfe_dmfit4",
    "pfe_sinusoid4_f64",
    "pfe_gauss7_f64",
    "pfe_subband3_f64",
    "pfe_bates22_f64",
    "pfe_pfd_dmprof",
    "pfe_pfd_bates22",
    "pfe_pfd_params4",
    "pfe_pfd_dmfit4",
    "pfe_pfd_subband3",
    "pfe_pfd_dmprof_f32",
    "pfe_pfd_bates22_f32",
    "pfe_pfd_params4_f32",
    "pfe_pfd_dmfit4_f32",
    "pfe_pfd_subband3_f32",
    "pfe_lyon8_f32",
    "pfe_sinusoid4_f32",
    "pfe_gauss7_f32",
    "pfe_subband3_f32",
    "pfe_bates22_f32",
    "pfe_pfd_avgprof",
    "pfe_pfd_avgprof_f32",
    "pfe_pfd_dmprof_i16",
    "pfe_pfd_bates22_i16",
    "pfe_pfd_params4_i16",
    "pfe_pfd_dmfit4_i16",
    "pfe_pfd_subband3_i16",
    "pfe_pfd_avgprof_i16",
    "pfe_pfd_dmprof_i16_pol",
    "pfe_pfd_bates22_i16_pol",
    "pfe_pfd_params4_i16_pol",
    "pfe_pfd_dmfit4_i16_pol",
    "pfe_pfd_subband3_i16_pol",
    "pfe_pfd_avgprof_i16_pol",
    "pfe_pfd_scrunch_i16_pol",
    "pfe_pfd_dmprof_kill",
    "pfe_pfd_bates22_kill",
    "pfe_pfd_params4_kill",
    "pfe_pfd_dmfit4_kill",
    "pfe_pfd_subband3_kill",
    "pfe_pfd_avgprof_kill",
    "pfe_pfd_dmprof_kill_f32",
    "pfe_pfd_bates22_kill_f32",
    "pfe_pfd_params4_kill_f32",
    "pfe_pfd_dmfit4_kill_f32",
    "pfe_pfd_subband3_kill_f32",
    "pfe_pfd_avgprof_kill_f32",
    "pfe_pfd_scrunch",
    "pfe_pfd_scrunch_f32",
    "pfe_pfd_scrunch_i16",
)
PFE_FLAG_PFD_AVGPROF = 0x2  # PFD calls: derive scal[:, PFE_PFD_AVGPROF] from the cube
PFE_FLAG_PFD_BSWAP = 0x4    # f64 and int16 PFD calls: the cube (int16: and scl, offs, wts) byte-reversed
PFE_PFD_AVGPROF = 2
PFE_PFD_NSCAL = 8
PFE_PFD_NDM = 100
PFE_ST_PFD_DMCURVE_FAIL = 0x020
# every symbol include/pfe_io.h declares
EXPORTED_IO_SYMBOLS = (
    "pfe_phcx_parse",
    "pfe_phcx_count",
    "pfe_phcx_info_get",
    "pfe_phcx_fetch",
    "pfe_phcx_pack",
    "pfe_phcx_free",
    "pfe_phcx_info_all",
    "pfe_format_rows",
    "pfe_pfd_scan",
    "pfe_pfd_count",
    "pfe_pfd_info_all",
    "pfe_pfd_fetch",
    "pfe_pfd_pack",
    "pfe_pfd_free",
)
PFE_PHCX_PROFILE, PFE_PHCX_LYON_DM, PFE_PHCX_SUBBANDS, PFE_PHCX_DM_CURVE, PFE_PHCX_FIT_BLOCK = range(5)
PFE_IO_STATUS = {0: "ok", 1: "open", 2: "gzip", 3: "xml", 4: "value", 5: "range", 6: "shape",
                 7: "header", 8: "cube"}
(PFE_PFD_F_DMS, PFE_PFD_F_PERIODS, PFE_PFD_F_PDOTS, PFE_PFD_F_STATS, PFE_PFD_F_SUBFREQS,
 PFE_PFD_F_HEAD, PFE_PFD_F_FILENM, PFE_PFD_F_CANDNM, PFE_PFD_F_TELESCOPE, PFE_PFD_F_PGDEV,
 PFE_PFD_F_RASTR, PFE_PFD_F_DECSTR) = range(12)
PFE_PFD_NHEAD = 23
# the doubles of PFE_PFD_F_HEAD, in order (PFDData attribute names; orb is seven of them)
PFD_HEAD_NAMES = ("dt", "startT", "endT", "tepoch", "bepoch", "avgvoverc", "lofreq", "chan_wid",
                  "bestdm", "topo_p1", "bary_p1", "fold_p1") + ("orb",) * 7 + (
                      "binspersec", "subdeltafreq", "losubfreq", "varprof")
assert len(PFD_HEAD_NAMES) == PFE_PFD_NHEAD


# handle options (include/pfe.h PFE_OPT_*): name -> (id, default)
OPTIONS = {
    "solver": 1,        # 0 pooled (default), 1 batched, 2 wave per fit
    "serial": 2,
    "handover": 3,
    "gslots": 4,
    "lyon8_blocks": 5,
    "lyon8_burst": 6,
    "pfd_waves": 7,
    "lyon8_dm": 8,      # DataBlock kernels: 0 default, 1 round 3, 2 exact power sums (pfe.h)
    "pfd_split": 9,     # 0 fused kernel (default), 1 part sums streamed beside the sweep
    "lyon8_dm_split": 10,  # 1 (default) chain splits + paired one-chunk rows, 2 splits only, 0 off
    "pfd_global": 11,   # 0 folds that fit stay in LDS (default), 1 every fold through global scratch
    "subf64_global": 12,  # float sub-bands: 0 shapes that fit stay in LDS (default), 1 all in scratch
    # float32 and byte-swapped folds: folds per pass (0, default: what 1 GiB of part sums holds)
    "pfd_f32_chunk": 13,
    "pfd_scrunch_direct": 14,  # scrunch calls: 0 rows that fit are summed in LDS (default), 1 one lane per bin
}
SOLVERS = {"pooled": 0, "batched": 1, "wave": 2}


class PfeError(RuntimeError):
    """Raised when a libpfe call fails (the message is pfe_last_error())."""


class BatesIn(C.Structure):
    _fields_ = [
        ("prof", C.c_void_p),
        ("lp", C.c_int32),
        ("sub", C.c_void_p),
        ("nsub", C.c_int32),
        ("lsb", C.c_int32),
        ("dmcurve", C.c_void_p),
        ("ndm", C.c_int32),
        ("scal", C.c_void_p),
        ("n", C.c_int64),
    ]


class BatesF64In(BatesIn):
    """pfe_bates_f64_in: the fields of pfe_bates_in, prof and sub pointing at doubles."""


class BatesF32In(BatesIn):
    """pfe_bates_f32_in: the fields of pfe_bates_in, prof, sub and dmcurve pointing at floats."""


class PfdIn(C.Structure):
    _fields_ = [
        ("profs", C.c_void_p),
        ("subfreqs", C.c_void_p),
        ("scal", C.c_void_p),
        ("npart", C.c_int32),
        ("nsub", C.c_int32),
        ("proflen", C.c_int32),
        ("n", C.c_int64),
    ]


class PfdF32In(PfdIn):
    """pfe_pfd_f32_in: the fields of pfe_pfd_in, profs pointing at floats."""


class PfdI16In(C.Structure):
    """pfe_pfd_i16_in: an int16 cube with its float32 scale, offset and weight per (fold, part,
    sub-band), dense (both strides 0) or in the rows of a table (byte strides)."""
    _fields_ = [
        ("data", C.c_void_p),
        ("scl", C.c_void_p),
        ("offs", C.c_void_p),
        ("wts", C.c_void_p),
        ("fold_stride", C.c_int64),
        ("part_stride", C.c_int64),
        ("subfreqs", C.c_void_p),
        ("scal", C.c_void_p),
        ("npart", C.c_int32),
        ("nsub", C.c_int32),
        ("proflen", C.c_int32),
        ("n", C.c_int64),
    ]


class PfdI16Pol(C.Structure):
    """pfe_pfd_i16_pol: the polarisations an int16 cube stores per (fold, part), 1..4, and the
    leading ones that are summed, 1 or 2."""
    _fields_ = [("npol", C.c_int32), ("nsum", C.c_int32)]


class PfdKill(C.Structure):
    """pfe_pfd_kill: the killed parts (n x npart) and sub-bands (n x nsub) of a batch of folds,
    one byte each, non-zero = killed; either may be null."""
    _fields_ = [("parts", C.c_void_p), ("subs", C.c_void_p)]


class PfdScrunchHow(C.Structure):
    """pfe_pfd_scrunch_how: the rotation per (fold, channel), or null, and the two factors."""
    _fields_ = [("rot", C.c_void_p), ("fscr", C.c_int32), ("bscr", C.c_int32)]


class PhcxInfo(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("superb", C.c_int32),
        ("section", C.c_int32),
        ("lp", C.c_int32),
        ("nsub", C.c_int32),
        ("lsb", C.c_int32),
        ("ndm", C.c_int32),
        ("reserved", C.c_int32),
        ("ld", C.c_int64),
        ("lfit", C.c_int64),
        ("scal", C.c_double * 8),
    ]


# numpy view of pfe_phcx_info (include/pfe_io.h), for pfe_phcx_info_all
PHCX_INFO_DTYPE = np.dtype([
    ("status", "<i4"), ("superb", "<i4"), ("section", "<i4"), ("lp", "<i4"),
    ("nsub", "<i4"), ("lsb", "<i4"), ("ndm", "<i4"), ("reserved", "<i4"),
    ("ld", "<i8"), ("lfit", "<i8"), ("scal", "<f8", (8,)),
])
assert PHCX_INFO_DTYPE.itemsize == C.sizeof(PhcxInfo)

# numpy view of pfe_pfd_info (include/pfe_io.h), for pfe_pfd_info_all
PFD_INFO_DTYPE = np.dtype([
    ("status", "<i4"), ("big_endian", "<i4"), ("npart", "<i4"), ("nsub", "<i4"),
    ("proflen", "<i4"), ("numdms", "<i4"), ("numperiods", "<i4"), ("numpdots", "<i4"),
    ("numchan", "<i4"), ("chanpersub", "<i4"), ("has_posn", "<i4"), ("slen", "<i4", (6,)),
    ("reserved", "<i4"), ("rows", "<i8"), ("stat_rows", "<i8"), ("cube_off", "<i8"),
    ("stats_off", "<i8"), ("scal", "<f8", (8,)),
])
assert PFD_INFO_DTYPE.itemsize == 168

_lib = None
_lock = threading.Lock()


def _preload_torch_hip_runtime():
    """Share ONE HIP runtime with PyTorch.

    torch ships its own libamdhip64.so (soname libamdhip64.so.7).  If libpfe.so resolved
    /opt/rocm's copy first, the process would hold two HIP runtimes and whichever initialises
    second sees no GPU.  Loading torch's copy globally first makes libpfe's NEEDED entry bind
    to it, and torch later recognises the same file (same inode) -- without importing torch.
    """
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return None
    for loc in spec.submodule_search_locations:
        p = os.path.join(loc, "lib", "libamdhip64.so")
        if os.path.exists(p):
            return C.CDLL(p, mode=C.RTLD_GLOBAL)
    return None


def load_library(path: str | None = None) -> C.CDLL:
    """Load libpfe.so and declare its signatures.  Raises OSError when it is missing."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise OSError(
                f"libpfe.so not found at {p}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)"
            )
        if os.environ.get("PFE_SYSTEM_HIP", "0") != "1":
            _preload_torch_hip_runtime()
        lib = C.CDLL(p)
        vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
        ptr, rc = C.POINTER, C.c_int
        lyon = [vp, vp, i64, i32, vp, i64, i32, i64, vp, vp, u32]
        bates = [vp, ptr(BatesIn), vp, vp, u32]
        pfd = [vp, ptr(PfdIn), vp, vp, u32]
        pfd_f32 = [vp, ptr(PfdF32In), vp, vp, u32]
        pfd_i16 = [vp, ptr(PfdI16In), vp, vp, u32]
        pfd_i16_pol = [vp, ptr(PfdI16In), ptr(PfdI16Pol), vp, vp, u32]
        f64 = [vp, vp, i32, i64, vp, vp, u32]
        bates_f64 = [vp, ptr(BatesF64In), vp, vp, u32]
        bates_f32 = [vp, ptr(BatesF32In), vp, vp, u32]
        avg = [vp, vp, i32, i32, i32, i64, vp, i64, u32]
        kill = ptr(PfdKill)
        pfd_kill = [vp, ptr(PfdIn), kill, vp, vp, u32]
        pfd_kill_f32 = [vp, ptr(PfdF32In), kill, vp, vp, u32]
        avg_kill = [vp, vp, i32, i32, i32, i64, kill, vp, i64, u32]
        how = ptr(PfdScrunchHow)
        scrunch = [vp, vp, i32, i32, i32, i64, how, vp, u32]
        signatures = {  # name: (restype, argtypes), as include/pfe.h and include/pfe_io.h declare
            "pfe_abi_version": (rc, []), "pfe_device_count": (rc, []),
            "pfe_create": (rc, [C.c_int, ptr(vp)]), "pfe_destroy": (None, [vp]),
            "pfe_last_error": (C.c_char_p, [vp]),
            "pfe_set_stream": (rc, [vp, vp]), "pfe_synchronize": (rc, [vp]),
            "pfe_set_option": (rc, [vp, i32, i64]), "pfe_get_option": (rc, [vp, i32, ptr(i64)]),
            "pfe_host_alloc": (rc, [C.c_size_t, ptr(vp)]), "pfe_host_free": (None, [vp]),
            "pfe_lyon8_u8": (rc, lyon), "pfe_lyon8_f64": (rc, lyon),
            "pfe_bates22": (rc, bates), "pfe_subband3": (rc, bates),
            "pfe_sinusoid4": (rc, bates), "pfe_gauss7": (rc, bates),
            "pfe_params4": (rc, bates), "pfe_dmfit4": (rc, bates),
            "pfe_sinusoid4_f64": (rc, f64), "pfe_gauss7_f64": (rc, f64),
            "pfe_subband3_f64": (rc, bates_f64), "pfe_bates22_f64": (rc, bates_f64),
            "pfe_pfd_dmprof": (rc, [vp, ptr(PfdIn), vp, vp, vp, vp, u32]),
            "pfe_pfd_bates22": (rc, pfd), "pfe_pfd_params4": (rc, pfd),
            "pfe_pfd_dmfit4": (rc, pfd), "pfe_pfd_subband3": (rc, pfd),
            "pfe_pfd_dmprof_f32": (rc, [vp, ptr(PfdF32In), vp, vp, vp, vp, u32]),
            "pfe_pfd_bates22_f32": (rc, pfd_f32), "pfe_pfd_params4_f32": (rc, pfd_f32),
            "pfe_pfd_dmfit4_f32": (rc, pfd_f32), "pfe_pfd_subband3_f32": (rc, pfd_f32),
            "pfe_lyon8_f32": (rc, lyon),
            "pfe_sinusoid4_f32": (rc, f64), "pfe_gauss7_f32": (rc, f64),
            "pfe_subband3_f32": (rc, bates_f32), "pfe_bates22_f32": (rc, bates_f32),
            "pfe_pfd_avgprof": (rc, avg), "pfe_pfd_avgprof_f32": (rc, avg),
            "pfe_pfd_dmprof_i16": (rc, [vp, ptr(PfdI16In), vp, vp, vp, vp, u32]),
            "pfe_pfd_bates22_i16": (rc, pfd_i16), "pfe_pfd_params4_i16": (rc, pfd_i16),
            "pfe_pfd_dmfit4_i16": (rc, pfd_i16), "pfe_pfd_subband3_i16": (rc, pfd_i16),
            "pfe_pfd_avgprof_i16": (rc, [vp, ptr(PfdI16In), vp, i64, u32]),
            "pfe_pfd_dmprof_i16_pol": (rc, [vp, ptr(PfdI16In), ptr(PfdI16Pol), vp, vp, vp, vp, u32]),
            "pfe_pfd_bates22_i16_pol": (rc, pfd_i16_pol), "pfe_pfd_params4_i16_pol": (rc, pfd_i16_pol),
            "pfe_pfd_dmfit4_i16_pol": (rc, pfd_i16_pol), "pfe_pfd_subband3_i16_pol": (rc, pfd_i16_pol),
            "pfe_pfd_avgprof_i16_pol": (rc, [vp, ptr(PfdI16In), ptr(PfdI16Pol), vp, i64, u32]),
            "pfe_pfd_scrunch_i16_pol": (rc, [vp, ptr(PfdI16In), ptr(PfdI16Pol), how, vp, u32]),
            "pfe_pfd_dmprof_kill": (rc, [vp, ptr(PfdIn), kill, vp, vp, vp, vp, u32]),
            "pfe_pfd_bates22_kill": (rc, pfd_kill), "pfe_pfd_params4_kill": (rc, pfd_kill),
            "pfe_pfd_dmfit4_kill": (rc, pfd_kill), "pfe_pfd_subband3_kill": (rc, pfd_kill),
            "pfe_pfd_dmprof_kill_f32": (rc, [vp, ptr(PfdF32In), kill, vp, vp, vp, vp, u32]),
            "pfe_pfd_bates22_kill_f32": (rc, pfd_kill_f32), "pfe_pfd_params4_kill_f32": (rc, pfd_kill_f32),
            "pfe_pfd_dmfit4_kill_f32": (rc, pfd_kill_f32), "pfe_pfd_subband3_kill_f32": (rc, pfd_kill_f32),
            "pfe_pfd_avgprof_kill": (rc, avg_kill), "pfe_pfd_avgprof_kill_f32": (rc, avg_kill),
            "pfe_pfd_scrunch": (rc, scrunch), "pfe_pfd_scrunch_f32": (rc, scrunch),
            "pfe_pfd_scrunch_i16": (rc, [vp, ptr(PfdI16In), how, vp, u32]),
            "pfe_phcx_parse": (rc, [ptr(C.c_char_p), i64, i32, i32, ptr(vp)]),
            "pfe_phcx_count": (i64, [vp]),
            "pfe_phcx_info_get": (rc, [vp, i64, ptr(PhcxInfo)]),
            "pfe_phcx_fetch": (rc, [vp, i64, i32, vp, i64]),
            "pfe_phcx_pack": (rc, [vp, vp, i64, i32, vp, i64, vp, i64, vp, i64, vp, i64, vp]),
            "pfe_phcx_free": (None, [vp]), "pfe_phcx_info_all": (rc, [vp, vp, i64]),
            "pfe_format_rows": (rc, [vp, vp, vp, i64, i32, i64, i32, vp, i32, vp, i64, ptr(i64)]),
            "pfe_pfd_scan": (rc, [ptr(C.c_char_p), i64, i32, ptr(vp)]),
            "pfe_pfd_count": (i64, [vp]), "pfe_pfd_info_all": (rc, [vp, vp, i64]),
            "pfe_pfd_fetch": (rc, [vp, i64, i32, vp, i64]),
            "pfe_pfd_pack": (rc, [vp, vp, i64, i32, vp, vp, vp]),
            "pfe_pfd_free": (None, [vp]),
        }
        assert set(signatures) == set(EXPORTED_SYMBOLS + EXPORTED_IO_SYMBOLS)
        for name, (restype, argtypes) in signatures.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        if path is None:
            _lib = lib
        return lib


def _row_stride(stride, a):
    """Row stride in elements; a single-row array may carry any stride on its row axis
    (numpy's and torch's relaxed strides, e.g. x[None, :] has stride 0): use the row length."""
    return a.shape[1] if a.shape[0] <= 1 else stride


def _ptr(a) -> int:
    """Raw address of a numpy array or a torch tensor (host or device)."""
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a.data_ptr())  # torch.Tensor


def _is_device(a) -> bool:
    if isinstance(a, np.ndarray):
        return False
    return bool(getattr(a, "is_cuda", False))


class _Pinned:
    """Owner of one pfe_host_alloc block; numpy arrays made by Engine.host_empty keep it
    alive as their base and it is freed with the last of them."""

    def __init__(self, lib, nbytes: int):
        self.lib = lib
        p = C.c_void_p()
        if lib.pfe_host_alloc(max(1, int(nbytes)), C.byref(p)) != PFE_OK or not p.value:
            raise MemoryError(f"pfe_host_alloc({nbytes}) failed")
        self.ptr = p.value
        self.nbytes = int(nbytes)
        self.__array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1",
                                    "data": (self.ptr, False), "version": 3}

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.pfe_host_free(self.ptr)
            self.ptr = None


def host_empty(shape, dtype=np.uint8) -> np.ndarray:
    """An uninitialised numpy array in pinned host memory (pfe_host_alloc): host-pointer
    engine calls DMA such buffers in place instead of staging them."""
    lib = load_library()
    dt = np.dtype(dtype)
    shape = tuple(int(v) for v in np.atleast_1d(shape))
    nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    raw = np.asarray(_Pinned(lib, nbytes))
    return raw.view(dt).reshape(shape) if nbytes else np.empty(shape, dtype=dt)


class Engine:
    """One libpfe handle: a GPU ordinal plus a HIP stream.

    Arguments may be numpy arrays (host; the call stages and synchronises) or torch CUDA
    tensors (device; the call is asynchronous on torch's current stream).  Mixed placements
    are rejected, and device tensors are checked for dtype, shape, contiguity and device
    before any pointer reaches the library.
    """

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.pfe_create(int(device), C.byref(h))
        if rc != PFE_OK:
            raise PfeError(self.lib.pfe_last_error(None).decode())
        self._h = h
        self.device = device

    # -- lifecycle -----------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.pfe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc != PFE_OK:
            raise PfeError(self.lib.pfe_last_error(self._h).decode())

    def set_stream(self, stream_handle: int | None):
        """Launch on an external hipStream_t (e.g. a torch.cuda.Stream's ``cuda_stream``;
        0/None is the HIP default stream)."""
        self._check(self.lib.pfe_set_stream(self._h, stream_handle or None))

    def _follow_torch(self):
        """Device-tensor calls run on torch's current stream, so they are ordered after the
        kernels that produced their inputs and before the ones that consume the outputs."""
        import torch

        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def synchronize(self):
        self._check(self.lib.pfe_synchronize(self._h))

    # -- options -------------------------------------------------------------------------
    def set_option(self, name: str, value):
        """pfe_set_option: name in OPTIONS ('solver' also takes 'pooled'/'batched'/'wave')."""
        if name == "solver" and isinstance(value, str):
            value = SOLVERS[value]
        self._check(self.lib.pfe_set_option(self._h, OPTIONS[name], int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        self._check(self.lib.pfe_get_option(self._h, OPTIONS[name], C.byref(v)))
        return int(v.value)

    def options(self, **kw):
        """Context manager: set options for a block, restore the previous values after."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = {k: self.get_option(k) for k in kw}
            try:
                for k, v in kw.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)

        return cm()

    # -- argument checks of the device path ----------------------------------------------
    def _dev(self, t, name, dtypes, shape=None, rows_contig=False):
        import torch

        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError(f"{name}: expected a CUDA tensor (all arguments device or all host)")
        if t.dtype not in dtypes:
            raise TypeError(f"{name}: dtype {t.dtype}, expected one of {tuple(dtypes)}")
        if t.device.index != self.device:
            raise ValueError(f"{name}: on cuda:{t.device.index}, engine is on cuda:{self.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
        if rows_contig:
            if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
                raise ValueError(f"{name}: rows must be contiguous (stride(1) == 1)")
        elif not t.is_contiguous():
            raise ValueError(f"{name}: device tensors must be contiguous")
        return t

    def _status_dev(self, status, n):
        import torch

        if status is None:
            return torch.empty((n,), dtype=torch.int32, device=f"cuda:{self.device}")
        return self._dev(status, "status", (torch.int32,), (n,))

    @staticmethod
    def _status_host(status, n):
        if status is None:
            return np.empty((n,), dtype=np.uint32)
        if not isinstance(status, np.ndarray) or status.dtype.itemsize != 4 or \
                status.dtype.kind not in "iu" or status.shape != (n,) or not status.flags.c_contiguous:
            raise ValueError("status must be a contiguous (n,) 4-byte integer array")
        return status

    @staticmethod
    def _out_host(out, n, width):
        if out is None:
            return np.empty((n, width), dtype=np.float64)
        if not isinstance(out, np.ndarray) or out.dtype != np.float64 or out.shape != (n, width) \
                or not out.flags.c_contiguous:
            raise ValueError(f"out must be a contiguous ({n}, {width}) float64 array")
        return out

    def _outputs(self, dev, like, n, k, out, status, need_status=True):
        """Make or check `out` (n, k) and `status` (n,) where the inputs live (device: beside
        the tensor `like`) -> (out, status, flags).  need_status False keeps a None status."""
        if dev:
            import torch

            if out is None:
                out = torch.empty((n, k), dtype=torch.float64, device=like.device)
            self._dev(out, "out", (torch.float64,), (n, k))
            if need_status or status is not None:
                status = self._status_dev(status, n)
            return out, status, PFE_FLAG_DEVICE_PTRS
        out = self._out_host(out, n, k)
        if need_status or status is not None:
            status = self._status_host(status, n)
        return out, status, 0

    # -- 8 Lyon features -----------------------------------------------------------------
    def lyon8(self, prof, dm, out=None, status=None):
        """[mean,std,skew,kurt] of each profile row then each DM row -> (n, 8) float64.
        Rows are uint8, float64 or float32 (both arrays the same): float32 rows go to
        pfe_lyon8_f32 as they are and give the bits of the float64 call on the widened rows
        (every sum in fp64; not numpy's float32 mean)."""
        if prof.ndim != 2 or dm.ndim != 2 or prof.shape[0] != dm.shape[0]:
            raise ValueError("prof and dm must be 2-D with the same number of rows")
        n = prof.shape[0]
        dev = _is_device(prof)
        if dev != _is_device(dm):
            raise ValueError("prof and dm must both be host arrays or both device tensors")
        if dev:
            import torch

            self._dev(prof, "prof", (torch.uint8, torch.float64, torch.float32), rows_contig=True)
            self._dev(dm, "dm", (prof.dtype,), rows_contig=True)
            kind = {torch.uint8: "u8", torch.float64: "f64", torch.float32: "f32"}[prof.dtype]
            self._follow_torch()
            ps, ds = _row_stride(prof.stride(0), prof), _row_stride(dm.stride(0), dm)
        else:
            if prof.dtype == np.uint8 and dm.dtype == np.uint8:
                kind = "u8"
            elif prof.dtype == np.float64 and dm.dtype == np.float64:
                kind = "f64"
            elif prof.dtype == np.float32 and dm.dtype == np.float32:
                kind = "f32"
            else:
                raise TypeError("lyon8: rows must be uint8, float64 or float32 (same dtype)")
            prof = prof if prof.strides[1] == prof.itemsize else np.ascontiguousarray(prof)
            dm = dm if dm.strides[1] == dm.itemsize else np.ascontiguousarray(dm)
            ps = _row_stride(prof.strides[0] // prof.itemsize, prof)
            ds = _row_stride(dm.strides[0] // dm.itemsize, dm)
        out, status, flags = self._outputs(dev, prof, n, 8, out, status, need_status=False)
        fn = getattr(self.lib, "pfe_lyon8_" + kind)
        st = None if status is None else _ptr(status)
        self._check(
            fn(self._h, _ptr(prof), ps, prof.shape[1], _ptr(dm), ds, dm.shape[1], n,
               _ptr(out), st, flags)
        )
        return out

    # -- 22 Bates scores / sub-band scores -----------------------------------------------
    def _bates_args(self, prof, sub, dmcurve, scal, with_dm):
        n = prof.shape[0]
        if prof.ndim != 2 or sub.ndim != 3 or scal.ndim != 2 or scal.shape[1] != PFE_NSCAL:
            raise ValueError("prof must be (n,lp), sub (n,nsub,lsb), scal (n,%d)" % PFE_NSCAL)
        if sub.shape[0] != n or scal.shape[0] != n or (with_dm and dmcurve.shape[0] != n):
            raise ValueError("inputs must have the same number of rows")
        if with_dm and dmcurve.ndim != 2:
            raise ValueError("dmcurve must be (n, ndm)")
        dev = _is_device(prof)
        if dev:
            import torch

            self._dev(prof, "prof", (torch.uint8,))
            self._dev(sub, "sub", (torch.uint8,))
            self._dev(scal, "scal", (torch.float64,))
            if with_dm:
                self._dev(dmcurve, "dmcurve", (torch.float64,))
            self._follow_torch()
        else:
            prof = np.ascontiguousarray(prof, dtype=np.uint8)
            sub = np.ascontiguousarray(sub, dtype=np.uint8)
            scal = np.ascontiguousarray(scal, dtype=np.float64)
            if with_dm:
                dmcurve = np.ascontiguousarray(dmcurve, dtype=np.float64)
        bi = BatesIn(
            _ptr(prof), prof.shape[1], _ptr(sub), sub.shape[1], sub.shape[2],
            _ptr(dmcurve) if with_dm else None, dmcurve.shape[1] if with_dm else 0,
            _ptr(scal), n,
        )
        return bi, dev, (prof, sub, dmcurve, scal)

    def bates22(self, prof, sub, dmcurve, scal, out=None, status=None):
        """22 scores per candidate -> ((n, 22) float64, (n,) status)."""
        bi, dev, keep = self._bates_args(prof, sub, dmcurve, scal, True)
        out, status, flags = self._outputs(dev, prof, bi.n, 22, out, status)
        self._check(self.lib.pfe_bates22(self._h, C.byref(bi), _ptr(out), _ptr(status), flags))
        del keep
        return out, status

    def subband3(self, prof, sub, scal, out=None, status=None):
        """Scores 20-22 alone (pfe_subband3, PHCXOperations.getSubbandParameters):
        -> ((n, 3) float64, (n,) status)."""
        bi, dev, keep = self._bates_args(prof, sub, None, scal, False)
        out, status, flags = self._outputs(dev, prof, bi.n, 3, out, status)
        self._check(self.lib.pfe_subband3(self._h, C.byref(bi), _ptr(out), _ptr(status), flags))
        del keep
        return out, status

    # ---- one score group (ProfileOperationsInterface.py:69-130; pfe.h per-group block) ----
    def _group(self, fn, k, prof, dmcurve, scal, out, status):
        n = scal.shape[0]
        dev = _is_device(scal)
        if dev:
            import torch

            for a, nm in ((prof, "prof"), (dmcurve, "dmcurve")):
                if a is not None:
                    self._dev(a, nm, (torch.uint8,) if nm == "prof" else (torch.float64,))
            self._dev(scal, "scal", (torch.float64,))
            self._follow_torch()
        else:
            prof = None if prof is None else np.ascontiguousarray(prof, dtype=np.uint8)
            dmcurve = None if dmcurve is None else np.ascontiguousarray(dmcurve, dtype=np.float64)
            scal = np.ascontiguousarray(scal, dtype=np.float64)
        out, status, flags = self._outputs(dev, scal, n, k, out, status)
        for a in (prof, dmcurve):
            if a is not None and a.shape[0] != n:
                raise ValueError("inputs must have the same number of rows")
        bi = BatesIn(_ptr(prof) if prof is not None else None, prof.shape[1] if prof is not None else 0,
                     None, 0, 0, _ptr(dmcurve) if dmcurve is not None else None,
                     dmcurve.shape[1] if dmcurve is not None else 0, _ptr(scal), n)
        self._check(getattr(self.lib, fn)(self._h, C.byref(bi), _ptr(out), _ptr(status), flags))
        return out, status

    def sinusoid4(self, prof, scal, out=None, status=None):
        """getSinusoidFittings (pfe_sinusoid4): s1-s4 -> ((n, 4), (n,) status)."""
        return self._group("pfe_sinusoid4", 4, prof, None, scal, out, status)

    def gauss7(self, prof, scal, out=None, status=None):
        """getGaussianFittings (pfe_gauss7): s5-s11 -> ((n, 7), (n,) status)."""
        return self._group("pfe_gauss7", 7, prof, None, scal, out, status)

    def params4(self, scal, out=None, status=None):
        """getCandidateParameters (pfe_params4): [period_ms, snr, dm, width], unfiltered."""
        return self._group("pfe_params4", 4, None, None, scal, out, status)

    def dmfit4(self, dmcurve, scal, out=None, status=None):
        """getDMFittings (pfe_dmfit4): [peak, |1 - Prop|, Shift (signed), chi_theo]."""
        return self._group("pfe_dmfit4", 4, None, dmcurve, scal, out, status)

    def _group_f64(self, fn, k, prof, out, status, bits=64):
        if prof.ndim != 2:
            raise ValueError("prof must be (n, lp)")
        n, lp = prof.shape
        dev = _is_device(prof)
        if dev:
            import torch

            self._dev(prof, "prof", (torch.float64 if bits == 64 else torch.float32,))
            self._follow_torch()
        else:
            if not isinstance(prof, np.ndarray) or prof.dtype != np.dtype(f"float{bits}"):
                raise TypeError(f"{fn}: float{bits} profile rows expected (byte profiles go through "
                                "sinusoid4 / gauss7)")
            prof = np.ascontiguousarray(prof)
        out, status, flags = self._outputs(dev, prof, n, k, out, status)
        self._check(getattr(self.lib, fn)(self._h, _ptr(prof), lp, n, _ptr(out), _ptr(status),
                                          flags))
        return out, status

    def sinusoid4_f64(self, prof, out=None, status=None):
        """getSinusoidFittings on float profiles (pfe_sinusoid4_f64): prof (n, lp) float64,
        e.g. pfd_dmprof's profile -> ((n, 4) s1-s4, (n,) status)."""
        return self._group_f64("pfe_sinusoid4_f64", 4, prof, out, status)

    def gauss7_f64(self, prof, out=None, status=None):
        """getGaussianFittings on float profiles (pfe_gauss7_f64) -> ((n, 7) s5-s11, status)."""
        return self._group_f64("pfe_gauss7_f64", 7, prof, out, status)

    def sinusoid4_f32(self, prof, out=None, status=None):
        """sinusoid4_f64 on float32 profiles (pfe_sinusoid4_f32): the bits of sinusoid4_f64 on
        the widened rows -> ((n, 4) s1-s4, (n,) status)."""
        return self._group_f64("pfe_sinusoid4_f32", 4, prof, out, status, bits=32)

    def gauss7_f32(self, prof, out=None, status=None):
        """gauss7_f64 on float32 profiles (pfe_gauss7_f32) -> ((n, 7) s5-s11, status)."""
        return self._group_f64("pfe_gauss7_f32", 7, prof, out, status, bits=32)

    # ---- candidates held as float arrays (pfe.h pfe_bates_f64_in, pfe_bates_f32_in) --------
    def _bates_f64_args(self, fn, prof, sub, dmcurve, scal, with_dm, bits=64):
        if prof.ndim != 2 or sub.ndim != 3 or scal.ndim != 2 or scal.shape[1] != PFE_NSCAL:
            raise ValueError("prof must be (n,lp), sub (n,nsub,lsb), scal (n,%d)" % PFE_NSCAL)
        n = prof.shape[0]
        if sub.shape[0] != n or scal.shape[0] != n:
            raise ValueError("inputs must have the same number of rows")
        if with_dm and (dmcurve.ndim != 2 or dmcurve.shape[0] != n):
            raise ValueError("dmcurve must be (n, ndm)")
        arrays = [("prof", prof), ("sub", sub), ("scal", scal)] + ([("dmcurve", dmcurve)] if with_dm else [])
        dev = _is_device(prof)
        if dev:
            import torch

            ft = torch.float64 if bits == 64 else torch.float32
            for nm, a in arrays:  # dense rows only: a strided tensor is refused, never copied
                self._dev(a, nm, (torch.float64 if nm == "scal" else ft,))
            self._follow_torch()
        elif bits == 64:
            for nm, a in arrays:
                if not isinstance(a, np.ndarray) or (nm in ("prof", "sub") and a.dtype != np.float64):
                    raise TypeError(f"{fn}: {nm}: float64 numpy rows expected (byte candidates go "
                                    "through subband3 / bates22)")
            prof, sub, scal = (np.ascontiguousarray(a, dtype=np.float64) for a in (prof, sub, scal))
            if with_dm:
                dmcurve = np.ascontiguousarray(dmcurve, dtype=np.float64)
        else:
            for nm, a in arrays:  # nothing is converted: a float32 call reads what it is given
                want = np.float64 if nm == "scal" else np.float32
                if not isinstance(a, np.ndarray) or a.dtype != want:
                    raise TypeError(f"{fn}: {nm}: {np.dtype(want).name} numpy rows expected "
                                    "(float64 candidates go through subband3_f64 / bates22_f64)")
            prof, sub, scal = (np.ascontiguousarray(a) for a in (prof, sub, scal))
            if with_dm:
                dmcurve = np.ascontiguousarray(dmcurve)
        bi = (BatesF64In if bits == 64 else BatesF32In)(
            _ptr(prof), prof.shape[1], _ptr(sub), sub.shape[1], sub.shape[2],
            _ptr(dmcurve) if with_dm else None, dmcurve.shape[1] if with_dm else 0,
            _ptr(scal), n,
        )
        return bi, dev, (prof, sub, dmcurve, scal)

    def subband3_f64(self, prof, sub, scal, out=None, status=None):
        """Scores 20-22 of candidates held as float arrays (pfe_subband3_f64): prof (n, lp),
        sub (n, nsub, lsb), scal (n, 8), all float64 -> ((n, 3) float64, (n,) status).  Host
        arrays of any strides are made dense; device tensors must be contiguous.  `sub` is
        never written."""
        bi, dev, keep = self._bates_f64_args("subband3_f64", prof, sub, None, scal, False)
        out, status, flags = self._outputs(dev, keep[0], bi.n, 3, out, status)
        self._check(self.lib.pfe_subband3_f64(self._h, C.byref(bi), _ptr(out), _ptr(status), flags))
        del keep
        return out, status

    def bates22_f64(self, prof, sub, dmcurve, scal, out=None, status=None):
        """The 22 scores of candidates held as float arrays (pfe_bates22_f64): the columns of
        sinusoid4_f64, gauss7_f64, params4 (filtered), dmfit4 (|Shift|) and subband3_f64
        -> ((n, 22) float64, (n,) status)."""
        bi, dev, keep = self._bates_f64_args("bates22_f64", prof, sub, dmcurve, scal, True)
        out, status, flags = self._outputs(dev, keep[0], bi.n, 22, out, status)
        self._check(self.lib.pfe_bates22_f64(self._h, C.byref(bi), _ptr(out), _ptr(status), flags))
        del keep
        return out, status

    def subband3_f32(self, prof, sub, scal, out=None, status=None):
        """subband3_f64 on float32 arrays (pfe_subband3_f32): prof (n, lp) and sub (n, nsub, lsb)
        float32, scal (n, 8) float64 -> ((n, 3) float64, (n,) status), the bits of subband3_f64
        on the widened arrays.  The sub-bands are read where they lie and never written."""
        bi, dev, keep = self._bates_f64_args("subband3_f32", prof, sub, None, scal, False, bits=32)
        out, status, flags = self._outputs(dev, keep[0], bi.n, 3, out, status)
        self._check(self.lib.pfe_subband3_f32(self._h, C.byref(bi), _ptr(out), _ptr(status), flags))
        del keep
        return out, status

    def bates22_f32(self, prof, sub, dmcurve, scal, out=None, status=None):
        """bates22_f64 on float32 arrays (pfe_bates22_f32): prof, sub and dmcurve float32 (the
        curve may be pfd_dmprof's chis), scal float64 -> ((n, 22) float64, (n,) status), the
        bits of bates22_f64 on the widened arrays."""
        bi, dev, keep = self._bates_f64_args("bates22_f32", prof, sub, dmcurve, scal, True, bits=32)
        out, status, flags = self._outputs(dev, keep[0], bi.n, 22, out, status)
        self._check(self.lib.pfe_bates22_f32(self._h, C.byref(bi), _ptr(out), _ptr(status), flags))
        del keep
        return out, status

    def features30(self, prof, lyon_dm, sub, dmcurve, scal, out=None):
        """Config 5's feature matrix: the 8 Lyon features (profile + Lyon DM rows) then the
        22 Bates scores of each candidate -> ((n, 30) float64, (n,) status)."""
        n = prof.shape[0]
        dev = _is_device(prof)
        if dev:
            import torch

            if out is None:
                out = torch.empty((n, 30), dtype=torch.float64, device=prof.device)
            self._dev(out, "out", (torch.float64,), (n, 30))
            o8 = self.lyon8(prof, lyon_dm)
            o22, st = self.bates22(prof, sub, dmcurve, scal)
            out[:, :8].copy_(o8)
            out[:, 8:].copy_(o22)
        else:
            out = self._out_host(out, n, 30)
            out[:, :8] = self.lyon8(prof, lyon_dm)
            o22, st = self.bates22(prof, sub, dmcurve, scal)
            out[:, 8:] = o22
        return out, st

    # -- PFD -----------------------------------------------------------------------------
    @staticmethod
    def _is_i16(profs) -> bool:
        if isinstance(profs, np.ndarray):
            return profs.dtype == np.int16
        return str(getattr(profs, "dtype", "")) == "torch.int16"

    @staticmethod
    def _pfd_pol(fn, profs, pol_sum):
        """The PfdI16Pol of a call, or None for a 4-D cube: pol_sum (the leading polarisations
        summed, 1 or 2) is required with a (n,npart,npol,nsub,L) int16 cube, refused with any
        other, and never guessed (an IQUV archive wants 1, an AABBCRCI one 2)."""
        if profs.ndim != 5:
            if pol_sum is not None:
                raise ValueError(f"{fn}: pol_sum goes with a 5-D int16 cube (n,npart,npol,nsub,L), "
                                 f"profs has {profs.ndim} dimensions")
            return None
        if not Engine._is_i16(profs):
            raise ValueError(f"{fn}: a 5-D cube (n,npart,npol,nsub,L) must be int16, profs is {profs.dtype}")
        if pol_sum is None:
            raise ValueError(f"{fn}: pol_sum (1 or 2) is required with a 5-D int16 cube: the "
                             "polarisations to sum are never guessed")
        npol = int(profs.shape[2])
        if pol_sum not in (1, 2):
            raise ValueError(f"{fn}: pol_sum must be 1 or 2, got {pol_sum!r}")
        if not 1 <= npol <= 4 or pol_sum > npol:
            raise ValueError(f"{fn}: npol {npol} must be 1..4 and pol_sum {pol_sum} <= npol")
        return PfdI16Pol(npol, int(pol_sum))

    def _pfd_i16_arrays(self, fn, profs, scl, offs, wts):
        """The four arrays of an int16 cube for pfe_pfd_i16_in -> (data, scl, offs, wts or None,
        fold_stride, part_stride): host arrays made dense; device tensors as they are -- all
        contiguous (strides 0, 0), or strided views of one uploaded table whose inner dimensions
        are dense and whose byte strides agree.  A 5-D cube (n,npart,npol,nsub,L) goes with scl
        and offs (n,npart,npol,nsub) and wts (n,npart,nsub): the polarisation axis counts among
        the inner, dense dimensions of the cube, scl and offs."""
        pol = profs.ndim == 5
        n, npart = profs.shape[:2]
        nsub, L = profs.shape[-2:]
        if scl is None or offs is None:
            raise ValueError(f"{fn}: scl and offs are required with an int16 cube")
        par = [("scl", scl), ("offs", offs)] + ([("wts", wts)] if wts is not None else [])
        for name, a in par:
            if pol and name != "wts":
                want = (n, npart, profs.shape[2], nsub)
                if tuple(a.shape) != want:
                    raise ValueError(f"{fn}: {name} must be (n,npart,npol,nsub) = {want}")
            elif tuple(a.shape) != (n, npart, nsub):
                raise ValueError(f"{fn}: {name} must be (n,npart,nsub) = {(n, npart, nsub)}")
        if not _is_device(profs):
            for name, a in [("profs", profs)] + par:
                if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
                    raise ValueError(f"{fn}: {name}: host arrays must be dense numpy arrays "
                                     "(strided input is for device tensors)")
                if name != "profs" and a.dtype != np.float32:
                    raise ValueError(f"{fn}: {name} must be float32")
            return (profs, scl, offs, wts, 0, 0)
        import torch

        strides = set()
        for name, a in [("profs", profs)] + par:
            dt = torch.int16 if name == "profs" else torch.float32
            if not isinstance(a, torch.Tensor) or not a.is_cuda:
                raise TypeError(f"{fn}: {name}: expected a CUDA tensor (all arguments device or all host)")
            if a.dtype != dt:
                raise ValueError(f"{fn}: {name} must be {dt}")
            if a.device.index != self.device:
                raise ValueError(f"{fn}: {name}: on cuda:{a.device.index}, engine is on cuda:{self.device}")
            if a.is_contiguous():
                strides.add((0, 0))
                continue
            want = 1  # the strides of dense inner dimensions, last to first
            inner = True
            for dim in range(a.ndim - 1, 1, -1):
                inner = inner and a.stride(dim) == want
                want *= a.shape[dim]
            if not inner:
                raise ValueError(f"{fn}: {name}: the inner dimension{'s' if name == 'profs' else ''} "
                                 "of a strided view must be dense")
            strides.add((a.stride(0) * a.element_size(), a.stride(1) * a.element_size()))
        if len(strides) != 1:
            raise ValueError(f"{fn}: profs, scl, offs and wts must all be contiguous or share one "
                             f"fold stride and one part stride in bytes, got {sorted(strides)}")
        fs, ps = strides.pop()
        return (profs, scl, offs, wts, fs, ps)

    def _pfd_args(self, profs, subfreqs, scal, fn, scl=None, offs=None, wts=None, pol=None):
        if profs.ndim != (5 if pol is not None else 4):
            raise ValueError(f"{fn}: profs must be (n,npart,nsub,L)")
        n, npart = profs.shape[:2]
        nsub, L = profs.shape[-2:]
        if tuple(subfreqs.shape) != (n, nsub) or tuple(scal.shape) != (n, PFE_PFD_NSCAL):
            raise ValueError(f"{fn}: subfreqs must be (n,nsub), scal (n,{PFE_PFD_NSCAL})")
        dev = _is_device(profs)
        if self._is_i16(profs):
            arrs = self._pfd_i16_arrays(fn, profs, scl, offs, wts)
            if dev:
                import torch

                self._dev(subfreqs, "subfreqs", (torch.float64,))
                self._dev(scal, "scal", (torch.float64,))
                self._follow_torch()
            else:
                subfreqs = np.ascontiguousarray(subfreqs, dtype=np.float64)
                scal = np.ascontiguousarray(scal, dtype=np.float64)
            pin = PfdI16In(_ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                           _ptr(arrs[3]) if arrs[3] is not None else None, arrs[4], arrs[5],
                           _ptr(subfreqs), _ptr(scal), npart, nsub, L, n)
            return pin, dev, (arrs, subfreqs, scal)
        if scl is not None or offs is not None or wts is not None:
            raise ValueError(f"{fn}: scl, offs and wts go with an int16 cube, profs is {profs.dtype}")
        if dev:
            import torch

            self._dev(profs, "profs", (torch.float64, torch.float32))
            self._dev(subfreqs, "subfreqs", (torch.float64,))
            self._dev(scal, "scal", (torch.float64,))
            self._follow_torch()
            f32 = profs.dtype == torch.float32
        else:
            # a float32 cube goes to the _f32 call as it is: no copy, nothing widened
            f32 = isinstance(profs, np.ndarray) and profs.dtype == np.float32
            profs = np.ascontiguousarray(profs, dtype=np.float32 if f32 else np.float64)
            subfreqs = np.ascontiguousarray(subfreqs, dtype=np.float64)
            scal = np.ascontiguousarray(scal, dtype=np.float64)
        pin = (PfdF32In if f32 else PfdIn)(_ptr(profs), _ptr(subfreqs), _ptr(scal), npart, nsub, L, n)
        return pin, dev, (profs, subfreqs, scal)

    def _pfd_fn(self, fn, pin, kill=None, pol=None):
        """The C entry point of a PFD call: its _f32 form for a float32 cube, its _i16 form for
        an int16 one; with masks (kill: a PfdKill) its _kill form, the masks behind `in`; with
        polarisations (pol: a PfdI16Pol) its _i16_pol form, pol behind `in`."""
        sfx = "_f32" if isinstance(pin, PfdF32In) else "_i16" if isinstance(pin, PfdI16In) else ""
        if pol is not None:
            f = getattr(self.lib, "pfe_" + fn + "_i16_pol")
            return lambda h, pin_ref, *rest: f(h, pin_ref, C.byref(pol), *rest)
        if kill is None:
            return getattr(self.lib, "pfe_" + fn + sfx)
        f = getattr(self.lib, "pfe_" + fn + "_kill" + sfx)
        return lambda h, pin_ref, *rest: f(h, pin_ref, C.byref(kill), *rest)

    def _pfd_kill(self, fn, profs, kill_parts, kill_subs):
        """The masks of a PFD call -> (PfdKill or None when both are None, the arrays it points
        into).  kill_parts (n,npart) and kill_subs (n,nsub), bool or uint8, non-zero = killed; a
        1-D mask is broadcast to every fold.  numpy arrays for a host cube, torch.bool /
        torch.uint8 tensors on the cube's device for a device cube."""
        if kill_parts is None and kill_subs is None:
            return None, None
        if profs.ndim != 4 and not (profs.ndim == 5 and self._is_i16(profs)):
            raise ValueError(f"{fn}: profs must be (n,npart,nsub,L)")
        if self._is_i16(profs):
            raise ValueError(f"{fn}: kill_parts and kill_subs are for float cubes; an int16 cube "
                             "is zapped through wts (a weight of 0 is the kill)")
        n, npart, nsub, _ = profs.shape
        dev = _is_device(profs)
        keep = []
        for name, m, width in (("kill_parts", kill_parts, npart), ("kill_subs", kill_subs, nsub)):
            if m is None:
                keep.append(None)
                continue
            if dev:
                import torch

                if not isinstance(m, torch.Tensor) or not m.is_cuda or m.device != profs.device:
                    raise TypeError(f"{fn}: {name}: expected a tensor on the cube's device")
                if m.dtype not in (torch.bool, torch.uint8):
                    raise ValueError(f"{fn}: {name} must be torch.bool or torch.uint8")
                if tuple(m.shape) not in ((width,), (n, width)):
                    raise ValueError(f"{fn}: {name} must be ({width},) or (n,{width}) = {(n, width)}")
                m = m.expand(n, width).contiguous()
                keep.append(m.view(torch.uint8) if m.dtype == torch.bool else m)
            else:
                m = np.asarray(m)
                if m.dtype not in (np.bool_, np.uint8):
                    raise ValueError(f"{fn}: {name} must be bool or uint8")
                if m.shape not in ((width,), (n, width)):
                    raise ValueError(f"{fn}: {name} must be ({width},) or (n,{width}) = {(n, width)}")
                keep.append(np.ascontiguousarray(np.broadcast_to(m, (n, width))).view(np.uint8))
        kill = PfdKill(_ptr(keep[0]) if keep[0] is not None else None,
                       _ptr(keep[1]) if keep[1] is not None else None)
        return kill, keep

    def pfd_avgprof(self, profs, byteswapped=False, scl=None, offs=None, wts=None,
                    kill_parts=None, kill_subs=None, pol_sum=None):
        """numpy's (profs / proflen).sum() of each fold of a (n,npart,nsub,L) cube, bit for
        bit (pfe_pfd_avgprof; a float32 cube -- numpy array or device tensor -- goes to
        pfe_pfd_avgprof_f32 as it is and gives the value of profs.astype(float64)): the
        scal[:, 2] every PFD call reads.  byteswapped: as in pfd_dmprof.  An int16 cube with scl,
        offs (and wts) as in pfd_dmprof goes to pfe_pfd_avgprof_i16 and gives the value of the
        decoded cube.  kill_parts, kill_subs: as in pfd_dmprof; the value is that of the zapped
        cube np.where(kill, 0.0, profs) (pfe_pfd_avgprof_kill).  pol_sum with a 5-D int16 cube:
        as in pfd_dmprof (pfe_pfd_avgprof_i16_pol).  Returns (n,) float64 where the cube lives."""
        pol = self._pfd_pol("pfd_avgprof", profs, pol_sum)
        if profs.ndim != 4 and pol is None:
            raise ValueError("pfd_avgprof: profs must be (n,npart,nsub,L)")
        n, npart = profs.shape[:2]
        nsub, L = profs.shape[-2:]
        kill, kkeep = self._pfd_kill("pfd_avgprof", profs, kill_parts, kill_subs)
        if self._is_i16(profs):
            arrs = self._pfd_i16_arrays("pfd_avgprof", profs, scl, offs, wts)
            if _is_device(profs):
                import torch

                self._follow_torch()
                out = torch.empty((n,), dtype=torch.float64, device=profs.device)
                flags = PFE_FLAG_DEVICE_PTRS
            else:
                out = np.empty((n,), dtype=np.float64)
                flags = 0
            if byteswapped:
                flags |= PFE_FLAG_PFD_BSWAP
            pin = PfdI16In(_ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                           _ptr(arrs[3]) if arrs[3] is not None else None, arrs[4], arrs[5],
                           None, None, npart, nsub, L, n)
            if pol is not None:
                self._check(self.lib.pfe_pfd_avgprof_i16_pol(self._h, C.byref(pin), C.byref(pol),
                                                             _ptr(out), 1, flags))
            else:
                self._check(self.lib.pfe_pfd_avgprof_i16(self._h, C.byref(pin), _ptr(out), 1, flags))
            return out
        if scl is not None or offs is not None or wts is not None:
            raise ValueError(f"pfd_avgprof: scl, offs and wts go with an int16 cube, profs is {profs.dtype}")
        if _is_device(profs):
            import torch

            self._dev(profs, "profs", (torch.float64, torch.float32))
            self._follow_torch()
            f32 = profs.dtype == torch.float32
            out = torch.empty((n,), dtype=torch.float64, device=profs.device)
            flags = PFE_FLAG_DEVICE_PTRS
        else:
            f32 = isinstance(profs, np.ndarray) and profs.dtype == np.float32
            profs = np.ascontiguousarray(profs, dtype=np.float32 if f32 else np.float64)
            out = np.empty((n,), dtype=np.float64)
            flags = 0
        if byteswapped:
            flags |= PFE_FLAG_PFD_BSWAP
        if kill is not None:
            fn = self.lib.pfe_pfd_avgprof_kill_f32 if f32 else self.lib.pfe_pfd_avgprof_kill
            self._check(fn(self._h, _ptr(profs), npart, nsub, L, n, C.byref(kill), _ptr(out), 1, flags))
            del kkeep
            return out
        fn = self.lib.pfe_pfd_avgprof_f32 if f32 else self.lib.pfe_pfd_avgprof
        self._check(fn(self._h, _ptr(profs), npart, nsub, L, n, _ptr(out), 1, flags))
        return out

    def pfd_scrunch(self, profs, fscr=1, bscr=1, rot=None, scl=None, offs=None, wts=None,
                    byteswapped=False, out=None, pol_sum=None):
        """Scrunch a batch of folds (pfe_pfd_scrunch): profs (n,npart,nchan,nbin) float64, float32
        (pfe_pfd_scrunch_f32) or int16 with scl, offs (and wts) as in pfd_dmprof
        (pfe_pfd_scrunch_i16; byteswapped as there).  The parts of every element are summed, each
        channel's row is rotated left by rot[i][c] mod nbin (rot: (n,nchan) or (nchan,) integers,
        None = no rotation), bscr bins and then fscr channels are summed, each in order and in
        fp64 (include/pfe.h states the steps).  Host arrays give a host array, device tensors (an
        int16 cube may be strided views of an uploaded table) a device tensor: (n,1,G,K) float64,
        G = nchan / fscr, K = nbin / bscr -- a fold of one part for the pfd_* calls, with
        pfd.scrunch_plan's subfreqs, pfd.scrunch_scal's scalars and derive_avgprof=True.
        pol_sum with a 5-D int16 cube (n,npart,npol,nchan,nbin): as in pfd_dmprof
        (pfe_pfd_scrunch_i16_pol)."""
        fn = "pfd_scrunch"
        pol = self._pfd_pol(fn, profs, pol_sum)
        if profs.ndim != 4 and pol is None:
            raise ValueError(f"{fn}: profs must be (n,npart,nchan,nbin)")
        n, npart = profs.shape[:2]
        nchan, nbin = profs.shape[-2:]
        fscr, bscr = int(fscr), int(bscr)
        if fscr < 1 or bscr < 1:
            raise ValueError(f"{fn}: fscr {fscr} and bscr {bscr} must be >= 1")
        if nchan % fscr:
            raise ValueError(f"{fn}: fscr {fscr} does not divide nchan {nchan}")
        if nbin % bscr:
            raise ValueError(f"{fn}: bscr {bscr} does not divide nbin {nbin}")
        shape = (n, 1, nchan // fscr, nbin // bscr)
        dev = _is_device(profs)
        i16 = self._is_i16(profs)
        if i16:
            arrs = self._pfd_i16_arrays(fn, profs, scl, offs, wts)
        elif scl is not None or offs is not None or wts is not None:
            raise ValueError(f"{fn}: scl, offs and wts go with an int16 cube, profs is {profs.dtype}")
        if dev:
            import torch

            if not i16:
                self._dev(profs, "profs", (torch.float64, torch.float32))
                f32 = profs.dtype == torch.float32
            if rot is not None:
                if tuple(rot.shape) not in ((nchan,), (n, nchan)):
                    raise ValueError(f"{fn}: rot must be ({nchan},) or (n,{nchan}) = {(n, nchan)}")
                rot = self._dev(rot.expand(n, nchan).contiguous(), "rot", (torch.int32,))
            if out is None:
                out = torch.empty(shape, dtype=torch.float64, device=profs.device)
            else:
                self._dev(out, "out", (torch.float64,), shape=shape)
            self._follow_torch()
            flags = PFE_FLAG_DEVICE_PTRS
        else:
            if not i16:
                f32 = isinstance(profs, np.ndarray) and profs.dtype == np.float32
                profs = np.ascontiguousarray(profs, dtype=np.float32 if f32 else np.float64)
            if rot is not None:
                r = np.asarray(rot)
                if r.dtype.kind not in "iu" or r.shape not in ((nchan,), (n, nchan)):
                    raise ValueError(f"{fn}: rot must be integers, ({nchan},) or (n,{nchan}) = {(n, nchan)}")
                if r.size and (r.min() < -2**31 or r.max() >= 2**31):
                    raise ValueError(f"{fn}: rot must fit int32")
                rot = np.ascontiguousarray(np.broadcast_to(r, (n, nchan)), dtype=np.int32)
            if out is None:
                out = np.empty(shape, dtype=np.float64)
            elif (not isinstance(out, np.ndarray) or out.dtype != np.float64 or out.shape != shape
                  or not out.flags.c_contiguous):
                raise ValueError(f"{fn}: out must be a contiguous float64 array of shape {shape}")
            flags = 0
        if byteswapped:
            flags |= PFE_FLAG_PFD_BSWAP
        how = PfdScrunchHow(_ptr(rot) if rot is not None else None, fscr, bscr)
        if i16:
            pin = PfdI16In(_ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                           _ptr(arrs[3]) if arrs[3] is not None else None, arrs[4], arrs[5],
                           None, None, npart, nchan, nbin, n)
            if pol is not None:
                self._check(self.lib.pfe_pfd_scrunch_i16_pol(self._h, C.byref(pin), C.byref(pol),
                                                             C.byref(how), _ptr(out), flags))
            else:
                self._check(self.lib.pfe_pfd_scrunch_i16(self._h, C.byref(pin), C.byref(how), _ptr(out), flags))
        else:
            call = self.lib.pfe_pfd_scrunch_f32 if f32 else self.lib.pfe_pfd_scrunch
            self._check(call(self._h, _ptr(profs), npart, nchan, nbin, n, C.byref(how), _ptr(out), flags))
        return out

    def pfd_dmprof(self, profs, subfreqs, scal, profile=True, chis=True, lyon8=True,
                   derive_avgprof=False, byteswapped=False, scl=None, offs=None, wts=None,
                   kill_parts=None, kill_subs=None, pol_sum=None):
        """PFD preprocessing + Lyon features (pfe_pfd_dmprof) for a batch of folds of one
        shape: profs (n,npart,nsub,L) f64, subfreqs (n,nsub), scal (n,PFE_PFD_NSCAL).
        A float32 cube (numpy array or device tensor) is scored as it is, by the _f32 call of
        this and the other PFD methods: the bits of the f64 call on profs widened to f64
        (parts summed in fp64; not numpy's float32 sum).  subfreqs and scal stay f64.
        derive_avgprof (this and the other PFD methods): scal[:, 2] is not read; the library
        derives it from the cube on the device (PFE_FLAG_PFD_AVGPROF, the value of
        pfd_avgprof), and scal is left as it is.
        byteswapped (this and the other PFD methods, f64 cubes only): profs holds 8-byte values
        whose bytes are reversed, as a big-endian .pfd file holds them (PFE_FLAG_PFD_BSWAP): the
        bits of the call on profs.byteswap(), the byte order dealt with on the device.
        scl, offs, wts (this and the other PFD methods): an int16 cube -- a fold-mode archive's
        values -- is scored as it is, by the _i16 call: scl and offs, float32 (n,npart,nsub), are
        then required, wts (the same) is optional, and the result is the bits of the f64 call on
        (profs * scl[..., None] + offs[..., None]) [* wts[..., None]] evaluated in float64.
        Device tensors may be strided views of one uploaded table (inner dimensions dense, one
        fold and one part stride in bytes shared by all); byteswapped then says that the int16
        and the float32 values are all byte-reversed.  Giving them with any other cube is a
        ValueError.
        kill_parts, kill_subs (this and the other PFD methods, f64 and float32 cubes): killed
        sub-integrations (n,npart) and sub-bands (n,nsub), bool or uint8, non-zero = killed, a 1-D
        mask for every fold alike; numpy arrays with a host cube, torch.bool / torch.uint8 tensors
        on the cube's device with a device cube.  The fold is scored by the _kill call where it
        lies: the bits of the plain call on np.where(kill, 0.0, profs), no copy of the cube made.
        scal[:, 2] and scal[:, 3] must be those of the zapped fold (pfd.varprof; derive_avgprof
        derives the average of the zapped cube).  With an int16 cube they are a ValueError: there
        wts = 0 is the kill.  Both None: the plain call.
        pol_sum (this and the other PFD methods, pfd_avgprof and pfd_scrunch): an int16 cube with a
        polarisation axis, (n,npart,npol,nsub,L) with scl and offs (n,npart,npol,nsub) and wts
        (n,npart,nsub), is scored as total intensity by the _i16_pol call: pol_sum = 2 sums the
        first two polarisations (AA + BB of an AABB or AABBCRCI archive), 1 reads the first alone
        (I of IQUV); the others are never read.  The result is the bits of the f64 call on
        dec[:, :, 0] + dec[:, :, 1] (pol_sum = 2), dec the decoded cube, times wts when given --
        the weight multiplies the sum.  pol_sum is required with a 5-D cube, refused with a 4-D
        one, never guessed.  Device tensors may be strided views of one uploaded table: the inner
        three dimensions of the cube and the inner two of scl and offs dense.
        Returns dict(profile (n,L) f64, chis (n,100) f32, lyon8 (n,8) f64, status (n,))."""
        pol = self._pfd_pol("pfd_dmprof", profs, pol_sum)
        kill, kkeep = self._pfd_kill("pfd_dmprof", profs, kill_parts, kill_subs)
        pin, dev, keep = self._pfd_args(profs, subfreqs, scal, "pfd_dmprof", scl, offs, wts, pol)
        n, L = pin.n, pin.proflen
        out = {}
        if dev:
            import torch

            mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=profs.device)  # noqa: E731
            f64, f32, i32 = torch.float64, torch.float32, torch.int32
            flags = PFE_FLAG_DEVICE_PTRS
        else:
            mk = lambda shape, dt: np.empty(shape, dtype=dt)  # noqa: E731
            f64, f32, i32 = np.float64, np.float32, np.uint32
            flags = 0
        if derive_avgprof:
            flags |= PFE_FLAG_PFD_AVGPROF
        if byteswapped:
            flags |= PFE_FLAG_PFD_BSWAP
        out["profile"] = mk((n, L), f64) if profile else None
        out["chis"] = mk((n, PFE_PFD_NDM), f32) if chis else None
        out["lyon8"] = mk((n, 8), f64) if lyon8 else None
        out["status"] = mk((n,), i32)
        self._check(self._pfd_fn("pfd_dmprof", pin, kill, pol)(
            self._h, C.byref(pin), _ptr(out["profile"]) if profile else None,
            _ptr(out["chis"]) if chis else None, _ptr(out["lyon8"]) if lyon8 else None,
            _ptr(out["status"]), flags))
        del keep, kkeep
        return out

    def _pfd_scores(self, fn, k, profs, subfreqs, scal, out, status, derive_avgprof=False,
                    byteswapped=False, scl=None, offs=None, wts=None, kill_parts=None,
                    kill_subs=None, pol_sum=None):
        pol = self._pfd_pol(fn, profs, pol_sum)
        kill, kkeep = self._pfd_kill(fn, profs, kill_parts, kill_subs)
        pin, dev, keep = self._pfd_args(profs, subfreqs, scal, fn, scl, offs, wts, pol)
        out, status, flags = self._outputs(dev, profs, pin.n, k, out, status)
        if derive_avgprof:
            flags |= PFE_FLAG_PFD_AVGPROF
        if byteswapped:
            flags |= PFE_FLAG_PFD_BSWAP
        self._check(self._pfd_fn(fn, pin, kill, pol)(self._h, C.byref(pin), _ptr(out), _ptr(status), flags))
        del keep, kkeep
        return out, status

    def pfd_bates22(self, profs, subfreqs, scal, out=None, status=None, derive_avgprof=False,
                    byteswapped=False, scl=None, offs=None, wts=None, kill_parts=None,
                    kill_subs=None, pol_sum=None):
        """The 22 scores of PFD folds (pfe_pfd_bates22, PFDFile.compute) for a batch of one
        shape: profs (n,npart,nsub,L) f64, subfreqs (n,nsub), scal (n,PFE_PFD_NSCAL) with
        scal[:, 7] = bary_p1.  Returns (out (n,22) f64, status (n,))."""
        return self._pfd_scores("pfd_bates22", 22, profs, subfreqs, scal, out, status,
                                derive_avgprof, byteswapped, scl, offs, wts, kill_parts, kill_subs, pol_sum)

    # one score group of a batch of folds (PFDOperations; inputs as pfd_bates22)
    def pfd_params4(self, profs, subfreqs, scal, out=None, status=None, derive_avgprof=False,
                    byteswapped=False, scl=None, offs=None, wts=None, kill_parts=None,
                    kill_subs=None, pol_sum=None):
        """getCandidateParameters (pfe_pfd_params4): [period_ms, snr, dm, width], unfiltered."""
        return self._pfd_scores("pfd_params4", 4, profs, subfreqs, scal, out, status,
                                derive_avgprof, byteswapped, scl, offs, wts, kill_parts, kill_subs, pol_sum)

    def pfd_dmfit4(self, profs, subfreqs, scal, out=None, status=None, derive_avgprof=False,
                   byteswapped=False, scl=None, offs=None, wts=None, kill_parts=None,
                   kill_subs=None, pol_sum=None):
        """getDMFittings (pfe_pfd_dmfit4): [s16, s17, Shift (signed), s19]."""
        return self._pfd_scores("pfd_dmfit4", 4, profs, subfreqs, scal, out, status,
                                derive_avgprof, byteswapped, scl, offs, wts, kill_parts, kill_subs, pol_sum)

    def pfd_subband3(self, profs, subfreqs, scal, out=None, status=None, derive_avgprof=False,
                     byteswapped=False, scl=None, offs=None, wts=None, kill_parts=None,
                     kill_subs=None, pol_sum=None):
        """getSubbandParameters (pfe_pfd_subband3): s20-s22."""
        return self._pfd_scores("pfd_subband3", 3, profs, subfreqs, scal, out, status,
                                derive_avgprof, byteswapped, scl, offs, wts, kill_parts, kill_subs, pol_sum)


class PhcxBatch:
    """Files parsed by the native reader (pfe_phcx_parse): per-file info and decoded fields."""

    def __init__(self, paths, mode: int = -1, threads: int = 0):
        self.lib = load_library()
        self.paths = [os.fsencode(p) for p in paths]
        arr = (C.c_char_p * max(1, len(self.paths)))(*self.paths)
        h = C.c_void_p()
        rc = self.lib.pfe_phcx_parse(arr, len(self.paths), int(mode), int(threads), C.byref(h))
        if rc != PFE_OK:
            raise PfeError(f"pfe_phcx_parse failed ({rc})")
        self._h = h

    def __len__(self):
        return len(self.paths)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pfe_phcx_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self, i: int) -> PhcxInfo:
        inf = PhcxInfo()
        if self.lib.pfe_phcx_info_get(self._h, i, C.byref(inf)) != PFE_OK:
            raise IndexError(i)
        return inf

    def infos(self) -> np.ndarray:
        """Every file's pfe_phcx_info as one structured array (PHCX_INFO_DTYPE)."""
        out = np.empty(len(self.paths), dtype=PHCX_INFO_DTYPE)
        if self.lib.pfe_phcx_info_all(self._h, out.ctypes.data if len(out) else None,
                                      len(out)) != PFE_OK:
            raise PfeError("pfe_phcx_info_all failed")
        return out

    def fetch(self, i: int, field: int, count: int, dtype=np.uint8) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if self.lib.pfe_phcx_fetch(self._h, i, field, out.ctypes.data, count) != PFE_OK:
            raise PfeError(f"pfe_phcx_fetch({i}, {field}) failed")
        return out

    def pack(self, rows, lp=None, ld=None, nsub_lsb=None, ndm=None, threads: int = 0,
             alloc=None):
        """Dense arrays of the given rows (all of one shape): dict of numpy arrays.
        alloc(name, shape, dtype) -> array supplies the destination buffers (e.g. views of
        reused pinned slabs); default np.empty."""
        alloc = alloc or (lambda _k, shape, dt: np.empty(shape, dtype=dt))
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        n = len(rows)
        out = {"scal": alloc("scal", (n, 8), np.float64)}
        ptr = {}
        if lp is not None:
            out["prof"] = alloc("prof", (n, lp), np.uint8)
        if ld is not None:
            out["lyon_dm"] = alloc("lyon_dm", (n, ld), np.uint8)
        if nsub_lsb is not None:
            out["sub"] = alloc("sub", (n,) + tuple(nsub_lsb), np.uint8)
        if ndm is not None:
            out["dmcurve"] = alloc("dmcurve", (n, ndm), np.float64)
        for k in ("prof", "lyon_dm", "sub", "dmcurve"):
            ptr[k] = out[k].ctypes.data if k in out else None
        rc = self.lib.pfe_phcx_pack(
            self._h, rows.ctypes.data, n, int(threads),
            ptr["prof"], lp or 0, ptr["lyon_dm"], ld or 0,
            ptr["sub"], (nsub_lsb[0] * nsub_lsb[1]) if nsub_lsb else 0,
            ptr["dmcurve"], ndm or 0, out["scal"].ctypes.data)
        if rc != PFE_OK:
            raise PfeError("pfe_phcx_pack: rows of another shape or failed files")
        return out


class PfdBatch:
    """.pfd files scanned by the native reader (pfe_pfd_scan): per-file info, the small arrays,
    and the cubes packed by pread into caller slabs (pfe_pfd_pack)."""

    def __init__(self, paths, threads: int = 0):
        self.lib = load_library()
        self.paths = [os.fsencode(p) for p in paths]
        arr = (C.c_char_p * max(1, len(self.paths)))(*self.paths)
        h = C.c_void_p()
        rc = self.lib.pfe_pfd_scan(arr, len(self.paths), int(threads), C.byref(h))
        if rc != PFE_OK:
            raise PfeError(f"pfe_pfd_scan failed ({rc})")
        self._h = h

    def __len__(self):
        return len(self.paths)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pfe_pfd_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def infos(self) -> np.ndarray:
        """Every file's pfe_pfd_info as one structured array (PFD_INFO_DTYPE)."""
        out = np.empty(len(self.paths), dtype=PFD_INFO_DTYPE)
        if self.lib.pfe_pfd_info_all(self._h, out.ctypes.data if len(out) else None,
                                     len(out)) != PFE_OK:
            raise PfeError("pfe_pfd_info_all failed")
        return out

    def fetch(self, i: int, field: int, count: int, dtype=np.float64) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if self.lib.pfe_pfd_fetch(self._h, i, field, out.ctypes.data if count else None,
                                  count) != PFE_OK:
            raise PfeError(f"pfe_pfd_fetch({i}, {field}) failed")
        return out

    def data(self, i: int, info=None):
        """File i as the PFDData pfd.read(path, avgprof=False) gives: every attribute from the
        native reader (the cube through pack, a big-endian one byte-swapped here).  For
        comparing the two readers; the product path packs and never builds one of these."""
        from .pfd import PFDData

        inf = self.infos()[i] if info is None else info
        if inf["status"] != 0:
            raise PfeError(f"file {i}: native reader status {PFE_IO_STATUS.get(int(inf['status']))}")
        npart, nsub, proflen = int(inf["npart"]), int(inf["nsub"]), int(inf["proflen"])
        head = self.fetch(i, PFE_PFD_F_HEAD, PFE_PFD_NHEAD)
        kw = {k: float(v) for k, v in zip(PFD_HEAD_NAMES, head) if k != "orb"}
        kw["orb"] = tuple(float(v) for v in head[12:19])
        names = ("filenm", "candnm", "telescope", "pgdev", "rastr", "decstr")
        for k, name in enumerate(names):
            kw[name] = self.fetch(i, PFE_PFD_F_FILENM + k, int(inf["slen"][k]), np.uint8).tobytes()
        a = self.pack([i], (npart, nsub, proflen))
        profs = a["profs"][0]
        if inf["big_endian"]:
            profs = profs.byteswap()
        return PFDData(
            swap=">" if inf["big_endian"] else "<", numdms=int(inf["numdms"]),
            numperiods=int(inf["numperiods"]), numpdots=int(inf["numpdots"]), nsub=nsub,
            npart=npart, proflen=proflen, numchan=int(inf["numchan"]),
            chanpersub=int(inf["chanpersub"]),
            dms=self.fetch(i, PFE_PFD_F_DMS, int(inf["numdms"])),
            periods=self.fetch(i, PFE_PFD_F_PERIODS, int(inf["numperiods"])),
            pdots=self.fetch(i, PFE_PFD_F_PDOTS, int(inf["numpdots"])), profs=profs,
            stats=self.fetch(i, PFE_PFD_F_STATS, npart * nsub * 7).reshape(npart, nsub, 7),
            subfreqs=self.fetch(i, PFE_PFD_F_SUBFREQS, nsub), avgprof=None, killed_subbands=[],
            killed_intervals=[], **kw)

    def pack(self, rows, shape, threads: int = 0, alloc=None, cube=True):
        """Dense inputs of the PFD calls for the given rows (all of one (npart, nsub, proflen)
        `shape` and one byte order): dict(profs (n,npart,nsub,proflen) float64 holding the
        files' cube bytes as they are -- byte-reversed values for big-endian files: score with
        byteswapped=True --, subfreqs (n,nsub), scal (n,8) with scal[:, 2] NaN: score with
        derive_avgprof=True).  alloc(name, shape, dtype) -> array supplies the destinations
        (e.g. views of reused pinned slabs); default np.empty.  cube False: no profs."""
        alloc = alloc or (lambda _k, shp, dt: np.empty(shp, dtype=dt))
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        n = len(rows)
        npart, nsub, proflen = (int(v) for v in shape)
        inf = self.infos()[rows]  # the destinations are sized by `shape`: it must be the files'
        if n and not ((inf["status"] == 0) & (inf["npart"] == npart) & (inf["nsub"] == nsub)
                      & (inf["proflen"] == proflen)).all():
            raise PfeError("pfe_pfd_pack: rows of another shape or failed files")
        out = {"subfreqs": alloc("subfreqs", (n, nsub), np.float64),
               "scal": alloc("scal", (n, PFE_PFD_NSCAL), np.float64)}
        if cube:
            out["profs"] = alloc("profs", (n, npart, nsub, proflen), np.float64)
        rc = self.lib.pfe_pfd_pack(self._h, rows.ctypes.data, n, int(threads),
                                   out["profs"].ctypes.data if cube else None,
                                   out["subfreqs"].ctypes.data, out["scal"].ctypes.data)
        if rc != PFE_OK:
            raise PfeError("pfe_pfd_pack: rows of another shape or byte order, failed files, "
                           "or a file that changed since the scan")
        return out


def format_rows(names, vals: np.ndarray, style: int = 0, skip=None, threads: int = 0) -> bytes:
    """pfe_format_rows: the text DataProcessor writes for score rows (storeScore style 0,
    storeScoreARFF style 1, outputScores style 2) -- see include/pfe_io.h.  names: str or
    bytes per row; vals (n, width) float64 with contiguous rows; skip: rows to leave out."""
    lib = load_library()
    vals = np.asarray(vals, dtype=np.float64)
    if vals.ndim != 2 or (vals.shape[0] and vals.strides[1] != 8):
        vals = np.ascontiguousarray(vals.reshape(len(vals), -1))
    n, width = vals.shape
    if n == 0:
        return b""
    enc = [os.fsencode(x) if isinstance(x, str) else bytes(x) for x in names]
    if len(enc) != n:
        raise ValueError("one name per row")
    blob = b"".join(enc)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    sk = None
    if skip is not None:
        sk = np.ascontiguousarray(skip, dtype=np.uint8)
        if sk.shape != (n,):
            raise ValueError("skip must have one entry per row")
    cap = len(blob) + n * (24 * width + 8) + 16
    buf = C.create_string_buffer(cap)
    used = C.c_int64()
    rc = lib.pfe_format_rows(blob, off.ctypes.data, vals.ctypes.data, n, width,
                             _row_stride(vals.strides[0] // 8, vals), int(style),
                             None if sk is None else sk.ctypes.data, int(threads), buf, cap,
                             C.byref(used))
    if rc != PFE_OK:
        raise PfeError("pfe_format_rows failed")
    return buf.raw[:used.value]
