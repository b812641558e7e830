"""Host side of the float32 forms of the float-array calls: the five symbols and the
pfe_bates_f32_in structure, the Engine method signatures, PHCXOperations' routing of float32
input to pfe_subband3_f32 (a stub engine records the call), and the input of the sub-band CPU
anchor of tests/test_cand_f32_gpu.py judged by the oracle alone."""
import inspect
import os
import re

import numpy as np

from pulsarfeatureextractor_amd import _native
from pulsarfeatureextractor_amd.profile_ops import PHCXOperations

NEW = ("pfe_lyon8_f32", "pfe_sinusoid4_f32", "pfe_gauss7_f32", "pfe_subband3_f32", "pfe_bates22_f32")
ANCHOR_SEED = 3100   # of anchor_batch: see test_anchor_rows_are_well_conditioned


def anchor_batch(n=32, nsub=16, lsb=128, seed=ANCHOR_SEED):
    """The float batch of test_subband_f64_gpu.float_batch, made in float32: (prof32, sub32,
    scal), scal float64."""
    from test_subband_f64_gpu import float_batch

    b = float_batch(n, nsub, lsb, seed=seed)
    return b["prof"].astype(np.float32), b["sub"].astype(np.float32), b["scal"]


def test_symbols_and_struct():
    assert set(NEW) <= set(_native.EXPORTED_SYMBOLS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pfe.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(pfe_handle\* h, const " % name, hdr, re.M), name
    assert re.search(r"#define PFE_ABI_VERSION 1$", hdr, re.M)
    m = re.search(r"typedef struct pfe_bates_f32_in \{(.*?)\} pfe_bates_f32_in;", hdr, re.S)
    fields = re.findall(r"(const float\*|const double\*|int32_t|int64_t) (\w+);", m.group(1))
    assert fields == [("const float*", "prof"), ("int32_t", "lp"), ("const float*", "sub"),
                      ("int32_t", "nsub"), ("int32_t", "lsb"), ("const float*", "dmcurve"),
                      ("int32_t", "ndm"), ("const double*", "scal"), ("int64_t", "n")]
    names = [f[0] for f in _native.BatesF32In._fields_]
    assert names == [f[1] for f in fields]
    import ctypes as C
    assert C.sizeof(_native.BatesF32In) == C.sizeof(_native.BatesF64In)
    lib = _native.load_library()
    assert lib.pfe_subband3_f32.argtypes[1]._type_ is _native.BatesF32In
    assert lib.pfe_bates22_f32.argtypes[1]._type_ is _native.BatesF32In
    assert lib.pfe_lyon8_f32.argtypes == lib.pfe_lyon8_f64.argtypes
    assert lib.pfe_sinusoid4_f32.argtypes == lib.pfe_sinusoid4_f64.argtypes
    assert lib.pfe_gauss7_f32.argtypes == lib.pfe_gauss7_f64.argtypes


def test_engine_method_signatures():
    E = _native.Engine
    for f32, f64 in ((E.sinusoid4_f32, E.sinusoid4_f64), (E.gauss7_f32, E.gauss7_f64),
                     (E.subband3_f32, E.subband3_f64), (E.bates22_f32, E.bates22_f64)):
        a, b = inspect.signature(f32), inspect.signature(f64)
        assert list(a.parameters) == list(b.parameters)
        assert a.parameters["out"].default is None and a.parameters["status"].default is None
    assert list(inspect.signature(E.bates22_f32).parameters) == \
        ["self", "prof", "sub", "dmcurve", "scal", "out", "status"]


class StubEngine:
    def __init__(self):
        self.calls = []

    def _record(self, name, prof, sub, scal):
        self.calls.append((name, prof, sub, scal))
        n = len(prof)
        return np.tile([1.0, 2.0, 3.0], (n, 1)), np.zeros(n, dtype=np.uint32)

    def subband3(self, prof, sub, scal, out=None, status=None):
        return self._record("subband3", prof, sub, scal)

    def subband3_f64(self, prof, sub, scal, out=None, status=None):
        return self._record("subband3_f64", prof, sub, scal)

    def subband3_f32(self, prof, sub, scal, out=None, status=None):
        return self._record("subband3_f32", prof, sub, scal)


def inputs(n=3, nsub=4, lsb=16, seed=0):
    rng = np.random.default_rng(seed)
    prof = rng.integers(0, 256, (n, lsb))
    sub = rng.integers(0, 256, (n, nsub, lsb))
    scal = np.zeros((n, 8))
    scal[:, 3] = 0.1
    return prof, sub, scal


def route(p, s, scal):
    eng = StubEngine()
    out, st = PHCXOperations(engine=eng).getSubbandParameters_batch(p, s, scal)
    (call,) = eng.calls
    assert out.shape == (len(s), 3) and st.shape == (len(s),)
    return call


def test_float32_input_reaches_subband3_f32_as_it_is():
    prof, sub, scal = inputs()
    p32 = (prof * 0.731 + 0.2).astype(np.float32)
    s32 = (sub * 1.3 - 4.0).astype(np.float32)
    keep_p, keep_s = p32.copy(), s32.copy()
    name, gp, gs, gscal = route(p32, s32, scal)
    assert name == "subband3_f32"
    assert gp.dtype == np.float32 and gs.dtype == np.float32 and gscal.dtype == np.float64
    assert gp.flags.c_contiguous and gs.flags.c_contiguous
    assert np.shares_memory(gp, p32) and np.shares_memory(gs, s32), "dense float32 input was copied"
    assert np.array_equal(p32, keep_p) and np.array_equal(s32, keep_s)
    assert np.array_equal(gp, keep_p) and np.array_equal(gs, keep_s)
    # strided float32 input is made dense, still float32; one profile row is accepted
    wide = np.zeros((3, 4, 32), dtype=np.float32)
    wide[:, :, ::2] = s32
    name, gp, gs, _ = route(p32, wide[:, :, ::2], scal)
    assert name == "subband3_f32" and gs.dtype == np.float32 and gs.flags.c_contiguous
    assert np.array_equal(gs, s32)
    name, gp, gs, _ = route(p32[0], s32[:1], scal[:1])
    assert name == "subband3_f32" and gp.shape == (1, 16) and gp.dtype == np.float32


def test_byte_valued_float32_still_reaches_subband3():
    prof, sub, scal = inputs()
    name, gp, gs, _ = route(prof.astype(np.float32), sub.astype(np.float32), scal)
    assert name == "subband3"
    assert gp.dtype == np.uint8 and gs.dtype == np.uint8
    assert np.array_equal(gp, prof) and np.array_equal(gs, sub)


def test_mixed_float_widths_still_reach_subband3_f64():
    prof, sub, scal = inputs()
    p32 = (prof * 0.731 + 0.2).astype(np.float32)
    s32 = (sub * 1.3 - 4.0).astype(np.float32)
    for p, s in ((p32, s32.astype(np.float64)),     # float32 profile, float64 sub-bands
                 (p32.astype(np.float64), s32),     # float64 profile, float32 sub-bands
                 (prof.astype(np.uint8), s32),      # byte profile, float32 sub-bands
                 (list(map(list, p32)), s32)):      # a profile that is no array
        name, gp, gs, _ = route(p, s, scal)
        assert name == "subband3_f64"
        assert gp.dtype == np.float64 and gs.dtype == np.float64
        assert np.array_equal(gp, np.asarray(p, dtype=np.float64)) and np.array_equal(gs, s)


def test_anchor_rows_are_well_conditioned():
    """The input of the GPU file's sub-band anchor, judged by the reference alone: s21 is a mean
    of correlations in [-1, 1], each good to a few ulp, so a mean below 1e-3 has cancelled away
    the digits a relative bar measures and such rows are left out there (as in
    test_subband_f64_gpu.py).  The seed keeps at least 90 % of the rows."""
    from test_subband_f64_gpu import oracle_sub

    p32, s32, scal = anchor_batch()
    ref, ok = oracle_sub(p32.astype(np.float64), s32.astype(np.float64), scal)
    keep = ok & (np.abs(ref[:, 1]) >= 1e-3)
    print(f"anchor: {int(ok.sum())}/{len(ok)} rows scored, {int(keep.sum())} kept")
    assert keep.sum() >= 0.9 * len(keep)
