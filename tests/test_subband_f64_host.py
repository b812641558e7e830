"""Host side of the float sub-band calls: PHCXOperations routes byte-valued input to
pfe_subband3 and anything else to pfe_subband3_f64 (a stub engine records the call), the
Engine methods have the documented signatures, and the new option is in the option table."""
import inspect

import numpy as np
import pytest

from pulsarfeatureextractor_amd import _native
from pulsarfeatureextractor_amd.profile_ops import PFDOperations, PHCXOperations


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


def inputs(n=3, nsub=4, lsb=16, seed=0):
    rng = np.random.default_rng(seed)
    prof = rng.integers(0, 256, (n, lsb))
    sub = rng.integers(0, 256, (n, nsub, lsb))
    scal = np.zeros((n, 8))
    scal[:, 3] = 0.1
    return prof, sub, scal


def test_float_input_reaches_subband3_f64():
    prof, sub, scal = inputs()
    for p, s in ((prof * 0.731 + 0.2, sub * 1.3 - 4.0),     # both float
                 (prof, sub * 1.3 - 4.0),                    # byte profile, float sub-bands
                 (prof - 10.5, sub)):                        # float profile, byte sub-bands
        eng = StubEngine()
        out, st = PHCXOperations(engine=eng).getSubbandParameters_batch(p, s, scal)
        (name, gp, gs, gscal), = eng.calls
        assert name == "subband3_f64"
        assert gp.dtype == np.float64 and gs.dtype == np.float64 and gscal.dtype == np.float64
        assert gp.flags.c_contiguous and gs.flags.c_contiguous
        assert np.array_equal(gp, p) and np.array_equal(gs, s)
        assert out.shape == (3, 3) and st.shape == (3,)


def test_byte_valued_input_still_reaches_subband3():
    prof, sub, scal = inputs()
    for p, s in ((prof.astype(np.uint8), sub.astype(np.uint8)),
                 (prof.astype(np.float64), sub.astype(np.float64)),   # floats holding integers 0-255
                 (prof.astype(np.int64), sub.astype(np.float32))):
        eng = StubEngine()
        PHCXOperations(engine=eng).getSubbandParameters_batch(p, s, scal)
        (name, gp, gs, _), = eng.calls
        assert name == "subband3"
        assert gp.dtype == np.uint8 and gs.dtype == np.uint8
        assert np.array_equal(gp, prof) and np.array_equal(gs, sub)


def test_one_profile_row_is_accepted():
    prof, sub, scal = inputs(n=1)
    eng = StubEngine()
    PHCXOperations(engine=eng).getSubbandParameters_batch(prof[0] + 0.5, sub, scal)
    assert eng.calls[0][0] == "subband3_f64" and eng.calls[0][1].shape == (1, 16)


def test_pfd_foreign_profile_stays_refused():
    with pytest.raises(ValueError):
        PFDOperations(engine=StubEngine()).getSubbandParameters(data=None, profile=np.arange(8.0))


def test_engine_method_signatures():
    sig = inspect.signature(_native.Engine.subband3_f64)
    assert list(sig.parameters) == ["self", "prof", "sub", "scal", "out", "status"]
    assert sig.parameters["out"].default is None and sig.parameters["status"].default is None
    sig = inspect.signature(_native.Engine.bates22_f64)
    assert list(sig.parameters) == ["self", "prof", "sub", "dmcurve", "scal", "out", "status"]
    assert sig.parameters["out"].default is None and sig.parameters["status"].default is None


def test_struct_and_symbols():
    assert {"pfe_subband3_f64", "pfe_bates22_f64"} <= set(_native.EXPORTED_SYMBOLS)
    names = [f[0] for f in _native.BatesF64In._fields_]
    assert names == ["prof", "lp", "sub", "nsub", "lsb", "dmcurve", "ndm", "scal", "n"]
    lib = _native.load_library()
    assert lib.pfe_subband3_f64.argtypes[1]._type_ is _native.BatesF64In
    assert lib.pfe_bates22_f64.argtypes[1]._type_ is _native.BatesF64In


def test_option_name_round_trips():
    import os
    import re

    assert _native.OPTIONS["subf64_global"] == 12
    assert len(set(_native.OPTIONS.values())) == len(_native.OPTIONS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pfe.h")).read()
    ids = {m.group(1).lower(): int(m.group(2))
           for m in re.finditer(r"^#define PFE_OPT_(\w+) (\d+)$", hdr, re.M)}
    assert ids == _native.OPTIONS
