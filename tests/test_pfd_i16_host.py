"""The int16 PFD calls on a CPU: the six symbols, the layout of pfe_pfd_i16_in, and the rounding
claim of the contract (include/pfe.h): numpy's float64 decode d * scl + offs [* wts] is exact
rational arithmetic rounded once at + offs and once at * wts, because the product of a 16-bit
integer and a float32 is exact in float64."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np

from pulsarfeatureextractor_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pfe_pfd_dmprof_i16", "pfe_pfd_bates22_i16", "pfe_pfd_params4_i16", "pfe_pfd_dmfit4_i16",
         "pfe_pfd_subband3_i16", "pfe_pfd_avgprof_i16")


def header():
    return open(os.path.join(ROOT, "include", "pfe.h")).read()


def test_symbols_are_declared_bound_and_exported():
    src = header()
    for name in NAMES:
        assert re.search(r"^int\s+" + name + r"\s*\(pfe_handle\* h, const pfe_pfd_i16_in\* in,", src, re.M), name
        assert name in _native.EXPORTED_SYMBOLS
    lib = _native.load_library()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes[1] == C.POINTER(_native.PfdI16In), name
    assert len(lib.pfe_pfd_avgprof_i16.argtypes) == 5
    assert len(lib.pfe_pfd_dmprof_i16.argtypes) == 7


C_TYPES = {"const int16_t*": C.c_void_p, "const float*": C.c_void_p, "const double*": C.c_void_p,
           "int64_t": C.c_int64, "int32_t": C.c_int32}


def test_struct_layout_matches_the_header():
    """The fields of the header's struct, in order, laid out by ctypes on their own, against
    PfdI16In's names, offsets and sizes."""
    body = re.search(r"typedef struct pfe_pfd_i16_in \{(.*?)\} pfe_pfd_i16_in;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const \w+\*|\w+)\s+(.*)", decl)
        for name in m.group(2).split(","):
            fields.append((name.strip(), C_TYPES[m.group(1)]))
    assert [f for f, _ in fields] == ["data", "scl", "offs", "wts", "fold_stride", "part_stride",
                                      "subfreqs", "scal", "npart", "nsub", "proflen", "n"]

    class FromHeader(C.Structure):
        _fields_ = fields

    assert [f for f, _ in _native.PfdI16In._fields_] == [f for f, _ in fields]
    for name, _ in fields:
        got, want = getattr(_native.PfdI16In, name), getattr(FromHeader, name)
        assert (got.offset, got.size) == (want.offset, want.size), name
    assert C.sizeof(_native.PfdI16In) == C.sizeof(FromHeader) == 88
    assert _native.PfdI16In.fold_stride.offset == 32 and _native.PfdI16In.npart.offset == 64
    assert _native.PfdI16In.n.offset == 80


def round_f64(q: Fraction) -> float:
    """The float64 nearest to q, ties to even (CPython's correctly rounded int / int)."""
    return q.numerator / q.denominator


def finite_f32(rng, count):
    """Random finite float32 bit patterns: every exponent, subnormals included."""
    bits = rng.integers(0, 1 << 32, size=2 * count, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    v = v[np.isfinite(v)][:count]
    assert v.size == count and (np.abs(v[v != 0]) < np.finfo(np.float32).tiny).any()
    return v


def test_the_decode_rounds_once_at_the_offset_and_once_at_the_weight():
    rng = np.random.default_rng(20261021)
    n = 3000
    d = rng.integers(-32768, 32768, size=n).astype(np.int16)
    d[:4] = (-32768, 32767, 0, 1)
    scl, offs, wts = finite_f32(rng, n), finite_f32(rng, n), finite_f32(rng, n)
    # offsets near the products, so the sum's rounding is not all absorbed
    near = (d[n // 2:].astype(np.float64) * scl[n // 2:].astype(np.float64)
            * rng.uniform(-2, 2, size=n - n // 2))
    with np.errstate(over="ignore"):
        near = near.astype(np.float32)
    offs[n // 2:] = np.where(np.isfinite(near), near, offs[n // 2:])
    prod = d.astype(np.float64) * scl.astype(np.float64)
    x = prod + offs.astype(np.float64)
    xw = x * wts.astype(np.float64)
    assert np.isfinite(xw).all()      # 2^15 x 2^128 x 2^128 is far inside float64
    inexact_sum = 0
    for i in range(n):
        di, a, o, w = int(d[i]), Fraction(float(scl[i])), Fraction(float(offs[i])), Fraction(float(wts[i]))
        assert Fraction(float(prod[i])) == di * a, "the product is exact"
        want = round_f64(di * a + o)
        assert float(x[i]) == want, i
        inexact_sum += Fraction(want) != di * a + o
        want_w = round_f64(Fraction(float(x[i])) * w)
        assert float(xw[i]) == want_w, i
    assert inexact_sum > n // 10      # the roundings the test is about did happen
