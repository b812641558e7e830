"""The float64 edge rows of synth.f64_edge_rows, checked on the CPU: that the reference of the
GPU test (oracle.lyon.lyon8_batched) is the reference's own row-by-row arithmetic on them,
and that they contain what gives tests/test_lyon8_f64_gpu.py its teeth -- constant rows on
both sides of scipy's zero-variance rule, and offset rows whose skew and kurtosis are finite.
These are conditions on the inputs, not on the kernel."""
import warnings

import numpy as np
import pytest
from scipy.stats import kurtosis

from oracle.lyon import lyon8, lyon8_batched
from pulsarfeatureextractor_amd.synth import F64_EDGE_ROWS, f64_edge_rows

# (lp, ld) of the GPU test: the seams of numpy's sum (sequential below 8, the remainder after
# the 8 accumulators, the 128-value leaf, the first split, floor8(n / 2) leaving uneven
# halves), and a row longer than the 160 KiB of LDS hold
SEAM_PAIRS = [(1, 2), (3, 7), (8, 9), (15, 16), (127, 128), (129, 136), (255, 257),
              (263, 1000), (969, 4097)]
LONG_PAIRS = [(33001, 129), (8193, 16391)]   # numpy sums a row in buffers of 8192 values
SEED = 20261101

_cache = {}


def edge_rows(L):
    """(rows, names) of length L: one draw per length, shared by every test, never changed."""
    if L not in _cache:
        rows, names = f64_edge_rows(L, np.random.default_rng(SEED + L))
        rows.setflags(write=False)
        _cache[L] = (rows, names)
    return _cache[L]


def all_lengths():
    return sorted({L for p in SEAM_PAIRS + LONG_PAIRS for L in p})


def reference(prof, dm):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return lyon8_batched(prof, dm)


def kurtosis_paths_agree(rows):
    """scipy's kurtosis divides m4 by m2**2.0.  On an array of rows that is m2 * m2; on one row
    at a time -- what the reference program does, and what scipy itself does for a whole batch
    as soon as any row of it holds a NaN -- m2 is a scalar and the power is libm's
    pow(m2, 2.0), which is not always the same double (about one m2 in a thousand).  True for
    the rows on which both give the same bits: only there is the reference's kurtosis one
    number rather than two."""
    fin = ~np.isnan(rows).any(axis=1)
    vec = np.full(len(rows), np.nan)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        vec[fin] = kurtosis(rows[fin], axis=1)
        loop = np.array([kurtosis(r) for r in rows])
    return (vec == loop) | (np.isnan(vec) & np.isnan(loop))


def test_block_shape_and_names():
    for L in (1, 2, 3, 129):
        rows, names = edge_rows(L)
        assert rows.shape == (F64_EDGE_ROWS, L) and rows.dtype == np.float64
        assert len(names) == F64_EDGE_ROWS == len(set(names))
        assert sum(n.startswith("const_") for n in names) == (14 if L >= 3 else 12)
        for want in ("exact_0.0", "exact_1.0", "exact_-2.5", "step_1ulp", "offset_1e9",
                     "offset_-1e6", "wide", "scale_1e-160", "scale_1e160", "spike",
                     "alternating", "ramp", "nan", "inf", "inf_-inf", "plain0"):
            assert want in names, (L, want)
    rows, names = edge_rows(129)
    step = rows[names.index("step_1ulp")]
    assert np.count_nonzero(step != step[0]) == 1 and step.max() == np.nextafter(step[0], np.inf)


@pytest.mark.parametrize("lp,ld", [(7, 129), (263, 1000), (33001, 4097)])
def test_batched_reference_is_the_row_loop(lp, ld):
    """lyon8 (numpy / scipy on one row at a time, as the reference calls them) and
    lyon8_batched agree bit for bit, NaN-aware, on the edge rows."""
    prof, dm = edge_rows(lp)[0], edge_rows(ld)[0]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        a = lyon8(prof, dm)
    b = reference(prof, dm)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    assert np.array_equal(a[m].view(np.uint64), b[m].view(np.uint64))


def test_constant_rows_fall_on_both_sides_of_the_zero_variance_rule():
    n_nan = n_one = 0
    for L in all_lengths():
        rows, names = edge_rows(L)
        sel = [i for i, n in enumerate(names) if n.startswith("const_")]
        sk = reference(rows[sel], rows[sel])[:, 2]
        n_nan += int(np.isnan(sk).sum())
        n_one += int((np.abs(sk) == 1.0).sum())
        assert (np.isnan(sk) | (np.abs(sk) == 1.0)).all(), (L, sk)
    print(f"constant non-dyadic rows: skew NaN in {n_nan}, +-1.0 in {n_one}")
    assert n_nan >= 10 and n_one >= 10


def test_offset_rows_have_finite_moments():
    for L in all_lengths():
        if L < 2:
            continue  # a single value has no variance
        rows, names = edge_rows(L)
        sel = [names.index("offset_1e9"), names.index("offset_-1e6")]
        ref = reference(rows[sel], rows[sel])[:, :4]
        assert (ref[:, 1] > 0).all(), L
        assert np.isfinite(ref[:, 2:]).all(), L


def test_reference_kurtosis_is_one_number_on_the_edge_rows():
    """A condition on the inputs (see kurtosis_paths_agree): should a seed not meet it, change
    the seed."""
    for L in all_lengths():
        rows, names = edge_rows(L)
        ok = kurtosis_paths_agree(rows)
        assert ok.all(), (L, [names[i] for i in np.nonzero(~ok)[0]])
