"""GPU parity of pfe_lyon8_f64 (the 8 Lyon features of float64 rows) against numpy / scipy
(oracle.lyon.lyon8_batched on the same arrays) at the edges of float rows.

Bar, on every row (none skipped, no share excused) -- the PFD path's bar in test_pfd_gpu.py:
  * the NaN pattern identical in all 8 columns;
  * mean, std and kurtosis (columns 0, 1, 3, 4, 5, 7) equal under == (infinities included,
    the sign of zero not distinguished);
  * skew (columns 2, 6) equal or within 1e-13 relative: the device's pow(m2, 1.5) is not libm's.

The rows are synth.f64_edge_rows (tests/test_lyon8_f64_rows_host.py shows on the CPU that they
hold constant rows on both sides of scipy's zero-variance rule); the lengths sit at the seams
of numpy's pairwise sum."""
import numpy as np
import pytest

from pulsarfeatureextractor_amd.synth import F64_EDGE_ROWS
from test_lyon8_f64_rows_host import (LONG_PAIRS, SEAM_PAIRS, edge_rows, kurtosis_paths_agree,
                                       reference)

pytestmark = pytest.mark.gpu
EXACT_COLS = (0, 1, 3, 4, 5, 7)
SKEW_COLS = (2, 6)
SKEW_TOL = 1e-13
COL = ("mean", "std", "skew", "kurt")


def eq_nan(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def compare(got, ref, names=None, what="", exact_cols=EXACT_COLS, skew_cols=SKEW_COLS):
    """Print every figure, then assert the bar.  names: (prof names, dm names) per row."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan_rows = np.nonzero((np.isnan(got) != np.isnan(ref)).any(axis=1))[0]
    both = ~np.isnan(got) & ~np.isnan(ref)
    with np.errstate(all="ignore"):
        rel = np.abs(got - ref) / np.abs(ref)
    rel[eq_nan(got, ref) | ~both] = 0.0   # rows of a differing NaN pattern are counted above
    bad = np.zeros(ref.shape, dtype=bool)
    for c in exact_cols:
        bad[:, c] = ~eq_nan(got[:, c], ref[:, c])
    for c in skew_cols:
        bad[:, c] = ~(eq_nan(got[:, c], ref[:, c]) | (rel[:, c] <= SKEW_TOL))
    worst = {COL[k]: float(max(rel[:, [c for c in range(ref.shape[1]) if c % 4 == k]].max(initial=0.0), 0.0))
             for k in range(4)}
    print(f"{what}: {len(ref)} rows, NaN pattern differs in {len(nan_rows)}, rows off the bar "
          f"{int(bad.any(axis=1).sum())}, worst rel err " +
          ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for r in np.nonzero(bad.any(axis=1))[0][:12]:
        for c in np.nonzero(bad[r])[0]:
            nm = names[c // 4][r] if names is not None else ""
            print(f"  row {r} {nm} col {c} ({COL[c % 4]}): got {got[r, c]!r} ref {ref[r, c]!r}")
    assert len(nan_rows) == 0, f"{what}: NaN pattern differs in rows {nan_rows[:20].tolist()}"
    assert not bad.any(), f"{what}: {int(bad.any(axis=1).sum())} rows off the bar, worst {worst}"


def edge_pair(lp, ld):
    (p, pn), (d, dn) = edge_rows(lp), edge_rows(ld)
    return p, d, (pn, dn)


_refs = {}


def ref_of(key, prof, dm):
    if key not in _refs:
        _refs[key] = reference(prof, dm)
        _refs[key].setflags(write=False)
    return _refs[key]


@pytest.mark.parametrize("lp,ld", SEAM_PAIRS)
def test_edge_rows_at_the_seams_of_numpys_sum(engine, lp, ld):
    prof, dm, names = edge_pair(lp, ld)
    got = engine.lyon8(prof, dm)
    compare(got, ref_of((lp, ld), prof, dm), names, f"seams ({lp}, {ld})")


@pytest.mark.parametrize("lp,ld", LONG_PAIRS)
def test_rows_longer_than_the_lds(engine, lp, ld):
    """33001 doubles: longer than anything the LDS can stage (160 KiB = 20 480 doubles), and
    lengths around the 8192 values numpy's reduction hands to its pairwise sum at a time."""
    (p, pn), (d, dn) = edge_rows(lp), edge_rows(ld)
    pick = [pn.index(k) for k in ("const_u0", "const_0.1", "step_1ulp", "offset_1e9", "wide",
                                  "scale_1e160", "nan", "plain0")]
    prof, dm = np.ascontiguousarray(p[pick]), np.ascontiguousarray(d[pick])
    names = ([pn[i] for i in pick], [dn[i] for i in pick])
    got = engine.lyon8(prof, dm)
    compare(got, ref_of(("long", lp, ld), prof, dm), names, f"long ({lp}, {ld})")


def batch_block(n, lp=129, ld=136):
    """n rows: the edge rows at the head and at the tail, plain noise between; the DM array
    holds the neighbour of the profile array's edge row.  A noise row on which scipy's own two
    evaluations of the kurtosis differ in the last bits (kurtosis_paths_agree: the reference
    is two numbers there, whichever the kernel gives) is drawn again; this looks at the
    reference alone."""
    (p, pn), (d, dn) = edge_rows(lp), edge_rows(ld)
    E = F64_EDGE_ROWS
    rng = np.random.default_rng(77 + n)
    prof = rng.normal(100.0, 10.0, (n, lp))
    dm = rng.normal(100.0, 10.0, (n, ld))
    for a in (prof, dm):
        while n and not (ok := kurtosis_paths_agree(a)).all():
            a[~ok] = rng.normal(100.0, 10.0, (int((~ok).sum()), a.shape[1]))
    pnames, dnames = ["noise"] * n, ["noise"] * n
    # head: rows 0.., tail: rows ..n-1 (for n < 2 * E the tail overwrites part of the head);
    # the head starts at a constant, an offset and a NaN row so that n = 1, 2, 5 meet them
    order = [pn.index(k) for k in ("const_u0", "offset_1e9", "nan", "const_0.1", "step_1ulp")]
    order += [i for i in range(E) if i not in order]
    for base in ((0, n - E) if n > E else (0,)):
        for j in range(min(E, n)):
            i, k = order[j], order[(j + 1) % E]
            prof[base + j], pnames[base + j] = p[i], pn[i]
            dm[base + j], dnames[base + j] = d[k], dn[k]
    return prof, dm, (pnames, dnames)


@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_small_batches(engine, n):
    prof, dm, names = batch_block(n)
    got = engine.lyon8(prof, dm)
    assert got.shape == (n, 8)
    if n:
        compare(got, reference(prof, dm), names, f"batch n={n}")


def test_one_block_walks_the_grid_stride_loop(engine):
    prof, dm, names = batch_block(1500)
    ref = ref_of(("b1500",), prof, dm)
    with engine.options(lyon8_blocks=1):
        one = engine.lyon8(prof, dm)
    compare(one, ref, names, "1500 rows, one block")
    got = engine.lyon8(prof, dm)
    assert np.array_equal(got.view(np.uint64), one.view(np.uint64)), "grid size changes the bits"


def test_strided_unaligned_device_rows_and_host_pointers(engine):
    """Rows that are views into a wider matrix (row stride > length, first element at an odd
    element offset: 8-byte but not 16-byte aligned) on the device, the same rows through the
    host-pointer call, and a dense copy: all 8 columns bit-identical, and on the bar."""
    import torch

    lp, ld = 129, 263
    prof, dm, names = edge_pair(lp, ld)
    n = len(prof)
    ref = ref_of((lp, ld), prof, dm)
    wp = torch.full((n, lp + 6), -7.0, dtype=torch.float64, device="cuda")
    wd = torch.full((n, ld + 11), 1e300, dtype=torch.float64, device="cuda")
    assert wp.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0
    vp, vd = wp[:, 3:3 + lp], wd[:, 5:5 + ld]
    vp.copy_(torch.from_numpy(prof))
    vd.copy_(torch.from_numpy(dm))
    assert vp.data_ptr() % 16 == 8 and vd.data_ptr() % 16 == 8 and vp.stride(0) > lp
    dev = engine.lyon8(vp, vd)
    dense = engine.lyon8(vp.contiguous(), vd.contiguous())
    engine.synchronize()
    dev, dense = dev.cpu().numpy(), dense.cpu().numpy()
    hp = np.full((n, lp + 6), -7.0)
    hd = np.full((n, ld + 11), 1e300)
    hp[:, 3:3 + lp] = prof
    hd[:, 5:5 + ld] = dm
    host_view = engine.lyon8(hp[:, 3:3 + lp], hd[:, 5:5 + ld])
    host = engine.lyon8(prof, dm)
    compare(dev, ref, names, "strided device rows")
    for other, what in ((dense, "dense device copy"), (host_view, "strided host rows"),
                        (host, "dense host rows")):
        assert np.array_equal(other.view(np.uint64), dev.view(np.uint64)), what


def test_the_two_float_paths_agree(engine):
    """pfe_pfd_dmprof scores the profile it folds with stats4_f64; the same profile fed to
    pfe_lyon8_f64 gives the same mean, std and kurtosis (==, NaN-aware) and the skew to 1e-13."""
    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    for shape, seed in (((4, 8, 256), 4100), ((2, 3, 300), 4200)):
        profs, subfreqs, scal = pfd.batch_inputs(pfd_fold_block(4, shape, seed))
        profs[2][:] = 100.0   # a flat fold: its profile is all NaN
        r = engine.pfd_dmprof(profs, subfreqs, scal)
        profile = np.ascontiguousarray(r["profile"], dtype=np.float64)
        assert profile.shape == (4, shape[2])
        assert np.isnan(profile[2]).all() and np.isfinite(profile[[0, 1, 3]]).all()
        got = engine.lyon8(profile, profile)
        compare(got[:, :4], r["lyon8"][:, :4], None, f"lyon8_f64 vs pfd_dmprof {shape}",
                exact_cols=(0, 1, 3), skew_cols=(2,))
        assert np.array_equal(got[:, :4].view(np.uint64), got[:, 4:].view(np.uint64))
