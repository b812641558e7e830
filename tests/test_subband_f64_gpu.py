"""GPU parity of pfe_subband3_f64 (scores 20-22 of candidates held as float arrays) against
oracle.bates.subband_scores called on the same float arrays, against the reference's own golden
sets cast to float64, and against the golden 22 scores of the PFD folds.

Bar: the failure pattern is the oracle's; s20 bit-exact; s21 and s22 within 1e-12 relative (the
bar tests/test_pfd22_gpu.py holds the same device function, pfd_subband_scores, to: numpy's dots
run in BLAS order).  On these inputs at 16 x 64, 5 x 37, 32 x 128 and 3 x 200 the oracle itself
sits within 4.7e-14 (s21) and 8.2e-16 (s22) of a long-double evaluation, so the reference alone
leaves about 20x headroom.

Strided input: the C-ABI takes dense rows only.  Engine.subband3_f64 makes host arrays dense
(the scores are those of the dense copy) and refuses a non-contiguous device tensor with
ValueError before any pointer reaches the library; both are pinned below.
"""
import warnings

import numpy as np
import pytest

from golden_util import bates_inputs, load
from oracle.bates import subband_scores
from pulsarfeatureextractor_amd.synth import bates_batch

pytestmark = pytest.mark.gpu

FAIL = 0x008


def float_batch(n, nsub, lsb, seed, lp=None):
    """synth.bates_batch made float: sub = bytes * U(0.3, 1.7) + N(0, 0.37),
    prof = bytes * 0.731 + N(0, 0.21)."""
    lp = lsb if lp is None else lp
    b = bates_batch(n, lp=lp, nsub=nsub, lsb=lsb, seed=seed)
    rng = np.random.default_rng(seed + 77)
    sub = b["sub"].astype(np.float64) * rng.uniform(0.3, 1.7, b["sub"].shape) + rng.normal(0, 0.37, b["sub"].shape)
    prof = b["prof"].astype(np.float64) * 0.731 + rng.normal(0, 0.21, b["prof"].shape)
    return {"prof": prof, "sub": sub, "scal": b["scal"].copy(), "dmcurve": b["dmcurve"]}


def adversarial(b):
    """The row edits of test_subband_gpu.adversarial (rows the reference fails or treats
    specially), restated for float sub-bands, and one row with a single NaN sample.  A batch of
    fewer than ten rows gets one failing row and the NaN row, so that plain rows remain."""
    sub, scal = b["sub"], b["scal"]
    n, nsub, lsb = sub.shape
    sub[0] = 0.0                      # every pair NaN: m = 0 -> ZeroDivisionError
    if n < 10:
        sub[1, nsub // 2, lsb // 3] = np.nan
        return b
    scal[1, 3] = 0.0                  # wb = 0: rms = stdev / 0
    scal[2, 3] = 2.0                  # wb > nBins: no window, max_bin unbound
    scal[3, 3] = np.nan               # int(ceil(nan)) raises
    sub[4, 1:] = 7.25                 # one varying band: no valid pair
    sub[5, nsub - 1] = 9.5            # a constant band among varying ones: its pairs skipped
    sub[6, :, :] = sub[6, :1, :]      # identical bands: cc = 1 (clipped)
    scal[7, 3] = 1.0 / lsb            # wb = 1
    scal[8, 3] = 1.0                  # wb = nBins: one window per band
    sub[9, nsub // 2, lsb // 3] = np.nan  # one NaN sample: its windows and its band's pairs drop out
    return b


def oracle_sub(prof, sub, scal):
    n = len(prof)
    out = np.zeros((n, 3))
    ok = np.zeros(n, dtype=bool)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for i in range(n):
            try:
                if prof.shape[1] != sub.shape[2]:
                    raise ValueError("corrcoef: all the input array dimensions must match")
                out[i] = subband_scores(sub[i], prof[i], float(scal[i, 3]))
                ok[i] = True
            except Exception:
                pass
    return out, ok


def rel(a, b):
    with np.errstate(all="ignore"):
        r = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    r[(a == b) | (np.isnan(a) & np.isnan(b))] = 0.0
    r[np.isnan(r)] = np.inf
    return r


def check(out, st, ref, ok, tag, pattern=True):
    st = np.asarray(st).view(np.uint32)
    gok = (st & 0xFF) == 0
    if pattern:
        assert np.array_equal(gok, ok), f"{tag}: failure pattern differs at {np.where(gok != ok)[0][:10]}"
        assert (st[~ok] == FAIL).all() and (out[~ok] == 0).all(), f"{tag}: failed rows"
    else:  # a golden set: the reference drops a row for any group, so only ok rows must score
        assert gok[ok].all(), f"{tag}: rows the reference scored fail at {np.where(~gok & ok)[0][:10]}"
    r = rel(out[ok], ref[ok])
    print(f"{tag}: rows {int(ok.sum())}/{len(ok)} max rel s20 {r[:, 0].max(initial=0):.3g} "
          f"s21 {r[:, 1].max(initial=0):.3g} s22 {r[:, 2].max(initial=0):.3g}")
    assert (r[:, 0] == 0).all(), f"{tag}: s20 not bit-exact ({(r[:, 0] > 0).sum()} rows)"
    assert (r[:, 1] <= 1e-12).all(), f"{tag}: s21 max rel {r[:, 1].max():.3g}"
    assert (r[:, 2] <= 1e-12).all(), f"{tag}: s22 max rel {r[:, 2].max():.3g}"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# 2 x 8 / 16 x 128: the edges of the 8-rows path; 5 x 37, 13 x 64: nsub no multiple of 8;
# 3 x 7, 6 x 129: the wave path on both sides of it; 80 x 256: beyond the LDS (global path)
@pytest.mark.parametrize("nsub,lsb,n", [(2, 8, 24), (5, 37, 24), (13, 64, 20), (16, 128, 16),
                                        (3, 7, 24), (6, 129, 16), (24, 200, 12), (3, 1024, 4),
                                        (80, 256, 4)])
def test_subband3_f64_vs_oracle(engine, nsub, lsb, n):
    b = adversarial(float_batch(n, nsub, lsb, seed=2100 + nsub + lsb))
    if lsb == 1024:
        b["scal"][:, 3] = np.minimum(b["scal"][:, 3], 0.03)  # keeps the oracle's Python boxcar loop short
    out, st = engine.subband3_f64(b["prof"], b["sub"], b["scal"])
    ref, ok = oracle_sub(b["prof"], b["sub"], b["scal"])
    assert ok.any()
    check(out, st, ref, ok, f"{nsub}x{lsb}")


def width_for(w, lsb):
    """A width with ceil(width * lsb) == w exactly, as the kernel and the oracle evaluate it."""
    wd = w / lsb
    if int(np.ceil(wd * lsb)) != w:
        wd = np.nextafter(wd, 0.0)
    assert int(np.ceil(wd * lsb)) == w
    return wd


@pytest.mark.parametrize("nsub,lsb", [(16, 128), (13, 64), (5, 37), (2, 8), (6, 129)])
def test_boxcar_widths_and_ties(engine, nsub, lsb):
    """wb = 1, 2, 7, 8, 9, lsb - 7, lsb - 1, lsb: both sides of the packed-stride condition
    nw >= 8 && (nw | 1) <= L and the one-window case; once on random bands and once on bands
    whose largest windows repeat exactly (ties): the first half of each band a period-4 pattern
    of values whose sums are exact in any order, above the band's random second half, so the
    maximum is reached by several equal windows and the first of them must win.  The random
    halves keep the pair correlations away from the +-1 values of purely periodic bands, whose
    mean cancels to an exact zero that no relative bar can hold."""
    wbs = sorted({w for w in (1, 2, 7, 8, 9, lsb - 7, lsb - 1, lsb) if 1 <= w <= lsb})
    n = 2 * len(wbs)
    b = float_batch(n, nsub, lsb, seed=2390 + nsub + lsb)
    rng = np.random.default_rng(2400 + lsb)
    half = lsb // 2
    for i in range(n):
        b["scal"][i, 3] = width_for(wbs[i % len(wbs)], lsb)
        if i >= len(wbs):
            b["sub"][i, :, :half] = 8.0
            b["sub"][i, :, :half:4] = 64.0
            b["sub"][i, :, half:] = rng.uniform(0.0, 4.0, size=(nsub, lsb - half))
    out, st = engine.subband3_f64(b["prof"], b["sub"], b["scal"])
    ref, ok = oracle_sub(b["prof"], b["sub"], b["scal"])
    # the inputs, judged by the reference alone: s21 is a mean of correlations in [-1, 1], each
    # good to a few ulp, so a mean below 1e-3 has cancelled away the digits a relative bar
    # measures -- with two windows (wb = lsb - 1) every correlation is +-1 and the mean of 16
    # bands is an exact 0 for one seed in four.  The seed above keeps every row clear of that.
    assert (np.abs(ref[ok][:, 1]) >= 1e-3).all()
    check(out, st, ref, ok, f"widths {nsub}x{lsb}")


@pytest.mark.parametrize("nsub,lsb", [(16, 128), (5, 37)])
def test_global_option_gives_the_same_bits(engine, nsub, lsb):
    b = adversarial(float_batch(20, nsub, lsb, seed=2500 + lsb))
    out, st = engine.subband3_f64(b["prof"], b["sub"], b["scal"])
    with engine.options(subf64_global=1):
        assert engine.get_option("subf64_global") == 1
        og, sg = engine.subband3_f64(b["prof"], b["sub"], b["scal"])
    assert engine.get_option("subf64_global") == 0
    assert ((st & 0xFF) == 0).any()
    assert np.array_equal(sg, st) and np.array_equal(bits(og), bits(out))


def test_device_pointers_input_untouched_and_strides(engine):
    import torch

    b = adversarial(float_batch(24, 16, 128, seed=2600))
    out, st = engine.subband3_f64(b["prof"], b["sub"], b["scal"])
    t = {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ("prof", "sub", "scal")}
    keep = t["sub"].clone()
    for glob in (0, 1):
        with engine.options(subf64_global=glob):
            od, sd = engine.subband3_f64(t["prof"], t["sub"], t["scal"])
            engine.synchronize()
        assert np.array_equal(sd.cpu().numpy().view(np.uint32), st)
        assert np.array_equal(bits(od.cpu().numpy()), bits(out))
        assert torch.equal(t["sub"].view(torch.int64), keep.view(torch.int64)), "sub was written"
    # host arrays of any strides are made dense: the same bits as the dense call
    wide = np.zeros((24, 16, 256))
    wide[:, :, ::2] = b["sub"]
    oh, sh = engine.subband3_f64(b["prof"][:, ::1], wide[:, :, ::2], b["scal"])
    assert np.array_equal(sh, st) and np.array_equal(bits(oh), bits(out))
    # a non-contiguous device tensor is refused before it reaches the library
    tw = torch.from_numpy(wide).cuda()
    with pytest.raises(ValueError):
        engine.subband3_f64(t["prof"], tw[:, :, ::2], t["scal"])


def test_shape_beyond_the_lds_is_refused(engine):
    from pulsarfeatureextractor_amd._native import PfeError

    b = float_batch(1, 16, 2, seed=5)
    sub = np.zeros((1, 7000, 2))
    with pytest.raises(PfeError, match="7000x2"):
        engine.subband3_f64(b["prof"], sub, b["scal"])
    # the largest shape the header promises is taken (one candidate, through global scratch)
    sub = np.random.default_rng(1).normal(10, 3, (1, 1024, 2048))
    prof = sub[0].sum(0)[None, :]
    scal = np.zeros((1, 8))
    scal[0, 3] = 0.999                # wb = 2046: three windows per band
    out, st = engine.subband3_f64(prof, sub, scal)
    assert st[0] == 0 and np.isfinite(out).all()
    cc = np.array([abs(np.corrcoef(sub[0, j], prof[0])[0, 1]) for j in range(1024)])
    s22 = 0.0
    for c in cc[cc > 0.0055]:
        s22 += c
    assert abs(out[0, 2] - s22) <= 1e-12 * s22


@pytest.mark.parametrize("name", ["bates22_phcx128", "bates22_superb64", "bates22_phcx128_nsub32",
                                  "bates22_cfg4_256x128"])
def test_reference_golden_sets_as_floats(engine, name):
    """The reference's own candidates with prof, sub and the width cast to float64: columns
    19-21 of its scores on the rows it scored.  The last set has lp != lsb: every row fails."""
    d = load(name)
    prof, sub, _curve, scal = bates_inputs(d)
    out, st = engine.subband3_f64(prof.astype(np.float64), sub.astype(np.float64),
                                  scal.astype(np.float64))
    ok = d["ok"].astype(bool)
    if prof.shape[1] != sub.shape[2]:
        assert not ok.any() and (st == FAIL).all()
        return
    assert ok.any()
    check(out, st, d["out"][:, 19:22], ok, name, pattern=False)


@pytest.mark.parametrize("name", ["pfd_64x16", "pfd_128x32"])
def test_pfd_folds_dedispersed_subbands(engine, tmp_path, name):
    """The dedispersed sub-bands, the profile and the width of each golden fold, as the oracle
    makes them, against columns 19-21 of the reference's 22 scores."""
    from oracle import pfd as opfd
    from pulsarfeatureextractor_amd import pfd
    from test_oracle_pfd import build_files, load_set

    g = load_set(name)
    files = build_files(tmp_path, g)
    profs, subs, widths = [], [], []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for f in files:
            d = pfd.read(f)
            s = opfd.PFDState(d)
            profile = s.profile()
            profs.append(profile)
            subs.append(s.profs.sum(0))
            widths.append(opfd.pfd_parameters(d, profile)[3])
    scal = np.zeros((len(files), 8))
    scal[:, 3] = widths
    out, st = engine.subband3_f64(np.array(profs), np.array(subs), scal)
    ok = g["bates22_ok"].astype(bool)
    assert ok.any()
    check(out, st, g["bates22"][:, 19:22], ok, name, pattern=False)
