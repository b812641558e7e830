"""The host side of scrunching a fold: pfd.scrunch_plan (which way and how far each channel is
rotated, and where a group's centre lies), pfd.scrunch_scal, the route rule, and the C structure
as ctypes lays it out.  No GPU: the dispersed-pulse test scrunches with a numpy restatement of
the contract of its own (that of tests/test_pfd_scrunch_gpu.py, stated again so that this file
imports no GPU test)."""
import ctypes as C

import numpy as np
import pytest

from pulsarfeatureextractor_amd import _native, pfd
from pulsarfeatureextractor_amd._native import PfdScrunchHow


def restate(x64, rot, fscr, bscr):
    """The contract of include/pfe.h, step by step: (n, npart, nchan, nbin) -> (n, 1, G, K)."""
    n, npart, nchan, nbin = x64.shape
    G, K = nchan // fscr, nbin // bscr
    z = np.empty((n, 1, G, K))
    for i in range(n):
        S = x64[i, 0].copy()
        for p in range(1, npart):
            S = S + x64[i, p]
        R = np.stack([np.roll(S[c], -(0 if rot is None else int(rot[i, c]) % nbin)) for c in range(nchan)])
        R = R.reshape(nchan, K, bscr)
        B = R[:, :, 0].copy()
        for j in range(1, bscr):
            B = B + R[:, :, j]
        B = B.reshape(G, fscr, K)
        Z = B[:, 0].copy()
        for c in range(1, fscr):
            Z = Z + B[:, c]
        z[i, 0] = Z
    return z


def test_struct_and_symbols():
    assert C.sizeof(PfdScrunchHow) == 16
    assert (PfdScrunchHow.rot.offset, PfdScrunchHow.fscr.offset, PfdScrunchHow.bscr.offset) == (0, 8, 12)
    for name in ("pfe_pfd_scrunch", "pfe_pfd_scrunch_f32", "pfe_pfd_scrunch_i16"):
        assert name in _native.EXPORTED_SYMBOLS
    lib = _native.load_library()
    assert len(lib.pfe_pfd_scrunch.argtypes) == len(lib.pfe_pfd_scrunch_f32.argtypes) == 9
    assert len(lib.pfe_pfd_scrunch_i16.argtypes) == 5
    assert _native.OPTIONS["pfd_scrunch_direct"] == 14


def delay(dm, f):
    return dm / (0.000241 * f * f)


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_scrunch_plan(descending):
    f = 1200.0 + 0.5 * np.arange(32)
    if descending:
        f = f[::-1].copy()
    dm, bps, nbin, fscr = 150.0, 20000.0, 256, 8
    rot, sub = pfd.scrunch_plan(f, dm, bps, nbin, fscr)
    assert rot.dtype == np.int32 and rot.shape == (32,) and sub.shape == (4,)
    g = f.reshape(4, 8)
    assert np.array_equal(sub, 0.5 * (g[:, 0] + g[:, -1]))          # the group centre
    want = np.array([int(np.floor((delay(dm, fc) - delay(dm, sub[c // 8])) * bps + 0.5))
                     for c, fc in enumerate(f)])
    assert np.array_equal(rot, want)
    r = rot.reshape(4, 8)
    lo, hi = (0, -1) if not descending else (-1, 0)
    # a lower frequency arrives later: a larger left rotation; channels above the centre go right
    assert (r[:, lo] > 0).all() and (r[:, hi] < 0).all()
    order = np.argsort(g, axis=1)
    assert (np.diff(np.take_along_axis(r, order, axis=1), axis=1) <= 0).all()
    assert (rot < 0).any() and np.abs(rot).max() < nbin
    # batched: one plan per fold, the leading dimensions kept
    rot2, sub2 = pfd.scrunch_plan(np.stack([f, f + 100.0]), np.array([dm, 2 * dm]), np.array([bps, bps]), nbin, fscr)
    assert rot2.shape == (2, 32) and sub2.shape == (2, 4) and np.array_equal(rot2[0], rot)
    assert not np.array_equal(rot2[1], rot)
    # no frequency scrunch: every channel is its own centre
    rot1, sub1 = pfd.scrunch_plan(f, dm, bps, nbin, 1)
    assert not rot1.any() and np.array_equal(sub1, f)
    with pytest.raises(ValueError, match="does not divide"):
        pfd.scrunch_plan(f, dm, bps, nbin, 5)
    # a rotation beyond int32 is reduced mod nbin on the host
    big, _ = pfd.scrunch_plan(np.array([10.0, 1000.0]), 1000.0, 1e9, 64, 2)
    assert big.dtype == np.int32 and (0 <= big).all() and (big < 64).all()


def test_a_dispersed_pulse_lines_up():
    """64 channels x 64 bins, a pulse one bin wide at DM 100, to 8 sub-bands: with the plan's
    rotations every sub-band's peak is strictly higher than without."""
    nchan, nbin, fscr, dm = 64, 64, 8, 100.0
    f = 1200.0 + np.arange(nchan)
    bps = nbin / 0.05
    x = np.zeros((1, 2, nchan, nbin))
    at = np.floor(delay(dm, f) * bps + 0.5).astype(np.int64) % nbin
    x[0, :, np.arange(nchan), at] = 1.0
    rot, sub = pfd.scrunch_plan(f, dm, bps, nbin, fscr)
    assert np.ptp(at.reshape(8, 8), axis=1).min() >= 2       # the pulse drifts inside every group
    aligned = restate(x, rot[None], fscr, 1)[0, 0]
    plain = restate(x, None, fscr, 1)[0, 0]
    assert aligned.shape == plain.shape == (8, 64)
    assert aligned.sum() == plain.sum() == 2.0 * nchan
    assert (aligned.max(axis=1) > plain.max(axis=1)).all()
    # aligned on each group's centre, not on one frequency: the sub-bands still drift
    assert len(set(aligned.argmax(axis=1))) > 1


def test_scrunch_scal():
    sc = np.array([[50.0, 12800.0, 3.5, 7.25, 0.0, 100.0, 100.0, 0.005],
                   [10.0, 6400.0, 1.0, 2.0, 5.0, 15.0, 50.0, 0.1]])
    keep = sc.copy()
    out = pfd.scrunch_scal(sc, 4)
    assert np.array_equal(sc, keep) and out is not sc
    assert np.array_equal(out[:, 1], keep[:, 1] / 4) and np.array_equal(out[:, 3], keep[:, 3] * 4)
    assert np.isnan(out[:, 2]).all()
    assert np.array_equal(out[:, [0, 4, 5, 6, 7]], keep[:, [0, 4, 5, 6, 7]])
    assert np.array_equal(pfd.scrunch_scal(sc[0], 1)[[0, 1, 3]], keep[0, [0, 1, 3]])
    with pytest.raises(ValueError):
        pfd.scrunch_scal(sc, 0)


def test_route_rule():
    assert pfd.scrunch_route(1024, 8) == pfd.scrunch_route(4100, 4) == pfd.scrunch_route(4096, 1) == "lds"
    assert pfd.scrunch_route(20000, 8) == pfd.scrunch_route(4097, 1) == "direct"
