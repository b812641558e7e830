"""A fold's average on the device: pfe_pfd_avgprof / _f32 against numpy's (x / L).sum(), bit for
bit, and PFE_FLAG_PFD_AVGPROF (derive_avgprof=True) on the PFD calls against the unflagged call
given numpy's value.

The reference is numpy on the host (for a float32 cube: on x.astype(float64)), never the call
under test.  Shapes are the sizes at which the kernel takes another path: a chunk of fewer than
8 values, one leaf (<= 128), a leaf with a remainder, the first splits (129, 136), the largest
four-level tree and one past it (968, 969), one short of, exactly and one past numpy's buffer of
8192 (8191, 8192, 8193), a second chunk that is a leaf (8200), three chunks (16393); proflen both
a power of two (scaled by the exact reciprocal) and not (the IEEE divide).
"""
import ctypes as C
import warnings

import numpy as np
import pytest

from oracle import pfd as opfd
from pulsarfeatureextractor_amd import pfd
from pulsarfeatureextractor_amd._native import (PFE_FLAG_DEVICE_PTRS, PFE_FLAG_PFD_AVGPROF,
                                                PFE_PFD_AVGPROF, PFE_PFD_NSCAL)
from pulsarfeatureextractor_amd.synth import pfd_fold_block
from test_oracle_pfd import SETS, build_files, load_set

pytestmark = pytest.mark.gpu

# E -> (npart, nsub, proflen)
E_SHAPES = {2: (1, 1, 2), 7: (1, 1, 7), 8: (1, 2, 4), 15: (1, 3, 5), 127: (1, 1, 127),
            128: (1, 4, 32), 129: (1, 3, 43), 136: (1, 17, 8), 968: (2, 4, 121), 969: (1, 1, 969),
            8191: (1, 1, 8191), 8192: (2, 32, 128), 8193: (1, 2731, 3), 8200: (2, 41, 100),
            16393: (13, 13, 97)}

_cubes = {}


def cube(shape, n=3):
    """(x64, x32, numpy's averages of each) of n folds of `shape`, built once."""
    key = (shape, n)
    if key not in _cubes:
        rng = np.random.default_rng(int(np.prod(shape)) + n)
        x64 = rng.normal(1000.0, 300.0, size=(n,) + shape)
        x32 = x64.astype(np.float32)
        for a in (x64, x32):
            a.setflags(write=False)
        _cubes[key] = (x64, x32, np_avg(x64), np_avg(x32))
    return _cubes[key]


def np_avg(x):
    """The reference: numpy's expression, fold by fold, on the values as doubles."""
    L = x.shape[-1]
    return np.array([(f.astype(np.float64) / L).sum() for f in x])


def same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), tag
        return
    # the same bits, but for which NaN it is
    assert np.array_equal(got, want, equal_nan=True), tag
    assert np.array_equal(np.signbit(got) | np.isnan(got), np.signbit(want) | np.isnan(want)), tag


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("E", sorted(E_SHAPES))
def test_against_numpy(engine, E):
    shape = E_SHAPES[E]
    assert int(np.prod(shape)) == E
    x64, x32, a64, a32 = cube(shape)
    same(engine.pfd_avgprof(x64), a64, f"E={E} f64 host")
    same(engine.pfd_avgprof(x32), a32, f"E={E} f32 host")
    d64, d32 = engine.pfd_avgprof(_dev(x64)), engine.pfd_avgprof(_dev(x32))
    engine.synchronize()
    same(d64.cpu().numpy(), a64, f"E={E} f64 device")
    same(d32.cpu().numpy(), a32, f"E={E} f32 device")


def test_many_tiny_folds(engine):
    x64, x32, a64, a32 = cube((1, 2, 5), 70)   # more folds than lanes of a wave
    same(engine.pfd_avgprof(x64), a64, "f64")
    same(engine.pfd_avgprof(x32), a32, "f32")
    x64, x32, a64, a32 = cube((2, 3, 11), 70)  # one leaf with a remainder each
    same(engine.pfd_avgprof(_dev(x64)).cpu().numpy(), a64, "f64 device")
    same(engine.pfd_avgprof(_dev(x32)).cpu().numpy(), a32, "f32 device")


def _raw(engine, x, shape, n, out, stride, flags, f32=False):
    """The C call -> (return code, pfe_last_error text); x, out: addresses."""
    fn = engine.lib.pfe_pfd_avgprof_f32 if f32 else engine.lib.pfe_pfd_avgprof
    rc = fn(engine._h, x, shape[0], shape[1], shape[2], n, out, stride, flags)
    return rc, engine.lib.pfe_last_error(engine._h).decode()


@pytest.mark.parametrize("f32", (False, True), ids=("f64", "f32"))
def test_out_stride_into_scal(engine, f32):
    """out = &scal[PFE_PFD_AVGPROF], stride PFE_PFD_NSCAL: the other columns stay untouched."""
    shape, n = (3, 4, 100), 3
    x64, x32, a64, a32 = cube(shape, n)
    x, want = (x32, a32) if f32 else (x64, a64)
    assert PFE_PFD_NSCAL == 8 and PFE_PFD_AVGPROF == 2
    scal = np.arange(n * 8, dtype=np.float64).reshape(n, 8) + 0.5
    exp = scal.copy()
    exp[:, 2] = want
    h = scal.copy()
    rc, msg = _raw(engine, x.ctypes.data, shape, n, h.ctypes.data + 16, 8, 0, f32)
    assert rc == 0, msg
    same(h, exp, "host, stride 8")
    dx, d = _dev(x), _dev(scal)
    rc, msg = _raw(engine, dx.data_ptr(), shape, n, d.data_ptr() + 16, 8, PFE_FLAG_DEVICE_PTRS, f32)
    assert rc == 0, msg
    engine.synchronize()
    same(d.cpu().numpy(), exp, "device, stride 8")
    d1 = _dev(np.zeros(n))
    rc, msg = _raw(engine, dx.data_ptr(), shape, n, d1.data_ptr(), 1, PFE_FLAG_DEVICE_PTRS, f32)
    assert rc == 0, msg
    engine.synchronize()
    same(d1.cpu().numpy(), want, "device, stride 1")


def test_float_cube_4_bytes_off_a_16_byte_boundary(engine):
    import torch

    for shape in ((2, 32, 128), (3, 4, 100)):
        _x64, x32, _a64, a32 = cube(shape)
        big = torch.zeros(x32.size + 4, dtype=torch.float32, device="cuda")
        assert big.data_ptr() % 16 == 0
        c = big[1:1 + x32.size].view(x32.shape)
        c.copy_(_dev(x32))
        assert c.data_ptr() % 16 == 4 and c.is_contiguous()
        got = engine.pfd_avgprof(c)
        engine.synchronize()
        same(got.cpu().numpy(), a32, str(shape))


def test_special_folds(engine):
    with np.errstate(all="ignore"):
        shape = (2, 5, 100)
        x = np.array(cube(shape, 4)[0])
        x[0, 1, 2, 3] = np.inf
        x[1, 0, 4, 99] = np.nan
        x[2] = 1.7e308                        # the sum overflows
        x[3] *= -1.0
        for f32 in (False, True):
            a = x.astype(np.float32) if f32 else x
            want = np_avg(a)
            assert np.isinf(want[0]) and np.isnan(want[1]) and (f32 or np.isinf(want[2]))
            same(engine.pfd_avgprof(a), want, f"inf / NaN / overflow f32={f32}")
        for shape in ((1, 2, 3), (1, 2, 8), (3, 43, 128)):    # E = 6, 16 and two chunks
            z = np.full((2,) + shape, -0.0)
            want = np_avg(z)
            same(engine.pfd_avgprof(z), want, f"-0.0 {shape}")
            same(engine.pfd_avgprof(z.astype(np.float32)), want, f"-0.0 {shape} f32")
        k = np.arange(1, 2 * 4 * 3 * 47 + 1, dtype=np.float64).reshape(2, 4, 47, 3)
        sub = 5e-324 * k                      # quotients by 3 are subnormal: rounded, not exact
        assert (sub / 3 < 2.3e-308).all()
        same(engine.pfd_avgprof(sub), np_avg(sub), "subnormal quotients")
        sub = (5e-324 * k).reshape(2, 1, 141, 4)   # and scaled by the power of two's reciprocal
        same(engine.pfd_avgprof(sub), np_avg(sub), "subnormal quotients, proflen 4")


# ---- the flag -----------------------------------------------------------------------------
FLAG_SHAPES = [(2, 3, 8), (3, 4, 100), (4, 8, 128)]
_folds = {}


def folds(shape, n):
    """(x64, x32, subfreqs, scal with numpy's average, the same with NaN there) for the f64 and
    the f32 cube of n synthetic folds."""
    key = (shape, n)
    if key not in _folds:
        x64, fr, sc = pfd.batch_inputs(pfd_fold_block(n, shape, 20261022))
        x32 = x64.astype(np.float32)
        out = {}
        for tag, x in (("f64", x64), ("f32", x32)):
            good = sc.copy()
            good[:, PFE_PFD_AVGPROF] = np_avg(x)
            bad = good.copy()
            bad[:, PFE_PFD_AVGPROF] = np.nan
            for a in (x, good, bad):
                a.setflags(write=False)
            out[tag] = (x, fr, good, bad)
        assert np.array_equal(out["f64"][2][:, 2], sc[:, 2])   # what the packer computed
        _folds[key] = out
    return _folds[key]


def same_dmprof(got, want, tag):
    for k in ("profile", "chis", "lyon8", "status"):
        same(got[k], want[k], f"{tag}: {k}")


def same_scores(got, want, tag):
    same(got[0], want[0], f"{tag}: out")
    same(got[1], want[1], f"{tag}: status")


def _host(r):
    if isinstance(r, dict):
        r = {k: v.cpu().numpy() for k, v in r.items()}
        r["status"] = r["status"].view(np.uint32)
        return r
    return r[0].cpu().numpy(), r[1].cpu().numpy().view(np.uint32)


def both_ways(engine, call, x, fr, good, bad, cmp, tag):
    """The flagged call on a poisoned scal == the unflagged call on numpy's value; host
    pointers, then device pointers, whose scal keeps its NaN."""
    want = call(x, fr, good)
    cmp(call(x, fr, bad, derive_avgprof=True), want, f"{tag} host")
    dbad = _dev(bad)
    got = call(_dev(x), _dev(fr), dbad, derive_avgprof=True)
    engine.synchronize()
    cmp(_host(got), want, f"{tag} device")
    same(dbad.cpu().numpy(), bad, f"{tag}: the caller's scal")
    return want


ROUTES = [("on_chip", {}), ("global", {"pfd_global": 1}), ("split", {"pfd_split": 1}),
          ("one_wave", {"pfd_waves": 1})]


@pytest.mark.parametrize("shape", FLAG_SHAPES, ids=["2x3x8", "3x4x100", "4x8x128"])
@pytest.mark.parametrize("route,opts", ROUTES, ids=[r[0] for r in ROUTES])
def test_flag_dmprof_routes(engine, route, opts, shape):
    x, fr, good, bad = folds(shape, 5)["f64"]
    with engine.options(**opts):
        want = both_ways(engine, engine.pfd_dmprof, x, fr, good, bad, same_dmprof, route)
    assert not np.isnan(want["chis"]).all()
    # the poison is read without the flag: the test would see a flag that does nothing
    poisoned = engine.pfd_dmprof(x, fr, bad)
    assert np.isnan(poisoned["chis"]).any()


@pytest.mark.parametrize("shape", FLAG_SHAPES, ids=["2x3x8", "3x4x100", "4x8x128"])
def test_flag_dmprof_f32_pass_seams(engine, shape):
    x, fr, good, bad = folds(shape, 7)["f32"]
    with engine.options(pfd_f32_chunk=3):       # passes of 3, 3 and 1 folds
        both_ways(engine, engine.pfd_dmprof, x, fr, good, bad, same_dmprof, "chunk 3")
        for o in ({"pfd_global": 1}, {"pfd_split": 1}):
            with engine.options(**o):
                both_ways(engine, engine.pfd_dmprof, x, fr, good, bad, same_dmprof, f"chunk 3 {o}")
    both_ways(engine, engine.pfd_dmprof, x, fr, good, bad, same_dmprof, "one pass")


@pytest.mark.parametrize("shape", FLAG_SHAPES, ids=["2x3x8", "3x4x100", "4x8x128"])
@pytest.mark.parametrize("kind", ("f64", "f32"))
def test_flag_score_calls(engine, kind, shape):
    x, fr, good, bad = folds(shape, 7)[kind]
    for call in (engine.pfd_bates22, engine.pfd_dmfit4):
        both_ways(engine, call, x, fr, good, bad, same_scores, call.__name__)
        if kind == "f32":
            with engine.options(pfd_f32_chunk=3):
                both_ways(engine, call, x, fr, good, bad, same_scores, call.__name__ + " chunk 3")
    # the calls that do not read the average: the flag changes nothing, poisoned or not
    for call in (engine.pfd_params4, engine.pfd_subband3):
        want = both_ways(engine, call, x, fr, good, bad, same_scores, call.__name__)
        same_scores(call(x, fr, bad), want, call.__name__ + " unflagged, poisoned")
        same_scores(call(x, fr, good, derive_avgprof=True), want, call.__name__ + " flagged")


def eq_nan(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name", SETS)
def test_reference_goldens_with_the_flag(engine, tmp_path, name):
    """tests/test_pfd_gpu.py's bars on the reference-made folds, the average derived on the
    device from a poisoned scal: profile, DM curve, mean, std and kurtosis bit-exact, the skews
    within 1e-13 (float64) and 1e-6 (float32) relative."""
    g = load_set(name)
    files = build_files(tmp_path, g)
    datas = [pfd.read(f, avgprof=False) for f in files]
    profs, subfreqs, scal = pfd.batch_inputs(datas)
    assert np.isnan(scal[:, PFE_PFD_AVGPROF]).all()
    r = engine.pfd_dmprof(profs, subfreqs, scal, derive_avgprof=True)
    assert eq_nan(r["profile"], g["profile"]).all(), "profile not bit-exact"
    ok = g["lyon8_ok"]
    assert np.array_equal((r["status"] & 0x20) == 0, ok)
    got, ref = r["lyon8"][ok], g["lyon8"][ok]
    for j in (0, 1, 3, 4, 5, 7):
        assert eq_nan(got[:, j], ref[:, j]).all(), f"feature {j} not bit-exact"
    for j, tol in ((2, 1e-13), (6, 1e-6)):
        with np.errstate(invalid="ignore"):
            rel = np.abs(got[:, j] - ref[:, j]) / np.abs(ref[:, j])
        rel[eq_nan(got[:, j], ref[:, j])] = 0.0
        assert (rel <= tol).all(), f"feature {j}: max rel {np.nanmax(rel):.3g}"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, f in enumerate(files):
            if ok[i]:
                chis = opfd.dm_curve(pfd.read(f))
                assert np.array_equal(r["chis"][i], chis) or eq_nan(r["chis"][i], chis).all(), i


def test_refusals(engine):
    x = _dev(np.ones((2, 2, 3, 8)))
    out = _dev(np.zeros(2))
    D = PFE_FLAG_DEVICE_PTRS
    shape = (2, 3, 8)
    for f32 in (False, True):
        for args, text in (((None, shape, 2, out.data_ptr(), 1, D), "pfd_avgprof: null argument"),
                           ((x.data_ptr(), shape, 2, None, 1, D), "pfd_avgprof: null argument"),
                           ((x.data_ptr(), shape, -1, out.data_ptr(), 1, D), "pfd_avgprof: n < 0"),
                           ((x.data_ptr(), (0, 3, 8), 2, out.data_ptr(), 1, D), "pfd_avgprof: shape 0x3x8"),
                           ((x.data_ptr(), (2, -1, 8), 2, out.data_ptr(), 1, D), "pfd_avgprof: shape 2x-1x8"),
                           ((x.data_ptr(), (2, 3, 1), 2, out.data_ptr(), 1, D), "pfd_avgprof: shape 2x3x1"),
                           ((x.data_ptr(), shape, 2, out.data_ptr(), 0, D), "pfd_avgprof: out_stride < 1"),
                           ((x.data_ptr(), shape, 2, out.data_ptr(), -8, 0), "pfd_avgprof: out_stride < 1")):
            rc, msg = _raw(engine, *args, f32)
            assert rc == 1 and msg == text, (args, rc, msg)
    rc, msg = _raw(engine, x.data_ptr() + 2, shape, 2, out.data_ptr(), 1, D, True)
    assert rc == 1 and msg == "pfd_avgprof: profs not 4-byte aligned"
    rc, msg = _raw(engine, x.data_ptr(), shape, 0, out.data_ptr(), 1, D)   # nothing to do
    assert rc == 0 and msg == ""
    engine.synchronize()
    assert not out.cpu().numpy().any()
    with pytest.raises(ValueError):
        engine.pfd_avgprof(np.ones((2, 3, 8)))
    with pytest.raises(TypeError):
        import torch

        engine.pfd_avgprof(x.to(torch.int32))
    assert C.sizeof(C.c_double) == 8 and PFE_FLAG_PFD_AVGPROF == 2
