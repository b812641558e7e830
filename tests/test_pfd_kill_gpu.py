"""Kill masks on the PFD calls (pfe_pfd_*_kill and their _f32 forms, reached through
Engine.pfd_* with kill_parts / kill_subs) against the contract include/pfe.h states: every
output and the status are, bit for bit, those of the plain call of the same name on the cube
z = np.where(kill, 0.0, x), with the same subfreqs, scal, options and other flags.

The reference is always the existing plain call on z -- never the call under test.  Folds are
synth.pfd_candidate's (pfd_fold_block's cube, with its foldstats); scal carries the zapped
fold's varprof (pfd.varprof) and average ((z / L).sum()).  Masks differ per fold: fold 0 kills
nothing, fold i kills parts {i % npart, npart - 1} and sub-band (i + 1) % nsub, the last fold
keeps a single part.  The bar is np.array_equal with equal_nan on every output.  Shapes are the
smallest that take each route of the f64 kernels and both load paths of k_pfd_partsum_kill."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from oracle import pfd as opfd
from pulsarfeatureextractor_amd import pfd
from pulsarfeatureextractor_amd._native import (PFE_FLAG_DEVICE_PTRS, PfdF32In, PfdIn, PfdKill,
                                                PfeError)
from pulsarfeatureextractor_amd.synth import pfd_candidate
from test_pfd22_gpu import check as check22
from test_pfd22_gpu import oracle_floor
from test_pfd_f32_gpu import ROUTES, _dev, _host, same, same_dmprof, same_scores

pytestmark = pytest.mark.gpu

SEED = 20261021
_blocks = {}


def candidates(shape, n):
    return [pfd_candidate(np.random.default_rng(SEED + i), *shape) for i in range(n)]


def masks(shape, n):
    """fold 0 kills nothing; fold i parts {i % npart, npart-1} and sub (i+1) % nsub; the last
    fold (n > 2) keeps part 0 alone."""
    npart, nsub, _ = shape
    kp = np.zeros((n, npart), dtype=bool)
    ks = np.zeros((n, nsub), dtype=bool)
    for i in range(1, n):
        kp[i, [i % npart, npart - 1]] = True
        ks[i, (i + 1) % nsub] = True
    if n > 2:
        kp[n - 1] = True
        kp[n - 1, 0] = False
    return kp, ks


def zap(x, kp, ks):
    """np.where(kill, 0.0, x) of a (n, npart, nsub, L) cube: the contract's z."""
    kill = kp[:, :, None, None] | ks[:, None, :, None]
    return np.where(kill, x.dtype.type(0.0), x)


def fold_inputs(cands, kp, ks, f32=False):
    """(x, z, subfreqs, scal) of the folds: z the zapped cube (float64: what the plain call
    takes; a float32 cube is rounded first, then widened), scal the zapped fold's."""
    n = len(cands)
    npart, nsub, L = cands[0]["profs"].shape
    x = np.stack([c["profs"] for c in cands])
    if f32:
        x = x.astype(np.float32)
    z = zap(x, kp, ks).astype(np.float64)
    fr = np.empty((n, nsub))
    sc = np.zeros((n, 8))
    var = pfd.varprof(np.stack([c["stats"][:, :, 5] for c in cands]), kp, ks)
    for i, c in enumerate(cands):
        sd = c["chan_wid"] * (c["numchan"] // nsub)
        fr[i] = np.arange(nsub, dtype="d") * sd + (c["lofreq"] + sd - c["chan_wid"])
        sc[i] = (c["bestdm"], c["fold_p1"] * L, (z[i] / L).sum(), var[i], c["dms"][0], c["dms"][-1],
                 len(c["dms"]), c["fold_p1"])
    return x, z, fr, sc


def block(shape, n, f32=False):
    key = (shape, n, f32)
    if key not in _blocks:
        kp, ks = masks(shape, n)
        ins = fold_inputs(candidates(shape, n), kp, ks, f32) + (kp, ks)
        for a in ins:
            a.setflags(write=False)
        _blocks[key] = ins
    return _blocks[key]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("route,opts,shape,n", ROUTES, ids=[r[0] for r in ROUTES])
def test_routes(engine, route, opts, shape, n, f32):
    x, z, fr, sc, kp, ks = block(shape, n, f32)
    with engine.options(**opts):
        same_dmprof(engine.pfd_dmprof(x, fr, sc, kill_parts=kp, kill_subs=ks),
                    engine.pfd_dmprof(z, fr, sc), route)
        same_scores(engine.pfd_bates22(x, fr, sc, kill_parts=kp, kill_subs=ks),
                    engine.pfd_bates22(z, fr, sc), route)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_straddle(engine, f32):
    """(9, 6, 34): E = 204 takes 16-byte loads and proflen = 34 is no multiple of 2 or 4, so a
    lane's elements span two sub-bands: the sub-band bit is per element."""
    shape, n = (9, 6, 34), 5
    cands = candidates(shape, n)
    kp = np.zeros((n, 9), dtype=bool)
    ks = np.zeros((n, 6), dtype=bool)
    kp[:, [0, 8]] = True
    ks[:, 1] = True
    x, z, fr, sc = fold_inputs(cands, kp, ks, f32)
    assert (6 * 34) % 4 == 0 and 34 % 4 != 0
    want_d, want_s = engine.pfd_dmprof(z, fr, sc), engine.pfd_bates22(z, fr, sc)
    for k in ("profile", "chis", "lyon8"):
        fin = np.isfinite(want_d[k]).all(axis=1).sum()
        assert fin >= 3, (k, fin)
    finite_rows = np.isfinite(want_s[0]).sum(axis=0)
    assert (finite_rows >= 3).all(), finite_rows
    same_dmprof(engine.pfd_dmprof(x, fr, sc, kill_parts=kp, kill_subs=ks), want_d, "straddle")
    same_scores(engine.pfd_bates22(x, fr, sc, kill_parts=kp, kill_subs=ks), want_s, "straddle")
    # 1-D masks are broadcast to every fold
    same_scores(engine.pfd_bates22(x, fr, sc, kill_parts=kp[0], kill_subs=ks[0]), want_s, "1-D")
    plain = engine.pfd_dmprof(x, fr, sc)
    assert not np.array_equal(plain["profile"], want_d["profile"], equal_nan=True)
    assert not np.array_equal(plain["chis"], want_d["chis"], equal_nan=True)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,n", [((7, 8, 64), 5), ((3, 5, 33), 9)], ids=["7x8x64", "3x5x33"])
def test_group_calls(engine, shape, n, f32):
    x, z, fr, sc, kp, ks = block(shape, n, f32)
    for call in (engine.pfd_params4, engine.pfd_dmfit4, engine.pfd_subband3):
        same_scores(call(x, fr, sc, kill_parts=kp, kill_subs=ks), call(z, fr, sc), call.__name__)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("chunk", [1, 2, 64])
def test_chunk_seams(engine, chunk, f32):
    """PFE_OPT_PFD_F32_CHUNK governs the masked calls, f64 included: passes of 1, 2 and (cut to
    n) 5 of n = 5 folds give the plain call's bits -- the masks advance with the pass."""
    x, z, fr, sc, kp, ks = block((3, 5, 33), 5, f32)
    kw = dict(kill_parts=kp, kill_subs=ks)
    calls = (engine.pfd_bates22, engine.pfd_dmfit4, engine.pfd_subband3, engine.pfd_params4)
    want_d = engine.pfd_dmprof(z, fr, sc)
    want = [c(z, fr, sc) for c in calls]
    want_a = engine.pfd_dmprof(z, fr, sc, derive_avgprof=True)
    with engine.options(pfd_f32_chunk=chunk):
        same_dmprof(engine.pfd_dmprof(x, fr, sc, **kw), want_d, f"chunk {chunk}")
        same_dmprof(engine.pfd_dmprof(x, fr, sc, derive_avgprof=True, **kw), want_a,
                    f"chunk {chunk} derived")
        for c, w in zip(calls, want):
            same_scores(c(x, fr, sc, **kw), w, f"chunk {chunk} {c.__name__}")
        for o in ({"pfd_global": 1}, {"pfd_split": 1}):
            with engine.options(**o):
                same_dmprof(engine.pfd_dmprof(x, fr, sc, **kw), want_d, f"chunk {chunk} {o}")


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_poison(engine, f32):
    """Killed rows hold NaN, +inf, -0.0 and 1e308 (float32: 3e38): replaced, never multiplied,
    so the outputs are those of the zeroed cube.  A fold with every part killed is the zero
    cube."""
    shape, n = (7, 8, 64), 5
    x, z, fr, sc, kp, ks = block(shape, n, f32)
    x = np.array(x)
    big = 3e38 if f32 else 1e308
    kill = np.broadcast_to(kp[:, :, None, None] | ks[:, None, :, None], x.shape)
    poison = np.resize(np.array([np.nan, np.inf, -0.0, big, -np.inf, -big], dtype=x.dtype), x.shape)
    x[kill] = poison[kill]
    assert np.isnan(x).any() and np.isinf(x).any()
    kw = dict(kill_parts=kp, kill_subs=ks)
    same_dmprof(engine.pfd_dmprof(x, fr, sc, **kw), engine.pfd_dmprof(z, fr, sc), "poison")
    same_scores(engine.pfd_bates22(x, fr, sc, **kw), engine.pfd_bates22(z, fr, sc), "poison")
    same_dmprof(engine.pfd_dmprof(x, fr, sc, derive_avgprof=True, **kw),
                engine.pfd_dmprof(z, fr, sc, derive_avgprof=True), "poison derived")
    # every part killed (and, separately, every sub-band): the plain call on the zero cube
    allp = np.ones_like(kp)
    zero = np.zeros_like(z)
    same_dmprof(engine.pfd_dmprof(x, fr, sc, kill_parts=allp), engine.pfd_dmprof(zero, fr, sc),
                "all parts")
    same_scores(engine.pfd_bates22(x, fr, sc, kill_parts=allp), engine.pfd_bates22(zero, fr, sc),
                "all parts")
    same_dmprof(engine.pfd_dmprof(x, fr, sc, kill_subs=np.ones_like(ks)),
                engine.pfd_dmprof(zero, fr, sc), "all sub-bands")


def test_flags(engine):
    """derive_avgprof with masks is the plain derived call on z; byteswapped on x.byteswap()
    with masks is the plain call on z (the word is reversed, then selected)."""
    for shape, n in (((7, 8, 64), 5), ((3, 5, 33), 9)):
        x, z, fr, sc, kp, ks = block(shape, n)
        kw = dict(kill_parts=kp, kill_subs=ks)
        nan_sc = np.array(sc)
        nan_sc[:, 2] = np.nan  # not read
        same_dmprof(engine.pfd_dmprof(x, fr, nan_sc, derive_avgprof=True, **kw),
                    engine.pfd_dmprof(z, fr, nan_sc, derive_avgprof=True), "derive")
        same_scores(engine.pfd_bates22(x, fr, nan_sc, derive_avgprof=True, **kw),
                    engine.pfd_bates22(z, fr, nan_sc, derive_avgprof=True), "derive 22")
        same_dmprof(engine.pfd_dmprof(x, fr, sc, **kw), engine.pfd_dmprof(z, fr, sc), "sanity")
        xs = x.byteswap()
        same_dmprof(engine.pfd_dmprof(xs, fr, sc, byteswapped=True, **kw),
                    engine.pfd_dmprof(z, fr, sc), "bswap")
        same_scores(engine.pfd_bates22(xs, fr, nan_sc, byteswapped=True, derive_avgprof=True, **kw),
                    engine.pfd_bates22(z, fr, nan_sc, derive_avgprof=True), "bswap derive 22")
        same(engine.pfd_avgprof(xs, byteswapped=True, **kw), (z / shape[2]).sum(axis=(1, 2, 3)),
             "bswap avgprof")
    x32, _z, fr, sc, kp, ks = block((7, 8, 64), 5, True)
    with pytest.raises(PfeError, match="pfd_dmprof_kill: PFE_FLAG_PFD_BSWAP is for the f64 calls"):
        engine.pfd_dmprof(x32, fr, sc, byteswapped=True, kill_parts=kp)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_device_tensors_carry_the_host_bits(engine, f32):
    import torch

    x, z, fr, sc, kp, ks = block((7, 8, 64), 5, f32)
    t = [_dev(a) for a in (x, fr, sc)]
    tkp, tks = _dev(kp), _dev(ks)
    assert tkp.dtype == torch.bool
    kw = dict(kill_parts=tkp, kill_subs=tks)
    d, s = engine.pfd_dmprof(*t, **kw), engine.pfd_bates22(*t, **kw)
    g = engine.pfd_subband3(*t, kill_parts=tkp.to(torch.uint8), kill_subs=tks)
    a = engine.pfd_avgprof(t[0], **kw)
    da = engine.pfd_dmprof(*t, derive_avgprof=True, kill_subs=tks)
    engine.synchronize()
    assert bool((t[0] == _dev(x)).all()) and bool((tkp == _dev(kp)).all())  # nothing written
    same_dmprof(_host(d), engine.pfd_dmprof(z, fr, sc), "device dmprof")
    same_scores(_host(s), engine.pfd_bates22(z, fr, sc), "device bates22")
    same_scores(_host(g), engine.pfd_subband3(z, fr, sc), "device subband3")
    same(a.cpu().numpy(), (z / 64).sum(axis=(1, 2, 3)), "device avgprof")
    zs = zap(np.asarray(x), np.zeros_like(kp), ks).astype(np.float64)
    same_dmprof(_host(da), engine.pfd_dmprof(zs, fr, sc, derive_avgprof=True), "device subs only")


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(1, 1, 4), (3, 5, 33), (3, 5, 600), (2, 4, 2048)],
                         ids=["1x1x4", "3x5x33", "3x5x600", "2x4x2048"])
def test_avgprof_with_masks(engine, shape, f32):
    """pfe_pfd_avgprof_kill against numpy's (z / L).sum(), bit for bit.  3x5x600 is 9000
    values: a chunk seam of 8192 inside a killed row, and L no power of two."""
    n = 4
    rng = np.random.default_rng(SEED)
    x = rng.normal(100.0, 10.0, size=(n,) + shape)
    if f32:
        x = x.astype(np.float32)
    kp, ks = masks(shape, n)
    if shape == (3, 5, 600):
        kp[1] = [False, False, True]   # values 6000 .. 8999: the seam at 8192 lies in a killed part
        ks[2] = [False, False, False, True, False]
    z = zap(x, kp, ks).astype(np.float64)
    want = np.array([(z[i] / shape[2]).sum() for i in range(n)])
    same(engine.pfd_avgprof(x, kill_parts=kp, kill_subs=ks), want, "both masks")
    same(engine.pfd_avgprof(x, kill_parts=kp), np.array(
        [(zap(x, kp, np.zeros_like(ks)).astype(np.float64)[i] / shape[2]).sum() for i in range(n)]),
        "parts only")
    same(engine.pfd_avgprof(x, kill_subs=ks), np.array(
        [(zap(x, np.zeros_like(kp), ks).astype(np.float64)[i] / shape[2]).sum() for i in range(n)]),
        "subs only")


def test_no_masks_is_the_plain_call(engine, monkeypatch):
    x, _z, fr, sc, kp, ks = block((7, 8, 64), 5)
    x32 = block((7, 8, 64), 5, True)[0]
    for cube in (x, x32):
        want_d, want_s = engine.pfd_dmprof(cube, fr, sc), engine.pfd_bates22(cube, fr, sc)
        want_a = engine.pfd_avgprof(cube)
        for kw in (dict(kill_parts=None, kill_subs=None),
                   dict(kill_parts=np.zeros_like(kp), kill_subs=np.zeros_like(ks))):
            same_dmprof(engine.pfd_dmprof(cube, fr, sc, **kw), want_d, "no masks")
            same_scores(engine.pfd_bates22(cube, fr, sc, **kw), want_s, "no masks")
            same(engine.pfd_avgprof(cube, **kw), want_a, "no masks")
    # a pfe_pfd_kill whose members are both null, and a null pfe_pfd_kill: the plain call's bits
    import torch

    t = [_dev(a) for a in (x, fr, sc)]
    pin = PfdIn(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 7, 8, 64, 5)
    for kill in (C.byref(PfdKill(None, None)), None):
        out = torch.zeros((5, 22), dtype=torch.float64, device="cuda")
        st = torch.zeros((5,), dtype=torch.int32, device="cuda")
        assert engine.lib.pfe_pfd_bates22_kill(engine._h, C.byref(pin), kill, out.data_ptr(),
                                               st.data_ptr(), PFE_FLAG_DEVICE_PTRS) == 0
        engine.synchronize()
        same_scores((out.cpu().numpy(), st.cpu().numpy().view(np.uint32)),
                    engine.pfd_bates22(x, fr, sc), "null masks")

    # both None: the plain symbol is the one called
    def kill_entry(*a):
        raise AssertionError("a call without masks went to a _kill entry point")

    for name in ("dmprof", "bates22", "params4", "dmfit4", "subband3", "avgprof"):
        monkeypatch.setattr(engine.lib, f"pfe_pfd_{name}_kill", kill_entry)
        monkeypatch.setattr(engine.lib, f"pfe_pfd_{name}_kill_f32", kill_entry)
    for cube in (x, x32):
        engine.pfd_dmprof(cube, fr, sc, kill_parts=None, kill_subs=None)
        engine.pfd_avgprof(cube, kill_parts=None, kill_subs=None)
        for call in (engine.pfd_bates22, engine.pfd_params4, engine.pfd_dmfit4, engine.pfd_subband3):
            call(cube, fr, sc, kill_parts=None, kill_subs=None)
    with pytest.raises(AssertionError):
        engine.pfd_bates22(x, fr, sc, kill_parts=kp)


def zapped_data(c, kp, ks):
    """A PFDData holding the zapped cube and its recomputed scalars."""
    npart, nsub, L = c["profs"].shape
    z = zap(c["profs"][None], kp[None], ks[None])[0]
    sd = c["chan_wid"] * (c["numchan"] // nsub)
    return pfd.PFDData(
        npart=npart, nsub=nsub, proflen=L, profs=z, bestdm=c["bestdm"], binspersec=c["fold_p1"] * L,
        avgprof=(z / L).sum(), varprof=float(pfd.varprof(c["stats"][:, :, 5], kp, ks)), dms=c["dms"],
        numdms=len(c["dms"]), bary_p1=c["fold_p1"],
        subfreqs=np.arange(nsub, dtype="d") * sd + (c["lofreq"] + sd - c["chan_wid"]))


def test_vs_oracle(engine):
    """An independent bar: three zapped folds of 7x8x64 against the CPU restatement, held to what
    tests/test_pfd_gpu.py and tests/test_pfd22_gpu.py hold plain folds to."""
    shape, n = (7, 8, 64), 3
    cands = candidates(shape, n)
    kp, ks = masks(shape, 5)
    kp, ks = kp[1:4], ks[1:4]
    x, _z, fr, sc = fold_inputs(cands, kp, ks)
    datas = [zapped_data(c, kp[i], ks[i]) for i, c in enumerate(cands)]
    r = engine.pfd_dmprof(x, fr, sc, kill_parts=kp, kill_subs=ks)
    eq_nan = lambda a, b: (a == b) | (np.isnan(a) & np.isnan(b))  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, d in enumerate(datas):
            assert eq_nan(r["profile"][i], opfd.PFDState(d).profile()).all(), i
            chis = opfd.dm_curve(d)
            assert np.array_equal(r["chis"][i], chis) or eq_nan(r["chis"][i], chis).all(), i
            ref = np.array(opfd.lyon8_one(d))
            for j in (0, 1, 3, 4, 5, 7):
                assert eq_nan(r["lyon8"][i][j], ref[j]), (i, j, r["lyon8"][i][j], ref[j])
            for j, tol in ((2, 1e-13), (6, 1e-6)):  # (a constant DM curve: NaN in both)
                got = r["lyon8"][i][j]
                assert eq_nan(got, ref[j]) or abs(got - ref[j]) <= tol * abs(ref[j]), (i, j)
        out, st = engine.pfd_bates22(x, fr, sc, kill_parts=kp, kill_subs=ks)
        ref, ok, floor = oracle_floor(datas)
    check22(out, st, ref, ok, "zapped 7x8x64", floor)


def _raw(engine, name, struct, profs, fr, sc, shape, n, nout, kill):
    import torch

    out = torch.zeros((n, nout), dtype=torch.float64, device="cuda")
    st = torch.zeros((n,), dtype=torch.int32, device="cuda")
    pin = struct(profs, fr.data_ptr(), sc.data_ptr(), *shape, n)
    fn = getattr(engine.lib, name)
    k = (C.byref(kill),) if kill is not None else ()
    if "dmprof" in name:
        rc = fn(engine._h, C.byref(pin), *k, None, None, out.data_ptr(), st.data_ptr(), PFE_FLAG_DEVICE_PTRS)
    else:
        rc = fn(engine._h, C.byref(pin), *k, out.data_ptr(), st.data_ptr(), PFE_FLAG_DEVICE_PTRS)
    return rc, engine.lib.pfe_last_error(engine._h).decode()


def test_errors(engine):
    """The plain call's PFE_EINVAL texts under the _kill names; ValueError for mask shapes and
    for masks with an int16 cube."""
    fr1, sc = np.full((1, 1), 1400.0), np.ones((1, 8))
    one = np.ones((1, 1, 1, 1))
    k1 = np.ones((1, 1), dtype=bool)
    for cube in (one, one.astype(np.float32)):
        with pytest.raises(PfeError, match="pfd_dmprof_kill: shape 1x1x1"):
            engine.pfd_dmprof(cube, fr1, sc, kill_parts=k1)
        with pytest.raises(PfeError, match="pfd_avgprof_kill: shape 1x1x1"):
            engine.pfd_avgprof(cube, kill_parts=k1)
    fr2 = np.full((1, 2), 1400.0)
    long_ = np.ones((1, 1, 2, 1025))
    for call in (engine.pfd_bates22, engine.pfd_params4, engine.pfd_dmfit4, engine.pfd_subband3):
        plain = None
        with pytest.raises(PfeError) as e:
            call(long_, fr2, sc)
        plain = str(e.value)
        assert "1x2x1025 unsupported" in plain
        for cube in (long_, long_.astype(np.float32)):
            with pytest.raises(PfeError) as e:
                call(cube, fr2, sc, kill_subs=np.array([True, False]))
            assert str(e.value) == plain.replace(call.__name__, call.__name__ + "_kill")
    # a null cube, straight at the C entry points
    tfr, tsc = _dev(np.full((2, 8), 1400.0)), _dev(np.ones((2, 8)))
    tkp = _dev(np.zeros((2, 3), dtype=np.uint8))
    kill = PfdKill(tkp.data_ptr(), None)
    for name, nout in (("pfe_pfd_dmprof", 8), ("pfe_pfd_bates22", 22), ("pfe_pfd_params4", 4),
                       ("pfe_pfd_dmfit4", 4), ("pfe_pfd_subband3", 3)):
        want = _raw(engine, name, PfdIn, None, tfr, tsc, (3, 8, 64), 2, nout, None)
        assert want[0] != 0 and "null input array" in want[1]
        short = name[4:]
        for sfx, struct in (("_kill", PfdIn), ("_kill_f32", PfdF32In)):
            got = _raw(engine, name + sfx, struct, None, tfr, tsc, (3, 8, 64), 2, nout, kill)
            assert got == (want[0], want[1].replace(short + ":", short + "_kill:")), name + sfx
    engine.synchronize()
    # mask shapes and dtypes
    x, _z, fr, sc5, kp, ks = block((7, 8, 64), 5)
    for kw in (dict(kill_parts=ks), dict(kill_subs=kp), dict(kill_parts=kp[:4]),
               dict(kill_subs=np.zeros((5, 8, 1), dtype=bool)), dict(kill_parts=np.zeros(8, dtype=bool)),
               dict(kill_parts=kp.astype(np.int32))):
        for call in (engine.pfd_dmprof, engine.pfd_bates22, engine.pfd_subband3):
            with pytest.raises(ValueError):
                call(x, fr, sc5, **kw)
        with pytest.raises(ValueError):
            engine.pfd_avgprof(x, **kw)
    with pytest.raises(ValueError, match="profs must be"):  # the cube is checked first
        engine.pfd_dmprof(x[0], fr, sc5, kill_parts=kp)
    with pytest.raises(TypeError):  # a host mask with a device cube
        engine.pfd_bates22(_dev(x), _dev(fr), _dev(sc5), kill_parts=kp)
    # an int16 cube is zapped through its weights
    d16 = np.zeros((5, 7, 8, 64), dtype=np.int16)
    par = np.ones((5, 7, 8), dtype=np.float32)
    for call in (engine.pfd_dmprof, engine.pfd_bates22, engine.pfd_params4, engine.pfd_dmfit4,
                 engine.pfd_subband3):
        with pytest.raises(ValueError, match="wts"):
            call(d16, fr, sc5, scl=par, offs=par, kill_parts=kp)
    with pytest.raises(ValueError, match="wts"):
        engine.pfd_avgprof(d16, scl=par, offs=par, kill_subs=ks)


def _write_files(tmp_path, cands, tag, zero=None):
    """pfd.write files of the folds, the second one big-endian; zero = (parts, subs): written
    with those rows zero in the cube and zero in stats[..., 5]."""
    files = []
    for i, c in enumerate(cands):
        c = dict(c)
        if zero is not None:
            profs, stats = np.array(c["profs"]), np.array(c["stats"])
            profs[zero[0]] = 0.0
            profs[:, zero[1]] = 0.0
            stats[zero[0], :, 5] = 0.0
            stats[:, zero[1], 5] = 0.0
            c["profs"], c["stats"] = profs, stats
        p = os.path.join(tmp_path, f"{tag}_{i}.pfd")
        pfd.write(p, big_endian=(i == 1), **c)
        files.append(p)
    return files


def test_pfdfile_kill_methods(engine, tmp_path):
    """PFDFile.kill_subbands([1]); kill_intervals([0]) gives the scores of Engine.pfd_bates22 on
    z, and leaves the cube as it was read."""
    from pulsarfeatureextractor_amd.candidate import PFDFile

    shape = (7, 8, 64)
    c = candidates(shape, 2)[1]
    path = _write_files(tmp_path, [c], "one")[0]
    f = PFDFile(False, path, engine=engine)
    before = np.array(f.data.profs)
    plain = f.compute()
    f.kill_intervals([])   # an RFI finder that found nothing: every score stays as it was
    f.kill_subbands([])
    assert np.array_equal(f.compute(), plain, equal_nan=True) and f.data.avgprof is not None
    f.kill_subbands([1])
    f.kill_intervals([0])
    assert f.killed_subbands == [1] and f.killed_intervals == [0]
    with pytest.raises(IndexError):
        f.kill_subbands([8])
    with pytest.raises(IndexError):
        f.kill_intervals([-1])
    kp = np.zeros((1, 7), dtype=bool)
    ks = np.zeros((1, 8), dtype=bool)
    kp[0, 0] = ks[0, 1] = True
    d = pfd.read(path)
    x, fr, sc = pfd.batch_inputs([d])
    z = zap(x, kp, ks)
    sc[0, 2] = (z[0] / 64).sum()
    sc[0, 3] = pfd.varprof(d.stats[:, :, 5], kp[0], ks[0])
    assert sc[0, 3] != d.varprof
    assert f.data.varprof == sc[0, 3] == f.calc_varprof()
    want, st = engine.pfd_bates22(z, fr, sc)
    assert (st[0] & 0xFF) == 0
    assert f.compute() == [float(v) for v in want[0]]
    d = engine.pfd_dmprof(z, fr, sc)
    same(np.asarray(f.getProfile()), d["profile"][0], "profile")
    same(np.asarray(f.getDMCurveData()), d["chis"][0], "DM curve")
    assert f.computeProfileStatScores() == [float(v) for v in d["lyon8"][0, :4]]
    f.scores = []
    f.computeDMCurveFittingScores()
    f.computeSubBandScores()
    assert f.scores[0] == float(want[0, 15]) and f.scores[-3:] == [float(v) for v in want[0, 19:]]
    assert np.array_equal(f.data.profs, before)


def _cli_run(work, monkeypatch, cands, tag, zero, extra):
    """A CLI run in a directory of its own over files at the same relative paths -> {name: bytes}
    of the output file and the error log."""
    from pulsarfeatureextractor_amd import cli

    d = work / tag
    (d / "cands").mkdir(parents=True)
    _write_files(str(d / "cands"), cands, "f", zero)
    monkeypatch.chdir(d)
    assert cli.main(["-c", "cands", "-o", "out.csv", "--pfd", "--workers", "2", *extra]) == 0
    return {name: open(d / name, "rb").read() for name in ("out.csv", "CandidateErrorLog.txt")}


@pytest.mark.parametrize("mode", [[], ["--dmprof"]], ids=["scores", "dmprof"])
def test_cli_kill_lists(tmp_path, monkeypatch, mode):
    """--killsubs 1,3:4 --killparts 0 over files from pfd.write is byte-identical to a plain run
    over the same files written with those rows zero in the cube and zero in stats[..., 5]; one
    of the files is big-endian (the native reader's byte order flag, with the masks)."""
    cands = candidates((7, 8, 64), 4)
    got = _cli_run(tmp_path, monkeypatch, cands, "kill", None,
                   mode + ["--killsubs", "1,3:4", "--killparts", "0"])
    want = _cli_run(tmp_path, monkeypatch, cands, "zero", ([0], [1, 3, 4]), mode)
    plain = _cli_run(tmp_path, monkeypatch, cands, "plain", None, mode)
    assert got["out.csv"].count(b"\n") >= 3
    assert got == want
    assert got["out.csv"] != plain["out.csv"]


def test_cli_kill_index_out_of_range_fails_the_fold_alone(tmp_path, monkeypatch, capsys):
    """A fold that has no sub-band 7 fails alone, with an error-log line (its path, as for a
    refused shape; the reason goes to the run's output) and no row."""
    from pulsarfeatureextractor_amd import cli

    d = tmp_path / "mixed"
    (d / "cands").mkdir(parents=True)
    for i, shape in enumerate(((7, 8, 64), (7, 8, 64), (3, 6, 40))):
        pfd.write(str(d / "cands" / f"f_{i}.pfd"),
                  **pfd_candidate(np.random.default_rng(SEED + i), *shape))
    monkeypatch.chdir(d)
    assert cli.main(["-c", "cands", "-o", "out.csv", "--pfd", "--dmprof", "--workers", "2",
                     "--killsubs", "7"]) == 0
    rows = open(d / "out.csv").read()
    log = open(d / "CandidateErrorLog.txt").read()
    assert "f_0.pfd" in rows and "f_1.pfd" in rows and "f_2.pfd" not in rows
    assert log.splitlines() == ["cands/f_2.pfd"]
    assert "killed sub-band 7 out of range: the fold has 6" in capsys.readouterr().out
    with pytest.raises(SystemExit):  # valid with --pfd only
        cli.main(["-c", "cands", "-o", "out2.csv", "--phcx", "--killsubs", "1"])
    assert not os.path.exists(d / "out2.csv")
