"""Scrunching a fold on the device (pfe_pfd_scrunch, _f32, _i16, reached through
Engine.pfd_scrunch) against the contract include/pfe.h states: the parts of every element summed
in order, each channel's row rotated left by rot mod nbin, bscr bins summed in order, fscr
channels summed in order, every step in fp64.

The reference is the numpy restatement `restate` below -- elementwise adds in sequential loops over
the parts, then the bscr bins, then the fscr channels, np.roll(S, -r) for the rotation, and the
int16 tests' numpy decode -- never the call under test.  The bar is np.array_equal with equal_nan
on every output, no tolerance.  rot is random int32 per fold and channel with negatives, 0,
nbin - 1 and values beyond +-nbin (the int32 extremes among them); n is 3 to 5 and the folds
differ."""
import ctypes as C

import numpy as np
import pytest

from pulsarfeatureextractor_amd import pfd
from pulsarfeatureextractor_amd._native import (PFE_FLAG_DEVICE_PTRS, PFE_FLAG_PFD_AVGPROF,
                                                PFE_FLAG_PFD_BSWAP, PfdI16In, PfdScrunchHow, PfeError)
from pulsarfeatureextractor_amd.synth import pfd_candidate
from test_pfd_i16_gpu import block, column, decode, table

pytestmark = pytest.mark.gpu

f4, f8, i2, i4 = np.float32, np.float64, np.int16, np.int32

# (npart, nchan, nbin, fscr, bscr), n.  15 parts: every burst size (8 + 4 + 2 + 1); 1 x 8 x 64:
# a pure rotation; 3 x 10 x 35: nothing a multiple of 4, so single-value loads, quads spanning
# channels and a slab that ends inside a quad; 64 x 32 -> one value a fold; 4100 bins, fscr 1: a
# row beyond the 4096-value slab, one slab a group; 20000 bins: the row does not fit the LDS, the
# direct route.  The shapes above take one slab a group (C = min(fscr, 4096 // nbin) = fscr).  The
# last four take several, so the barrier in front of a slab, the running sums kept in the LDS
# between slabs and the switch to the store after the last one run: 8 x 1024 = 2 slabs of 4 rows,
# wide loads; 6 x 1001 = a slab of 4 rows and a partial one of 2, single-value loads, quads across
# channels; 4 x 4100, fscr 2 = one row a slab, two slabs; 12 x 512, fscr 12 = a slab of 8 and a
# partial one of 4
SHAPES = [((15, 12, 96, 3, 4), 3), ((1, 8, 64, 1, 1), 4), ((3, 10, 35, 5, 7), 5), ((2, 6, 33, 2, 1), 4),
          ((9, 4, 128, 1, 16), 3), ((4, 64, 32, 64, 32), 5), ((2, 3, 4100, 1, 4), 3),
          ((1, 2, 20000, 2, 8), 3), ((2, 8, 1024, 8, 8), 3), ((3, 6, 1001, 6, 7), 3),
          ((1, 4, 4100, 2, 4), 3), ((2, 24, 512, 12, 4), 3)]
SLABS = {(8, 1024): 2, (6, 1001): 2, (2, 4100): 2, (12, 512): 2}   # slabs a group where more than one
ROUTE = {4100: "lds", 20000: "direct"}  # the route each long row is expected to take
IDS = ["x".join(map(str, s)) for s, _ in SHAPES]
shapes = pytest.mark.parametrize("shape,n", SHAPES, ids=IDS)


def restate(x64, rot, fscr, bscr):
    """The contract, step by step, on a float64 cube (n, npart, nchan, nbin) -> (n, 1, G, K)."""
    n, npart, nchan, nbin = x64.shape
    G, K = nchan // fscr, nbin // bscr
    z = np.empty((n, 1, G, K), dtype=f8)
    for i in range(n):
        S = x64[i, 0].copy()
        for p in range(1, npart):
            S = S + x64[i, p]
        R = np.empty_like(S)
        for c in range(nchan):
            r = 0 if rot is None else ((int(rot[i, c]) % nbin) + nbin) % nbin
            R[c] = np.roll(S[c], -r)
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


_cases = {}


def case(shape, n):
    """The inputs of one shape and their restated results, built once and left unchanged."""
    key = (shape, n)
    if key in _cases:
        return _cases[key]
    npart, nchan, nbin, fscr, bscr = shape
    rng = np.random.default_rng(20261021 + nbin)
    x64 = rng.normal(100.0, 30.0, size=(n, npart, nchan, nbin)) * 10.0 ** rng.integers(-3, 4, size=(n, 1, nchan, 1))
    x32 = x64.astype(f4)
    d = rng.integers(-32768, 32768, size=x64.shape).astype(i2)
    scl = rng.uniform(1e-3, 2.0, size=(n, npart, nchan)).astype(f4)
    offs = rng.normal(0.0, 50.0, size=(n, npart, nchan)).astype(f4)
    wts = rng.uniform(0.05, 1.0, size=(n, npart, nchan)).astype(f4)
    wts[0] = 1.0                       # ones
    wts[1, :, nchan // 2] = 0.0        # a zapped channel
    wts[2, npart - 1, 0] = np.nan      # one NaN weight
    rot = rng.integers(-3 * nbin, 3 * nbin + 1, size=(n, nchan)).astype(i4)
    edge = np.array([0, nbin - 1, -1, nbin, -nbin, 2 ** 31 - 1, -2 ** 31, -nbin - 1], dtype=i4)
    flat = rot.reshape(-1)
    flat[:min(flat.size, edge.size)] = edge[:flat.size]
    assert (rot < 0).any() and (rot == 0).any() and (np.abs(rot.astype(np.int64)) > nbin).any()
    c = dict(x64=x64, x32=x32, d=d, scl=scl, offs=offs, wts=wts, rot=rot,
             z64=restate(x64, rot, fscr, bscr), z32=restate(x32.astype(f8), rot, fscr, bscr),
             z16=restate(decode(d, scl, offs), rot, fscr, bscr),
             z16w=restate(decode(d, scl, offs, wts), rot, fscr, bscr))
    assert np.isnan(c["z16w"][2]).any() and not np.isnan(c["z16w"][:2]).any()
    assert not np.array_equal(c["z64"][0], c["z64"][1])
    for a in c.values():
        a.setflags(write=False)
    _cases[key] = c
    return c


def same(got, want, tag):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    assert np.array_equal(got, want, equal_nan=True), tag


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def forms(c):
    """(tag, cube, keywords, expected) of the dense forms."""
    return [("f64", c["x64"], {}, c["z64"]), ("f32", c["x32"], {}, c["z32"]),
            ("i16", c["d"], dict(scl=c["scl"], offs=c["offs"]), c["z16"]),
            ("i16w", c["d"], dict(scl=c["scl"], offs=c["offs"], wts=c["wts"]), c["z16w"])]


@shapes
def test_host_arrays(engine, shape, n):
    """Host pointers, every dense form; the inputs are the same bytes afterwards."""
    c = case(shape, n)
    fscr, bscr = shape[3:]
    for tag, x, kw, want in forms(c):
        ins = [x, c["rot"]] + list(kw.values())
        before = [a.tobytes() for a in ins]
        got = engine.pfd_scrunch(x, fscr, bscr, rot=c["rot"], **kw)
        assert isinstance(got, np.ndarray)
        same(got, want, tag)
        assert [a.tobytes() for a in ins] == before, tag


@shapes
def test_device_tensors(engine, shape, n):
    """Device pointers give the bits of the host path, and leave their inputs alone; the
    byte-swapped int16 form; rot=None is rot of zeros; a caller's out= is filled."""
    import torch

    c = case(shape, n)
    nbin, fscr, bscr = shape[2:]
    assert pfd.scrunch_route(nbin, bscr) == ROUTE.get(nbin, "lds")
    chans = max(1, min(fscr, 4096 // nbin))          # csrc/launch.h pfd_scrunch_slab_chans
    if pfd.scrunch_route(nbin, bscr) == "lds":       # the direct route has no slabs
        assert -(-fscr // chans) == SLABS.get((fscr, nbin), 1)
    trot = _dev(c["rot"])
    for tag, x, kw, want in forms(c):
        tx, tkw = _dev(x), {k: _dev(v) for k, v in kw.items()}
        got = engine.pfd_scrunch(tx, fscr, bscr, rot=trot, **tkw)
        assert got.is_cuda and tuple(got.shape) == want.shape
        same(got, want, "device " + tag)
        same(tx, x, "input " + tag)
        for k in kw:
            same(tkw[k], kw[k], f"input {tag} {k}")
    same(trot, c["rot"], "rot")
    # byte-reversed values, as a file holds them
    swapped = {k: _dev(c[k].byteswap()) for k in ("scl", "offs", "wts")}
    got = engine.pfd_scrunch(_dev(c["d"].byteswap()), fscr, bscr, rot=trot, byteswapped=True, **swapped)
    same(got, c["z16w"], "swapped")
    host = engine.pfd_scrunch(c["d"].byteswap(), fscr, bscr, rot=c["rot"], byteswapped=True,
                              **{k: c[k].byteswap() for k in ("scl", "offs", "wts")})
    same(host, c["z16w"], "swapped, host")
    # no rotation
    want0 = restate(c["x64"], None, fscr, bscr)
    zeros = torch.zeros_like(trot)
    out = torch.full(want0.shape, -1.0, dtype=torch.float64, device="cuda")
    assert engine.pfd_scrunch(_dev(c["x64"]), fscr, bscr, out=out) is out
    same(out, want0, "rot=None")
    same(engine.pfd_scrunch(_dev(c["x64"]), fscr, bscr, rot=zeros), want0, "rot of zeros")
    same(engine.pfd_scrunch(c["x64"], fscr, bscr), want0, "rot=None, host")
    same(engine.pfd_scrunch(c["x32"], fscr, bscr, rot=np.zeros(shape[1], dtype=i4)),
         restate(c["x32"].astype(f8), None, fscr, bscr), "one row of zeros for every fold")


@shapes
def test_direct_route_gives_the_same_bits(engine, shape, n):
    """No result depends on the route: every form again with one lane per output bin."""
    c = case(shape, n)
    fscr, bscr = shape[3:]
    assert engine.get_option("pfd_scrunch_direct") == 0
    with engine.options(pfd_scrunch_direct=1):
        for tag, x, kw, want in forms(c):
            same(engine.pfd_scrunch(x, fscr, bscr, rot=c["rot"], **kw), want, "direct " + tag)
    assert engine.get_option("pfd_scrunch_direct") == 0
    with pytest.raises(PfeError):
        engine.set_option("pfd_scrunch_direct", 2)


@shapes
def test_table_rows(engine, shape, n):
    """int16 from the big-endian rows of a binary table through strided device views (the row
    layout of tests/test_pfd_i16_gpu.py), and from little-endian rows."""
    import torch

    c = case(shape, n)
    npart, nchan, nbin, fscr, bscr = shape
    trot = _dev(c["rot"])
    for order, swapped, pad in ((">", True, 0), ("<", False, 4)):
        t = table(c["d"], c["scl"], c["offs"], c["wts"], np.zeros((n, nchan)), order, pad, False)
        row = t.dtype.itemsize
        if row % 4:  # the rule of the _i16 calls: part_stride a multiple of 4
            t = table(c["d"], c["scl"], c["offs"], c["wts"], np.zeros((n, nchan)), order, pad + 4 - row % 4, False)
            row = t.dtype.itemsize
        buf = torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).cuda()
        cd = column(buf, t.dtype, "DATA", torch.int16, (n, npart, nchan, nbin))
        kw = dict(scl=column(buf, t.dtype, "DAT_SCL", torch.float32, (n, npart, nchan)),
                  offs=column(buf, t.dtype, "DAT_OFFS", torch.float32, (n, npart, nchan)),
                  wts=column(buf, t.dtype, "DAT_WTS", torch.float32, (n, npart, nchan)))
        assert not cd.is_contiguous() and cd.stride(1) * 2 == row
        before = buf.clone()
        same(engine.pfd_scrunch(cd, fscr, bscr, rot=trot, byteswapped=swapped, **kw), c["z16w"], "table " + order)
        del kw["wts"]
        same(engine.pfd_scrunch(cd, fscr, bscr, rot=trot, byteswapped=swapped, **kw), c["z16"],
             "table, no weights " + order)
        with engine.options(pfd_scrunch_direct=1):
            same(engine.pfd_scrunch(cd, fscr, bscr, rot=trot, byteswapped=swapped, **kw), c["z16"],
                 "table, direct " + order)
        assert torch.equal(buf, before)


@shapes
def test_cube_one_element_past_a_16_byte_boundary(engine, shape, n):
    """A slice of a larger buffer: where nbin is a multiple of 4 the single-value loads run in
    place of the wide ones.  Device tensors and host arrays."""
    import torch

    c = case(shape, n)
    fscr, bscr = shape[3:]
    trot = _dev(c["rot"])
    for tag, x, kw, want in forms(c):
        tx = _dev(x)
        big = torch.zeros(x.size + 16, dtype=tx.dtype, device="cuda")
        assert big.data_ptr() % 16 == 0
        cube = big[1:1 + x.size].view(x.shape)
        cube.copy_(tx)
        assert cube.data_ptr() % 16 == x.itemsize
        same(engine.pfd_scrunch(cube, fscr, bscr, rot=trot, **{k: _dev(v) for k, v in kw.items()}), want,
             "offset " + tag)
        raw = np.zeros(x.nbytes + 32, dtype=np.uint8)
        at = (-raw.ctypes.data) % 16 + x.itemsize
        hx = raw[at:at + x.nbytes].view(x.dtype).reshape(x.shape)
        hx[...] = x
        assert hx.ctypes.data % 16 == x.itemsize
        same(engine.pfd_scrunch(hx, fscr, bscr, rot=c["rot"], **kw), want, "offset, host " + tag)


# ---- refusals, each by its text --------------------------------------------------------------
def _raw(engine, x, npart, nchan, nbin, n, fscr, bscr, out, flags=0, rot=None, f32=False):
    how = PfdScrunchHow(rot, fscr, bscr)
    fn = engine.lib.pfe_pfd_scrunch_f32 if f32 else engine.lib.pfe_pfd_scrunch
    rc = fn(engine._h, x, npart, nchan, nbin, n, C.byref(how), out, flags)
    return rc, engine.lib.pfe_last_error(engine._h).decode()


def test_refusals(engine):
    x = np.zeros((2, 3, 4, 8), dtype=f8)
    x32 = x.astype(f4)
    out = np.zeros((2, 1, 4, 8), dtype=f8)
    px, po = x.ctypes.data, out.ctypes.data
    bad = [
        (dict(x=None), "pfd_scrunch: null input array"),
        (dict(out=None), "pfd_scrunch: null argument"),
        (dict(n=-1), "pfd_scrunch: n < 0"),
        (dict(nbin=0), "pfd_scrunch: shape 3x4x0"),
        (dict(npart=0), "pfd_scrunch: shape 0x4x8"),
        (dict(fscr=0), "pfd_scrunch: fscr 0 and bscr 1 must be >= 1"),
        (dict(bscr=-2), "pfd_scrunch: fscr 1 and bscr -2 must be >= 1"),
        (dict(fscr=3), "pfd_scrunch: fscr 3 does not divide nchan 4"),
        (dict(bscr=3), "pfd_scrunch: bscr 3 does not divide nbin 8"),
        (dict(x=px + 4), "pfd_scrunch: profs not 8-byte aligned"),
        (dict(x=x32.ctypes.data + 2, f32=True), "pfd_scrunch_f32: profs not 4-byte aligned"),
        (dict(rot=px + 2), "pfd_scrunch: rot not 4-byte aligned"),
        (dict(out=po + 4), "pfd_scrunch: out not 8-byte aligned"),
        (dict(flags=PFE_FLAG_PFD_BSWAP), "pfd_scrunch: PFE_FLAG_PFD_BSWAP is for the _i16 form"),
        (dict(flags=PFE_FLAG_PFD_BSWAP, x=x32.ctypes.data, f32=True),
         "pfd_scrunch_f32: PFE_FLAG_PFD_BSWAP is for the _i16 form"),
        (dict(flags=PFE_FLAG_PFD_AVGPROF), "pfd_scrunch: PFE_FLAG_PFD_AVGPROF is for the calls that read scal"),
        (dict(flags=PFE_FLAG_PFD_AVGPROF, x=x32.ctypes.data, f32=True),
         "pfd_scrunch_f32: PFE_FLAG_PFD_AVGPROF is for the calls that read scal"),
    ]
    for kw, text in bad:
        a = dict(x=px, npart=3, nchan=4, nbin=8, n=2, fscr=1, bscr=1, out=po)
        a.update(kw)
        rc, msg = _raw(engine, **a)
        assert rc != 0 and msg == text, (kw, msg)
    how = PfdScrunchHow(None, 1, 1)
    assert engine.lib.pfe_pfd_scrunch(engine._h, px, 3, 4, 8, 2, None, po, 0) != 0
    assert engine.lib.pfe_last_error(engine._h).decode() == "pfd_scrunch: null argument"
    assert engine.lib.pfe_pfd_scrunch_i16(engine._h, None, C.byref(how), po, 0) != 0
    assert engine.lib.pfe_last_error(engine._h).decode() == "pfd_scrunch_i16: null argument"
    # the int16 form: the rules of the _i16 calls, under this name
    d = np.zeros((2, 3, 4, 8), dtype=i2)
    par = np.ones((2, 3, 4), dtype=f4)
    pd, pp = d.ctypes.data, par.ctypes.data

    def i16(data=pd, scl=pp, offs=pp, wts=None, fs=0, ps=0, flags=0):
        pin = PfdI16In(data, scl, offs, wts, fs, ps, None, None, 3, 4, 8, 2)
        rc = engine.lib.pfe_pfd_scrunch_i16(engine._h, C.byref(pin), C.byref(how), po, flags)
        return rc, engine.lib.pfe_last_error(engine._h).decode()

    assert i16() == (0, "")  # subfreqs and scal are not read
    for kw, text in [
        (dict(scl=None), "pfd_scrunch_i16: null input array"),
        (dict(data=pd + 1), "pfd_scrunch_i16: data not 2-byte aligned"),
        (dict(wts=pp + 2), "pfd_scrunch_i16: scl, offs and wts must be 4-byte aligned"),
        (dict(fs=192), "pfd_scrunch_i16: fold_stride 192 and part_stride 0: both 0 (dense arrays) or both non-zero"),
        (dict(fs=192, ps=64), "pfd_scrunch_i16: strided input is for device pointers (PFE_FLAG_DEVICE_PTRS); a "
                              "host-pointer call takes dense arrays (both strides 0)"),
        (dict(fs=192, ps=60, flags=PFE_FLAG_DEVICE_PTRS),
         "pfd_scrunch_i16: part_stride 60 must be >= 2 x nsub x proflen = 64 and a multiple of 4"),
        (dict(fs=128, ps=64, flags=PFE_FLAG_DEVICE_PTRS),
         "pfd_scrunch_i16: fold_stride 128 must be >= npart x part_stride = 3 x 64 and a multiple of 4"),
        (dict(flags=PFE_FLAG_PFD_AVGPROF), "pfd_scrunch_i16: PFE_FLAG_PFD_AVGPROF is for the calls that read scal"),
    ]:
        rc, msg = i16(**kw)
        assert rc != 0 and msg == text, (kw, msg)
    # the wrapper names the same rules before it sizes the result
    for kw, text in [(dict(fscr=3), "fscr 3 does not divide nchan 4"), (dict(bscr=5), "bscr 5 does not divide nbin 8"),
                     (dict(fscr=0), "fscr 0 and bscr 1 must be >= 1")]:
        with pytest.raises(ValueError, match=text):
            engine.pfd_scrunch(x, **kw)
    with pytest.raises(PfeError, match="PFE_FLAG_PFD_BSWAP is for the _i16 form"):
        engine.pfd_scrunch(x, byteswapped=True)
    with pytest.raises(ValueError, match="scl and offs are required"):
        engine.pfd_scrunch(d)
    with pytest.raises(ValueError, match="go with an int16 cube"):
        engine.pfd_scrunch(x, scl=par, offs=par)
    with pytest.raises(ValueError, match="rot must be"):
        engine.pfd_scrunch(x, rot=np.zeros((2, 3), dtype=i4))
    with pytest.raises(ValueError, match="out must be"):
        engine.pfd_scrunch(x, out=np.zeros((2, 4, 8)))


# ---- the scrunched fold is a fold the library scores ------------------------------------------
@pytest.mark.parametrize("shape,n", [((7, 8, 64), 5), ((3, 5, 33), 67)], ids=["7x8x64", "3x5x33"])
def test_identity_is_the_part_sums_the_pfd_calls_form(engine, shape, n):
    """fscr = bscr = 1, no rot: pfd_dmprof and pfd_bates22 on the result as a fold of one part
    give the bits they give on the original float64, float32 and int16 cube."""
    d, scl, offs, wts, fr, sc = (a[:5] for a in block(shape, n))
    x64 = decode(d, scl, offs)
    for tag, x, kw in (("f64", x64, {}), ("f32", x64.astype(f4), {}), ("i16", d, dict(scl=scl, offs=offs)),
                       ("i16w", d, dict(scl=scl, offs=offs, wts=wts))):
        z = engine.pfd_scrunch(x, **kw)
        assert z.shape == (5, 1) + shape[1:]
        want_d, got_d = engine.pfd_dmprof(x, fr, sc, **kw), engine.pfd_dmprof(z, fr, sc)
        for k in ("profile", "chis", "lyon8", "status"):
            same(got_d[k], want_d[k], f"{tag} dmprof {k}")
        want_s, got_s = engine.pfd_bates22(x, fr, sc, **kw), engine.pfd_bates22(z, fr, sc)
        same(got_s[0], want_s[0], tag + " bates22")
        same(got_s[1], want_s[1], tag + " bates22 status")


def test_composition_stays_on_the_device(engine):
    """6 x 32 x 128 int16 -> 8 x 64 as a device tensor, then pfd_bates22 with the plan's subfreqs
    and the scrunched scalars and a derived average: the scores of the same call on the
    restated z."""
    shape, n, fscr, bscr = (6, 32, 128), 4, 4, 2
    rng = np.random.default_rng(5)
    cands = [pfd_candidate(rng, *shape) for _ in range(n)]
    datas = [pfd.PFDData(npart=shape[0], nsub=shape[1], proflen=shape[2], profs=c["profs"], bestdm=c["bestdm"],
                         binspersec=c["fold_p1"] * shape[2], avgprof=0.0, varprof=float(c["stats"][:, :, 5].sum()),
                         dms=c["dms"], numdms=len(c["dms"]), bary_p1=c["fold_p1"],
                         subfreqs=np.arange(shape[1], dtype="d") * c["chan_wid"] * (c["numchan"] // shape[1])
                         + c["lofreq"]) for c in cands]
    x, fr, sc = pfd.batch_inputs(datas)
    from test_pfd_i16_gpu import quantise

    d, scl, offs = quantise(x)
    rot, subfreqs = pfd.scrunch_plan(fr, sc[:, 0], sc[:, 1], shape[2], fscr)
    assert rot.shape == (n, 32) and subfreqs.shape == (n, 8) and rot.any()
    sc2 = pfd.scrunch_scal(sc, bscr)
    zref = restate(decode(d, scl, offs), rot, fscr, bscr)
    z = engine.pfd_scrunch(_dev(d), fscr, bscr, rot=_dev(rot), scl=_dev(scl), offs=_dev(offs))
    assert z.is_cuda and tuple(z.shape) == (n, 1, 8, 64)
    got = engine.pfd_bates22(z, _dev(subfreqs), _dev(sc2), derive_avgprof=True)
    want = engine.pfd_bates22(zref, subfreqs, sc2, derive_avgprof=True)
    same(z, zref, "z")
    same(got[0], want[0], "scores")
    assert np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1])
    assert np.isfinite(want[0]).any()


def test_pfdfile_scrunch(engine, tmp_path):
    """PFDFile.scrunch(nsub=4, proflen=32) on a 4 x 16 x 64 fold from pfd.write: compute() and
    computeProfileStatScores() are the engine calls on the restated arrays."""
    from pulsarfeatureextractor_amd.candidate import PFDFile

    c = pfd_candidate(np.random.default_rng(11), 4, 16, 64)
    path = str(tmp_path / "fold.pfd")
    pfd.write(path, **c)
    f = PFDFile(False, path, engine=engine)
    with pytest.raises(ValueError, match="does not divide"):
        f.scrunch(nsub=5)
    with pytest.raises(ValueError, match="does not divide"):
        f.scrunch(proflen=48)
    src = pfd.read(path)
    x, fr, sc = pfd.batch_inputs([src])
    f.scrunch(nsub=4, proflen=32)
    rot, subfreqs = pfd.scrunch_plan(fr, sc[:, 0], sc[:, 1], 64, 4)
    z = restate(x, rot, 4, 2)
    sc2 = pfd.scrunch_scal(sc, 2)
    assert np.isnan(sc2[0, 2]) and sc2[0, 1] == sc[0, 1] / 2 and sc2[0, 3] == sc[0, 3] * 2
    assert (f.data.npart, f.data.nsub, f.data.proflen) == (1, 4, 32) and f.data.avgprof is None
    assert np.array_equal(f.data.profs, z[0]) and np.array_equal(f.data.subfreqs, subfreqs[0])
    assert f.data.binspersec == sc2[0, 1] and f.data.varprof == sc2[0, 3]
    want, st = engine.pfd_bates22(z, subfreqs, sc2, derive_avgprof=True)
    assert (st[0] & 0xFF) == 0
    assert f.compute() == [float(v) for v in want[0]]
    lyon = engine.pfd_dmprof(z, subfreqs, sc2, derive_avgprof=True)["lyon8"]
    assert f.computeProfileStatScores() == [float(v) for v in lyon[0, :4]]
    g = PFDFile(False, path, engine=engine)
    g.kill_subbands([1])
    with pytest.raises(ValueError, match="kill after scrunching"):
        g.scrunch(nsub=4)
    f.kill_subbands([1])  # killing after scrunching works on the new rows
    assert f.killed_subbands == [1] and len(f.compute()) == 22
