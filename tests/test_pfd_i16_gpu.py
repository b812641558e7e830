"""The int16 forms of the PFD calls (pfe_pfd_*_i16, reached through Engine.pfd_* with an int16
cube and scl=, offs=, wts=) against the contract include/pfe.h states: every output and the
status are, bit for bit, those of the f64 call of the same name on the cube decoded in fp64.

The reference is always the existing f64 call on the cube numpy decodes,
    x64 = d.astype(f8) * scl.astype(f8)[..., None] + offs.astype(f8)[..., None]   [* wts ...]
-- never the call under test, never a golden.  Inputs are synth.pfd_fold_block folds quantised
per (fold, part, sub-band) the way a fold-mode archive holds them; the bar is np.array_equal with
equal_nan on every output and the status, no tolerance.  Shapes are those of
tests/test_pfd_f32_gpu.py: the smallest that take each route of the f64 kernels and both load
paths of k_pfd_partsum_i16 (8-byte loads when nsub x proflen is a multiple of 4 and the data is
8-byte aligned at every part, 2-byte loads otherwise)."""
import ctypes as C

import numpy as np
import pytest

from pulsarfeatureextractor_amd import pfd
from pulsarfeatureextractor_amd._native import (PFE_FLAG_DEVICE_PTRS, PFE_FLAG_PFD_BSWAP,
                                                PFE_PFD_AVGPROF, PfdI16In, PfeError)
from pulsarfeatureextractor_amd.synth import pfd_fold_block

pytestmark = pytest.mark.gpu

f4, f8, i2 = np.float32, np.float64, np.int16


def quantise(x):
    """(d, scl, offs) of a float64 cube, per (fold, part, sub-band): the codes span
    -32767..32767 and the decoded cube is within a few 1e-6 relative of x."""
    mx, mn = x.max(axis=-1), x.min(axis=-1)
    offs = ((mx + mn) / 2).astype(f4)
    scl = ((mx - mn) / 65534).astype(f4)
    scl[scl == 0] = 1
    d = np.clip(np.rint((x - offs[..., None]) / scl[..., None]), -32768, 32767).astype(i2)
    return d, scl, offs


def decode(d, scl, offs, wts=None):
    """The reference cube: numpy, in float64."""
    x64 = d.astype(f8) * scl.astype(f8)[..., None] + offs.astype(f8)[..., None]
    if wts is not None:
        x64 = x64 * wts.astype(f8)[..., None]
    return x64


def weights(shape4, seed=7):
    """Random float32 weights in (0, 1], every seventh (fold, part, sub-band) zapped."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.05, 1.0, size=shape4[:3]).astype(f4)
    w.reshape(-1)[::7] = 0.0
    return w


_blocks = {}


def block(shape, n):
    """(d, scl, offs, wts, subfreqs, scal) of n quantised synthetic folds of `shape`, built once."""
    key = (shape, n)
    if key not in _blocks:
        profs, subfreqs, scal = pfd.batch_inputs(pfd_fold_block(n, shape, 20261021))
        d, scl, offs = quantise(profs)
        assert d.min() >= -32767 and d.max() == 32767
        # the folds keep their pulses: half a code (range / 131068) and the float32 roundings
        # of scl (times a code of at most 2^15) and offs
        rng = profs.max(axis=-1) - profs.min(axis=-1)
        bound = rng / 131068 + 2.0 ** -23 * (rng + np.abs(profs).max(axis=-1))
        assert (np.abs(decode(d, scl, offs) - profs) <= bound[..., None]).all()
        ins = (d, scl, offs, weights(d.shape), subfreqs, scal)
        for a in ins:
            a.setflags(write=False)
        _blocks[key] = ins
    return _blocks[key]


_refs = {}


def ref(engine, call, shape, n, weighted, opts=()):
    """The f64 call `call` (a method name) on the decoded block, computed once per route."""
    key = (call, shape, n, weighted, tuple(sorted(dict(opts).items())))
    if key not in _refs:
        d, scl, offs, wts, fr, sc = block(shape, n)
        with engine.options(**dict(opts)):
            _refs[key] = getattr(engine, call)(decode(d, scl, offs, wts if weighted else None), fr, sc)
    return _refs[key]


def same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    assert np.array_equal(got, want, equal_nan=True), tag


def same_dmprof(got, want, tag):
    for k in ("profile", "chis", "lyon8", "status"):
        same(got[k], want[k], f"{tag}: {k}")


def same_scores(got, want, tag):
    same(got[0], want[0], f"{tag}: out")
    same(got[1], want[1], f"{tag}: status")


def same_any(got, want, tag):
    (same_dmprof if isinstance(want, dict) else same_scores)(got, want, tag)


# route, handle options, (npart, nsub, proflen), n
ROUTES = [
    ("four_wave_pow2", {}, (7, 8, 64), 5),
    ("four_wave_pow2_128", {}, (4, 16, 128), 5),
    ("four_wave_generic", {}, (3, 5, 33), 67),   # E = 165: 2-byte loads, quads across folds
    ("single_wave_long", {}, (2, 4, 200), 3),
    ("single_wave_option", {"pfd_waves": 1}, (3, 5, 33), 67),
    ("slab_by_shape", {}, (2, 128, 256), 3),
    ("slab_option", {"pfd_global": 1}, (3, 5, 33), 67),
    ("split", {"pfd_split": 1}, (4, 16, 128), 5),
    ("one_part", {}, (1, 2, 8), 1),
]


@pytest.mark.parametrize("route,opts,shape,n", ROUTES, ids=[r[0] for r in ROUTES])
def test_routes(engine, route, opts, shape, n):
    d, scl, offs, wts, fr, sc = block(shape, n)
    for weighted in (False, True):
        kw = dict(scl=scl, offs=offs, wts=wts if weighted else None)
        want_d = ref(engine, "pfd_dmprof", shape, n, weighted, opts)
        want_s = ref(engine, "pfd_bates22", shape, n, weighted, opts)
        with engine.options(**opts):
            same_dmprof(engine.pfd_dmprof(d, fr, sc, **kw), want_d, f"{route} w={weighted}")
            same_scores(engine.pfd_bates22(d, fr, sc, **kw), want_s, f"{route} w={weighted}")


@pytest.mark.parametrize("shape,n", [((7, 8, 64), 5), ((3, 5, 33), 67)], ids=["7x8x64", "3x5x33"])
def test_group_calls(engine, shape, n):
    d, scl, offs, wts, fr, sc = block(shape, n)
    for name in ("pfd_params4", "pfd_dmfit4", "pfd_subband3"):
        for weighted in (False, True):
            got = getattr(engine, name)(d, fr, sc, scl=scl, offs=offs, wts=wts if weighted else None)
            same_scores(got, ref(engine, name, shape, n, weighted), f"{name} w={weighted}")


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def _host(r):
    """Device results as the host path returns them (status as uint32)."""
    if isinstance(r, dict):
        r = {k: v.cpu().numpy() for k, v in r.items()}
        r["status"] = r["status"].view(np.uint32)
        return r
    return r[0].cpu().numpy(), r[1].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape,n", [((7, 8, 64), 5), ((3, 5, 33), 67)], ids=["7x8x64", "3x5x33"])
def test_device_tensors_carry_the_host_bits(engine, shape, n):
    d, scl, offs, wts, fr, sc = block(shape, n)
    td, tfr, tsc = _dev(d), _dev(fr), _dev(sc)
    for weighted in (False, True):
        kw = dict(scl=_dev(scl), offs=_dev(offs), wts=_dev(wts) if weighted else None)
        got = [engine.pfd_dmprof(td, tfr, tsc, **kw), engine.pfd_bates22(td, tfr, tsc, **kw),
               engine.pfd_subband3(td, tfr, tsc, **kw)]
        engine.synchronize()
        for g, name in zip(got, ("pfd_dmprof", "pfd_bates22", "pfd_subband3")):
            same_any(_host(g), ref(engine, name, shape, n, weighted), f"device {name} w={weighted}")


def test_int16_cubes_reach_the_i16_entry_points(engine, monkeypatch):
    """Nothing decodes an int16 cube on the way: the f64 and f32 entry points are not called."""
    d, scl, offs, wts, fr, sc = block((1, 2, 8), 1)

    def other_entry(*a):
        raise AssertionError("an int16 cube went to another entry point")

    for name in ("pfe_pfd_dmprof", "pfe_pfd_bates22", "pfe_pfd_params4", "pfe_pfd_dmfit4",
                 "pfe_pfd_subband3", "pfe_pfd_avgprof"):
        monkeypatch.setattr(engine.lib, name, other_entry)
        monkeypatch.setattr(engine.lib, name + "_f32", other_entry)
    engine.pfd_dmprof(d, fr, sc, scl=scl, offs=offs)
    for call in (engine.pfd_bates22, engine.pfd_params4, engine.pfd_dmfit4, engine.pfd_subband3):
        call(d, fr, sc, scl=scl, offs=offs, wts=wts)
    engine.pfd_avgprof(d, scl=scl, offs=offs)
    engine.synchronize()


def test_data_two_bytes_past_an_8_byte_boundary(engine):
    """A slice of a larger tensor: nsub x proflen is a multiple of 4, the base is not 8-byte
    aligned, so the 2-byte loads run where the 8-byte ones would."""
    import torch

    shape, n = (7, 8, 64), 5
    d, scl, offs, wts, fr, sc = block(shape, n)
    big = torch.zeros(d.size + 4, dtype=torch.int16, device="cuda")
    assert big.data_ptr() % 8 == 0
    cube = big[1:1 + d.size].view(d.shape)
    cube.copy_(_dev(d))
    assert cube.data_ptr() % 8 == 2 and cube.is_contiguous()
    got = engine.pfd_dmprof(cube, _dev(fr), _dev(sc), scl=_dev(scl), offs=_dev(offs), wts=_dev(wts))
    engine.synchronize()
    same_dmprof(_host(got), ref(engine, "pfd_dmprof", shape, n, True), "offset cube")


@pytest.mark.parametrize("shape,n", [((3, 5, 33), 5), ((7, 8, 64), 5)], ids=["3x5x33", "7x8x64"])
def test_weights(engine, shape, n):
    d, scl, offs, wts, fr, sc = block(shape, n)
    assert (wts == 0).any() and (wts != 0).any()
    ones = np.ones_like(wts)
    none_d = engine.pfd_dmprof(d, fr, sc, scl=scl, offs=offs)
    none_s = engine.pfd_bates22(d, fr, sc, scl=scl, offs=offs)
    same_dmprof(none_d, ref(engine, "pfd_dmprof", shape, n, False), "no weights")
    # weights of 1.0 change nothing on finite data
    assert np.isfinite(decode(d, scl, offs)).all()
    same_dmprof(engine.pfd_dmprof(d, fr, sc, scl=scl, offs=offs, wts=ones), none_d, "all ones")
    same_scores(engine.pfd_bates22(d, fr, sc, scl=scl, offs=offs, wts=ones), none_s, "all ones")
    # random weights, some sub-bands zapped: the reference decides what the scores are
    same_dmprof(engine.pfd_dmprof(d, fr, sc, scl=scl, offs=offs, wts=wts),
                ref(engine, "pfd_dmprof", shape, n, True), "zapped")
    same_scores(engine.pfd_bates22(d, fr, sc, scl=scl, offs=offs, wts=wts),
                ref(engine, "pfd_bates22", shape, n, True), "zapped")
    # one NaN and one infinite weight
    w = np.array(wts)
    w[1, 0, 1], w[2, shape[0] - 1, 2] = np.nan, np.inf
    got = engine.pfd_dmprof(d, fr, sc, scl=scl, offs=offs, wts=w)
    want = engine.pfd_dmprof(decode(d, scl, offs, w), fr, sc)
    same_dmprof(got, want, "NaN and inf weight")
    assert np.isnan(got["profile"][1]).any()
    same(got["profile"][3:], ref(engine, "pfd_dmprof", shape, n, True)["profile"][3:], "untouched folds")


def test_value_edges(engine):
    """The ends of the int16 range, scales of 0, negative, the smallest subnormal and the largest
    finite float32, offsets of -0.0, infinity and NaN, each in a chosen element."""
    shape, n = (3, 5, 33), 5
    d0, scl0, offs0, wts, fr, sc = block(shape, n)
    d, scl, offs = np.array(d0), np.array(scl0), np.array(offs0)
    d[0, 0, 0, 0], d[0, 0, 0, 1], d[0, 0, 0, 2] = -32768, 32767, 0
    d[0, 1, 4, 32], d[0, 2, 4, 32] = -32768, -32768
    scl[0, 0, 1] = 0.0
    scl[0, 1, 2] = -scl[0, 1, 2]
    scl[1, 0, 3] = np.float32(1e-45)
    assert scl[1, 0, 3] > 0 and scl[1, 0, 3] == np.finfo(f4).smallest_subnormal
    offs[0, 0, 1] = -0.0            # 0 * d + -0.0, in every bin of the sub-band
    offs[1, :, 4] = -0.0
    scl[1, :, 4] = 0.0              # every part -0.0 or +0.0 as numpy's d * 0.0 + -0.0 has it
    for weighted in (False, True):
        w = wts if weighted else None
        x64 = decode(d, scl, offs, w)
        assert np.isfinite(x64).all()
        kw = dict(scl=scl, offs=offs, wts=w)
        same_dmprof(engine.pfd_dmprof(d, fr, sc, **kw), engine.pfd_dmprof(x64, fr, sc), f"finite w={weighted}")
        same_scores(engine.pfd_bates22(d, fr, sc, **kw), engine.pfd_bates22(x64, fr, sc), f"finite w={weighted}")
    # values no float32 holds, and the non-finite ones
    scl[2, 0, 0] = np.finfo(f4).max
    d[2, 0, 0, :4] = (32767, -32768, 0, 1)
    offs[3, 1, 1] = np.inf
    offs[3, 2, 2] = -np.inf
    offs[4, 2, 3] = np.nan
    scl[4, 0, 0], offs[4, 0, 0] = np.inf, -np.inf
    for weighted in (False, True):
        w = wts if weighted else None
        with np.errstate(invalid="ignore"):
            x64 = decode(d, scl, offs, w)
        assert np.abs(x64[2, 0, 0, 0]) > 1e42 or weighted
        got, want = engine.pfd_dmprof(d, fr, sc, scl=scl, offs=offs, wts=w), engine.pfd_dmprof(x64, fr, sc)
        same_dmprof(got, want, f"non-finite w={weighted}")
        for k in ("profile", "chis", "lyon8"):
            assert np.array_equal(np.isinf(got[k]), np.isinf(want[k])), k
            assert np.array_equal(np.signbit(got[k]) & ~np.isnan(got[k]),
                                  np.signbit(want[k]) & ~np.isnan(want[k])), k


# ---- the rows of a binary table ---------------------------------------------------------------
def table(d, scl, offs, wts, fr, order, pad, align):
    """An (n x npart)-row structured array shaped like a PSRFITS SUBINT table: one row per
    sub-integration, `order` '>' (as the file holds it) or '<'.  align: numpy's aligned layout
    (the row padded to a multiple of 8 bytes); pad: that many bytes more behind the columns."""
    n, npart, nsub, L = d.shape
    fields = [("TSUBINT", order + "f8"), ("DAT_FREQ", order + "f4", (nsub,)),
              ("DAT_WTS", order + "f4", (nsub,)), ("DAT_OFFS", order + "f4", (nsub,)),
              ("DAT_SCL", order + "f4", (nsub,)), ("DATA", order + "i2", (nsub, L))]
    if pad:
        fields.append(("PAD", "u1", (pad,)))
    dt = np.dtype(fields, align=align)
    t = np.zeros(n * npart, dtype=dt)
    t["TSUBINT"] = 10.0
    t["DAT_FREQ"] = np.repeat(fr, npart, axis=0)
    t["DAT_WTS"] = wts.reshape(n * npart, nsub)
    t["DAT_OFFS"] = offs.reshape(n * npart, nsub)
    t["DAT_SCL"] = scl.reshape(n * npart, nsub)
    t["DATA"] = d.reshape(n * npart, nsub, L)
    if pad:
        t["PAD"] = 0xA5
    return t


def column(buf, dt, name, torch_dtype, shape):
    """A strided view of the uploaded bytes `buf`: column `name` of every row as (n, npart, ...)."""
    n, npart = shape[:2]
    off, es, row = dt.fields[name][1], torch_dtype.itemsize, dt.itemsize
    assert off % es == 0 and row % es == 0
    flat = buf[off:]
    flat = flat[: flat.numel() // es * es].view(torch_dtype)
    inner = shape[2:]
    istr = tuple(int(np.prod(inner[i + 1:])) for i in range(len(inner)))
    return flat.as_strided(tuple(shape), (npart * row // es, row // es) + istr)


# (npart, nsub, proflen), n, padding bytes, numpy-aligned rows.  3x5x33: the columns need 418
# bytes, which is no multiple of 4; the aligned layout makes the row 424.  4x16x128: 4360 bytes
# (a multiple of 8: the 8-byte loads run through the strides); + 4: a row of 4364, which puts
# every second row's data off the 8-byte grid (2-byte loads) and leaves bytes no column owns
TABLES = [((3, 5, 33), 4, 0, True), ((4, 16, 128), 3, 0, False), ((4, 16, 128), 3, 4, False),
          ((3, 5, 33), 4, 16, True)]


@pytest.mark.parametrize("shape,n,pad,align", TABLES,
                         ids=[f"{'x'.join(map(str, s))}_pad{p}" for s, _n, p, _a in TABLES])
def test_table_rows(engine, shape, n, pad, align):
    import torch

    d, scl, offs, wts, fr, sc = (a[:n] for a in block(shape, 5 if shape != (3, 5, 33) else 67))
    x64 = decode(d, scl, offs, wts)
    want_d, want_s = engine.pfd_dmprof(x64, fr, sc), engine.pfd_bates22(x64, fr, sc)
    want_a = np.array([(f / shape[2]).sum() for f in x64])
    tfr, tsc = _dev(fr), _dev(sc)
    npart, nsub, L = shape
    for order, swapped in ((">", True), ("<", False)):
        t = table(d, scl, offs, wts, fr, order, pad, align)
        row = t.dtype.itemsize
        assert row % 4 == 0 and row >= 8 + 16 * nsub + 2 * nsub * L + pad
        raw = t.view(np.uint8).reshape(-1)
        buf = torch.from_numpy(raw.copy()).cuda()          # the table's bytes, uploaded once
        cd = column(buf, t.dtype, "DATA", torch.int16, (n, npart, nsub, L))
        kw = dict(scl=column(buf, t.dtype, "DAT_SCL", torch.float32, (n, npart, nsub)),
                  offs=column(buf, t.dtype, "DAT_OFFS", torch.float32, (n, npart, nsub)),
                  wts=column(buf, t.dtype, "DAT_WTS", torch.float32, (n, npart, nsub)),
                  byteswapped=swapped)
        assert not cd.is_contiguous() and cd.stride(1) * 2 == row
        got_d = engine.pfd_dmprof(cd, tfr, tsc, **kw)
        got_s = engine.pfd_bates22(cd, tfr, tsc, **kw)
        got_g = engine.pfd_dmfit4(cd, tfr, tsc, derive_avgprof=True, **kw)
        got_a = engine.pfd_avgprof(cd, **kw)
        engine.synchronize()
        same_dmprof(_host(got_d), want_d, f"table {order}")
        same_scores(_host(got_s), want_s, f"table {order}")
        same(got_a.cpu().numpy(), want_a, f"table {order}: average")
        sc2 = np.array(sc)
        sc2[:, PFE_PFD_AVGPROF] = want_a
        same_scores(_host(got_g), engine.pfd_dmfit4(x64, fr, sc2), f"table {order}: derived")
        assert np.array_equal(buf.cpu().numpy(), raw), "the table was written to"
        # without the weights column: wts=None
        kw["wts"] = None
        got = engine.pfd_dmprof(cd, tfr, tsc, **kw)
        engine.synchronize()
        same_dmprof(_host(got), engine.pfd_dmprof(decode(d, scl, offs), fr, sc), f"table {order} no wts")


@pytest.mark.parametrize("chunk", [1, 2, 64])
def test_chunk_seams(engine, chunk):
    """PFE_OPT_PFD_F32_CHUNK governs this path too: passes of 1, 2 and (cut to n) 5 of n = 5 folds
    give the bits of the default's single pass."""
    shape, n = (3, 5, 33), 5
    d, scl, offs, wts, fr, sc = block(shape, n)
    kw = dict(scl=scl, offs=offs, wts=wts)
    names = ("pfd_dmprof", "pfd_bates22", "pfd_dmfit4", "pfd_subband3", "pfd_params4")
    assert engine.get_option("pfd_f32_chunk") == 0
    want = [getattr(engine, c)(d, fr, sc, **kw) for c in names]
    for c, w in zip(names, want):
        same_any(w, ref(engine, c, shape, n, True), f"default pass {c}")
    derived = [getattr(engine, c)(d, fr, sc, derive_avgprof=True, **kw) for c in names[:3]]
    with engine.options(pfd_f32_chunk=chunk):
        assert engine.get_option("pfd_f32_chunk") == chunk
        for c, w in zip(names, want):
            same_any(getattr(engine, c)(d, fr, sc, **kw), w, f"chunk {chunk} {c}")
        for c, w in zip(names, derived):
            same_any(getattr(engine, c)(d, fr, sc, derive_avgprof=True, **kw), w,
                     f"chunk {chunk} {c} derived")
        for o in ({"pfd_global": 1}, {"pfd_split": 1}):  # slabs / part-sum buffers per pass
            with engine.options(**o):
                same_dmprof(engine.pfd_dmprof(d, fr, sc, **kw), want[0], f"chunk {chunk} {o}")
    assert engine.get_option("pfd_f32_chunk") == 0


# one fold of more than 8192 values (a chunk of numpy's that spans parts), one whose E = 495 is
# no multiple of 8, and the power-of-two proflen beside the divide
@pytest.mark.parametrize("shape,n", [((3, 32, 128), 2), ((3, 5, 33), 5), ((7, 8, 64), 5)],
                         ids=["3x32x128", "3x5x33", "7x8x64"])
def test_derived_average(engine, shape, n):
    d, scl, offs, wts, fr, sc = block(shape, n)
    assert shape != (3, 32, 128) or int(np.prod(shape)) > 8192
    assert shape != (3, 5, 33) or int(np.prod(shape)) % 8
    for weighted in (False, True):
        w = wts if weighted else None
        kw = dict(scl=scl, offs=offs, wts=w)
        x64 = decode(d, scl, offs, w)
        want = np.array([(f / shape[2]).sum() for f in x64])
        avg = engine.pfd_avgprof(d, **kw)
        same(avg, want, f"average w={weighted}")
        dkw = dict(scl=_dev(scl), offs=_dev(offs), wts=_dev(w) if weighted else None)
        davg = engine.pfd_avgprof(_dev(d), **dkw)
        engine.synchronize()
        same(davg.cpu().numpy(), want, f"device average w={weighted}")
        sc_nan = np.array(sc)
        sc_nan[:, PFE_PFD_AVGPROF] = np.nan         # not read under the flag
        sc_avg = np.array(sc)
        sc_avg[:, PFE_PFD_AVGPROF] = avg
        for name in ("pfd_dmprof", "pfd_bates22", "pfd_params4", "pfd_dmfit4", "pfd_subband3"):
            call = getattr(engine, name)
            same_any(call(d, fr, sc_nan, derive_avgprof=True, **kw), call(d, fr, sc_avg, **kw),
                     f"{name} w={weighted}")
        got = engine.pfd_bates22(_dev(d), _dev(fr), _dev(sc_nan), derive_avgprof=True, **dkw)
        engine.synchronize()
        same_scores(_host(got), engine.pfd_bates22(x64, fr, sc_avg), f"device derived w={weighted}")


def test_inputs_are_not_written(engine):
    shape, n = (3, 5, 33), 5
    ins = [np.array(a) for a in block(shape, n)]
    keep = [a.copy() for a in ins]
    d, scl, offs, wts, fr, sc = ins
    t = [_dev(a) for a in ins]
    for swapped in (False, True):
        kw = dict(scl=scl, offs=offs, wts=wts, byteswapped=swapped, derive_avgprof=True)
        dkw = dict(scl=t[1], offs=t[2], wts=t[3], byteswapped=swapped, derive_avgprof=True)
        engine.pfd_dmprof(d, fr, sc, **kw)
        engine.pfd_bates22(d, fr, sc, **kw)
        engine.pfd_dmprof(t[0], t[4], t[5], **dkw)
        engine.pfd_bates22(t[0], t[4], t[5], **dkw)
    engine.pfd_avgprof(d, scl=scl, offs=offs, wts=wts)
    engine.pfd_avgprof(t[0], scl=t[1], offs=t[2], wts=t[3])
    engine.synchronize()
    for a, k, dev in zip(ins, keep, t):
        assert a.tobytes() == k.tobytes()
        assert dev.cpu().numpy().tobytes() == k.tobytes()


def test_byteswapped_dense_arrays(engine):
    """PFE_FLAG_PFD_BSWAP on dense host arrays: 2-byte and 4-byte values reversed, same bits."""
    shape, n = (3, 5, 33), 5
    d, scl, offs, wts, fr, sc = block(shape, n)
    kw = dict(scl=scl.byteswap(), offs=offs.byteswap(), wts=wts.byteswap(), byteswapped=True)
    same_dmprof(engine.pfd_dmprof(d.byteswap(), fr, sc, **kw), ref(engine, "pfd_dmprof", shape, n, True), "swapped")
    same_scores(engine.pfd_bates22(d.byteswap(), fr, sc, **kw), ref(engine, "pfd_bates22", shape, n, True),
                "swapped")


# ---- refusals ---------------------------------------------------------------------------------
def _raw(engine, name, flags, **over):
    """pfe_<name>_i16 on device arrays of 2 folds of 3 x 5 x 33 lying in rows of 424 bytes, with
    fields of the struct replaced -> the PfeError text.  Every case is refused before any launch."""
    import torch

    npart, nsub, L, n, row = 3, 5, 33, 2, 424
    buf = torch.zeros(n * npart * row + 64, dtype=torch.uint8, device="cuda")
    fr, sc = torch.zeros((n, nsub), dtype=torch.float64, device="cuda"), torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    out = torch.zeros((n, 22), dtype=torch.float64, device="cuda")
    st = torch.zeros((n,), dtype=torch.int32, device="cuda")
    base = buf.data_ptr()
    assert base % 8 == 0
    f = dict(data=base + 88, scl=base + 68, offs=base + 48, wts=base + 28, fold_stride=npart * row,
             part_stride=row, subfreqs=fr.data_ptr(), scal=sc.data_ptr(), npart=npart, nsub=nsub,
             proflen=L, n=n)
    f.update(over)
    pin = PfdI16In(**f)
    fn = getattr(engine.lib, f"pfe_{name}_i16")
    if name == "pfd_dmprof":
        rc = fn(engine._h, C.byref(pin), None, None, out.data_ptr(), st.data_ptr(), flags)
    elif name == "pfd_avgprof":
        rc = fn(engine._h, C.byref(pin), out.data_ptr(), 1, flags)
    else:
        rc = fn(engine._h, C.byref(pin), out.data_ptr(), st.data_ptr(), flags)
    assert rc != 0, (name, over)
    with pytest.raises(PfeError) as e:
        engine._check(rc)
    engine.synchronize()
    assert f"{name}_i16:" in str(e.value)
    return str(e.value)


CALLS = ("pfd_dmprof", "pfd_bates22", "pfd_params4", "pfd_dmfit4", "pfd_subband3", "pfd_avgprof")


@pytest.mark.parametrize("name", CALLS)
def test_refused_strides_and_alignment(engine, name):
    D = PFE_FLAG_DEVICE_PTRS
    for over in (dict(fold_stride=0), dict(part_stride=0)):
        assert "both 0 (dense arrays) or both non-zero" in _raw(engine, name, D, **over)
    assert "part_stride 328 must be >= 2 x nsub x proflen = 330" in _raw(engine, name, D, part_stride=328)
    assert "a multiple of 4" in _raw(engine, name, D, part_stride=426, fold_stride=3 * 426)
    assert "fold_stride 1268 must be >= npart x part_stride" in _raw(engine, name, D, fold_stride=1268)
    assert "fold_stride 1274" in _raw(engine, name, D, fold_stride=1274)
    assert "both 0" in _raw(engine, name, D | PFE_FLAG_PFD_BSWAP, part_stride=0)


@pytest.mark.parametrize("name", CALLS)
def test_refused_pointers(engine, name):
    import torch

    D = PFE_FLAG_DEVICE_PTRS
    probe = torch.zeros(64, dtype=torch.uint8, device="cuda").data_ptr()
    assert "data not 2-byte aligned" in _raw(engine, name, D, data=probe + 1)
    assert "4-byte aligned" in _raw(engine, name, D, scl=probe + 2)
    assert "4-byte aligned" in _raw(engine, name, D, wts=probe + 6)
    assert "null input array" in _raw(engine, name, D, offs=None)
    # strides with host pointers
    assert "strided input is for device pointers" in _raw(engine, name, 0)


def test_null_struct_is_refused_under_the_i16_name(engine):
    import torch

    out = torch.zeros((2, 22), dtype=torch.float64, device="cuda")
    st = torch.zeros((2,), dtype=torch.int32, device="cuda")
    D = PFE_FLAG_DEVICE_PTRS
    for name in CALLS:
        fn = getattr(engine.lib, f"pfe_{name}_i16")
        if name == "pfd_dmprof":
            rc = fn(engine._h, None, None, None, out.data_ptr(), st.data_ptr(), D)
        elif name == "pfd_avgprof":
            rc = fn(engine._h, None, out.data_ptr(), 1, D)
        else:
            rc = fn(engine._h, None, out.data_ptr(), st.data_ptr(), D)
        assert rc != 0
        assert engine.lib.pfe_last_error(engine._h).decode() == f"{name}_i16: null argument"
    engine.synchronize()


def test_refused_by_the_binding(engine):
    shape, n = (3, 5, 33), 5
    d, scl, offs, wts, fr, sc = block(shape, n)
    x64 = decode(d, scl, offs)
    for call in (engine.pfd_dmprof, engine.pfd_bates22, engine.pfd_params4, engine.pfd_dmfit4,
                 engine.pfd_subband3):
        with pytest.raises(ValueError, match="scl and offs are required with an int16 cube"):
            call(d, fr, sc)
        with pytest.raises(ValueError, match="scl and offs are required"):
            call(d, fr, sc, offs=offs)
        with pytest.raises(ValueError, match="go with an int16 cube"):
            call(x64, fr, sc, scl=scl, offs=offs)
        with pytest.raises(ValueError, match="go with an int16 cube"):
            call(x64.astype(f4), fr, sc, wts=wts)
        with pytest.raises(ValueError, match=r"scl must be \(n,npart,nsub\)"):
            call(d, fr, sc, scl=scl[:, :, :4], offs=offs)
        with pytest.raises(ValueError, match="host arrays must be dense"):
            call(np.asfortranarray(d), fr, sc, scl=scl, offs=offs)
    with pytest.raises(ValueError, match="scl and offs are required"):
        engine.pfd_avgprof(d)
    with pytest.raises(ValueError, match="go with an int16 cube"):
        engine.pfd_avgprof(x64, scl=scl, offs=offs)
    # device views that do not agree on the strides
    td, ts, to = _dev(d), _dev(scl), _dev(offs)
    wide = _dev(np.zeros((n, 3, 2 * 5), dtype=f4))[:, :, :5]
    assert not wide.is_contiguous()
    with pytest.raises(ValueError, match="share one fold stride and one part stride"):
        engine.pfd_dmprof(td, _dev(fr), _dev(sc), scl=wide, offs=to)
    with pytest.raises(ValueError, match="must be dense"):
        engine.pfd_dmprof(td, _dev(fr), _dev(sc), scl=_dev(np.zeros((n, 3, 10), dtype=f4))[:, :, ::2], offs=to)
    del ts


def test_shape_limits_are_those_of_the_f64_calls(engine):
    fr1, sc = np.full((1, 1), 1400.0), np.ones((1, 8))
    one, p1 = np.ones((1, 1, 1, 1), dtype=i2), np.ones((1, 1, 1), dtype=f4)
    with pytest.raises(PfeError, match=r"pfd_dmprof_i16: shape 1x1x1"):
        engine.pfd_dmprof(one, fr1, sc, scl=p1, offs=p1)
    with pytest.raises(PfeError, match=r"pfd_dmprof: shape 1x1x1"):
        engine.pfd_dmprof(one.astype(f8), fr1, sc)
    fr2 = np.full((1, 2), 1400.0)
    long_, p2 = np.ones((1, 1, 2, 1025), dtype=i2), np.ones((1, 1, 2), dtype=f4)
    for name in ("pfd_bates22", "pfd_params4", "pfd_dmfit4", "pfd_subband3"):
        with pytest.raises(PfeError, match=name + "_i16: shape 1x2x1025 unsupported"):
            getattr(engine, name)(long_, fr2, sc, scl=p2, offs=p2)
        with pytest.raises(PfeError, match=name + ": shape 1x2x1025 unsupported"):
            getattr(engine, name)(long_.astype(f8), fr2, sc)
