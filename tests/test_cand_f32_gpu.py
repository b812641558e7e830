"""The float32 forms of the float-array calls (pfe_lyon8_f32, pfe_sinusoid4_f32, pfe_gauss7_f32,
pfe_subband3_f32, pfe_bates22_f32) against the contract include/pfe.h states: every value a
call returns and its status are, bit for bit, those of the f64 call of the same name on the
same arrays widened value by value.

The reference is always the existing f64 call on x32.astype(float64) (.double() for tensors)
-- never the call under test.  Inputs are built in float32 first.  Where no NaN is expected
the bar is array_equal on the uint64 view; elsewhere the NaN mask and the bits of every other
value.  Two CPU anchors (oracle.lyon, oracle.bates on the widened arrays) hold the float32
calls to the bars include/pfe.h states for the f64 calls."""
import numpy as np
import pytest

from pulsarfeatureextractor_amd._native import PfeError
from pulsarfeatureextractor_amd.synth import bates_batch
from test_cand_f32_host import anchor_batch
from test_subband_f64_gpu import adversarial, float_batch, oracle_sub, rel

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
FAIL = 0x008


def wide(a):
    return np.asarray(a).astype(np.float64)


def same_bits(got, want, tag, nan=False):
    """nan False: no NaN anywhere and equal bits.  nan True: the same NaN mask, equal bits
    elsewhere."""
    got = np.ascontiguousarray(np.asarray(got), dtype=np.float64)
    want = np.ascontiguousarray(np.asarray(want), dtype=np.float64)
    assert got.shape == want.shape, tag
    gn, wn = np.isnan(got), np.isnan(want)
    if not nan:
        assert not gn.any() and not wn.any(), f"{tag}: NaN where none is expected"
    assert np.array_equal(gn, wn), f"{tag}: NaN mask differs at {np.argwhere(gn != wn)[:8].tolist()}"
    g, w = got.view(np.uint64), want.view(np.uint64)
    bad = (g != w) & ~wn
    assert not bad.any(), f"{tag}: bits differ at {np.argwhere(bad)[:8].tolist()}"


def same_scores(got, want, tag, nan=True):
    same_bits(got[0], want[0], f"{tag}: out", nan=nan)
    gs, ws = (np.asarray(x).view(np.uint32) for x in (got[1], want[1]))
    assert np.array_equal(gs, ws), f"{tag}: status"


def dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ---- Lyon-8 ------------------------------------------------------------------------------------
_rows = {}


def rows32(L, n=17, seed=0):
    """n float32 rows of L values, N(100, 10) with a pulse; built once per length."""
    key = (L, n, seed)
    if key not in _rows:
        rng = np.random.default_rng(20261021 + 7 * L + seed)
        r = rng.normal(100.0, 10.0, (n, L))
        r[:, L // 3] += 60.0
        r = r.astype(np.float32)
        r.setflags(write=False)
        _rows[key] = r
    return _rows[key]


# 1, 7, 8, 9: the leaf's short form and its remainder; 127-136: the first split at floor8(n/2);
# 968 | 969: inlined | called tree; 8192 | 8193: numpy's buffer seam
@pytest.mark.parametrize("L", [1, 7, 8, 9, 127, 128, 129, 136, 968, 969, 8192, 8193])
def test_lyon8_lengths_and_row_counts(engine, L):
    p, d = rows32(L), rows32(L, seed=1)
    for n in (1, 7, 8, 9, 17):  # eight rows per wave: idle groups redo the last row
        got = engine.lyon8(p[:n], d[:n])
        assert got.shape == (n, 8)
        same_bits(got, engine.lyon8(wide(p[:n]), wide(d[:n])), f"L={L} n={n}", nan=L == 1)


def at_offset(a, extra_floats, pad=0, tensor=False):
    """A copy of the 2-D float32 array `a` whose first element lies extra_floats floats past a
    16-byte boundary and whose row stride is its row length + pad (numpy view or device
    tensor)."""
    n, L = a.shape
    stride = L + pad
    if tensor:
        import torch

        flat = torch.zeros(n * stride + 8, dtype=torch.float32, device="cuda")
        assert flat.data_ptr() % 16 == 0
        v = flat[extra_floats:extra_floats + n * stride].as_strided((n, L), (stride, 1))
        v.copy_(torch.from_numpy(np.array(a)))
        assert v.data_ptr() % 16 == 4 * extra_floats
        return v
    buf = np.zeros(n * stride + 8, dtype=np.float32)
    off = (-(buf.ctypes.data // 4) % 4 + extra_floats) % 4
    v = np.lib.stride_tricks.as_strided(buf[off:], (n, L), (4 * stride, 4))
    v[...] = a
    assert v.ctypes.data % 16 == 4 * extra_floats
    return v


@pytest.mark.parametrize("tensor", [False, True], ids=["host", "device"])
def test_lyon8_layouts(engine, tensor):
    """Row strides beyond the length, an odd stride (every second row 4 bytes off an 8-byte
    boundary), a base pointer one float past a 16-byte boundary; host arrays and device tensors."""
    p, d = rows32(129, n=9), rows32(100, n=9)
    want = engine.lyon8(wide(p), wide(d))
    for extra, pp, dp in ((0, 0, 0), (0, 7, 3), (0, 2, 1), (1, 0, 0), (1, 2, 5), (3, 4, 0)):
        a, b = at_offset(p, extra, pp, tensor), at_offset(d, extra, dp, tensor)
        got = engine.lyon8(a, b)
        if tensor:
            engine.synchronize()
            got = host(got)
        same_bits(got, want, f"offset {extra} pads {pp},{dp} tensor={tensor}")


def special_rows(L):
    rng = np.random.default_rng(5 + L)
    base = rng.normal(100.0, 10.0, L).astype(np.float32)
    rows, names = [], []

    def add(name, r):
        names.append(name)
        rows.append(np.asarray(r, dtype=np.float32))

    # scipy's zero-variance rule, m2 <= (eps * mean)^2.  A constant float32 row is always on its
    # NaN side: L copies of a 24-bit value sum exactly in float64 for every L < 2^29, so numpy's
    # mean is the value itself and m2 = 0 -- the float64 rows whose mean lands an ulp off
    # (synth.f64_edge_rows) do not survive the rounding to float32.  The other side is reached
    # by the least a float32 row can vary: one value, or every second one, a float32 ulp up.
    for c in (1.0, 0.5, 0.1, 3.3, 1e9, 16777217.0, -7.7):
        add(f"const_{c}", np.full(L, c))
    for c in (0.1, 1e9, -7.7):
        r = np.full(L, c, dtype=np.float32)
        r[L // 2] = np.nextafter(r[0], np.float32(np.inf))
        add(f"step_one_{c}", r)
        r = np.full(L, c, dtype=np.float32)
        r[1::2] = np.nextafter(r[0], np.float32(np.inf))
        add(f"step_half_{c}", r)
    add("subnormal", np.full(L, 1e-45))
    r = np.full(L, 1e-45)
    r[::3] = 3e-45
    add("subnormals", r)
    add("zeros", np.zeros(L))
    add("neg_zeros", np.full(L, -0.0))
    r = np.zeros(L)
    r[1::2] = -0.0
    add("mixed_zeros", r)
    add("flt_max", np.full(L, FLT_MAX))
    add("neg_flt_max", np.full(L, -FLT_MAX))
    r = np.full(L, FLT_MAX)
    r[L // 2:] = -FLT_MAX
    add("both_flt_max", r)
    r = base.copy()
    r[L // 2] = np.nan
    add("one_nan", r)
    r = base.copy()
    r[L - 1] = np.inf
    add("one_inf", r)
    r = base.copy()
    r[0] = -np.inf
    add("one_neg_inf", r)
    add("plain", base)
    return np.stack(rows), names


@pytest.mark.parametrize("L", [100, 129, 969])
def test_lyon8_special_rows(engine, L):
    rows, names = special_rows(L)
    assert np.array_equal(rows[names.index("subnormal")].view(np.uint32), np.full(L, 1, np.uint32))
    assert np.signbit(rows[names.index("neg_zeros")]).all()
    other = np.roll(rows, 1, axis=0).copy()
    got = engine.lyon8(rows, other)
    want = engine.lyon8(wide(rows), wide(other))
    same_bits(got, want, f"special rows L={L}", nan=True)
    # what the rows were built to reach: zero variance (NaN skew) and its other side, NaN rows
    nan_skew = dict(zip(names, np.isnan(got[:, 2])))
    assert nan_skew["one_nan"] and nan_skew["one_inf"] and nan_skew["zeros"]
    assert all(v for k, v in nan_skew.items() if k.startswith("const_"))
    assert not any(v for k, v in nan_skew.items() if k.startswith("step_"))
    assert not nan_skew["plain"] and not nan_skew["subnormals"]


@pytest.mark.parametrize("L", [100, 128])
def test_lyon8_cpu_anchor(engine, L):
    """oracle.lyon.lyon8_batched (numpy / scipy) on the widened rows: mean, std and kurtosis the
    same bits, skew within 1e-13 relative -- the bar include/pfe.h states for pfe_lyon8_f64."""
    from oracle.lyon import lyon8_batched

    p, d = rows32(L), rows32(L, seed=1)
    got = engine.lyon8(p, d)
    ref = lyon8_batched(wide(p), wide(d))
    with np.errstate(all="ignore"):
        r = np.abs(got - ref) / np.abs(ref)
    print(f"L={L}: worst rel skew {r[:, [2, 6]].max():.3g}, other columns {r[:, [0, 1, 3, 4, 5, 7]].max():.3g}")
    same_bits(got[:, [0, 1, 3, 4, 5, 7]], ref[:, [0, 1, 3, 4, 5, 7]], f"anchor L={L}")
    assert (r[:, [2, 6]] <= 1e-13).all(), f"skew {r[:, [2, 6]].max():.3g}"


def test_engine_lyon8_takes_float32_and_refuses_mixed(engine):
    p, d = rows32(128), rows32(100)
    assert engine.lyon8(p, d).shape == (17, 8)
    pt, dt = dev(p), dev(d)
    got = engine.lyon8(pt, dt)
    engine.synchronize()
    same_bits(host(got), engine.lyon8(wide(p), wide(d)), "device tensors")
    u8 = np.zeros((17, 128), dtype=np.uint8)
    for a, b in ((u8, d), (p, u8[:, :100]), (wide(p), d), (p, wide(d))):
        with pytest.raises(TypeError):
            engine.lyon8(a, b)
    with pytest.raises(TypeError):
        engine.lyon8(pt, dev(wide(d)))
    with pytest.raises(TypeError):
        engine.lyon8(dev(u8), dt)


# ---- the batch every score test draws from ------------------------------------------------------
_batches = {}


def batch32(n, nsub, lsb, seed, ndm=120, lp=None, adv=True):
    """float_batch (+ adversarial rows) of test_subband_f64_gpu made float32: prof, sub and
    dmcurve float32, scal float64; built once."""
    key = (n, nsub, lsb, seed, ndm, lp, adv)
    if key not in _batches:
        lp_ = lsb if lp is None else lp
        b = float_batch(n, nsub, lsb, seed, lp=lp_)
        if adv:
            b = adversarial(b)
        c = bates_batch(n, lp=lp_, nsub=2, lsb=8, ndm=ndm, seed=seed + 1)
        rng = np.random.default_rng(seed + 5)
        curve = c["dmcurve"] * 0.37 + rng.normal(0, 0.05, c["dmcurve"].shape)
        scal = b["scal"].copy()
        scal[:, 4:7] = c["scal"][:, 4:7]
        out = {"prof": b["prof"].astype(np.float32), "sub": b["sub"].astype(np.float32),
               "dmcurve": curve.astype(np.float32), "scal": scal}
        for a in out.values():
            a.setflags(write=False)
        _batches[key] = out
    return _batches[key]


# ---- sub-bands ---------------------------------------------------------------------------------
# 16 x 128: eight waves a block; 32 x 128: four; 3 x 5: odd total, head and tail floats; 2 x 8;
# 16 x 968 | 16 x 976: inlined | called row sums; 96 x 256: beyond the LDS, the slab
SUB_SHAPES = [(16, 128, 64), (32, 128, 64), (3, 5, 64), (2, 8, 64), (16, 968, 64), (16, 976, 64),
              (96, 256, 8)]


@pytest.mark.parametrize("glob", [0, 1], ids=["default", "subf64_global"])
@pytest.mark.parametrize("nsub,lsb,n", SUB_SHAPES)
def test_subband3_f32_shapes(engine, nsub, lsb, n, glob):
    b = batch32(n, nsub, lsb, seed=4000 + nsub + lsb)
    with engine.options(subf64_global=glob):
        got = engine.subband3_f32(b["prof"], b["sub"], b["scal"])
        want = engine.subband3_f64(wide(b["prof"]), wide(b["sub"]), b["scal"])
    assert ((want[1] & 0xFF) == 0).any() and ((want[1] & 0xFF) != 0).any()
    same_scores(got, want, f"{nsub}x{lsb} global={glob}")


@pytest.mark.parametrize("nsub,lsb", [(3, 5), (16, 128)])
def test_subband3_f32_pointers_and_input_untouched(engine, nsub, lsb):
    """`sub` starting 0, 4, 8 and 12 bytes past a 16-byte boundary (at 3 x 5 each candidate's 15
    floats then start at every alignment in turn); the device input is the same before and after."""
    import torch

    n = 24
    b = batch32(n, nsub, lsb, seed=4100 + lsb)
    want = engine.subband3_f64(wide(b["prof"]), wide(b["sub"]), b["scal"])
    prof, scal = dev(b["prof"]), dev(b["scal"])
    total = n * nsub * lsb
    for k in range(4):
        flat = torch.zeros(total + 4, dtype=torch.float32, device="cuda")
        sub = flat[k:k + total].view(n, nsub, lsb)
        sub.copy_(torch.from_numpy(np.array(b["sub"])))
        assert sub.data_ptr() % 16 == 4 * k and sub.is_contiguous()
        keep = flat.clone()
        for glob in (0, 1):
            with engine.options(subf64_global=glob):
                out, st = engine.subband3_f32(prof, sub, scal)
                engine.synchronize()
            same_scores((host(out), host(st)), want, f"{nsub}x{lsb} +{4 * k} bytes global={glob}")
            assert torch.equal(flat.view(torch.int32), keep.view(torch.int32)), "sub was written"
    assert torch.equal(prof.view(torch.int32), dev(b["prof"]).view(torch.int32)), "prof was written"


def test_subband3_f32_failure_rows(engine):
    """nsub == 1, lp != lsb, width 0, wb > lsb and a NaN width: the f64 call's status and zeros."""
    b = batch32(24, 16, 128, seed=4200)      # adversarial: widths 0, 2.0, NaN in rows 1-3
    want = engine.subband3_f64(wide(b["prof"]), wide(b["sub"]), b["scal"])
    got = engine.subband3_f32(b["prof"], b["sub"], b["scal"])
    same_scores(got, want, "widths")
    assert (got[1][[1, 2, 3]] == FAIL).all() and (got[0][[1, 2, 3]] == 0).all()
    one = batch32(8, 1, 16, seed=4201, adv=False)
    got = engine.subband3_f32(one["prof"], one["sub"], one["scal"])
    same_scores(got, engine.subband3_f64(wide(one["prof"]), wide(one["sub"]), one["scal"]), "nsub 1")
    assert (got[1] == FAIL).all() and (got[0] == 0).all()
    mis = batch32(8, 16, 128, seed=4202, lp=64, adv=False)
    got = engine.subband3_f32(mis["prof"], mis["sub"], mis["scal"])
    same_scores(got, engine.subband3_f64(wide(mis["prof"]), wide(mis["sub"]), mis["scal"]), "lp != lsb")
    assert (got[1] == FAIL).all() and (got[0] == 0).all()


def test_subband3_f32_cpu_anchor(engine):
    """oracle.bates.subband_scores on the widened arrays at 16 x 128: s20 the same bits, s21 and
    s22 within 1e-12 relative, on the rows whose oracle |s21| >= 1e-3 (a smaller mean of
    correlations has cancelled away the digits a relative bar measures; see
    test_subband_f64_gpu.py).  test_cand_f32_host.py shows on the CPU that this seed keeps at
    least 90 % of the rows."""
    p32, s32, scal = anchor_batch()
    out, st = engine.subband3_f32(p32, s32, scal)
    ref, ok = oracle_sub(wide(p32), wide(s32), scal)
    assert np.array_equal((st & 0xFF) == 0, ok)
    keep = ok & (np.abs(ref[:, 1]) >= 1e-3)
    assert keep.sum() >= 0.9 * len(keep)
    r = rel(out[keep], ref[keep])
    print(f"anchor: rows {int(keep.sum())}/{len(keep)} max rel s20 {r[:, 0].max():.3g} "
          f"s21 {r[:, 1].max():.3g} s22 {r[:, 2].max():.3g}")
    same_bits(out[keep][:, 0], ref[keep][:, 0], "anchor s20")
    assert (r[:, 1] <= 1e-12).all() and (r[:, 2] <= 1e-12).all()


# ---- the profile fits ------------------------------------------------------------------------------
# lp 8: the minimum; 64, 128: the 16-lane pooled groups; 200: the 32-lane ones; 300: batched
@pytest.mark.parametrize("solver", ["pooled", "batched"])
@pytest.mark.parametrize("lp", [8, 64, 128, 200, 300])
def test_profile_fits_f32(engine, lp, solver):
    p32 = batch32(64, 2, lp, seed=4300 + lp, adv=False)["prof"]
    with engine.options(solver=solver):
        for f32, f64 in ((engine.sinusoid4_f32, engine.sinusoid4_f64),
                         (engine.gauss7_f32, engine.gauss7_f64)):
            got, want = f32(p32), f64(wide(p32))
            same_scores(got, want, f"{f32.__name__} lp={lp} {solver}")
            gd = f32(dev(p32))
            engine.synchronize()
            same_scores((host(gd[0]), host(gd[1])), want, f"{f32.__name__} lp={lp} {solver} device")


# ---- the 22 scores ---------------------------------------------------------------------------------
@pytest.mark.parametrize("serial", [0, 1])
@pytest.mark.parametrize("ndm", [3, 120])
def test_bates22_f32(engine, ndm, serial):
    b = batch32(24, 16, 128, seed=4400, ndm=ndm)
    p, s, c, sc = b["prof"], b["sub"], b["dmcurve"], b["scal"]
    with engine.options(serial=serial):
        got = engine.bates22_f32(p, s, c, sc)
        want = engine.bates22_f64(wide(p), wide(s), wide(c), sc)
        same_scores(got, want, f"ndm={ndm} serial={serial}")
        out = got[0]
        same_bits(out[:, 0:4], engine.sinusoid4_f32(p)[0], "columns 0-3", nan=True)
        same_bits(out[:, 4:11], engine.gauss7_f32(p)[0], "columns 4-10", nan=True)
        s3, st3 = engine.subband3_f32(p, s, sc)
        ok = (st3 & 0xFF) == 0
        assert ok.any() and (~ok).any()
        same_bits(out[ok][:, 19:22], s3[ok], "columns 19-21", nan=True)
        assert np.array_equal((got[1] & FAIL) != 0, ~ok)
        dv = engine.bates22_f32(dev(p), dev(s), dev(c), dev(sc))
        engine.synchronize()
        same_scores((host(dv[0]), host(dv[1])), got, f"device pointers ndm={ndm} serial={serial}")


def test_bates22_f32_takes_the_chis_of_pfd_dmprof(engine):
    """The float32 DM curve pfe_pfd_dmprof returns (n x 100) goes in as it is, on the device."""
    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    n = 5
    profs, subfreqs, scal8 = pfd.batch_inputs(pfd_fold_block(n, (4, 16, 128), 20261021))
    r = engine.pfd_dmprof(dev(profs), dev(subfreqs), dev(scal8), lyon8=False)
    chis = r["chis"]
    assert str(chis.dtype) == "torch.float32" and tuple(chis.shape) == (n, 100)
    b = batch32(n, 16, 128, seed=4500, adv=False)
    p, s, sc = r["profile"].float(), dev(b["sub"]), dev(b["scal"])
    got = engine.bates22_f32(p, s, chis, sc)
    want = engine.bates22_f64(p.double(), s.double(), chis.double(), sc)
    engine.synchronize()
    same_scores((host(got[0]), host(got[1])), (host(want[0]), host(want[1])), "chis")


# ---- call level ------------------------------------------------------------------------------------
def test_empty_batches_return_ok(engine):
    f32 = np.float32
    assert engine.lyon8(np.zeros((0, 8), f32), np.zeros((0, 9), f32)).shape == (0, 8)
    assert engine.sinusoid4_f32(np.zeros((0, 64), f32))[0].shape == (0, 4)
    assert engine.gauss7_f32(np.zeros((0, 64), f32))[0].shape == (0, 7)
    sub, scal = np.zeros((0, 4, 64), f32), np.zeros((0, 8))
    assert engine.subband3_f32(np.zeros((0, 64), f32), sub, scal)[0].shape == (0, 3)
    assert engine.bates22_f32(np.zeros((0, 64), f32), sub, np.zeros((0, 9), f32), scal)[0].shape == (0, 22)


def message(call, *args):
    with pytest.raises(PfeError) as e:
        call(*args)
    return str(e.value)


def test_refusals_carry_the_f64_text_under_the_new_name(engine):
    b = batch32(8, 16, 128, seed=4600, adv=False)
    p7 = np.ascontiguousarray(b["prof"][:, :7])
    for name in ("sinusoid4", "gauss7"):
        m32 = message(getattr(engine, name + "_f32"), p7)
        m64 = message(getattr(engine, name + "_f64"), wide(p7))
        assert m32 == m64.replace("_f64", "_f32") and m32.startswith(name + "_f32: lp=7 outside")
    args = (b["prof"], b["sub"], np.ascontiguousarray(b["dmcurve"][:, :2]), b["scal"])
    m32 = message(engine.bates22_f32, *args)
    m64 = message(engine.bates22_f64, *(wide(a) for a in args))
    assert m32 == m64.replace("_f64", "_f32") and m32.startswith("bates22_f32: ndm=2 outside")
    sub7 = np.zeros((8, 16, 7), np.float32)
    m32 = message(engine.bates22_f32, p7, sub7, b["dmcurve"], b["scal"])
    m64 = message(engine.bates22_f64, wide(p7), wide(sub7), wide(b["dmcurve"]), b["scal"])
    assert m32 == m64.replace("_f64", "_f32") and "lp=7" in m32
    big = np.zeros((1, 7000, 2), np.float32)
    m32 = message(engine.subband3_f32, b["prof"][:1, :2], big, b["scal"][:1])
    m64 = message(engine.subband3_f64, wide(b["prof"][:1, :2]), wide(big), b["scal"][:1])
    assert m32 == m64.replace("_f64", "_f32") and "7000x2" in m32


def unaligned(a, shift):
    """The float32 array `a` at an address that is `shift` bytes off a multiple of 4."""
    raw = np.zeros(a.nbytes + 8, dtype=np.uint8)
    off = (-raw.ctypes.data) % 4 + shift
    v = raw[off:off + a.nbytes].view(np.float32).reshape(a.shape)
    v[...] = a
    assert v.ctypes.data % 4 == shift and v.flags.c_contiguous
    return v


def test_wrong_alignment_and_dtype_raise(engine):
    b = batch32(8, 16, 128, seed=4600, adv=False)
    p, s, c, sc = b["prof"], b["sub"], b["dmcurve"], b["scal"]
    for shift in (1, 2):
        with pytest.raises(PfeError, match="aligned"):
            engine.subband3_f32(unaligned(p, shift), s, sc)
        with pytest.raises(PfeError, match="aligned"):
            engine.subband3_f32(p, unaligned(s, shift), sc)
        with pytest.raises(PfeError, match="aligned"):
            engine.bates22_f32(p, s, unaligned(c, shift), sc)
        with pytest.raises(PfeError, match="aligned"):
            engine.sinusoid4_f32(unaligned(p, shift))
        with pytest.raises(PfeError, match="aligned"):
            engine.lyon8(unaligned(p, shift), p)
    for args in ((wide(p), s, sc), (p, wide(s), sc), (p, s, sc.astype(np.float32)),
                 (p.astype(np.uint8), s, sc)):
        with pytest.raises(TypeError):
            engine.subband3_f32(*args)
    with pytest.raises(TypeError):
        engine.bates22_f32(p, s, wide(c), sc)
    with pytest.raises(TypeError):
        engine.gauss7_f32(wide(p))
    with pytest.raises(TypeError):
        engine.bates22_f32(dev(p), dev(s), dev(wide(c)), dev(sc))
    # the f64 methods keep refusing float32
    with pytest.raises(TypeError):
        engine.subband3_f64(p, s, sc)
    with pytest.raises(TypeError):
        engine.sinusoid4_f64(p)
