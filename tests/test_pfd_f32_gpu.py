"""The float32 forms of the five PFD calls (pfe_pfd_*_f32, reached through Engine.pfd_* with a
float32 cube) against the contract include/pfe.h states: every output and the status are, bit
for bit, those of the f64 call of the same name on the same cube widened value by value.

The reference is always the existing f64 call on x32.astype(float64) -- never the call under
test, never a golden (casting the cube changes its values).  Inputs are synth.pfd_fold_block
folds packed by pfd.batch_inputs with the cube cast to float32; the bar is np.array_equal with
equal_nan on every output.  Shapes are the smallest that take each route of the f64 kernels
and both load paths of k_pfd_partsum_f32 (16-byte loads when nsub x proflen is a multiple of 4
and the cube is 16-byte aligned, 4-byte loads otherwise)."""
import ctypes as C

import numpy as np
import pytest

from pulsarfeatureextractor_amd import pfd
from pulsarfeatureextractor_amd._native import PFE_FLAG_DEVICE_PTRS, PfdF32In, PfdIn, PfeError
from pulsarfeatureextractor_amd.synth import pfd_fold_block

pytestmark = pytest.mark.gpu

_blocks = {}


def block(shape, n):
    """(x32, x64 = x32 widened, subfreqs, scal) of n synthetic folds of `shape`, built once."""
    key = (shape, n)
    if key not in _blocks:
        profs, subfreqs, scal = pfd.batch_inputs(pfd_fold_block(n, shape, 20261021))
        x32 = profs.astype(np.float32)
        ins = (x32, x32.astype(np.float64), subfreqs, scal)
        for a in ins:
            a.setflags(write=False)
        _blocks[key] = ins
    return _blocks[key]


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


# route, handle options, (npart, nsub, proflen), n
ROUTES = [
    ("four_wave_pow2", {}, (7, 8, 64), 5),
    ("four_wave_pow2_128", {}, (4, 16, 128), 5),
    ("four_wave_generic", {}, (3, 5, 33), 67),   # E = 165: 4-byte loads, quads across folds
    ("single_wave_long", {}, (2, 4, 200), 3),
    ("single_wave_option", {"pfd_waves": 1}, (3, 5, 33), 67),
    ("slab_by_shape", {}, (2, 128, 256), 3),
    ("slab_option", {"pfd_global": 1}, (3, 5, 33), 67),
    ("split", {"pfd_split": 1}, (4, 16, 128), 5),
    ("one_part", {}, (1, 2, 8), 1),
]


@pytest.mark.parametrize("route,opts,shape,n", ROUTES, ids=[r[0] for r in ROUTES])
def test_routes(engine, route, opts, shape, n):
    x32, x64, fr, sc = block(shape, n)
    with engine.options(**opts):
        same_dmprof(engine.pfd_dmprof(x32, fr, sc), engine.pfd_dmprof(x64, fr, sc), route)
        same_scores(engine.pfd_bates22(x32, fr, sc), engine.pfd_bates22(x64, fr, sc), route)


@pytest.mark.parametrize("shape,n", [((7, 8, 64), 5), ((3, 5, 33), 67)], ids=["7x8x64", "3x5x33"])
def test_group_calls(engine, shape, n):
    x32, x64, fr, sc = block(shape, n)
    for call in (engine.pfd_params4, engine.pfd_dmfit4, engine.pfd_subband3):
        same_scores(call(x32, fr, sc), call(x64, fr, sc), call.__name__)


@pytest.mark.parametrize("chunk", [1, 2, 64])
def test_chunk_seams(engine, chunk):
    """PFE_OPT_PFD_F32_CHUNK: passes of 1, 2 and (cut to n) 5 of n = 5 folds give the bits of the
    default's single pass, in the chain's outputs and in a group call's column scratch."""
    x32, _x64, fr, sc = block((3, 5, 33), 5)
    assert engine.get_option("pfd_f32_chunk") == 0
    calls = (engine.pfd_bates22, engine.pfd_dmfit4, engine.pfd_subband3, engine.pfd_params4)
    want_d = engine.pfd_dmprof(x32, fr, sc)
    want = [c(x32, fr, sc) for c in calls]
    with engine.options(pfd_f32_chunk=chunk):
        assert engine.get_option("pfd_f32_chunk") == chunk
        same_dmprof(engine.pfd_dmprof(x32, fr, sc), want_d, f"chunk {chunk}")
        for c, w in zip(calls, want):
            same_scores(c(x32, fr, sc), w, f"chunk {chunk} {c.__name__}")
        for o in ({"pfd_global": 1}, {"pfd_split": 1}):  # slabs / part-sum buffers per pass
            with engine.options(**o):
                same_dmprof(engine.pfd_dmprof(x32, fr, sc), want_d, f"chunk {chunk} {o}")
    assert engine.get_option("pfd_f32_chunk") == 0
    with pytest.raises(PfeError):
        engine.set_option("pfd_f32_chunk", -1)


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


def test_float32_arrays_reach_the_f32_entry_points(engine, monkeypatch):
    """Nothing widens a float32 cube on the way: the f64 entry points are not called."""
    x32, _x64, fr, sc = block((1, 2, 8), 1)

    def f64_entry(*a):
        raise AssertionError("a float32 cube went to the f64 entry point")

    for name in ("pfe_pfd_dmprof", "pfe_pfd_bates22", "pfe_pfd_params4", "pfe_pfd_dmfit4",
                 "pfe_pfd_subband3"):
        monkeypatch.setattr(engine.lib, name, f64_entry)
    t = [_dev(a) for a in (x32, fr, sc)]
    for ins in ((x32, fr, sc), t):
        engine.pfd_dmprof(*ins)
        for call in (engine.pfd_bates22, engine.pfd_params4, engine.pfd_dmfit4,
                     engine.pfd_subband3):
            call(*ins)
    engine.synchronize()


def test_device_tensors_carry_the_host_bits(engine):
    x32, _x64, fr, sc = block((7, 8, 64), 5)
    t = [_dev(a) for a in (x32, fr, sc)]
    d, s = engine.pfd_dmprof(*t), engine.pfd_bates22(*t)
    g = engine.pfd_subband3(*t)
    engine.synchronize()
    same_dmprof(_host(d), engine.pfd_dmprof(x32, fr, sc), "device dmprof")
    same_scores(_host(s), engine.pfd_bates22(x32, fr, sc), "device bates22")
    same_scores(_host(g), engine.pfd_subband3(x32, fr, sc), "device subband3")


def test_cube_one_float_past_a_16_byte_boundary(engine):
    """A slice of a larger tensor: nsub x proflen is a multiple of 4, the base is not 16-byte
    aligned, so the 4-byte loads run where the 16-byte ones would."""
    import torch

    x32, _x64, fr, sc = block((7, 8, 64), 5)
    big = torch.zeros(x32.size + 4, dtype=torch.float32, device="cuda")
    assert big.data_ptr() % 16 == 0
    cube = big[1:1 + x32.size].view(x32.shape)
    cube.copy_(_dev(x32))
    assert cube.data_ptr() % 16 == 4 and cube.is_contiguous()
    t = [cube, _dev(fr), _dev(sc)]
    d, s = engine.pfd_dmprof(*t), engine.pfd_bates22(*t)
    engine.synchronize()
    same_dmprof(_host(d), engine.pfd_dmprof(x32, fr, sc), "offset cube dmprof")
    same_scores(_host(s), engine.pfd_bates22(x32, fr, sc), "offset cube bates22")


def test_special_values(engine):
    """Signed zeros, float32 subnormals, values whose float32 sum overflows or cancels, a NaN
    and an inf: the same bits and the same NaN / inf pattern as the f64 call."""
    shape, n = (7, 8, 64), 5
    x32 = np.array(block(shape, n)[0])
    _a, _b, fr, sc = block(shape, n)
    f = x32[0]
    f[:, 0, 0] = -0.0                     # every part -0.0: the sum is -0.0, 0.0 + it is not
    f[0, 0, 1], f[1, 0, 1] = 0.0, -0.0
    f[:, 1, 2] = np.float32(1e-45)        # the smallest subnormal, seven times
    f[0, 1, 3], f[1, 1, 3] = np.float32(1.2e-38), np.float32(-1e-40)
    f[0, 2, 4], f[1, 2, 4] = np.float32(3e38), np.float32(3e38)    # inf in float32
    f[2, 2, 4], f[3, 2, 4] = np.float32(-3e38), np.float32(-3e38)
    f[0, 3, 5], f[1, 3, 5], f[2, 3, 5] = np.float32(1e30), np.float32(1e-30), np.float32(-1e30)
    x32[1, 3, 4, 17] = np.nan
    x32[2, 5, 7, 63] = np.inf
    x64 = x32.astype(np.float64)
    got, want = engine.pfd_dmprof(x32, fr, sc), engine.pfd_dmprof(x64, fr, sc)
    same_dmprof(got, want, "special values")
    for k in ("profile", "chis", "lyon8"):
        assert np.array_equal(np.isinf(got[k]), np.isinf(want[k])), k
    # the folds beside them are the ones the plain cube gives
    plain = engine.pfd_dmprof(block(shape, n)[0], fr, sc)
    for k in ("profile", "chis", "lyon8", "status"):
        same(got[k][3:], plain[k][3:], f"untouched folds: {k}")


def test_part_sums_in_order_against_numpy(engine):
    """k_pfd_partsum_f32 alone: the f64 call with npart = 1 on part sums numpy forms on the host,
    each fold's parts added in fp64 in order from part 0."""
    shape, n = (5, 6, 50), 9
    x32, _x64, fr, sc = block(shape, n)
    s = x32[:, 0].astype(np.float64)
    for p in range(1, shape[0]):
        s = s + x32[:, p]
    assert s.dtype == np.float64
    same_dmprof(engine.pfd_dmprof(x32, fr, sc), engine.pfd_dmprof(s[:, None], fr, sc), "part sums")


def _raw(engine, name, struct, profs, fr, sc, shape, n, nout):
    """A C call on device pointers -> (return code, pfe_last_error text)."""
    import torch

    out = torch.zeros((n, nout), dtype=torch.float64, device="cuda")
    st = torch.zeros((n,), dtype=torch.int32, device="cuda")
    pin = struct(profs, fr.data_ptr(), sc.data_ptr(), *shape, n)
    fn = getattr(engine.lib, name)
    if "dmprof" in name:
        rc = fn(engine._h, C.byref(pin), None, None, out.data_ptr(), st.data_ptr(), PFE_FLAG_DEVICE_PTRS)
    else:
        rc = fn(engine._h, C.byref(pin), out.data_ptr(), st.data_ptr(), PFE_FLAG_DEVICE_PTRS)
    return rc, engine.lib.pfe_last_error(engine._h).decode()


def _error(call, *args):
    with pytest.raises(PfeError) as e:
        call(*args)
    return str(e.value)


def test_errors_are_those_of_the_f64_calls(engine):
    fr1, sc = np.full((1, 1), 1400.0), np.ones((1, 8))
    one = np.ones((1, 1, 1, 1))
    msg = _error(engine.pfd_dmprof, one, fr1, sc)
    assert "shape 1x1x1" in msg
    assert _error(engine.pfd_dmprof, one.astype(np.float32), fr1, sc) == msg
    fr2 = np.full((1, 2), 1400.0)
    long_ = np.ones((1, 1, 2, 1025))
    for call in (engine.pfd_bates22, engine.pfd_params4, engine.pfd_dmfit4, engine.pfd_subband3):
        msg = _error(call, long_, fr2, sc)
        assert "1x2x1025 unsupported" in msg
        assert _error(call, long_.astype(np.float32), fr2, sc) == msg
    # a null cube, straight at the C entry points
    tfr, tsc = _dev(np.full((2, 8), 1400.0)), _dev(np.ones((2, 8)))
    for name, nout in (("pfe_pfd_dmprof", 8), ("pfe_pfd_bates22", 22), ("pfe_pfd_params4", 4),
                       ("pfe_pfd_dmfit4", 4), ("pfe_pfd_subband3", 3)):
        want = _raw(engine, name, PfdIn, None, tfr, tsc, (3, 8, 64), 2, nout)
        got = _raw(engine, name + "_f32", PfdF32In, None, tfr, tsc, (3, 8, 64), 2, nout)
        assert want[0] != 0 and "null input array" in want[1]
        assert got == want, name
    engine.synchronize()


def test_device_dtypes(engine):
    """A float32 device cube is scored; any dtype that is neither float is still a TypeError."""
    import torch

    x32, _x64, fr, sc = block((1, 2, 8), 1)
    tfr, tsc = _dev(fr), _dev(sc)
    r = engine.pfd_dmprof(_dev(x32), tfr, tsc)
    engine.synchronize()
    assert r["profile"].dtype == torch.float64 and tuple(r["profile"].shape) == (1, 8)
    with pytest.raises(TypeError):
        engine.pfd_dmprof(_dev(x32).to(torch.int32), tfr, tsc)
    with pytest.raises(TypeError):
        engine.pfd_bates22(_dev(x32).to(torch.int32), tfr, tsc)
