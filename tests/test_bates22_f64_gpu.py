"""pfe_bates22_f64 composes the five groups: every column group holds the bits of its group
call (compared as int64 views), the status word is the OR of the groups' bits, under the
default schedule, PFE_OPT_SERIAL = 1 and PFE_SOLVER_BATCHED; rows come back in order."""
import numpy as np
import pytest

from pulsarfeatureextractor_amd._native import PfeError
from test_subband_f64_gpu import adversarial, float_batch

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def filter_neg(v):
    """CandidateFileInterface.filterScore(13 | 14) (CandidateFileInterface.py:97-107)."""
    return np.where((np.abs(v - 0.0) > 0.000005) & (v < 0.0), 0.0, v)


def batch(nsub, lsb, n=64):
    b = adversarial(float_batch(n, nsub, lsb, seed=3100 + lsb))
    b["scal"][10, 1] = -3.0   # a negative S/N and DM: filterScore(13 / 14) -> 0
    b["scal"][11, 2] = -1e-7  # within 0.000005 of zero: kept
    return b


def groups(engine, b):
    s4, st_s = engine.sinusoid4_f64(b["prof"])
    g7, st_g = engine.gauss7_f64(b["prof"])
    p4, st_p = engine.params4(b["scal"])
    d4, st_d = engine.dmfit4(b["dmcurve"], b["scal"])
    s3, st_3 = engine.subband3_f64(b["prof"], b["sub"], b["scal"])
    p4 = p4.copy()
    p4[:, 1:3] = filter_neg(p4[:, 1:3])
    d4 = d4.copy()
    d4[:, 2] = np.abs(d4[:, 2])
    return np.hstack([s4, g7, p4, d4, s3]), st_s | st_g | st_p | st_d | st_3


@pytest.mark.parametrize("nsub,lsb", [(16, 128), (16, 64)])
@pytest.mark.parametrize("opts", [{}, {"serial": 1}, {"solver": "batched"}])
def test_columns_are_the_group_calls(engine, nsub, lsb, opts):
    b = batch(nsub, lsb)
    with engine.options(**opts):
        want, wst = groups(engine, b)
        out, st = engine.bates22_f64(b["prof"], b["sub"], b["dmcurve"], b["scal"])
    assert out.shape == (64, 22)
    for name, lo, hi in (("sinusoid4_f64", 0, 4), ("gauss7_f64", 4, 11), ("params4", 11, 15),
                         ("dmfit4", 15, 19), ("subband3_f64", 19, 22)):
        assert np.array_equal(bits(out[:, lo:hi]), bits(want[:, lo:hi])), name
    assert np.array_equal(st, wst)
    assert (st & 0x008).any() and not (st & 0x008).all()


def test_rows_come_back_in_order(engine):
    b = batch(16, 128)
    out, st = engine.bates22_f64(b["prof"], b["sub"], b["dmcurve"], b["scal"])
    perm = np.random.default_rng(4).permutation(64)
    op, sp = engine.bates22_f64(b["prof"][perm], b["sub"][perm], b["dmcurve"][perm], b["scal"][perm])
    assert np.array_equal(sp, st[perm]) and np.array_equal(bits(op), bits(out[perm]))


def test_device_pointers_match_host(engine):
    import torch

    b = batch(16, 64)
    out, st = engine.bates22_f64(b["prof"], b["sub"], b["dmcurve"], b["scal"])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}
    od, sd = engine.bates22_f64(t["prof"], t["sub"], t["dmcurve"], t["scal"])
    engine.synchronize()
    assert np.array_equal(sd.cpu().numpy().view(np.uint32), st)
    assert np.array_equal(bits(od.cpu().numpy()), bits(out))


def test_short_profile_is_refused_and_empty_batch_is_ok(engine):
    e = float_batch(4, 16, 64, seed=9)
    with pytest.raises(PfeError, match="lp=4"):
        engine.bates22_f64(e["prof"][:, :4], e["sub"][:, :, :4], e["dmcurve"], e["scal"])
    out, st = engine.bates22_f64(e["prof"][:0], e["sub"][:0], e["dmcurve"][:0], e["scal"][:0])
    assert out.shape == (0, 22) and st.shape == (0,)
    out, st = engine.subband3_f64(e["prof"][:0], e["sub"][:0], e["scal"][:0])
    assert out.shape == (0, 3) and st.shape == (0,)
