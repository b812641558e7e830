"""GPU parity of the PFD path for folds beyond the on-chip limit (k_pfd_dmprof_g: the fold's
sub-band profiles in global scratch) and of that kernel against the LDS-resident ones.

Shapes are (npart, nsub, proflen).  pfd_lds_bytes is 163 840 B at the limit: (2, 76, 256)
needs 161 936 B and stays on chip, (2, 77, 256) needs 164 012 B and does not.

Bars: tests/test_pfd_gpu.py (profile, DM curve and the moment columns bit-exact against the
CPU restatement, the two pow(m2, 1.5) skews within 1e-13 / 1e-6 relative) and
tests/test_pfd22_gpu.py (check / oracle_floor, unchanged).  The global-memory kernel adds in
the order of the LDS kernels, so forcing it (option pfd_global=1) gives identical bits."""
import os
import warnings

import numpy as np
import pytest

from oracle import pfd as opfd
from pulsarfeatureextractor_amd import pfd
from pulsarfeatureextractor_amd._native import PfeError
from pulsarfeatureextractor_amd.synth import pfd_candidate
from test_oracle_pfd import SETS, build_files, load_set
from test_pfd22_gpu import check, oracle_floor

pytestmark = pytest.mark.gpu

OVER = [(2, 77, 256), (2, 40, 512), (3, 21, 1000), (2, 300, 70), (2, 11, 2048)]


def eq_nan(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def folds(tmp_path, shape, n, seed, pulsar=lambda i: True):
    """n synthetic folds of one shape, written and re-read as .pfd files."""
    npart, nsub, L = shape
    datas = []
    for i in range(n):
        c = pfd_candidate(np.random.default_rng(seed + i), npart, nsub, L, pulsar=pulsar(i))
        p = os.path.join(tmp_path, f"f{nsub}x{L}_{i}.pfd")
        pfd.write(p, **c)
        datas.append(pfd.read(p))
    return datas


def dmprof_vs_oracle(engine, datas, tag):
    r = engine.pfd_dmprof(*pfd.batch_inputs(datas))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, d in enumerate(datas):
            assert int(r["status"][i]) == 0, (tag, i)
            assert eq_nan(r["profile"][i], opfd.PFDState(d).profile()).all(), (tag, i, "profile")
            chis = opfd.dm_curve(d)
            assert np.isfinite(chis).all(), (tag, i)
            assert eq_nan(r["chis"][i], chis).all(), (tag, i, "chis")
            ref = np.array(opfd.lyon8_one(d))
            got = r["lyon8"][i]
            for j in (0, 1, 3, 4, 5, 7):
                assert eq_nan(got[j], ref[j]), (tag, i, j, got[j], ref[j])
            for j, tol in ((2, 1e-13), (6, 1e-6)):
                assert eq_nan(got[j], ref[j]) or abs(got[j] - ref[j]) <= tol * abs(ref[j]), \
                    (tag, i, j, got[j], ref[j])


@pytest.mark.parametrize("shape", OVER)
def test_over_limit_dmprof_vs_oracle(engine, tmp_path, shape):
    """Folds that do not fit the LDS: profile, DM curve and Lyon features against the oracle."""
    dmprof_vs_oracle(engine, folds(tmp_path, shape, 3, 500 + shape[2]), shape)


@pytest.mark.parametrize("shape", [(2, 76, 256), (2, 77, 256)])
def test_dispatch_boundary(engine, tmp_path, shape):
    """The last shape on chip and the first one off it."""
    dmprof_vs_oracle(engine, folds(tmp_path, shape, 3, 700 + shape[1]), shape)


def same_bits(a, b, tag):
    """Every output bit-identical (NaN-aware).  A numdms == 1 fold has no DM curve: no kernel
    writes its chis row, so that row is compared nowhere."""
    assert np.array_equal(a["status"], b["status"]), (tag, "status")
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "chis":
            live = (np.asarray(a["status"]) & 0x20) == 0
            x, y = x[live], y[live]
        assert eq_nan(x, y).all(), (tag, k)


@pytest.mark.parametrize("name", SETS)
def test_forced_global_vs_reference_and_default(engine, tmp_path, name):
    """pfd_global=1 on the golden sets: the reference's own outputs under test_pfd_gpu's bar,
    and the default path's bits, for both entry points."""
    g = load_set(name)
    inp = pfd.batch_inputs([pfd.read(f) for f in build_files(tmp_path, g)])
    d0 = engine.pfd_dmprof(*inp)
    o0, s0 = engine.pfd_bates22(*inp)
    with engine.options(pfd_global=1):
        r = engine.pfd_dmprof(*inp)
        o1, s1 = engine.pfd_bates22(*inp)
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
    same_bits(r, d0, name)
    same_bits({"out": o1, "status": s1}, {"out": o0, "status": s0}, name + " bates22")


@pytest.mark.parametrize("shape", [(4, 8, 256), (2, 3, 300), (8, 16, 128)])
def test_forced_global_identity(engine, tmp_path, shape):
    """The single-wave kernel's shape, a ragged length and the sweep_pow2 shape: the same bits
    from the global-memory kernel."""
    inp = pfd.batch_inputs(folds(tmp_path, shape, 4, 900 + shape[2], lambda i: i % 3 != 1))
    d0 = engine.pfd_dmprof(*inp)
    o0, s0 = engine.pfd_bates22(*inp)
    with engine.options(pfd_global=1):
        d1 = engine.pfd_dmprof(*inp)
        o1, s1 = engine.pfd_bates22(*inp)
    same_bits(d1, d0, shape)
    same_bits({"out": o1, "status": s1}, {"out": o0, "status": s0}, (shape, "bates22"))


@pytest.mark.parametrize("shape,n", [((2, 77, 256), 8), ((2, 40, 512), 6), ((2, 168, 128), 6)])
def test_over_limit_bates22_vs_oracle(engine, tmp_path, shape, n):
    """The 22 scores of folds beyond the limit; 168 x 128 takes the sub-band scores' 8-lane
    row path on the slab."""
    datas = folds(tmp_path, shape, n, 900 + shape[2], lambda i: i % 3 != 1)
    out, st = engine.pfd_bates22(*pfd.batch_inputs(datas))
    ref, ok, floor = oracle_floor(datas)
    assert ok.all(), "the oracle scores every fold of these shapes"
    check(out, st, ref, ok, f"oracle {shape}", floor)


def test_slab_reuse_device_pointers(engine, tmp_path):
    """2048 folds of 1 x 77 x 256 (four distinct ones tiled, ~320 MB resident) through far
    fewer persistent blocks: every tile has tile 0's bits (a block reusing its slab before the
    previous fold is finished, or reading part sums of another wave too early, breaks that),
    and the first four rows are a host-pointer call's on the four folds alone."""
    import torch

    profs, sf, sc = pfd.batch_inputs(folds(tmp_path, (1, 77, 256), 4, 1300))
    alone = engine.pfd_dmprof(profs, sf, sc)
    reps = 512

    def tile(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t.repeat((reps,) + (1,) * (t.dim() - 1)).contiguous()

    r = engine.pfd_dmprof(tile(profs), tile(sf), tile(sc))
    engine.synchronize()
    for k, view in (("profile", torch.int64), ("chis", torch.int32), ("lyon8", torch.int64),
                    ("status", torch.int32)):
        t = r[k].view(view).view(reps, 4, -1)
        bad = (t != t[:1]).any(dim=2).any(dim=1)
        assert not bool(bad.any()), f"{k}: tiles differing from tile 0: {torch.nonzero(bad)[:10].flatten().tolist()}"
        got = r[k][:4].cpu().numpy()
        assert np.array_equal(got.view(np.uint8), np.asarray(alone[k]).view(np.uint8)), k
    del r
    torch.cuda.empty_cache()


def test_option_and_refusal(engine):
    assert engine.get_option("pfd_global") == 0
    with engine.options(pfd_global=1):
        assert engine.get_option("pfd_global") == 1
    assert engine.get_option("pfd_global") == 0
    with pytest.raises(PfeError):
        engine.set_option("pfd_global", 2)
    assert engine.get_option("pfd_global") == 0
    # outside the envelope: refused by name, nothing launched
    L = 70000
    with pytest.raises(PfeError, match="proflen=70000.*65535"):
        engine.pfd_dmprof(np.ones((1, 1, 1, L)), np.full((1, 1), 1400.0), np.ones((1, 8)))
    engine.synchronize()
