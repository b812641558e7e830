"""The group calls of a PFD fold -- pfe_sinusoid4_f64, pfe_gauss7_f64, pfe_pfd_params4,
pfe_pfd_dmfit4, pfe_pfd_subband3 -- against the whole chain (pfe_pfd_bates22) on the same
handle: every group's columns carry the chain's bits on the rows the chain scored (compared as
int64 views, NaN included), and its status is exactly its group's bit of the chain's status.
The 22 columns put together from the groups also meet tests/test_pfd22_gpu.py's bar against
the reference's own outputs."""
import os

import numpy as np
import pytest

from pulsarfeatureextractor_amd import pfd
from pulsarfeatureextractor_amd._native import (PFE_ST_DMFIT_FAIL, PFE_ST_FAIL_MASK,
                                                PFE_ST_GAUSS_FAIL, PFE_ST_SINE_FAIL,
                                                PFE_ST_SUBBAND_FAIL)
from test_oracle_pfd import SETS, build_files, load_set
from test_pfd22_gpu import FLOOR, check

pytestmark = pytest.mark.gpu

_cache = {}


def inputs(name, tmp_path_factory):
    """(profs, subfreqs, scal) of a golden set or of the ragged 2 x 3 x 300 shape, built once."""
    if name not in _cache:
        tmp = str(tmp_path_factory.mktemp(name))
        if name == "ragged":
            from pulsarfeatureextractor_amd.synth import pfd_candidate

            npart, nsub, L = 2, 3, 300
            files = []
            for i in range(6):  # seeded as tests/test_pfd22_gpu.py's fresh shapes
                c = pfd_candidate(np.random.default_rng(900 + 7 * i + L), npart, nsub, L,
                                  pulsar=(i % 3 != 1))
                files.append(os.path.join(tmp, f"f{L}_{i}.pfd"))
                pfd.write(files[-1], **c)
        else:
            files = build_files(tmp, load_set(name))
        ins = pfd.batch_inputs([pfd.read(f) for f in files])
        for a in ins:
            a.setflags(write=False)
        _cache[name] = ins
    return _cache[name]


def filter_neg(v):
    """CandidateFileInterface.filterScore(13 | 14) on an array."""
    v = v.copy()
    v[(np.abs(v - 0.0) > 0.000005) & (v < 0.0)] = 0.0
    return v


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def run_groups(engine, ins, to=lambda a: a, back=lambda a: a):
    """The five group calls -> dict name -> (values, status) as host arrays."""
    t = [to(a) for a in ins]
    prof = engine.pfd_dmprof(*t, chis=False, lyon8=False)["profile"]
    g = {"sine": engine.sinusoid4_f64(prof), "gauss": engine.gauss7_f64(prof),
         "params": engine.pfd_params4(*t), "dmfit": engine.pfd_dmfit4(*t),
         "sub": engine.pfd_subband3(*t)}
    engine.synchronize()
    return {k: (back(v), back(s).view(np.uint32)) for k, (v, s) in g.items()}


def assemble(g):
    """The 22-score rows and status from the groups, as PFDFile's five methods store them."""
    p, d = g["params"][0], g["dmfit"][0]
    out = np.concatenate([g["sine"][0], g["gauss"][0], p[:, :1], filter_neg(p[:, 1:3]), p[:, 3:],
                          d[:, :2], np.abs(d[:, 2:3]), d[:, 3:], g["sub"][0]], axis=1)
    st = np.zeros(len(out), dtype=np.uint32)
    for v, s in g.values():
        st |= s
    return out, st


GROUP_BIT = {"sine": PFE_ST_SINE_FAIL, "gauss": PFE_ST_GAUSS_FAIL, "params": 0,
             "dmfit": PFE_ST_DMFIT_FAIL, "sub": PFE_ST_SUBBAND_FAIL}


def compare(g, full, fst, tag):
    fst = fst.view(np.uint32)
    for k, (v, s) in g.items():
        # exactly this group's failure bit of the whole chain, and no other group's
        assert np.array_equal(s & PFE_ST_FAIL_MASK, fst & GROUP_BIT[k]), (tag, k, s, fst)
    # the informational bit of the double-Gaussian fit travels with its group
    assert np.array_equal(g["gauss"][1] & ~np.uint32(PFE_ST_FAIL_MASK), fst & ~np.uint32(PFE_ST_FAIL_MASK))
    ok = (fst & PFE_ST_FAIL_MASK) == 0
    out, _st = assemble(g)
    assert ok.any(), tag
    for j in range(22):
        assert np.array_equal(bits(out[ok, j]), bits(full[ok, j])), f"{tag}: column {j}"
    p, d = g["params"][0], g["dmfit"][0]
    assert np.array_equal(bits(p[ok][:, [0, 3]]), bits(full[ok][:, [11, 14]])), tag
    assert np.array_equal(bits(filter_neg(p[ok, 1:3])), bits(full[ok, 12:14])), tag
    assert np.array_equal(bits(d[ok][:, [0, 1, 3]]), bits(full[ok][:, [15, 16, 18]])), tag
    assert np.array_equal(bits(np.abs(d[ok, 2])), bits(full[ok, 17])), tag
    assert np.array_equal(bits(g["sub"][0][ok]), bits(full[ok, 19:22])), tag
    return out


@pytest.mark.parametrize("name", SETS + ["ragged"])
def test_groups_against_the_whole_chain(engine, tmp_path_factory, name):
    ins = inputs(name, tmp_path_factory)
    full, fst = engine.pfd_bates22(*ins)
    g = run_groups(engine, ins)
    out = compare(g, full, fst, name)
    if name != "ragged":  # the reference's own outputs, under test_pfd22_gpu's bar
        ref = load_set(name)
        _o, st = assemble(g)
        check(out, st, ref["bates22"], ref["bates22_ok"], name + " from groups", FLOOR[name])


@pytest.mark.parametrize("opts", [{"pfd_global": 1}, {"pfd_waves": 1}, {"solver": "batched"}],
                         ids=["pfd_global", "pfd_waves1", "batched"])
def test_groups_under_handle_options(engine, tmp_path_factory, opts):
    """The mask in k_pfd_dmprof_g, in the single-wave kernel, and the batched DM-fit kernel:
    chain and groups on the same handle options."""
    ins = inputs("pfd_64x16", tmp_path_factory)
    with engine.options(**opts):
        full, fst = engine.pfd_bates22(*ins)
        g = run_groups(engine, ins)
    compare(g, full, fst, str(opts))


def test_device_pointers_carry_the_host_bits(engine, tmp_path_factory):
    import torch

    ins = [a[:8] for a in inputs("pfd_64x16", tmp_path_factory)]
    host = run_groups(engine, ins)
    dev = run_groups(engine, ins, to=lambda a: torch.from_numpy(np.array(a)).cuda(),
                     back=lambda t: t.cpu().numpy())
    for k in host:
        assert np.array_equal(bits(dev[k][0]), bits(host[k][0])), k
        assert np.array_equal(dev[k][1], host[k][1]), k


def test_order_independence(engine, tmp_path_factory):
    """The group calls share the handle's scratch: the order they are made in leaks nothing."""
    ins = inputs("pfd_64x16", tmp_path_factory)
    calls = (engine.pfd_params4, engine.pfd_subband3, engine.pfd_dmfit4)
    fwd = [c(*ins) for c in calls]
    rev = [c(*ins) for c in calls[::-1]][::-1]
    for (a, sa), (b, sb), c in zip(fwd, rev, calls):
        assert np.array_equal(bits(a), bits(b)), c.__name__
        assert np.array_equal(sa, sb), c.__name__


def test_all_zero_fold(engine):
    """255/0 in the profile scaling: the reference raises.  Each group call sets the bit
    pfe_pfd_bates22 sets for it and leaves the other groups' bits clear."""
    npart, nsub, L = 8, 16, 64
    d = pfd.PFDData(npart=npart, nsub=nsub, proflen=L, profs=np.zeros((npart, nsub, L)),
                    subfreqs=1200.0 + 4.0 * np.arange(nsub), bestdm=50.0, binspersec=L / 0.1,
                    avgprof=0.0, varprof=1.0, dms=np.linspace(0.0, 100.0, 50), numdms=50,
                    bary_p1=0.1)
    ins = pfd.batch_inputs([d])
    full, fst = engine.pfd_bates22(*ins)
    fst = fst.view(np.uint32)
    assert fst[0] & PFE_ST_FAIL_MASK, "the chain scores an all-zero fold"
    g = run_groups(engine, ins)
    for k, (v, s) in g.items():
        assert (s[0] & PFE_ST_FAIL_MASK) == (fst[0] & GROUP_BIT[k]), (k, hex(s[0]), hex(fst[0]))
