"""A call's results do not depend on what the handle's device scratch held before.

One handle makes every compute call at batch sizes 3 -> 67 -> 5, so its scratch is allocated,
regrown, then reused larger than needed, with every other call's regions left behind in it.
Each result must equal, bit for bit (NaN included) and status word for status word, the same
call on a fresh handle of its own; the host-array and device-tensor forms must agree in the
same way.  The shapes are the smallest that make every scratch region live: 64-bin profiles
with 4 x 64 sub-bands, a 257 x 16 sub-band shape no on-chip kernel takes (the any-shape
kernel's slabs), one batch of wide histograms (the wide queue and its slabs) and PFD folds of
2 x 4 x 32 under both PFD pipelines and the global-memory kernel.  Correctness itself is the
golden and oracle tests' business.
"""
import numpy as np
import pytest

from pulsarfeatureextractor_amd import pfd, synth
from pulsarfeatureextractor_amd._native import Engine

pytestmark = pytest.mark.gpu

SIZES = (3, 67, 5)
PFD_OPTS = [dict(pfd_split=s, pfd_global=g) for s in (0, 1) for g in (0, 1)]


def _inputs(n):
    b = synth.bates_batch(n, lp=64, nsub=4, lsb=64, ndm=48, seed=900 + n)
    g = synth.bates_batch(n, lp=16, nsub=257, lsb=16, ndm=48, seed=950 + n)   # any-shape sub-bands
    lp, ld = synth.lyon_batch(n, lp=64, ld=96, seed=800 + n)
    folds = pfd.batch_inputs(synth.pfd_fold_block(n, (2, 4, 32), seed=700 + n))
    fprof = np.ascontiguousarray(b["prof"], dtype=np.float64) * 0.75 + 3.0
    return dict(b=b, g=g, lyon=(lp, ld), lyon_f64=(lp.astype(np.float64), ld.astype(np.float64)),
                folds=folds, fprof=fprof)


def _bates(k):
    return lambda x: (x[k]["prof"], x[k]["sub"], x[k]["dmcurve"], x[k]["scal"])


def _sub(k):
    return lambda x: (x[k]["prof"], x[k]["sub"], x[k]["scal"])


def _folds(x):
    return x["folds"]


# (name, options, method, arguments of the inputs x) of every compute call
CALLS = [
    ("lyon8_u8", {}, "lyon8", lambda x: x["lyon"]),
    ("lyon8_f64", {}, "lyon8", lambda x: x["lyon_f64"]),
    ("bates22", {}, "bates22", _bates("b")),
    ("subband3", {}, "subband3", _sub("b")),
    ("bates22_anyshape", {}, "bates22", _bates("g")),
    ("subband3_anyshape", {}, "subband3", _sub("g")),
    ("sinusoid4", {}, "sinusoid4", lambda x: (x["b"]["prof"], x["b"]["scal"])),
    ("gauss7", {}, "gauss7", lambda x: (x["b"]["prof"], x["b"]["scal"])),
    ("params4", {}, "params4", lambda x: (x["b"]["scal"],)),
    ("dmfit4", {}, "dmfit4", lambda x: (x["b"]["dmcurve"], x["b"]["scal"])),
    ("sinusoid4_f64", {}, "sinusoid4_f64", lambda x: (x["fprof"],)),
    ("gauss7_f64", {}, "gauss7_f64", lambda x: (x["fprof"],)),
] + [
    (f"pfd_dmprof_split{o['pfd_split']}_global{o['pfd_global']}", o, "pfd_dmprof", _folds)
    for o in PFD_OPTS
] + [
    (m, {}, m, _folds) for m in ("pfd_bates22", "pfd_params4", "pfd_dmfit4", "pfd_subband3")
] + [
    ("pfd_bates22_global", dict(pfd_global=1), "pfd_bates22", _folds),
    # once, at the middle size: the wide queue and its slabs
    ("bates22_wide", {}, "bates22", _bates("wide")),
]
CALL_NAMES = [c[0] for c in CALLS]


def _bits(r):
    """A call's result as a list of integer arrays: float values as their bit patterns."""
    if isinstance(r, dict):
        r = [r[k] for k in sorted(r)]
    elif not isinstance(r, (tuple, list)):
        r = [r]
    out = []
    for a in r:
        a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
        out.append(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f"
                   else a.astype(np.int64))
    return out


def _run(eng, opts, method, args, dev):
    if dev:
        import torch

        args = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{eng.device}") for a in args)
    with eng.options(**opts):
        return _bits(getattr(eng, method)(*args))


@pytest.fixture(scope="module")
def history():
    """{call name: [(batch size, placement, shared handle's result, fresh handle's result)]}"""
    got = {name: [] for name in CALL_NAMES}
    wide = synth.wide_histogram_batch(80, 5)
    with Engine(0) as shared:
        for i, n in enumerate(SIZES):
            x = dict(_inputs(n), wide=wide)
            for name, opts, method, pick in CALLS:
                if name == "bates22_wide" and i != 1:
                    continue
                for dev in (False, True):
                    mine = _run(shared, opts, method, pick(x), dev)
                    with Engine(0) as fresh:
                        want = _run(fresh, opts, method, pick(x), dev)
                    got[name].append((n, "device" if dev else "host", mine, want))
    return got


@pytest.mark.parametrize("name", CALL_NAMES)
def test_result_is_independent_of_the_scratch_history(history, name):
    runs = history[name]
    assert len(runs) == (2 if name == "bates22_wide" else 2 * len(SIZES))
    for n, where, mine, want in runs:
        assert len(mine) == len(want)
        for k, (a, b) in enumerate(zip(mine, want)):
            assert a.shape == b.shape and np.array_equal(a, b), (name, n, where, k)
    # the host-array and the device-tensor form of each batch
    for (n, _, host, _), (n2, _, dev, _) in zip(runs[0::2], runs[1::2]):
        assert n == n2
        for k, (a, b) in enumerate(zip(host, dev)):
            assert np.array_equal(a, b), (name, n, "host vs device", k)
