"""A fold's average, host side (no GPU): the rule pfe_pfd_avgprof implements, pinned against
numpy; the reader and packer without the average; the scratch of the call and of
PFE_FLAG_PFD_AVGPROF under ASan + UBSan.

The rule (include/pfe.h): y[e] = x[e] / L in fp64; the fold's E values in chunks of 8192 (numpy's
reduction buffer), each summed pairwise -- n < 8: 0.0 + y0 + ...; n <= 128: eight accumulators,
((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 last in order; else split at floor8(n / 2)
-- and the chunk sums added in order onto numpy's initial 0.0 (all -0.0 sums to +0.0).  `model` is that in plain Python floats
(IEEE doubles).  A numpy that sums otherwise fails here, on the host, not as a GPU mystery.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pulsarfeatureextractor_amd import pfd
from test_scratch_layout_host import PFD_G_ALL, PFD_NSCAL, SAN_ENV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pulsarfeatureextractor_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "pfd_avgprof_layout_driver.cpp")
BUF = 8192
GIB = 1 << 30

# E -> a (npart, nsub, proflen) with that many values
E_SHAPES = {2: (1, 1, 2), 7: (1, 1, 7), 8: (1, 2, 4), 15: (1, 3, 5), 127: (1, 1, 127),
            128: (2, 4, 16), 129: (1, 3, 43), 136: (2, 4, 17), 968: (2, 4, 121), 969: (1, 3, 323),
            8191: (1, 1, 8191), 8192: (2, 32, 128), 8193: (1, 3, 2731), 8200: (5, 8, 205),
            16393: (13, 13, 97)}
TREE_SHAPES = [(9, 11, 128 + 8 * t) for t in range(0, 30, 3)]
DIVISORS = (3, 100, 128, 969)


def pairwise(y, lo, n):
    if n < 8:
        r = 0.0
        for i in range(n):
            r += y[lo + i]
        return r
    if n <= 128:
        nb = n - n % 8
        r = list(y[lo:lo + 8])
        for i in range(8, nb, 8):
            for j in range(8):
                r[j] += y[lo + i + j]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(nb, n):
            res += y[lo + i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(y, lo, n2) + pairwise(y, lo + n2, n - n2)


def model(x, L, chunked=True):
    """(x / L).sum() of the values x in memory order; chunked False: one tree over all of x."""
    y = (np.asarray(x, dtype=np.float64).ravel() / float(L)).tolist()
    if not chunked:
        return pairwise(y, 0, len(y))
    r = 0.0
    for lo in range(0, len(y), BUF):
        r += pairwise(y, lo, min(BUF, len(y) - lo))
    return r


def cube(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(1000.0, 300.0, size=shape)


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("L", DIVISORS)
def test_model_is_numpy(L):
    for E, shape in E_SHAPES.items():
        assert int(np.prod(shape)) == E
        x = cube(shape, 100 + E)
        assert same_bits(model(x, L), (x / L).sum()), (E, L)
    for shape in TREE_SHAPES:
        x = cube(shape, shape[2])
        assert same_bits(model(x, L), (x / L).sum()), (shape, L)


def test_chunks_are_not_one_tree():
    """On some 9 x 11 x (128 + 8t) the chunked rule and one tree over the cube part ways, and
    numpy goes with the chunks."""
    apart = 0
    for shape in TREE_SHAPES:
        x = cube(shape, shape[2])
        for L in DIVISORS:
            ref = (x / L).sum()
            assert same_bits(model(x, L), ref)
            apart += not same_bits(model(x, L, chunked=False), ref)
    assert apart >= 1


def test_signed_zero_and_big_endian():
    for shape in ((1, 2, 3), (1, 2, 8), (3, 43, 128)):  # E = 6, 16 and two chunks
        z = np.full(shape, -0.0)
        assert same_bits(model(z, shape[2]), 0.0) and same_bits((z / shape[2]).sum(), 0.0)
    assert same_bits(pairwise([-0.0] * 16, 0, 16), -0.0)  # the leaf itself keeps the sign
    x = cube((9, 11, 136), 5)
    assert same_bits((x.astype(">f8") / 136).sum(), model(x, 136))


# ---- reader and packer -------------------------------------------------------------------
def write_fold(path, shape, seed, big_endian=False):
    rng = np.random.default_rng(seed)
    profs = rng.normal(500.0, 40.0, size=shape)
    pfd.write(str(path), profs=profs, dms=np.linspace(10.0, 30.0, 21), bestdm=20.0,
              fold_p1=0.0123, big_endian=big_endian)
    return profs


@pytest.mark.parametrize("big_endian", (False, True))
def test_read_without_the_average(tmp_path, big_endian):
    p = tmp_path / "a.pfd"
    profs = write_fold(p, (3, 4, 100), 7, big_endian)
    full, bare = pfd.read(str(p)), pfd.read(str(p), avgprof=False)
    assert bare.avgprof is None
    assert same_bits(full.avgprof, (profs / 100).sum())       # the default read is unchanged
    assert same_bits(full.avgprof, model(profs, 100))
    for name, v in vars(full).items():
        if name == "avgprof":
            continue
        w = getattr(bare, name)
        assert np.array_equal(v, w) if isinstance(v, np.ndarray) else v == w, name
    pf, sf, sc = pfd.batch_inputs([full, bare])
    assert np.array_equal(pf[0], pf[1]) and np.array_equal(sf[0], sf[1])
    assert same_bits(sc[0, 2], full.avgprof) and np.isnan(sc[1, 2])
    assert np.array_equal(np.delete(sc[0], 2), np.delete(sc[1], 2))


def test_processor_fills_a_missing_average_for_a_foreign_engine(tmp_path):
    """A non-libpfe engine has no derive_avgprof: it gets scal complete."""
    from pulsarfeatureextractor_amd import processor

    p = tmp_path / "a.pfd"
    profs = write_fold(p, (2, 4, 16), 9)

    class Stub:
        def pfd_bates22(self, profs, subfreqs, scal, out=None, status=None):
            self.scal = scal
            return np.zeros((len(profs), 22)), np.zeros(len(profs), dtype=np.uint32)

    d, err = processor._read_pfd(str(p))
    assert err is None and d.avgprof is None
    eng = Stub()
    processor.score_pfd22([d], eng)
    assert same_bits(eng.scal[0, 2], (profs / 16).sum())


# ---- the scratch ------------------------------------------------------------------------
def nch(E):
    return (E + BUF - 1) // BUF


def f32_chunk(nsub, L, n, opt):
    c = max(1, GIB // (8 * nsub * L))
    if opt > 0:
        c = min(c, opt)
    return min(c, n)


def layout_cases():
    """(line, folds per pass, the regions the flag adds) per case of the driver."""
    out = []
    for (npart, nsub, L), n in (((2, 3, 8), 5), ((3, 4, 100), 7), ((4, 8, 128), 3),
                                ((13, 13, 97), 4), ((2, 128, 256), 3)):
        E = npart * nsub * L
        for host in (0, 1):
            for f32 in (0, 1):
                alone = [("profs32", n * E * 4) if f32 else ("profs", n * E * 8), ("out", n * 8)] if host else []
                out.append((f"avgprof {n} {npart} {nsub} {L} {host} {f32}", n,
                            alone + [("avg_csum", n * nch(E) * 8)]))
                for opt in ((0, 3) if f32 else (0,)):
                    folds = f32_chunk(nsub, L, n, opt) if f32 else n
                    new = [("avg_csum", folds * nch(E) * 8)]
                    new += [] if host else [("avg_scal", n * PFD_NSCAL * 8)]
                    for ws in (0, 3 * 256 * 17):
                        out.append((f"dmprof {n} {npart} {nsub} {L} {host} {f32} {opt} {ws}", folds, new))
                    for groups, k in ((PFD_G_ALL, 22), (3, 4)):
                        for tail in (0, 1):
                            if tail and (not f32 or n % folds == 0):
                                continue
                            out.append((f"scores {n} {npart} {nsub} {L} {host} {f32} {opt} {groups} {k} {tail}",
                                        folds, new))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"))
               if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("san") / "pfd_avgprof_layout_san")
    cmd = [cc, "--offload-host-only", "-x", "hip", "-std=c++17", "-g", "-O1",
           "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + CSRC, DRIVER, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr:
            pytest.skip("sanitizer runtimes not available: " + r.stderr[-200:])
        raise AssertionError(r.stderr[-4000:])
    return exe


def test_layouts_hold_the_new_regions(driver, tmp_path):
    grid = layout_cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _, _ in grid))
    r = subprocess.run([driver, str(path)], capture_output=True, text=True,
                       env={**os.environ, **SAN_ENV}, timeout=600)
    assert r.returncode == 0, f"layout driver failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done"
    got, cur = [], None
    for ln in lines[:-1]:
        w = ln.split(" ")
        if w[0] == "case":
            cur = {"line": ln[5:], "folds": None, "regions": [], "base": [], "total": None, "base_total": None}
            got.append(cur)
        elif w[0] == "folds":
            cur["folds"] = int(w[1])
        elif w[0] == "total":
            cur["total"] = int(w[1])
        elif w[0] == "base":
            if w[1] == "total":
                cur["base_total"] = int(w[2])
            else:
                cur["base"].append((w[1], int(w[2])))
        else:
            cur["regions"].append((w[0], int(w[1])))
    assert [g["line"] for g in got] == [line for line, _, _ in grid]
    rounded = lambda regions: sum((b + 255) // 256 * 256 for _, b in regions)  # noqa: E731
    for (line, folds, new), g in zip(grid, got):
        assert g["folds"] == folds, line
        assert g["total"] == rounded(g["regions"]), line
        if line.startswith("avgprof"):
            assert g["regions"] == new, line
            continue
        # the flag adds its regions and moves nothing out: without them, the unflagged layout
        names = [nm for nm, _ in new]
        assert [r for r in g["regions"] if r[0] in names] == new, line
        assert [r for r in g["regions"] if r[0] not in names] == g["base"], line
        assert g["base_total"] == rounded(g["base"]), line
        # behind the staged arrays and the part sums, in front of the pass's workspace
        order = [nm for nm, _ in g["regions"]]
        first = order.index("avg_csum")
        assert set(order[:first]) <= {"profs", "profs32", "subfreqs", "scal", "profile", "chis", "lyon8",
                                      "out", "status", "psum"}, line


def test_layout_grid_covers_what_it_should():
    lines = [ln.split() for ln, _, _ in layout_cases()]
    assert {w[0] for w in lines} == {"avgprof", "dmprof", "scores"}
    for kind in ("avgprof", "dmprof", "scores"):
        for host in "01":
            for f32 in "01":
                assert any(w[0] == kind and w[5] == host and w[6] == f32 for w in lines)
    assert any(w[0] == "scores" and w[10] == "1" for w in lines)  # a shorter last pass
    assert f32_chunk(4, 100, 7, 3) == 3 and 7 % 3 == 1
