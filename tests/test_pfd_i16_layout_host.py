"""The scratch of the pfe_pfd_*_i16 calls (csrc/launch.h: pfd_f32_chunk and the int16 forms of
pfd_dmprof_layout, pfd_scores_layout and pfd_avgprof_layout) on a CPU, under ASan + UBSan.

tests/native/pfd_i16_layout_driver.cpp sizes the pass and walks the layouts for host and device
pointers, with and without weights and PFE_FLAG_PFD_AVGPROF, over shapes of every route of the
f64 kernels -- no workspace (the fold in LDS), the two part-sum buffers of the split pipeline,
the slabs of the global-memory kernel -- with the default pass, a pass of one fold, and a shape
whose default pass the 1 GiB bound cuts: it measures, allocates exactly that many bytes, places,
fills every region over its whole length and reads it back (an overrun or an overlap ends it),
and prints the pass and each region's byte count.  This test recomputes the pass and every count
on its own, from the rule include/pfe.h states: the arrays a host call stages (the cube as int16,
then scl, offs and, when given, wts as floats), chunk x nsub x proflen doubles of part sums, then
the scratch of the f64 call on the folds of one pass.  CPU only: a stand-alone program, nothing
loaded into Python; skipped when hipcc or the sanitizer runtimes are absent.
"""
import os
import shutil
import subprocess

import pytest

from test_scratch_layout_host import PFD_G_ALL, PFD_NDM, PFD_NSCAL, SAN_ENV, pfd22_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pulsarfeatureextractor_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "pfd_i16_layout_driver.cpp")
GIB = 1 << 30


def chunk_of(nsub, L, n, opt):
    """Folds per pass: min(n, max(1, 2^30 / (8 x nsub x proflen))), or the option when smaller."""
    c = max(1, GIB // (8 * nsub * L))
    if opt > 0:
        c = min(c, opt)
    return min(c, n)


def staged(n, npart, nsub, L, wts):
    """What a host-pointer call stages of the cube: int16 values, float parameters."""
    par = n * npart * nsub * 4
    return ([("data16", n * npart * nsub * L * 2), ("scl16", par), ("offs16", par)]
            + ([("wts16", par)] if wts else []))


def inputs(n, npart, nsub, L, wts):
    return staged(n, npart, nsub, L, wts) + [("subfreqs", n * nsub * 8), ("scal", n * PFD_NSCAL * 8)]


def avg_work(n, npart, nsub, L, host, folds):
    """PFE_FLAG_PFD_AVGPROF: the chunk sums of one pass, and a copy of scal for device pointers."""
    r = [("avg_csum", folds * -(-npart * nsub * L // 8192) * 8)]
    return r + ([] if host else [("avg_scal", n * PFD_NSCAL * 8)])


# (npart, nsub, proflen), n: the routes' shapes of tests/test_pfd_i16_gpu.py, the fold of more
# than 8192 values of its average test, and 5000 folds of 128 x 256 (256 KiB of part sums each:
# 4096 to the GiB)
SHAPES = [((7, 8, 64), 5), ((4, 16, 128), 5), ((3, 5, 33), 67), ((2, 4, 200), 3),
          ((2, 128, 256), 3), ((1, 2, 8), 1), ((3, 32, 128), 2)]
BIG = ((2, 128, 256), 5000)


def cases():
    out = []
    for (npart, nsub, L), n in SHAPES + [BIG]:
        big = n == 5000
        for host, opt, wts, avg in ((0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 1, 1), (1, 1, 0, 1), (0, 2, 0, 0),
                                    (1, 64, 1, 1)):
            if big and (host or opt):
                continue        # 2.6 GB of values to stage; the cut pass is the point
            c = chunk_of(nsub, L, n, opt)
            psum = [("psum", c * nsub * L * 8)]
            psum += avg_work(n, npart, nsub, L, host, c) if avg else []
            # pfe_pfd_dmprof_i16: fused in LDS, the split pipeline's two buffers, slabs
            for (prof, chis, lyon8), ws in (((1, 1, 1), 0), ((1, 0, 0), 2 * min(c, 4096) * nsub * L * 8),
                                            ((0, 1, 1), 3 * 256 * 17)):
                if big and ws:
                    continue
                r = []
                if host:
                    r = inputs(n, npart, nsub, L, wts)
                    r += [("profile", n * L * 8)] if prof else []
                    r += [("chis", n * PFD_NDM * 4)] if chis else []
                    r += [("lyon8", n * 8 * 8)] if lyon8 else []
                    r.append(("status", n * 4))
                r += psum
                r += [("ws", ws)] if ws else []
                out.append((f"dmprof {n} {npart} {nsub} {L} {host} {opt} {wts} {prof} {chis} {lyon8} {ws} {avg}",
                            c, r))
            # pfe_pfd_avgprof_i16
            line = f"avgprof {n} {npart} {nsub} {L} {host} 0 {wts}"
            if not big and all(line != ln for ln, _, _ in out):
                r = staged(n, npart, nsub, L, wts) + [("out", n * 8)] if host else []
                r.append(("avg_csum", n * -(-npart * nsub * L // 8192) * 8))
                out.append((line, n, r))
            # the score calls: the chain and the three groups; the last pass where there is one
            if nsub < 2 or not 8 <= L <= 1024:
                continue
            for groups, k, gb in ((PFD_G_ALL, 22, 0), (1, 4, 0), (3, 4, 5 * 256 * 31), (5, 3, 0)):
                if big and groups != 5:
                    continue
                # only the chi^2 sweep reads the average
                gavg = avg and bool(groups & 2)
                for tail in (0, 1):
                    if tail and n % c == 0:
                        continue
                    wn = n % c if tail else c
                    r = []
                    if host:
                        r = inputs(n, npart, nsub, L, wts) + [("out", n * k * 8), ("status", n * 4)]
                    r.append(psum[0])
                    r += avg_work(n, npart, nsub, L, host, c) if gavg else []
                    if groups != PFD_G_ALL:
                        r.append(("d22", wn * 22 * 8))
                    r += pfd22_regions(wn, L, groups, 256)
                    r += [("tg", gb)] if gb else []
                    out.append((f"scores {n} {npart} {nsub} {L} {host} {opt} {wts} {groups} {k} {gb} 256 "
                                f"{tail} {int(gavg)}", c, r))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"))
               if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("san") / "pfd_i16_layout_san")
    cmd = [cc, "--offload-host-only", "-x", "hip", "-std=c++17", "-g", "-O1",
           "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + CSRC, DRIVER, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr:
            pytest.skip("sanitizer runtimes not available: " + r.stderr[-200:])
        raise AssertionError(r.stderr[-4000:])
    return exe


def test_pass_and_layout_match_the_documented_rule(driver, tmp_path):
    grid = cases()
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
        name, _, val = ln.partition(" ")
        if name == "case":
            cur = {"line": val, "chunk": None, "regions": [], "total": None}
            got.append(cur)
        elif name in ("chunk", "total"):
            cur[name] = int(val)
        else:
            cur["regions"].append((name, int(val)))
    assert [g["line"] for g in got] == [line for line, _, _ in grid]
    for (line, c, want), g in zip(grid, got):
        assert g["chunk"] == c, line
        assert g["regions"] == want, line
        assert g["total"] == sum((b + 255) // 256 * 256 for _, b in want), line


def test_grid_covers_what_it_should():
    grid = cases()
    lines = [ln.split() for ln, _, _ in grid]
    assert {w[0] for w in lines} == {"dmprof", "scores", "avgprof"}
    for kind in ("dmprof", "scores", "avgprof"):
        for host in "01":
            for wts in "01":
                assert any(w[0] == kind and w[5] == host and w[7] == wts for w in lines), (kind, host, wts)
    assert any(w[0] == "scores" and w[12] == "1" for w in lines)       # a shorter last pass
    assert any(w[0] == "scores" and w[13] == "1" for w in lines)       # a derived average
    assert any(w[0] == "dmprof" and w[12] == "1" and w[5] == "0" for w in lines)
    assert {w[6] for w in lines} >= {"0", "1"}                         # default and one fold
    # the bound cuts 5000 folds of 128 x 256 to 4096, exactly 1 GiB of part sums
    assert chunk_of(128, 256, 5000, 0) == 4096 and 4096 * 128 * 256 * 8 == GIB
    assert any(w[1] == "5000" and c == 4096 for w, (_, c, _) in zip(lines, grid))
    assert chunk_of(5, 33, 67, 0) == 67 and chunk_of(5, 33, 67, 64) == 64 and chunk_of(5, 33, 5, 64) == 5
