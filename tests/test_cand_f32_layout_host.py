"""The scratch of the float32 forms of the float-array calls (csrc/launch.h: subband_f32_layout,
the f32 form of group_layout, lyon8_slot_layout<float>) on a CPU, under ASan + UBSan.

tests/native/cand_f32_layout_driver.cpp walks the layouts for host and device pointers over the
shapes of tests/test_cand_f32_gpu.py: it measures, allocates exactly that many bytes, places,
fills every region over its whole length and reads it back (an overrun or an overlap ends it),
writes the last element each kernel or copy touches, and prints each region's byte count.  This
test recomputes every count on its own, from the rule include/pfe.h states: the scratch of the
f64 call of the same name, plus n x lp doubles (the profile fits and the 22-score call) and
n x ndm doubles (the 22-score call) of widened copies, with the arrays a host call stages held
as floats; the sub-bands are never widened in memory, so pfe_subband3_f32 on device pointers
takes the f64 call's slabs and nothing else.  CPU only: a stand-alone program, nothing loaded
into Python; skipped when hipcc or the sanitizer runtimes are absent.
"""
import os
import shutil
import subprocess

import pytest

from test_scratch_layout_host import BG_GAUSS, BG_SINE, NSCAL, SAN_ENV, bates_regions
from test_subband_f64_layout_host import plan, up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pulsarfeatureextractor_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "cand_f32_layout_driver.cpp")

# (nsub, lsb), n: the sub-band shapes of the GPU tests
SUB_SHAPES = [((16, 128), 64), ((32, 128), 64), ((3, 5), 64), ((2, 8), 64), ((16, 968), 64),
              ((16, 976), 64), ((96, 256), 8), ((1, 16), 8)]
LPS = (8, 64, 128, 200, 300)


def score_case(n, lp, nsub, lsb, ndm, host, chain, force, cus):
    p = plan(nsub, lsb, n, cus, force)
    assert p[0]
    slab = p[4] * p[5] * p[6] if p[1] else 0
    r = []
    if host:
        r = [("prof", n * lp * 4), ("sub", n * nsub * lsb * 4)]
        r += [("dmcurve", n * ndm * 4)] if chain else []
        r += [("scal", n * NSCAL * 8), ("out", n * (22 if chain else 3) * 8), ("status", n * 4)]
    if chain:
        r += [("fprof", n * lp * 8), ("fdm", n * ndm * 8)] + bates_regions(n, lp, 0, cus)
    if slab:
        r.append(("slabs", slab))
    return f"score {n} {lp} {nsub} {lsb} {ndm} {host} {chain} {force} {cus}", slab, r


def cases():
    out = []
    for (nsub, lsb), n in SUB_SHAPES:
        for host in (0, 1):
            for force in (0, 1):
                out.append(score_case(n, lsb, nsub, lsb, 0, host, 0, force, 256))
                if 8 <= lsb <= 1024 and nsub > 1:
                    for ndm in (3, 120):
                        out.append(score_case(n, lsb, nsub, lsb, ndm, host, 1, force, 8))
    out.append(score_case(64, 64, 16, 128, 0, 1, 0, 0, 256))      # lp != lsb: every row fails
    for lp in LPS:
        for g, k in ((BG_SINE, 4), (BG_GAUSS, 7)):
            for host in (0, 1):
                n = 64
                r = [("prof32", n * lp * 4)] if host else []
                r += [("fprof", n * lp * 8), ("d22", n * 22 * 8)]
                r += [("out", n * k * 8), ("status", n * 4)] if host else []
                r += bates_regions(n, lp, 0, 8)
                out.append((f"group {n} {lp} {g} {k} {host} 8", None, r))
    for chunk, lp, ld in ((1, 1, 1), (17, 969, 8193), (1024, 128, 100)):
        out.append((f"lyon8 {chunk} {lp} {ld}", None,
                    [("prof", chunk * lp * 4), ("dm", chunk * ld * 4), ("out", chunk * 8 * 8)]))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"))
               if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("san") / "cand_f32_layout_san")
    cmd = [cc, "--offload-host-only", "-x", "hip", "-std=c++17", "-g", "-O1",
           "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + CSRC, DRIVER, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr:
            pytest.skip("sanitizer runtimes not available: " + r.stderr[-200:])
        raise AssertionError(r.stderr[-4000:])
    return exe


def test_layouts_match_the_documented_rule(driver, tmp_path):
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
            cur = {"line": val, "slab": None, "regions": [], "total": None}
            got.append(cur)
        elif name in ("slab", "total"):
            cur[name] = int(val)
        else:
            cur["regions"].append((name, int(val)))
    assert [g["line"] for g in got] == [line for line, _, _ in grid]
    for (line, slab, want), g in zip(grid, got):
        assert g["slab"] == slab, line
        assert g["regions"] == want, line
        assert g["total"] == sum(up(b, 256) for _, b in want), line


def test_grid_covers_what_it_should():
    grid = cases()
    words = [ln.split() for ln, _, _ in grid]
    assert {w[0] for w in words} == {"score", "group", "lyon8"}
    for host in "01":
        for chain in "01":
            assert any(w[0] == "score" and w[6] == host and w[7] == chain for w in words)
        assert any(w[0] == "group" and w[5] == host for w in words)
    # the sub-band call on device pointers: on chip nothing at all, else the f64 call's slabs
    by = {ln: (slab, r) for ln, slab, r in grid}
    assert by["score 64 128 16 128 0 0 0 0 256"] == (0, [])
    slab, r = by["score 8 256 96 256 0 0 0 0 256"]
    assert slab > 0 and r == [("slabs", slab)]
    slab, r = by["score 64 128 16 128 0 0 0 1 256"]
    assert slab == 64 * up(16 * 128 * 8, 256) and r == [("slabs", slab)]
