"""The scratch of pfe_subband3_f64 / pfe_bates22_f64 (csrc/launch.h: subf64_plan and
subband_f64_layout) on a CPU, under ASan + UBSan.

tests/native/subband_f64_layout_driver.cpp plans and walks the layout over on-chip and global
shapes, for host and device pointers: it measures, allocates exactly that many bytes, places,
fills each region and each wave's slab over its whole length and reads the regions back (an
overrun or an overlap ends it), and prints the plan and each region's byte count.  This test
recomputes the plan and every count on its own, from the rule include/pfe.h documents.  CPU
only: a stand-alone program, nothing loaded into Python; skipped when hipcc or the sanitizer
runtimes are absent.
"""
import os
import shutil
import subprocess

import pytest

from test_scratch_layout_host import SAN_ENV, bates_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pulsarfeatureextractor_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "subband_f64_layout_driver.cpp")
LDS = 160 * 1024
NSCAL = 8


def up(x, a):
    return (x + a - 1) // a * a


def plan(nsub, lsb, n, cus, force):
    """(ok, global, LDS bytes per wave, of which T, slab bytes, waves per block, blocks)."""
    vec = up((2 * lsb + 3 * nsub) * 8, 16)
    if vec > LDS:
        return (0, 0, 0, 0, 0, 0, 0)
    t = up(nsub * lsb * 8, 16)
    glob = bool(force) or t + vec > LDS
    t_lds = 0 if glob else t
    wave = t_lds + vec
    wpb = min(LDS // wave, 8)
    per_cu = min(LDS // (wpb * wave), 32 // wpb)
    blocks = min(cus * per_cu, -(-n // wpb))
    slab = 0
    if glob:
        slab = up(nsub * lsb * 8, 256)
        budget = (1 << 30) // slab
        wpb = min(wpb, budget)
        if blocks * wpb > budget:
            blocks = budget // wpb
    return (1, int(glob), wave, t_lds, slab, wpb, max(blocks, 1))


def cases():
    out = []
    # on chip by default; beyond the LDS (global either way); the last two refused
    shapes = [(16, 128), (32, 128), (2, 8), (5, 37), (3, 1024), (1, 1),
              (9, 2047), (80, 256), (1024, 2048), (600, 300), (6000, 1239),
              (7000, 2), (1, 10241)]
    for (nsub, lsb) in shapes:
        big = nsub * lsb > 100000
        for n in ((1, 3) if big else (1, 5, 67, 4096)):
            for host in (0, 1):
                if host and n * nsub * lsb * 8 > (64 << 20):
                    continue
                for force in (0, 1):
                    for chain in (0, 1):
                        cus = 8 if (chain or n == 4096) else 256
                        lp = lsb if 8 <= lsb <= 1024 else 64
                        if chain and (big or n == 4096 and lp > 64):
                            continue    # the chain's own workspace is the other layout test's
                        ndm = 41
                        p = plan(nsub, lsb, n, cus, force)
                        r = []
                        if p[0]:
                            if host:
                                r = [("prof", n * lp * 8), ("sub", n * nsub * lsb * 8)]
                                r += [("dmcurve", n * ndm * 8)] if chain else []
                                r += [("scal", n * NSCAL * 8), ("out", n * (22 if chain else 3) * 8),
                                      ("status", n * 4)]
                            if chain:
                                r += bates_regions(n, lp, 0, cus)
                            if p[1]:
                                r.append(("slabs", p[4] * p[5] * p[6]))
                        out.append((f"{n} {lp} {nsub} {lsb} {ndm} {host} {chain} {force} {cus}", p, r))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"))
               if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("san") / "subband_f64_layout_san")
    cmd = [cc, "--offload-host-only", "-x", "hip", "-std=c++17", "-g", "-O1",
           "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + CSRC, DRIVER, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr:
            pytest.skip("sanitizer runtimes not available: " + r.stderr[-200:])
        raise AssertionError(r.stderr[-4000:])
    return exe


def test_plan_and_layout_match_the_documented_rule(driver, tmp_path):
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
            cur = {"line": val, "plan": None, "regions": [], "total": None}
            got.append(cur)
        elif name == "plan":
            cur["plan"] = tuple(int(x) for x in val.split())
        elif name == "total":
            cur["total"] = int(val)
        else:
            cur["regions"].append((name, int(val)))
    assert [g["line"] for g in got] == [line for line, _, _ in grid]
    for (line, p, want), g in zip(grid, got):
        assert g["plan"] == p, line
        if not p[0]:
            assert g["total"] is None and not g["regions"], line
            continue
        assert g["regions"] == want, line
        assert g["total"] == sum(up(b, 256) for _, b in want), line


def test_grid_covers_what_it_should():
    grid = cases()
    plans = {(line.split()[2], line.split()[3], line.split()[7]): p for line, p, _ in grid}
    assert plans[("16", "128", "0")][:2] == (1, 0) and plans[("16", "128", "1")][:2] == (1, 1)
    assert plans[("80", "256", "0")][:2] == (1, 1)
    assert plans[("1024", "2048", "0")][0] == 1      # the largest shape the header promises
    assert plans[("7000", "2", "0")][0] == 0 and plans[("1", "10241", "0")][0] == 0
    # 16 x 128: about 19 KiB per wave, eight waves to a block; 32 x 128: four
    assert plan(16, 128, 65536, 256, 0)[2:] == (18816, 16384, 0, 8, 256)
    assert plan(32, 128, 65536, 256, 0)[2:] == (35584, 32768, 0, 4, 256)
    for host in "01":
        for chain in "01":
            assert any(ln.split()[5] == host and ln.split()[6] == chain for ln, _, _ in grid)
