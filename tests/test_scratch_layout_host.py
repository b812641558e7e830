"""The device-scratch layouts (csrc/arena.h, csrc/launch.h) on a CPU, under ASan + UBSan.

tests/native/layout_driver.cpp walks every layout function over a grid of shapes: it measures,
allocates exactly that many bytes, places, fills each region over its whole length and reads
all of them back (an overrun or an overlap ends it), and prints each region's byte count.
This test recomputes every count on its own: caller-visible arrays from the shapes
include/pfe.h documents, internal regions from the formulas the workspace has always used
(restated below, not read from the code under test).  Every count must match exactly and the
total must be the sum of the parts, each rounded up to 256 bytes.  CPU only: a stand-alone
program, nothing loaded into Python; skipped when hipcc or the sanitizer runtimes are absent.
"""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pulsarfeatureextractor_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "native", "layout_driver.cpp")
SAN_ENV = {"ASAN_OPTIONS": "abort_on_error=0:halt_on_error=1:detect_leaks=0:exitcode=66",
           "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1:exitcode=67"}

# ---- the workspace of the 22-score chain, as the kernels were written to find it ----------
SIZEOF_GAUSS_WS = 160            # 19 doubles + the bin count, padded to 8
NCOUNTERS = 16
WIDE_SLAB_BYTES = 16384 * (5 * 8 + 4)
GDG8_FPW, GLM_FPW, GLM4_FPW, BLM_FPW = 53, 32, 44, 32
NSCAL = PFD_NSCAL = 8
PFD_NDM = 100
BG_SINE, BG_GAUSS, BG_DM = 1, 2, 4
PFD_G_DM, PFD_G_ALL = 2, 7


def hand_bytes(n, region, lp, cus):
    k = (24, 24, 8)[region]                      # Gaussian, DM, sine
    slots = GDG8_FPW if region == 0 else GLM_FPW
    waves = min(max(n, 1), cus * (8 if region == 0 else 12))
    return waves * slots * k * (32 if lp > 128 else 16) * 8


def persistent_waves(n, cus):
    fpw = min(max(n // (cus * 64), 4), BLM_FPW)
    return min(max(-(-n // fpw), 1), cus * 8)


def gdg_wave_scratch_doubles(lp):
    mpl = 1 if lp <= 64 else 2 if lp <= 128 else 4 if lp <= 256 else 16
    return max(GLM4_FPW, BLM_FPW) * 64 * mpl * 2


def bates_regions(n, lp, sub_bytes, cus):
    r = [("gauss_ws", n * SIZEOF_GAUSS_WS), ("counters", NCOUNTERS * 4),
         ("hand_gauss", hand_bytes(n, 0, lp, cus)), ("hand_dm", hand_bytes(n, 1, lp, cus)),
         ("hand_sine", hand_bytes(n, 2, lp, cus)), ("wide_list", n * 4),
         ("wide_slabs", min(max(n // 64, 1), 256) * WIDE_SLAB_BYTES),
         ("wave_scratch", persistent_waves(n, cus) * gdg_wave_scratch_doubles(lp) * 8)]
    return r + ([("sub_work", sub_bytes)] if sub_bytes else [])


def subband_work_bytes(n, nsub, lsb):
    """0 for the shapes the on-chip kernels hold, else one slab per wave of the any-shape one."""
    if 2 <= nsub <= 256 and 1 <= lsb <= 1024 and nsub * (lsb + 1) <= 32768:
        return 0
    slab = ((lsb + 1) * 4 + 15) // 16 * 16 + lsb * 8 + (nsub * 4 + 15) // 16 * 16
    return min(max(n, 1), 1024) * slab


def pfd22_regions(n, L, groups, cus):
    r = [("profile", n * L * 8)] if groups == PFD_G_ALL else []
    if groups & PFD_G_DM:
        r.append(("chis", n * PFD_NDM * 4))
    r.append(("par22", n * 8 * 8))
    return r + (bates_regions(n, L, 0, cus) if groups & PFD_G_DM else [])


def pfd_inputs(n, npart, nsub, L):
    return [("profs", n * npart * nsub * L * 8), ("subfreqs", n * nsub * 8), ("scal", n * PFD_NSCAL * 8)]


# ---- the grid: (case line, expected regions) -------------------------------------------------
NS = (1, 3, 67, 4096)
LPS = (8, 64, 128, 200, 256, 512, 1024)
SUBS = ((16, 64), (257, 16))
PFDS = ((2, 4, 32), (4, 40, 300))


def n_lp_cus(full):
    """(n, lp, compute units).  full (the chain's workspace by itself): every n with every lp,
    the 90-700 MB per-wave scratch of 4096 profiles of over 64 bins on a whole device kept to
    an 8-CU one.
    Else (the calls around it): every lp at 1 and 3 candidates; the workspace of 67 is
    20-50 MB and that of 4096 more, which the driver fills and reads back, so two lengths
    and one."""
    for n, lp in itertools.product(NS, LPS):
        if full or n < 67 or lp == 64 or (n == 67 and lp == 200):
            yield n, lp, (8 if n == 4096 and (lp > 64 or not full) else 256)
    yield 67, 64, 8


def few(n, *primary):
    """The caps that 4096 candidates reach belong to the chain's workspace, so the calls around
    it see 4096 in their primary configuration only (host arrays, hand-over on, ...)."""
    return n == 4096 and not all(primary)


def cases():
    out = []
    for (n, lp, cus), ho in itertools.product(n_lp_cus(True), (0, 1)):
        for nsub, lsb in SUBS:
            if few(n, ho):
                continue
            sw = subband_work_bytes(n, nsub, lsb)
            out.append((f"bates {n} {lp} {sw} {cus} {ho}", bates_regions(n, lp, sw, cus)))
    for (n, lp, cus), host, ho in itertools.product(n_lp_cus(False), (0, 1), (0, 1)):
        for (nsub, lsb), chain in itertools.product(SUBS, (0, 1)):
            if (ho == 0 and not chain) or few(n, host, ho, chain):
                continue
            ndm = 41
            sw = subband_work_bytes(n, nsub, lsb)
            r = []
            if host:
                r = [("prof", n * lp), ("sub", n * nsub * lsb)]
                r += [("dmcurve", n * ndm * 8)] if chain else []
                r += [("scal", n * NSCAL * 8), ("out", n * (22 if chain else 3) * 8), ("status", n * 4)]
            if chain:
                r += bates_regions(n, lp, sw, cus)
            elif sw:
                r.append(("sub_work", sw))
            out.append((f"score {n} {lp} {nsub} {lsb} {ndm} {host} {chain} {sw} {cus} {ho}", r))
        # the group calls: sinusoid4, gauss7, dmfit4 (no profile: lp = 0), the f64 forms, params4
        for g, f64, k in ((BG_SINE, 0, 4), (BG_GAUSS, 0, 7), (BG_DM, 0, 4), (BG_SINE, 1, 4),
                          (BG_GAUSS, 1, 7), (0, 0, 4)):
            if (g == 0 and ho == 0) or few(n, host, ho):
                continue
            glp, ndm = (0, 57) if g == BG_DM else (lp, 0)
            r = []
            if host:
                if g == BG_DM:
                    r.append(("dmcurve", n * ndm * 8))
                elif f64:
                    r.append(("fprof", n * glp * 8))
                elif g:
                    r.append(("prof", n * glp))
                if not f64:
                    r.append(("scal", n * NSCAL * 8))
            if g:
                r.append(("d22", n * 22 * 8))
            if host:
                r += [("out", n * k * 8), ("status", n * 4)]
            if g:
                r += bates_regions(n, glp, 0, cus)
            out.append((f"group {n} {glp if g else 0} {ndm} {g} {f64} {k} {host} {cus if g else 0} {ho}", r))
    for (npart, nsub, L), n in itertools.product(PFDS, NS):
        if n == 4096 and L == 300:
            continue    # 1.5 GB of folds; the small shape carries n = 4096
        for groups, ho in itertools.product(range(1, 8), (0, 1)):
            if few(n, ho):
                continue
            out.append((f"pfd22 {n} {L} {groups} 256 {ho}", pfd22_regions(n, L, groups, 256)))
        chunk = min(n, 4096)
        for host, (prof, chis, lyon8), ws in itertools.product(
                (0, 1), ((1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 1)),
                (0, 2 * chunk * nsub * L * 8, 3 * 256 * 17)):
            r = []
            if host:
                r = pfd_inputs(n, npart, nsub, L)
                r += [("profile", n * L * 8)] if prof else []
                r += [("chis", n * PFD_NDM * 4)] if chis else []
                r += [("lyon8", n * 8 * 8)] if lyon8 else []
                r.append(("status", n * 4))
            r += [("ws", ws)] if ws else []
            out.append((f"pfd_dmprof {n} {npart} {nsub} {L} {host} {prof} {chis} {lyon8} {ws}", r))
        for host, groups, gb, ho in itertools.product((0, 1), range(1, 8), (0, 5 * 256 * 31), (0, 1)):
            k = 22 if groups == PFD_G_ALL else 4
            if few(n, host, ho, gb, groups in (1, 3, 7)) or (n == 67 and ho != (gb != 0)):
                continue
            r = []
            if host:
                r = pfd_inputs(n, npart, nsub, L) + [("out", n * k * 8), ("status", n * 4)]
            if groups != PFD_G_ALL:
                r.append(("d22", n * 22 * 8))
            r += pfd22_regions(n, L, groups, 256)
            r += [("tg", gb)] if gb else []
            out.append((f"pfd_scores {n} {npart} {nsub} {L} {host} {groups} {k} {gb} 256 {ho}", r))
    for size, (chunk, lp, ld) in itertools.product((1, 8), ((1, 1, 1), (3, 64, 128), (67, 129, 3), (1024, 128, 257))):
        out.append((f"lyon8 {size} {chunk} {lp} {ld}",
                    [("prof", chunk * lp * size), ("dm", chunk * ld * size), ("out", chunk * 8 * 8)]))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"))
               if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("san") / "layout_san")
    cmd = [cc, "--offload-host-only", "-x", "hip", "-std=c++17", "-g", "-O1",
           "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + CSRC, DRIVER, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr:
            pytest.skip("sanitizer runtimes not available: " + r.stderr[-200:])
        raise AssertionError(r.stderr[-4000:])
    return exe


def test_every_layout_matches_its_formulas(driver, tmp_path):
    grid = cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _ in grid))
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
            cur = [val, [], None]
            got.append(cur)
        elif name == "total":
            cur[2] = int(val)
        else:
            cur[1].append((name, int(val)))
    assert [g[0] for g in got] == [line for line, _ in grid]
    for (line, want), (_, regions, total) in zip(grid, got):
        assert regions == want, line
        assert total == sum((b + 255) // 256 * 256 for _, b in want), line


def test_grid_covers_what_it_should():
    lines = [line for line, _ in cases()]
    kinds = {ln.split()[0] for ln in lines}
    assert kinds == {"bates", "pfd22", "score", "group", "pfd_dmprof", "pfd_scores", "lyon8"}
    assert subband_work_bytes(67, 16, 64) == 0 and subband_work_bytes(67, 257, 16) == 67 * 1248
    for n, lp in itertools.product(NS, LPS):
        assert any(ln.startswith(f"bates {n} {lp} ") for ln in lines)
    assert {int(ln.split()[3]) for ln in lines if ln.startswith("pfd22 ")} == set(range(1, 8))
