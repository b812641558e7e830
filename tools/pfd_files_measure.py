"""What the .pfd file path delivers, end to end: files/s and bytes/s of the reader alone and of
dmprofPFD, for this tree and for a checkout of another revision (the parent commit), alternating.

  python tools/pfd_files_measure.py --other PATH_TO_PARENT_CHECKOUT [--reps 3] [--workers 16]

writes synthetic files to a temporary directory -- 512 at 64 x 32 x 128 and 64 at 64 x 96 x 256,
half of each big-endian (1.9 GB) --, reads them once so they sit in the page cache, and then runs,
for each tree in turn and --reps times over, a fresh Python process that imports that tree's
package and times, for each of the four (shape, byte order) groups,
  (a) the reader alone: this tree's native scan + pack into a pinned slab (pfe_pfd_scan,
      pfe_pfd_pack); a tree without them: pfd.read of every file and pfd.batch_inputs, what its
      processor does before it calls the engine;
  (b) DataProcessor.dmprofPFD on the group's directory, from the walk to the written score file.
Both are timed by the host clock around work that ends synchronised (the packed slab is complete;
the score file is written).  Each process first runs (b) on a few files to load the code objects.
It also measures, for this tree: the host-to-device rate of a pinned 256 MiB copy (for scale), and
for byte-reversed cubes on the host the flagged call (byteswapped=True) against cube.byteswap() on
the host followed by the unflagged call, alternating.  Prints a report; profiles/
pfd_native_measure.txt is one.  --workers: the host threads of both trees' readers (the share of
a machine a job may use, not os.cpu_count())."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = [((64, 32, 128), 256), ((64, 96, 256), 32)]  # shape, files per byte order
SLAB = 256 << 20


def group_dirs(root):
    return [(shape, big, os.path.join(root, f"{shape[1]}x{shape[2]}_{'be' if big else 'le'}"), n)
            for shape, n in GROUPS for big in (False, True)]


def make_files(root):
    sys.path.insert(0, ROOT)
    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd.synth import pfd_candidate

    total = 0
    for shape, big, d, n in group_dirs(root):
        os.makedirs(d)
        for k in range(n):
            c = pfd_candidate(np.random.default_rng(1000 * shape[2] + 2 * k + big), *shape)
            p = os.path.join(d, f"c{k:04d}.pfd")
            pfd.write(p, big_endian=big, **c)
            total += os.path.getsize(p)
    for dirpath, _dn, files in os.walk(root):  # once through the page cache
        for f in files:
            with open(os.path.join(dirpath, f), "rb") as fh:
                while fh.read(1 << 24):
                    pass
    return total


# ---- one tree, one process -------------------------------------------------------------------
def reader_alone(paths, shape, workers):
    """Seconds to bring every file's inputs to where the engine call takes them from."""
    from pulsarfeatureextractor_amd import _native, pfd

    fold = 8 * shape[0] * shape[1] * shape[2]
    per = max(1, SLAB // fold)
    if hasattr(_native, "PfdBatch"):
        slab = _native.host_empty((per * fold,), np.uint8)
        small = {}

        def alloc(name, shp, dt):
            if name == "profs":
                return slab[:shp[0] * fold].view(np.float64).reshape(shp)
            a = small.get((name, shp))
            if a is None:
                a = small[(name, shp)] = np.empty(shp, dtype=dt)
            return a

        t0 = time.perf_counter()
        b = _native.PfdBatch(paths, threads=workers)
        inf = b.infos()
        assert (inf["status"] == 0).all()
        rows = np.arange(len(paths))
        for s0 in range(0, len(rows), per):
            b.pack(rows[s0:s0 + per], shape, threads=workers, alloc=alloc)
        dt = time.perf_counter() - t0
        b.close()
        return dt
    t0 = time.perf_counter()
    datas = [pfd.read(p, avgprof=False) for p in paths]
    for s0 in range(0, len(datas), per):
        pfd.batch_inputs(datas[s0:s0 + per])
    return time.perf_counter() - t0


def end_to_end(directory, out, engine, workers):
    from pulsarfeatureextractor_amd import processor

    if os.path.exists(out):
        os.remove(out)
    t0 = time.perf_counter()
    dp = processor.DataProcessor(engine=engine, workers=workers, log=lambda *a: None)
    dp.dmprofPFD(directory + "/", False, out, False, False)
    dt = time.perf_counter() - t0
    with open(out) as f:
        lines = sum(1 for _ in f)
    return dt, lines


def h2d_rate():
    import torch

    src = torch.empty(SLAB, dtype=torch.uint8).pin_memory()
    dst = torch.empty(SLAB, dtype=torch.uint8, device="cuda")
    dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    best = None
    for _ in range(5):
        t0 = time.perf_counter()
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return SLAB / best


def swap_compare(engine, files, shape, reps):
    """Byte-reversed cubes in host memory: the flagged call against cube.byteswap() on the host
    plus the unflagged call, alternating -> [(flagged s, host swap + unflagged s)]."""
    from pulsarfeatureextractor_amd import pfd

    datas = [pfd.read(p, avgprof=False) for p in files]
    profs, fr, sc = pfd.batch_inputs(datas)
    xs = profs.byteswap()
    out = []
    a = engine.pfd_dmprof(xs, fr, sc, chis=False, derive_avgprof=True, byteswapped=True)
    b = engine.pfd_dmprof(xs.byteswap(), fr, sc, chis=False, derive_avgprof=True)
    same = all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))
               for k in ("profile", "lyon8", "status"))
    for _ in range(reps):
        t0 = time.perf_counter()
        engine.pfd_dmprof(xs, fr, sc, chis=False, derive_avgprof=True, byteswapped=True)
        t1 = time.perf_counter()
        engine.pfd_dmprof(xs.byteswap(), fr, sc, chis=False, derive_avgprof=True)
        out.append((t1 - t0, time.perf_counter() - t1))
    return out, same, len(files)


def one_tree(tree, root, workers, extras):
    """Runs inside the fresh process of one tree."""
    sys.path.insert(0, tree)
    os.chdir(tempfile.mkdtemp(dir=root))  # CandidateErrorLog.txt of the runs
    from pulsarfeatureextractor_amd import _native

    assert os.path.dirname(os.path.abspath(_native.__file__)).startswith(os.path.abspath(tree))
    engine = _native.Engine(0)
    res = {"tree": tree, "native": hasattr(_native, "PfdBatch"), "groups": []}
    warm = os.path.join(os.getcwd(), "warm")
    os.makedirs(warm)
    for shape, big, d, n in group_dirs(root):
        for k in range(2):
            shutil.copy(os.path.join(d, f"c{k:04d}.pfd"), os.path.join(warm, f"{shape[2]}{int(big)}{k}.pfd"))
    end_to_end(warm, "warm.csv", engine, workers)
    for shape, big, d, n in group_dirs(root):
        paths = sorted(os.path.join(d, f) for f in os.listdir(d))
        nbytes = sum(os.path.getsize(p) for p in paths)
        rd = reader_alone(paths, shape, workers)
        e2e, lines = end_to_end(d, "out.csv", engine, workers)
        assert lines == len(paths), (lines, len(paths))
        res["groups"].append({"shape": list(shape), "big_endian": big, "files": len(paths),
                              "bytes": nbytes, "reader_s": rd, "e2e_s": e2e})
    if extras:
        res["h2d_bytes_per_s"] = h2d_rate()
        res["swap"] = []
        for shape, big, d, n in group_dirs(root):
            if big:
                continue
            files = sorted(os.path.join(d, f) for f in os.listdir(d))[:max(8, n // 2)]
            t, same, nf = swap_compare(engine, files, shape, 3)
            res["swap"].append({"shape": list(shape), "folds": nf, "same_bits": bool(same),
                                "flagged_s": [x[0] for x in t], "host_swap_s": [x[1] for x in t]})
    engine.close()
    print("RESULT " + json.dumps(res), flush=True)


def report(runs, total, workers):
    def rate(g, key):
        return g["files"] / g[key], g["bytes"] / g[key] / 1e9

    print(f"synthetic .pfd files: {total / 1e9:.2f} GB in the page cache; {workers} reader threads")
    trees = []
    for r in runs:
        if r["tree"] not in trees:
            trees.append(r["tree"])
    names = {t: ("this tree (native reader)" if any(r["native"] for r in runs if r["tree"] == t)
                 else "other tree (pfd.read)") for t in trees}
    summary = {}
    for key, title in (("reader_s", "(a) reader alone"), ("e2e_s", "(b) dmprofPFD end to end")):
        print(f"\n{title}: files/s (GB/s), one column per repetition, then min-max spread")
        for gi in range(len(runs[0]["groups"])):
            g0 = runs[0]["groups"][gi]
            tag = f"{g0['shape'][0]}x{g0['shape'][1]}x{g0['shape'][2]} {'big' if g0['big_endian'] else 'little'}-endian"
            for t in trees:
                vals = [rate(r["groups"][gi], key) for r in runs if r["tree"] == t]
                fps = [v[0] for v in vals]
                cols = "  ".join(f"{f:9.1f} ({b:5.2f})" for f, b in vals)
                spread = (max(fps) - min(fps)) / np.median(fps) * 100
                print(f"  {tag:28s} {names[t]:26s} {cols}   spread {spread:4.1f} %")
                summary[(key, tag, names[t])] = (min(fps), max(fps))
    print("\nfaster than the other tree by more than the spread (slowest run of this tree against "
          "the fastest of the other)?")
    for (key, tag, name), (lo, hi) in summary.items():
        if "native" in name:
            other = [v for (k, t, n), v in summary.items() if k == key and t == tag and n != name]
            if other:
                print(f"  {key[:-2]:7s} {tag:28s} {lo:9.1f} vs {other[0][1]:9.1f} files/s: "
                      f"{'yes' if lo > other[0][1] else 'NO'} ({lo / other[0][1]:.2f}x)")
    for r in runs:
        if "h2d_bytes_per_s" in r:
            print(f"\nhost-to-device, pinned 256 MiB copy: {r['h2d_bytes_per_s'] / 1e9:.1f} GB/s")
            print("byte-reversed cubes in host memory, pfd_dmprof with the derived average: flagged "
                  "call vs cube.byteswap() on the host + unflagged call (ms, alternating)")
            for s in r["swap"]:
                f = "  ".join(f"{x * 1e3:8.2f}" for x in s["flagged_s"])
                h = "  ".join(f"{x * 1e3:8.2f}" for x in s["host_swap_s"])
                print(f"  {s['folds']} folds of {'x'.join(map(str, s['shape']))}: flagged {f} | "
                      f"host swap + unflagged {h} | same bits: {s['same_bits']}")
            break


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--other", help="checkout of the revision to compare with (built)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--tmp", default=None, help="where the files go (default: the system's)")
    ap.add_argument("--one", nargs=2, metavar=("TREE", "FILES"), help=argparse.SUPPRESS)
    ap.add_argument("--extras", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        one_tree(args.one[0], args.one[1], args.workers, args.extras)
        return
    root = tempfile.mkdtemp(prefix="pfd_measure_", dir=args.tmp)
    try:
        total = make_files(root)
        trees = [ROOT] + ([os.path.abspath(args.other)] if args.other else [])
        runs = []
        for rep in range(args.reps):
            for t in trees:
                cmd = [sys.executable, os.path.abspath(__file__), "--one", t, root, "--workers",
                       str(args.workers)] + (["--extras"] if t == ROOT and rep == 0 else [])
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                    raise SystemExit(f"the run of {t} failed ({r.returncode})")
                runs.append(json.loads(line[0][7:]))
                print(f"# repetition {rep + 1}, {t}: done", file=sys.stderr, flush=True)
        report(runs, total, args.workers)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
