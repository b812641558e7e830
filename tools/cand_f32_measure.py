"""What a candidate held as float32 arrays costs through pfe_subband3_f32, pfe_bates22_f32 and
pfe_lyon8_f32, against the two ways a float32 holder had before: device pointers, event-timed
on the handle's stream.

Per shape, n candidates (synth.bates_batch made float as tests/test_subband_f64_gpu.py makes
it, a block tiled to n; Lyon rows N(100, 10)) cast to float32 and resident on the device, and
three ways to the same bits, alternating inside one process round by round:

  (a) the f64 call on the arrays widened once, outside the timed region (what a caller holding
      doubles pays; the f64 kernels are the parent revision's)
  (b) the same plus the on-device .double() of every float32 array, inside the timed region
      (what a float32 holder had to do)
  (c) the _f32 call on the float32 arrays

    python tools/cand_f32_measure.py [--calls subband3,bates22,lyon8] [--rounds 20] [--warmup 3]
        [--sub-shapes 16x128,32x128] [--n-subband3 65536] [--n-bates22 262144]
        [--lyon-shapes 128+100,128+128] [--n-lyon8 1048576] [--ways abc]

Prints one JSON line per call and shape: milliseconds per call (median, min, max over the
rounds) of each way, candidates per second at the median, each way's own round-to-round spread
((max - min) / median), the ratios of medians c/a and c/b, the bytes of float input (c) reads,
and whether (c)'s outputs are (a)'s bits.  --ways c (or a) runs one way alone, for a kernel trace.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, n):
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / med, 4), "cands_per_s": round(n / med * 1e3)}


def same_bits(got, want):
    import torch

    g, w = got.view(torch.int64), want.view(torch.int64)
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan) and torch.equal(g[~nan], w[~nan]))


def measure(ways, n, rounds, warmup, keep="abc"):
    import torch

    ways = {k: fn for k, fn in ways.items() if k in keep}
    ms = {k: [] for k in ways}
    for i in range(warmup + rounds):
        t = {k: timed(fn) for k, fn in ways.items()}
        if i >= warmup:
            for k in ways:
                ms[k].append(t[k])
    torch.cuda.synchronize()
    r = {k: stats(ms[k], n) for k in ways}
    for k in "ab":
        if "c" in r and k in r:
            r["c_over_" + k] = round(r["c"]["median_ms"] / r[k]["median_ms"], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", default="subband3,bates22,lyon8")
    ap.add_argument("--sub-shapes", default="16x128,32x128", help="nsub x lsb, comma-separated")
    ap.add_argument("--n-subband3", type=int, default=65536)
    ap.add_argument("--n-bates22", type=int, default=262144)
    ap.add_argument("--lyon-shapes", default="128+100,128+128", help="lp + ld, comma-separated")
    ap.add_argument("--n-lyon8", type=int, default=1 << 20)
    ap.add_argument("--ndm", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ways", default="abc", help="a subset, e.g. c alone under rocprofv3 --kernel-trace")
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd._native import Engine
    from pulsarfeatureextractor_amd.synth import bates_batch

    calls = args.calls.split(",")

    def tile(a, n):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        reps = (n + len(a) - 1) // len(a)
        return t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()

    def mk(*s, dt=torch.float64):
        return torch.empty(s, dtype=dt, device="cuda")

    with Engine(0) as e:
        for shape in args.sub_shapes.split(","):
            nsub, lsb = (int(v) for v in shape.split("x"))
            blk = 1024
            b = bates_batch(blk, lp=lsb, nsub=nsub, lsb=lsb, ndm=args.ndm, seed=20261021)
            rng = np.random.default_rng(20261021 + 77)
            sub = b["sub"] * rng.uniform(0.3, 1.7, b["sub"].shape) + rng.normal(0, 0.37, b["sub"].shape)
            prof = b["prof"] * 0.731 + rng.normal(0, 0.21, b["prof"].shape)
            curve = b["dmcurve"] * 0.37 + rng.normal(0, 0.05, b["dmcurve"].shape)
            for call in ("subband3", "bates22"):
                if call not in calls:
                    continue
                n = args.n_subband3 if call == "subband3" else args.n_bates22
                k = 3 if call == "subband3" else 22
                p32, s32, c32 = (tile(a.astype(np.float32), n) for a in (prof, sub, curve))
                sc = tile(b["scal"], n)
                p64, s64, c64 = p32.double(), s32.double(), c32.double()
                out = {w: mk(n, k) for w in "abc"}
                st = {w: mk(n, dt=torch.int32) for w in "abc"}
                if call == "subband3":
                    ways = {
                        "a": lambda: e.subband3_f64(p64, s64, sc, out=out["a"], status=st["a"]),
                        "b": lambda: e.subband3_f64(p32.double(), s32.double(), sc, out=out["b"], status=st["b"]),
                        "c": lambda: e.subband3_f32(p32, s32, sc, out=out["c"], status=st["c"]),
                    }
                    f32_bytes = 4 * n * (nsub * lsb + lsb)
                else:
                    ways = {
                        "a": lambda: e.bates22_f64(p64, s64, c64, sc, out=out["a"], status=st["a"]),
                        "b": lambda: e.bates22_f64(p32.double(), s32.double(), c32.double(), sc,
                                                   out=out["b"], status=st["b"]),
                        "c": lambda: e.bates22_f32(p32, s32, c32, sc, out=out["c"], status=st["c"]),
                    }
                    f32_bytes = 4 * n * (nsub * lsb + lsb + args.ndm)
                r = measure(ways, n, args.rounds, args.warmup, args.ways)
                r.update({"call": call, "shape": shape, "n": n, "rounds": args.rounds, "f32_bytes": f32_bytes,
                          "rows_scored": int((st["c"] == 0).sum()),
                          "c_is_a_bits": args.ways == "abc" and same_bits(out["c"], out["a"]) and
                          bool(torch.equal(st["c"], st["a"]))})
                print(json.dumps(r), flush=True)
                del p32, s32, c32, p64, s64, c64, sc, out, st, ways
                torch.cuda.empty_cache()
        if "lyon8" in calls:
            for shape in args.lyon_shapes.split(","):
                lp, ld = (int(v) for v in shape.split("+"))
                n = args.n_lyon8
                rng = np.random.default_rng(20261021 + lp + ld)
                p32 = tile(rng.normal(100.0, 10.0, (4096, lp)).astype(np.float32), n)
                d32 = tile(rng.normal(100.0, 10.0, (4096, ld)).astype(np.float32), n)
                p64, d64 = p32.double(), d32.double()
                out = {w: mk(n, 8) for w in "abc"}
                ways = {
                    "a": lambda: e.lyon8(p64, d64, out=out["a"]),
                    "b": lambda: e.lyon8(p32.double(), d32.double(), out=out["b"]),
                    "c": lambda: e.lyon8(p32, d32, out=out["c"]),
                }
                r = measure(ways, n, args.rounds, args.warmup, args.ways)
                r.update({"call": "lyon8", "shape": shape, "n": n, "rounds": args.rounds,
                          "f32_bytes": 4 * n * (lp + ld),
                          "c_is_a_bits": args.ways == "abc" and same_bits(out["c"], out["a"])})
                print(json.dumps(r), flush=True)
                del p32, d32, p64, d64, out, ways
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
