"""What an int16 fold cube costs through pfe_pfd_dmprof_i16, against the two ways a caller
holding a fold-mode archive had before: device pointers, event-timed on the handle's stream.

Per shape, n folds of a synthetic block (synth.pfd_fold_block, seed 20261021, tiled), quantised
per (fold, part, sub-band) to int16 with a float32 scale and offset, random float32 weights, all
resident on the device, and these ways, alternating inside one process round by round:

  f64          pfe_pfd_dmprof on the decoded doubles, already resident (what a caller holding
               doubles pays)
  torch_f64    the same plus the torch decode to float64 on the device inside the timed region
               (d.double() * scl + offs, * wts: what an int16 caller had to do)
  i16          pfe_pfd_dmprof_i16, dense arrays, no weights
  i16_w        ... with weights
  i16_sw       ... with weights, every value byte-reversed (PFE_FLAG_PFD_BSWAP)
  rows_w       ... with weights, the four arrays in the rows of one uploaded table (one row per
               sub-integration: an 8-byte scalar, nsub float32 frequencies, weights, offsets
               and scales, nsub x proflen int16 values), native byte order
  rows_sw      ... the same table big-endian, with PFE_FLAG_PFD_BSWAP

    python tools/pfd_i16_measure.py [--shapes 16x32x128:8192,64x96x256:320] [--rounds 20]
                                    [--warmup 3] [--out profiles/pfd_i16_measure.txt]

pfe_pfd_dmprof with the lyon8 output only.  Prints (and appends to --out) one JSON line per
shape: milliseconds per call (median, min, max over the rounds) of each way, folds per second at
the median, f64's own round-to-round spread ((max - min) / median), the ratios of medians of
each int16 way over f64 and over torch_f64, and whether every int16 way's output is f64's bits.

--trace runs i16, i16_w and rows_sw alone three times each, for
    rocprofv3 --kernel-trace --stats -- python tools/pfd_i16_measure.py --trace
and prints what k_pfd_partsum_i16 moves and computes per call, to set against its time there:
  bytes   n x E x (2 x npart + 8) of values and part sums, E = nsub x proflen, plus
          n x npart x nsub x 4 per parameter array (2 without weights, 3 with)
  fp64    n x npart x E x 3 VALU instructions per lane without weights (convert, multiply-add,
          add to the sum), x 4 with (the multiply by the weight)
against 8.0 TB/s of HBM (data sheet) and 39.3e12 fp64 lane-instructions per second (half the
157.3 TFLOP/s = 78.6e12 lane-instructions per second of the fp32 vector unit).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
FP64_VALU_PEAK = 157.3e12 / 2 / 2   # lane-instructions per second


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
            "folds_per_s": round(n / med * 1e3)}


def quantise(x):
    mx, mn = x.max(axis=-1), x.min(axis=-1)
    offs = ((mx + mn) / 2).astype(np.float32)
    scl = ((mx - mn) / 65534).astype(np.float32)
    scl[scl == 0] = 1
    d = np.clip(np.rint((x - offs[..., None]) / scl[..., None]), -32768, 32767).astype(np.int16)
    return d, scl, offs


def swapped(t):
    """A tensor of the same dtype holding every value of t byte-reversed."""
    import torch

    b = t.contiguous().view(torch.uint8).view(-1, t.element_size()).flip(1).contiguous()
    return b.view(t.dtype).view(t.shape)


def table(d, scl, offs, wts, fr, swap):
    """The bytes of an (n x npart)-row table on the device and the four strided views into it."""
    import torch

    n, npart, nsub, L = d.shape
    row = 8 + 16 * nsub + 2 * nsub * L
    assert row % 4 == 0
    buf = torch.zeros(n * npart * row, dtype=torch.uint8, device=d.device)

    def col(off, dt, inner):
        es = dt.itemsize
        flat = buf[off:]
        flat = flat[: flat.numel() // es * es].view(dt)
        istr = tuple(int(np.prod(inner[i + 1:])) for i in range(len(inner)))
        return flat.as_strided((n, npart) + tuple(inner), (npart * row // es, row // es) + istr)

    cols = {"wts": col(8 + 4 * nsub, torch.float32, (nsub,)), "offs": col(8 + 8 * nsub, torch.float32, (nsub,)),
            "scl": col(8 + 12 * nsub, torch.float32, (nsub,)), "d": col(8 + 16 * nsub, torch.int16, (nsub, L))}
    f = swapped if swap else (lambda t: t)
    col(8, torch.float32, (nsub,)).copy_(f(fr.float()[:, None, :].expand(n, npart, nsub).contiguous()))
    for k, src in (("wts", wts), ("offs", offs), ("scl", scl), ("d", d)):
        cols[k].copy_(f(src))
    return buf, cols, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x32x128:8192,64x96x256:320",
                    help="npart x nsub x proflen : n, comma-separated")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--trace", action="store_true", help="three int16 ways alone, three calls each, no timing")
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd._native import Engine
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    with Engine(0) as e:
        for spec in args.shapes.split(","):
            shape, n = spec.split(":")
            npart, nsub, L = (int(v) for v in shape.split("x"))
            n = int(n)
            blk = max(1, min(n, (64 << 20) // (npart * nsub * L * 8)))
            profs, fr, sc = pfd.batch_inputs(pfd_fold_block(blk, (npart, nsub, L), 20261021))
            d, scl, offs = quantise(profs)
            wts = np.random.default_rng(7).uniform(0.05, 1.0, size=scl.shape).astype(np.float32)
            wts.reshape(-1)[::7] = 0.0
            reps = (n + blk - 1) // blk

            def tile(a):
                t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
                return t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()

            td, ts, to, tw, tfr, tsc = (tile(a) for a in (d, scl, offs, wts, fr, sc))

            def decode(w):
                x = td.double() * ts.double()[..., None] + to.double()[..., None]
                return x * tw.double()[..., None] if w else x

            E = nsub * L
            par = n * npart * nsub * 4
            counts = {w: {"bytes": n * E * (2 * npart + 8) + par * (3 if w else 2),
                          "fp64_lane_instructions": n * npart * E * (4 if w else 3)} for w in (0, 1)}
            sd, ss, so, sw = (swapped(t) for t in (td, ts, to, tw))
            _buf_n, rows_n, row = table(td, ts, to, tw, tfr, False)
            _buf_s, rows_s, _ = table(td, ts, to, tw, tfr, True)
            ly = {}

            def run(key, cube, **kw):
                def go():
                    ly[key] = e.pfd_dmprof(cube, tfr, tsc, profile=False, chis=False, **kw)["lyon8"]
                return go

            ways = {
                "i16": run("i16", td, scl=ts, offs=to),
                "i16_w": run("i16_w", td, scl=ts, offs=to, wts=tw),
                "i16_sw": run("i16_sw", sd, scl=ss, offs=so, wts=sw, byteswapped=True),
                "rows_w": run("rows_w", rows_n["d"], scl=rows_n["scl"], offs=rows_n["offs"], wts=rows_n["wts"]),
                "rows_sw": run("rows_sw", rows_s["d"], scl=rows_s["scl"], offs=rows_s["offs"],
                               wts=rows_s["wts"], byteswapped=True),
            }
            if args.trace:
                for _ in range(3):
                    for k in ("i16", "i16_w", "rows_sw"):
                        ways[k]()
                torch.cuda.synchronize()
                emit({"shape": shape, "n": n, "trace": True, "calls_each": 3,
                      "kernels": {"i16": "k_pfd_partsum_i16<true, false, false>",
                                  "i16_w": "k_pfd_partsum_i16<true, false, true>",
                                  "rows_sw": "k_pfd_partsum_i16<true, true, true>"},
                      "partsum_no_weights": counts[0], "partsum_weights": counts[1],
                      "hbm_peak_bytes_per_s": HBM_PEAK, "fp64_valu_peak_lane_instructions_per_s": FP64_VALU_PEAK})
                continue
            x64, x64w = decode(False), decode(True)
            ways["f64"] = run("f64", x64)
            ways["f64_w"] = run("f64_w", x64w)
            ways["torch_f64"] = lambda: ly.__setitem__(
                "torch_f64", e.pfd_dmprof(decode(True), tfr, tsc, profile=False, chis=False)["lyon8"])
            order = ("f64", "f64_w", "torch_f64", "i16", "i16_w", "i16_sw", "rows_w", "rows_sw")
            ms = {k: [] for k in order}
            for i in range(args.warmup + args.rounds):
                t = {k: timed(ways[k]) for k in order}
                if i >= args.warmup:
                    for k in order:
                        ms[k].append(t[k])
            torch.cuda.synchronize()
            res = {"shape": shape, "n": n, "rounds": args.rounds, "row_bytes": row,
                   "f64_cube_bytes": n * npart * E * 8, "i16_cube_bytes": n * npart * E * 2,
                   "partsum_no_weights": counts[0], "partsum_weights": counts[1]}
            r = {k: stats(ms[k], n) for k in order}
            f = r["f64_w"]
            r["f64_w_spread"] = round((f["max_ms"] - f["min_ms"]) / f["median_ms"], 4)
            for k in order[3:]:
                base = r["f64"] if k == "i16" else f
                r[k + "_over_f64"] = round(r[k]["median_ms"] / base["median_ms"], 4)
                r[k + "_over_torch_f64"] = round(r[k]["median_ms"] / r["torch_f64"]["median_ms"], 4)
                r[k + "_slower_than_f64_beyond_spread"] = bool(r[k]["min_ms"] > base["max_ms"])
            same = lambda a, b: bool(torch.equal(ly[a].view(torch.int64), ly[b].view(torch.int64)))  # noqa: E731
            r["i16_is_f64_bits"] = same("i16", "f64")
            r["weighted_are_f64_bits"] = all(same(k, "f64_w") for k in ("i16_w", "i16_sw", "rows_w", "rows_sw",
                                                                           "torch_f64"))
            res["dmprof"] = r
            emit(res)
            del td, ts, to, tw, x64, x64w, sd, ss, so, sw, _buf_n, _buf_s, rows_n, rows_s, ly
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
