"""What total intensity of an int16 fold cube costs through the _i16_pol calls, against what a
caller holding an AABBCRCI archive did before and against the _i16 call on one polarisation:
device pointers, everything resident, event-timed on the handle's stream.

Per shape, n folds of a synthetic block (synth.pfd_fold_block, seed 20261021, tiled) split into two
polarisations 0.6 x + r and 0.4 x - r, quantised per (fold, part, polarisation, sub-band), laid with
two more polarisations into the rows of one big-endian table (npol = 4: one row per
sub-integration: an 8-byte scalar, nsub float32 frequencies and weights, 4 x nsub offsets and
scales, 4 x nsub x proflen int16 values), and these ways, alternating inside one process round by
round:

  torch_f64    what a caller does today for total intensity: the torch decode of both
               polarisations to float64 on the device (byte order included), add, weight, then
               pfe_pfd_dmprof on the doubles
  i16_pol0     pfe_pfd_dmprof_i16 on polarisation 0 of the same table (PFE_FLAG_PFD_BSWAP): half
               the bytes, and not total intensity
  pol          pfe_pfd_dmprof_i16_pol {4, 2} on the table: the sum, formed where it is loaded

    python tools/pfd_pol_measure.py [--shapes 64x96x256:320,16x32x128:8192] [--rounds 20]
                                    [--warmup 3] [--scrunch 64x1024x1024:8:32x8]
                                    [--out profiles/pfd_pol_measure.txt]

pfe_pfd_dmprof with the lyon8 output only.  --scrunch npart x nchan x nbin : n : fscr x bscr runs
the same three ways through pfe_pfd_scrunch (no rotation).  Prints (and appends to --out) one JSON
line per shape: milliseconds per call (median, min, max over the rounds) of each way, i16_pol0's
own round-to-round spread, the ratios of medians pol / torch_f64 and pol / i16_pol0, whether pol's
output is torch_f64's bits, and the bytes each part-sum (or scrunch) kernel moves a call.

--trace runs i16_pol0 and pol alone three times each, for
    rocprofv3 --kernel-trace --stats -- python tools/pfd_pol_measure.py --trace
and prints the bytes each way's kernel moves a call, to set against its time there: values read
(n x E x 2 x npart x polarisations read, E = nsub x proflen), parameters (two float32 a (fold,
part, polarisation, sub-band), one weight a (fold, part, sub-band)) and sums written (n x E x 8; the
scrunch: n x G x K x 8).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPOL = 4


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


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


def table(d, scl, offs, wts):
    """The bytes of a big-endian (n x npart)-row table on the device and the strided views into it."""
    import torch

    n, npart, npol, nsub, L = d.shape
    row = 8 + 8 * nsub + 8 * npol * nsub + 2 * npol * nsub * L
    assert row % 4 == 0
    buf = torch.zeros(n * npart * row, dtype=torch.uint8, device=d.device)

    def col(off, dt, inner):
        es = dt.itemsize
        flat = buf[off:]
        flat = flat[: flat.numel() // es * es].view(dt)
        istr = tuple(int(np.prod(inner[i + 1:])) for i in range(len(inner)))
        return flat.as_strided((n, npart) + tuple(inner), (npart * row // es, row // es) + istr)

    cols = {"wts": col(8 + 4 * nsub, torch.float32, (nsub,)),
            "offs": col(8 + 8 * nsub, torch.float32, (npol, nsub)),
            "scl": col(8 + 8 * nsub + 4 * npol * nsub, torch.float32, (npol, nsub)),
            "d": col(8 + 8 * nsub + 8 * npol * nsub, torch.int16, (npol, nsub, L))}
    for k, src in (("wts", wts), ("offs", offs), ("scl", scl), ("d", d)):
        cols[k].copy_(swapped(src))
    return buf, cols, row


def build(kind, dims, n):
    """The table of n folds of `dims` = (npart, nsub, L) on the device -> (buf, cols, row)."""
    import torch

    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    npart, nsub, L = dims
    blk = max(1, min(n, (32 << 20) // (npart * nsub * L * 8)))
    rng = np.random.default_rng(20261021)
    if kind == "dmprof":
        x, fr, sc = pfd.batch_inputs(pfd_fold_block(blk, dims, 20261021))
    else:   # an every-channel cube: no pulse needed, nothing is scored
        x, fr, sc = rng.normal(100.0, 30.0, size=(blk,) + dims), np.zeros((blk, nsub)), np.zeros((blk, 8))
    span = x.max(axis=(1, 2, 3)) - x.min(axis=(1, 2, 3))
    r = rng.uniform(-0.5, 0.5, size=x.shape) * span[:, None, None, None]
    pols = np.stack([0.6 * x + r, 0.4 * x - r, r, -r], axis=2)
    del x, r
    d, scl, offs = quantise(pols)
    del pols
    wts = np.random.default_rng(7).uniform(0.05, 1.0, size=(blk, npart, nsub)).astype(np.float32)
    wts.reshape(-1)[::7] = 0.0
    reps = (n + blk - 1) // blk

    def tile(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()

    td, ts, to, tw, tfr, tsc = (tile(a) for a in (d, scl, offs, wts, fr, sc))
    buf, cols, row = table(td, ts, to, tw)
    del td, ts, to, tw
    torch.cuda.empty_cache()
    return buf, cols, row, tfr, tsc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x96x256:320,16x32x128:8192",
                    help="npart x nsub x proflen : n, comma-separated (empty: none)")
    ap.add_argument("--scrunch", default="64x1024x1024:8:32x8",
                    help="npart x nchan x nbin : n : fscr x bscr (empty: none)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--trace", action="store_true", help="i16_pol0 and pol alone, three calls each, no timing")
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd._native import Engine

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    jobs = [("dmprof", s, None) for s in args.shapes.split(",") if s]
    if args.scrunch:
        shape, n, how = args.scrunch.split(":")
        jobs.append(("scrunch", f"{shape}:{n}", tuple(int(v) for v in how.split("x"))))
    with Engine(0) as e:
        for kind, spec, how in jobs:
            shape, n = spec.split(":")
            dims = tuple(int(v) for v in shape.split("x"))
            npart, nsub, L = dims
            n = int(n)
            buf, c, row, tfr, tsc = build(kind, dims, n)
            d0, s0, o0 = c["d"][:, :, 0], c["scl"][:, :, 0], c["offs"][:, :, 0]
            res_ = {}

            def decode():
                # big-endian int16 and float32 to native, both polarisations to float64, add, weight
                dd = swapped(c["d"][:, :, :2].contiguous()).double()
                ss = swapped(c["scl"][:, :, :2].contiguous()).double()
                oo = swapped(c["offs"][:, :, :2].contiguous()).double()
                y = dd * ss[..., None] + oo[..., None]
                return (y[:, :, 0] + y[:, :, 1]) * swapped(c["wts"].contiguous()).double()[..., None]

            if kind == "dmprof":
                call = lambda cube, **kw: e.pfd_dmprof(cube, tfr, tsc, profile=False, chis=False, **kw)["lyon8"]  # noqa: E731
                out_bytes = n * nsub * L * 8
            else:
                call = lambda cube, **kw: e.pfd_scrunch(cube, how[0], how[1], **kw)  # noqa: E731
                out_bytes = n * (nsub // how[0]) * (L // how[1]) * 8
            ways = {
                "torch_f64": lambda: res_.__setitem__("torch_f64", call(decode())),
                "i16_pol0": lambda: res_.__setitem__("i16_pol0", call(d0, scl=s0, offs=o0, wts=c["wts"],
                                                                      byteswapped=True)),
                "pol": lambda: res_.__setitem__("pol", call(c["d"], scl=c["scl"], offs=c["offs"], wts=c["wts"],
                                                            byteswapped=True, pol_sum=2)),
            }
            E = nsub * L
            moved = {k: n * npart * E * 2 * p + n * npart * nsub * 4 * (2 * p + 1) + out_bytes
                     for k, p in (("i16_pol0", 1), ("pol", 2))}
            kernels = ({"i16_pol0": "k_pfd_partsum_i16<.., true, true, 0>", "pol": "k_pfd_partsum_i16<.., true, true, 2>"}
                       if kind == "dmprof" else
                       {"i16_pol0": "k_pfd_scrunch<short, .., true, true, 0>", "pol": "k_pfd_scrunch<short, .., true, true, 2>"})
            head = {"call": "pfd_" + kind, "shape": shape, "n": n, "npol": NPOL, "nsum": 2, "row_bytes": row,
                    "how": how, "kernel_bytes_per_call": moved, "kernels": kernels}
            if args.trace:
                for _ in range(3):
                    for k in ("i16_pol0", "pol"):
                        ways[k]()
                torch.cuda.synchronize()
                emit({**head, "trace": True, "calls_each": 3})
            else:
                order = ("torch_f64", "i16_pol0", "pol")
                ms = {k: [] for k in order}
                for i in range(args.warmup + args.rounds):
                    t = {k: timed(ways[k]) for k in order}
                    if i >= args.warmup:
                        for k in order:
                            ms[k].append(t[k])
                torch.cuda.synchronize()
                r = {k: stats(ms[k]) for k in order}
                one = r["i16_pol0"]
                r["i16_pol0_spread"] = round((one["max_ms"] - one["min_ms"]) / one["median_ms"], 4)
                r["pol_over_torch_f64"] = round(r["pol"]["median_ms"] / r["torch_f64"]["median_ms"], 4)
                r["pol_over_i16_pol0"] = round(r["pol"]["median_ms"] / one["median_ms"], 4)
                r["pol_is_torch_f64_bits"] = bool(torch.equal(res_["pol"].view(torch.int64),
                                                              res_["torch_f64"].view(torch.int64)))
                emit({**head, "rounds": args.rounds, **r})
            del buf, c, d0, s0, o0, res_, ways
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
