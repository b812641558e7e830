"""Throughput of pfe_subband3_f64 against pfe_pfd_subband3 as the yardstick, at the same
nsub x proflen with npart = 1: n folds of the synthetic block of tools/pfd_group_times.py
(seed 20261019, tiled), device pointers, event-timed on the handle's stream.

The yardstick reads the same bytes (n x 1 x nsub x L doubles) and does strictly more work
(dedispersion, the candidate parameters) before the same sub-band scores.  The float call is
given each fold's only part as its sub-bands, and the profile and the width the fold kernels
derive (pfe_pfd_dmprof's profile, column 3 of pfe_pfd_params4), so both score windows of the
same width.  The two calls alternate inside one process; the yardstick's run-to-run spread is
the range of its own per-round times.

    python tools/subband_f64_measure.py [--n 65536] [--shapes 16x128,32x128] [--rounds 20] [--warmup 3]

Prints one JSON line per shape: milliseconds per call (median, min, max over the rounds) of both
calls, candidates per second at the median, the yardstick's spread and the ratio of medians.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
            "cands_per_s": round(n / med * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--shapes", default="16x128,32x128")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd._native import Engine
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    n, blk = args.n, 1024
    reps = (n + blk - 1) // blk
    with Engine(0) as e:
        for shape in args.shapes.split(","):
            nsub, L = (int(v) for v in shape.split("x"))
            ins = pfd.batch_inputs(pfd_fold_block(blk, (1, nsub, L), 20261019))

            def tile(a):
                t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
                return t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()

            t = [tile(a) for a in ins]
            sub = t[0].view(n, nsub, L)
            prof = e.pfd_dmprof(*t, chis=False, lyon8=False)["profile"]
            par, _ = e.pfd_params4(*t)
            scal = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
            scal[:, 3] = par[:, 3]
            out_y = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            out_f = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            st_y = torch.empty((n,), dtype=torch.int32, device="cuda")
            st_f = torch.empty((n,), dtype=torch.int32, device="cuda")
            ms_y, ms_f = [], []
            for i in range(args.warmup + args.rounds):
                y = timed(lambda: e.pfd_subband3(*t, out=out_y, status=st_y))
                f = timed(lambda: e.subband3_f64(prof, sub, scal, out=out_f, status=st_f))
                if i >= args.warmup:
                    ms_y.append(y)
                    ms_f.append(f)
            res = {"shape": shape, "n": n, "rounds": args.rounds,
                   "bytes_read_per_call": n * nsub * L * 8,
                   "pfe_pfd_subband3": stats(ms_y, n), "pfe_subband3_f64": stats(ms_f, n),
                   "rows_scored": [int((st_y == 0).sum()), int((st_f == 0).sum())]}
            y, f = res["pfe_pfd_subband3"], res["pfe_subband3_f64"]
            res["yardstick_spread"] = round((y["max_ms"] - y["min_ms"]) / y["median_ms"], 4)
            res["f64_over_yardstick"] = round(f["median_ms"] / y["median_ms"], 4)
            print(json.dumps(res), flush=True)
            del t, sub, prof, par, scal


if __name__ == "__main__":
    main()
