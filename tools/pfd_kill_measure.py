"""What killed intervals and sub-bands cost through the pfe_pfd_*_kill calls, against the plain
call and against what a caller had to do before: device pointers, event-timed on the handle's
stream.

Per shape, element type (f64, float32) and killed fraction (0, 1/8 and 1/2 of the parts, plus one
sub-band), n folds of a synthetic block (synth.pfd_fold_block, seed 20261019, tiled) resident on
the device, and three ways, alternating inside one process round by round:

  (k) the _kill call on the cube as it is, masks as torch.bool tensors
  (p) the plain call on the same cube (nothing killed: what the cube costs to score at all)
  (u) what a user did before: clone() + masked zero in torch + the plain call

    python tools/pfd_kill_measure.py [--shapes 16x32x128:2048,64x96x256:64] [--rounds 12]
                                     [--warmup 2] [--call dmprof|bates22]

Prints one JSON line per (shape, type, fraction): milliseconds per call (median, min, max over
the rounds) of each way, folds per second at the median, the ratios of medians k/p and k/u, and
whether (k)'s outputs are (u)'s bits.  --trace runs (k) alone three times per case, for a
kernel-trace run of its own: k_pfd_partsum_kill moves partsum_bytes =
n x E x (bytes per value x npart x (nsub - 1) / nsub + 8): every part of every sub-band but the
killed one is loaded, killed parts included, and the sums are stored.
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
            "folds_per_s": round(n / med * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x32x128:2048,64x96x256:64",
                    help="npart x nsub x proflen : n, comma-separated")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--call", default="dmprof", choices=("dmprof", "bates22"))
    ap.add_argument("--trace", action="store_true", help="(k) alone, three calls each, no timing")
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd._native import Engine
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    with Engine(0) as e:
        def score(x, fr, sc, **kw):
            if args.call == "dmprof":
                return e.pfd_dmprof(x, fr, sc, profile=False, chis=False, derive_avgprof=True, **kw)["lyon8"]
            return e.pfd_bates22(x, fr, sc, derive_avgprof=True, **kw)[0]

        for spec in args.shapes.split(","):
            shape, n = spec.split(":")
            npart, nsub, L = (int(v) for v in shape.split("x"))
            n = int(n)
            blk = max(1, min(n, (64 << 20) // (npart * nsub * L * 8)))
            profs, fr, sc = pfd.batch_inputs(pfd_fold_block(blk, (npart, nsub, L), 20261019))
            reps = (n + blk - 1) // blk

            def tile(a):
                t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
                return t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()

            tfr, tsc = tile(fr), tile(sc)
            for dt in (torch.float64, torch.float32):
                x = tile(profs).to(dt)
                for frac in (0.0, 0.125, 0.5):
                    kp = torch.zeros((n, npart), dtype=torch.bool, device="cuda")
                    ks = torch.zeros((n, nsub), dtype=torch.bool, device="cuda")
                    kp[:, :int(round(frac * npart))] = True
                    ks[:, nsub // 2] = True
                    dead = kp[:, :, None, None] | ks[:, None, :, None]
                    out = {}

                    def way_k():
                        out["k"] = score(x, tfr, tsc, kill_parts=kp, kill_subs=ks)

                    def way_p():
                        out["p"] = score(x, tfr, tsc)

                    def way_u():
                        z = x.clone()
                        z.masked_fill_(dead, 0.0)
                        out["u"] = score(z, tfr, tsc)

                    name = "f64" if dt == torch.float64 else "f32"
                    bpv = 8 if dt == torch.float64 else 4
                    if args.trace:
                        for _ in range(3):
                            way_k()
                        torch.cuda.synchronize()
                        print(json.dumps({"shape": shape, "n": n, "type": name, "killed_parts": frac,
                                          "trace": True,
                                          "partsum_bytes": n * L * (bpv * npart * (nsub - 1) + 8 * nsub)}),
                              flush=True)
                        continue
                    ways = {"k": way_k, "p": way_p, "u": way_u}
                    ms = {k: [] for k in ways}
                    for i in range(args.warmup + args.rounds):
                        t = {k: timed(w) for k, w in ways.items()}
                        if i >= args.warmup:
                            for k in ways:
                                ms[k].append(t[k])
                    torch.cuda.synchronize()
                    r = {k: stats(ms[k], n) for k in ways}
                    res = {"shape": shape, "n": n, "type": name, "call": args.call, "killed_parts": frac,
                           "killed_subs": 1, "rounds": args.rounds, "cube_bytes": x.numel() * bpv, **r,
                           "k_over_p": round(r["k"]["median_ms"] / r["p"]["median_ms"], 4),
                           "k_over_u": round(r["k"]["median_ms"] / r["u"]["median_ms"], 4),
                           "k_is_u_bits": bool(torch.equal(out["k"].view(torch.int64),
                                                           out["u"].view(torch.int64)))}
                    print(json.dumps(res), flush=True)
                del x
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
