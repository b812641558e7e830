"""What scrunching a fold costs through pfe_pfd_scrunch, against reading the same bytes with the
part-sum kernels and against what a caller had to do before: device pointers, everything
resident, event-timed on the handle's stream.

Per case (npart x nchan x nbin -> G x K, a form, n folds): a random cube in the form's values
(int16 with float32 scale, offset and weights; float32), a rotation per channel from
pfd.scrunch_plan at DM 100 over 1200-1600 MHz, and these ways, alternating inside one process
round by round:

  scrunch      Engine.pfd_scrunch with the rotations, into a preallocated result
  norot        ... without rotations (rot=None)
  direct       ... with the rotations, handle option pfd_scrunch_direct = 1 (one lane per bin)
  params4      yardstick (a): Engine.pfd_params4 on the same cube -- the part-sum kernel of the
               form (k_pfd_partsum_i16 / _f32: the same bytes read, fscr x bscr times the bytes
               stored) followed by the scalar-score kernel; the part-sum kernel alone is in the
               --trace run
  torch        yardstick (b): torch decode to float64, sum of the parts, per-channel roll by
               gather, reshape-sum -- what a caller does today

    python tools/pfd_scrunch_measure.py [--cases i16w:64x1024x1024:32x8:8,f32:16x128x256:4x2:512]
                                        [--rounds 20] [--warmup 3] [--out profiles/...txt]

Prints (and appends to --out) one JSON line per case: milliseconds per call (median, min, max) of
each way, the spread of params4 ((max - min) / median), the ratios of medians, the bytes the
scrunch kernel has to move (the cube and its parameters once, rot, the result) and what that is
per second at the median against 8.0 TB/s, whether scrunch, norot-with-zero-rot and direct agree
bit for bit, and the largest difference of the torch way (whose sums run in another order) over the
largest value.

--trace runs scrunch and params4 alone, five calls each, alternating, for
    rocprofv3 --kernel-trace --stats -- python tools/pfd_scrunch_measure.py --trace
whose kernel times set k_pfd_scrunch against k_pfd_partsum_* on the same cube.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="i16w:64x1024x1024:32x8:8,f32:16x128x256:4x2:512",
                    help="form : npart x nchan x nbin : fscr x bscr : n, comma-separated; form i16w or f32")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--trace", action="store_true", help="scrunch and params4 alone, five calls each, no timing")
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd._native import Engine, PfeError

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    with Engine(0) as e:
        for spec in args.cases.split(","):
            form, shape, factors, n = spec.split(":")
            npart, nchan, nbin = (int(v) for v in shape.split("x"))
            fscr, bscr = (int(v) for v in factors.split("x"))
            n = int(n)
            G, K = nchan // fscr, nbin // bscr
            g = torch.Generator(device="cuda").manual_seed(20261021)
            freqs = np.linspace(1200.0, 1600.0, nchan)
            rot_np, subfreqs = pfd.scrunch_plan(freqs, 100.0, nbin / 0.005, nbin, fscr)
            rot = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(rot_np, (n, nchan)))).cuda()
            zero = torch.zeros_like(rot)
            kw = {}
            if form == "i16w":
                cube = torch.randint(-32768, 32768, (n, npart, nchan, nbin), dtype=torch.int16, device="cuda", generator=g)
                kw = dict(scl=torch.rand((n, npart, nchan), device="cuda", generator=g) + 0.5,
                          offs=torch.randn((n, npart, nchan), device="cuda", generator=g) * 50.0,
                          wts=torch.rand((n, npart, nchan), device="cuda", generator=g))
                kw["wts"].view(-1)[::7] = 0.0
                in_bytes = cube.numel() * 2 + 3 * kw["scl"].numel() * 4
            elif form == "f32":
                cube = torch.randn((n, npart, nchan, nbin), device="cuda", generator=g) * 30.0 + 100.0
                in_bytes = cube.numel() * 4
            else:
                raise SystemExit(f"form {form!r}: i16w or f32")
            moved = in_bytes + rot.numel() * 4 + n * G * K * 8
            partsum_moved = in_bytes + n * nchan * nbin * 8
            fr = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(freqs, (n, nchan)))).cuda()
            sc = torch.tensor([100.0, nbin / 0.005, 100.0, 50.0, 0.0, 200.0, 100.0, 0.005],
                              dtype=torch.float64, device="cuda").repeat(n, 1)
            outs = {k: torch.empty((n, 1, G, K), dtype=torch.float64, device="cuda")
                    for k in ("scrunch", "norot", "direct", "zero")}

            def scrunch(key, r, **opt):
                def go():
                    with e.options(**opt):
                        e.pfd_scrunch(cube, fscr, bscr, rot=r, out=outs[key], **kw)
                return go

            def params4():
                e.pfd_params4(cube, fr, sc, **kw)

            def decode():
                if form == "f32":
                    return cube.double()
                x = cube.double() * kw["scl"].double()[..., None] + kw["offs"].double()[..., None]
                return x * kw["wts"].double()[..., None]

            idx = (torch.arange(nbin, device="cuda")[None, None, :] + (rot % nbin)[:, :, None].long()) % nbin
            tz = {}

            def torch_way():
                s = decode().sum(dim=1)
                r = torch.gather(s, 2, idx)
                tz["z"] = r.view(n, G, fscr, K, bscr).sum(dim=(2, 4))

            ways = {"scrunch": scrunch("scrunch", rot), "norot": scrunch("norot", None),
                    "direct": scrunch("direct", rot, pfd_scrunch_direct=1), "params4": params4,
                    "torch": torch_way}
            try:
                params4()
                torch.cuda.synchronize()
            except PfeError as err:   # the scoring calls do not take every shape
                del ways["params4"]
                emit({"case": spec, "params4_refused": str(err)})
            if args.trace:
                for _ in range(5):
                    ways["scrunch"]()
                    if "params4" in ways:
                        ways["params4"]()
                torch.cuda.synchronize()
                emit({"case": spec, "trace": True, "calls_each": 5, "route": pfd.scrunch_route(nbin, bscr),
                      "scrunch_bytes": moved, "partsum_bytes": partsum_moved, "hbm_peak_bytes_per_s": HBM_PEAK})
                continue
            order = tuple(ways)
            ms = {k: [] for k in order}
            for i in range(args.warmup + args.rounds):
                t = {k: timed(ways[k]) for k in order}
                if i >= args.warmup:
                    for k in order:
                        ms[k].append(t[k])
            scrunch("zero", zero)()
            torch.cuda.synchronize()
            r = {k: stats(ms[k]) for k in order}
            res = {"case": spec, "rounds": args.rounds, "route": pfd.scrunch_route(nbin, bscr),
                   "input_bytes": in_bytes, "scrunch_bytes": moved, "partsum_bytes": partsum_moved, "ms": r}
            med = r["scrunch"]["median_ms"]
            res["scrunch_call_bytes_per_s"] = round(moved / med * 1e3)
            res["scrunch_call_share_of_hbm_peak"] = round(moved / med * 1e3 / HBM_PEAK, 4)
            if "params4" in r:
                p = r["params4"]
                res["params4_spread"] = round((p["max_ms"] - p["min_ms"]) / p["median_ms"], 4)
                res["scrunch_over_params4"] = round(med / p["median_ms"], 4)
            res["norot_over_scrunch"] = round(r["norot"]["median_ms"] / med, 4)
            res["direct_over_scrunch"] = round(r["direct"]["median_ms"] / med, 4)
            res["scrunch_over_torch"] = round(med / r["torch"]["median_ms"], 4)
            bits = lambda a, b: bool(torch.equal(outs[a].view(torch.int64), outs[b].view(torch.int64)))  # noqa: E731
            res["direct_is_scrunch_bits"] = bits("direct", "scrunch")
            res["zero_rot_is_norot_bits"] = bits("zero", "norot")
            z = outs["scrunch"][:, 0]
            res["torch_max_diff_over_max"] = float((tz["z"] - z).abs().max() / z.abs().max())
            emit(res)
            del cube, kw, outs, tz, idx, rot, zero
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
