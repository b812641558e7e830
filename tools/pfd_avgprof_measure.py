"""What deriving a fold's average on the device costs: pfe_pfd_avgprof alone, PFE_FLAG_PFD_AVGPROF
on pfe_pfd_dmprof, and numpy's (x / L).sum() on this machine's CPU.  Device pointers,
event-timed on the handle's stream, every way alternating inside one process round by round.

Per shape, n folds of a synthetic block (synth.pfd_fold_block, seed 20261022, tiled), resident on
the device as float64 and as float32:

  (a) pfe_pfd_avgprof / pfe_pfd_avgprof_f32 alone: ms, bytes read per second, share of the HBM
      peak (8.0 TB/s by the data sheet; --hbm-peak-gbs)
  (b) pfe_pfd_dmprof (lyon8 only) on the same resident cube: the parent revision's library
      (built beside this one:  python tools/build_variant.py parent --rev <parent revision>),
      this build without the flag, this build with it; and the same for pfe_pfd_dmprof_f32
  (c) numpy's (x / L).sum() per fold on the host, over a few folds

    python tools/pfd_avgprof_measure.py [--shapes 16x32x128:32768,64x96x256:1024] [--rounds 20]
                                        [--warmup 3] [--parent-lib PATH]

Prints one JSON line per shape: milliseconds per call (median, min, max over the rounds), folds
per second at the median, the parent's own round-to-round spread ((max - min) / median), the
ratios of medians, and whether the flagged call's outputs are the bits of the unflagged call
given numpy's value.  --trace runs (a) alone three times per dtype, for rocprofv3 --kernel-trace
--stats.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


class Parent:
    """pfe_pfd_dmprof / _f32 of another build of the library, on device pointers and on torch's
    current stream (the signatures of include/pfe.h, which this change left as they were)."""

    def __init__(self, path):
        from pulsarfeatureextractor_amd import _native

        _native.load_library()  # this build first: one HIP runtime, shared with torch
        self.lib = C.CDLL(path)
        vp, u32 = C.c_void_p, C.c_uint32
        self.lib.pfe_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.lib.pfe_destroy.argtypes = [vp]
        self.lib.pfe_set_stream.argtypes = [vp, vp]
        self.lib.pfe_last_error.restype = C.c_char_p
        self.lib.pfe_last_error.argtypes = [vp]
        self.lib.pfe_pfd_dmprof.argtypes = [vp, C.POINTER(_native.PfdIn), vp, vp, vp, vp, u32]
        self.lib.pfe_pfd_dmprof_f32.argtypes = [vp, C.POINTER(_native.PfdF32In), vp, vp, vp, vp, u32]
        self.n = _native
        self.h = vp()
        if self.lib.pfe_create(0, C.byref(self.h)):
            raise RuntimeError("pfe_create failed in " + path)

    def dmprof(self, x, fr, sc, lyon8, status):
        import torch

        self.lib.pfe_set_stream(self.h, torch.cuda.current_stream(0).cuda_stream or None)
        n, npart, nsub, L = x.shape
        f32 = x.dtype == torch.float32
        pin = (self.n.PfdF32In if f32 else self.n.PfdIn)(x.data_ptr(), fr.data_ptr(), sc.data_ptr(),
                                                         npart, nsub, L, n)
        fn = self.lib.pfe_pfd_dmprof_f32 if f32 else self.lib.pfe_pfd_dmprof
        if fn(self.h, C.byref(pin), None, None, lyon8.data_ptr(), status.data_ptr(),
              self.n.PFE_FLAG_DEVICE_PTRS):
            raise RuntimeError(self.lib.pfe_last_error(self.h).decode())

    def close(self):
        self.lib.pfe_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x32x128:32768,64x96x256:1024",
                    help="npart x nsub x proflen : n, comma-separated")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-peak-gbs", type=float, default=8000.0)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "pulsarfeatureextractor_amd", "lib",
                                                         "libpfe_parent.so"))
    ap.add_argument("--trace", action="store_true", help="(a) alone, three calls per dtype, no timing")
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd._native import Engine
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    parent = None if args.trace else Parent(os.path.abspath(args.parent_lib))
    with Engine(0) as e:
        for spec in args.shapes.split(","):
            shape, n = spec.split(":")
            npart, nsub, L = (int(v) for v in shape.split("x"))
            n = int(n)
            E = npart * nsub * L
            blk = max(1, min(n, (64 << 20) // (E * 8)))
            profs, fr, sc = pfd.batch_inputs(pfd_fold_block(blk, (npart, nsub, L), 20261022))
            reps = (n + blk - 1) // blk

            def tile(a):
                t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
                return t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()

            x = {"f64": tile(profs), "f32": tile(profs.astype(np.float32))}
            tfr = tile(fr)
            if args.trace:
                for k in x:
                    for _ in range(3):
                        e.pfd_avgprof(x[k])
                torch.cuda.synchronize()
                print(json.dumps({"shape": shape, "n": n, "trace": True, "f64_cube_bytes": n * E * 8,
                                  "f32_cube_bytes": n * E * 4}), flush=True)
                continue
            # (c) the host expression, fold by fold
            host = []
            for f in profs[:min(blk, 8)]:
                t0 = time.perf_counter()
                (f / L).sum()
                host.append((time.perf_counter() - t0) * 1e3)
            res = {"shape": shape, "n": n, "rounds": args.rounds, "chunks_per_fold": (E + 8191) // 8192,
                   "numpy_ms_per_fold": round(float(np.median(host)), 4),
                   "numpy_folds_per_s": round(1e3 / float(np.median(host)))}
            mk = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device="cuda")  # noqa: E731
            for k, cube in x.items():
                # scal with numpy's value (of the widened cube) and with the average poisoned
                good = sc.copy()
                xb = profs.astype(np.float32).astype(np.float64) if k == "f32" else profs
                good[:, 2] = [(f / L).sum() for f in xb]
                bad = good.copy()
                bad[:, 2] = np.nan
                tgood, tbad = tile(good), tile(bad)
                ly = {w: mk(n, 8) for w in ("parent", "plain", "flag")}
                st = mk(n, dt=torch.int32)
                avg = {}

                def w_avg():
                    avg["v"] = e.pfd_avgprof(cube)

                def w_plain():
                    ly["plain"] = e.pfd_dmprof(cube, tfr, tgood, profile=False, chis=False)["lyon8"]

                def w_flag():
                    ly["flag"] = e.pfd_dmprof(cube, tfr, tbad, profile=False, chis=False,
                                              derive_avgprof=True)["lyon8"]

                ways = {"avgprof": w_avg, "parent": lambda: parent.dmprof(cube, tfr, tgood, ly["parent"], st),
                        "plain": w_plain, "flag": w_flag}
                ms = {w: [] for w in ways}
                for i in range(args.warmup + args.rounds):
                    t = {w: timed(fn) for w, fn in ways.items()}
                    if i >= args.warmup:
                        for w in ways:
                            ms[w].append(t[w])
                torch.cuda.synchronize()
                r = {w: stats(ms[w], n) for w in ways}
                nbytes = n * E * (8 if k == "f64" else 4)
                a, p = r["avgprof"], r["parent"]
                a["read_gb_per_s"] = round(nbytes / a["median_ms"] / 1e6, 1)
                a["share_of_hbm_peak"] = round(nbytes / a["median_ms"] / 1e6 / args.hbm_peak_gbs, 4)
                a["spread"] = round((a["max_ms"] - a["min_ms"]) / a["median_ms"], 4)
                r["cube_bytes"] = nbytes
                r["parent_spread"] = round((p["max_ms"] - p["min_ms"]) / p["median_ms"], 4)
                r["plain_over_parent"] = round(r["plain"]["median_ms"] / p["median_ms"], 4)
                r["flag_over_plain"] = round(r["flag"]["median_ms"] / r["plain"]["median_ms"], 4)
                r["flag_minus_plain_ms"] = round(r["flag"]["median_ms"] - r["plain"]["median_ms"], 4)
                r["avgprof_over_plain"] = round(a["median_ms"] / r["plain"]["median_ms"], 4)
                bits = lambda t: t.view(torch.int64)  # noqa: E731
                r["flag_is_plain_bits"] = bool(torch.equal(bits(ly["flag"]), bits(ly["plain"])))
                r["plain_is_parent_bits"] = bool(torch.equal(bits(ly["plain"]), bits(ly["parent"])))
                r["avgprof_is_numpy_bits"] = bool(torch.equal(bits(avg["v"]), bits(tgood[:, 2].contiguous())))
                res[k] = r
                del tgood, tbad, ly, st
            print(json.dumps(res), flush=True)
            del x, tfr
            torch.cuda.empty_cache()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
