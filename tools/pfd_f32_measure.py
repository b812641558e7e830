"""What a float32 fold cube costs through pfe_pfd_dmprof_f32 / pfe_pfd_bates22_f32, against
the two ways a float32 caller had before: device pointers, event-timed on the handle's stream.

Per shape, n folds of a synthetic block (synth.pfd_fold_block, seed 20261019, tiled) cast to
float32 and resident on the device, and three ways to the same bits, alternating inside one
process round by round:

  (a) the parent revision's pfe_pfd_dmprof / pfe_pfd_bates22 on the cube widened once, outside
      the timed region (what a caller holding doubles pays) -- from the parent's library,
      built beside this one:  python tools/build_variant.py parent --rev <parent revision>
  (b) the same plus the on-device .double() of the float32 cube, inside the timed region
      (what a float32 caller had to do)
  (c) the _f32 calls on the float32 cube
  (d) (c) with PFE_OPT_PFD_F32_CHUNK at a quarter of the default pass

    python tools/pfd_f32_measure.py [--shapes 64x96x256:320,16x32x128:8192] [--rounds 20]
                                    [--warmup 3] [--parent-lib PATH]

Prints one JSON line per shape: milliseconds per call (median, min, max over the rounds) of
each way for both calls, folds per second at the median, (a)'s own round-to-round spread
((max - min) / median), the ratios of medians c/a, c/b and d/c, and whether (c)'s outputs are
(a)'s bits.  --trace runs (c) alone a few times, for rocprofv3 --kernel-trace --stats: the time
of k_pfd_partsum_f32 moves n x E x (4 x npart + 8) bytes.
"""
import argparse
import ctypes as C
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


class Parent:
    """The two f64 calls of another build of the library, on device pointers and on torch's
    current stream (the signatures of include/pfe.h, which the _f32 calls did not change)."""

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
        self.lib.pfe_pfd_bates22.argtypes = [vp, C.POINTER(_native.PfdIn), vp, vp, u32]
        self.PfdIn, self.flag = _native.PfdIn, _native.PFE_FLAG_DEVICE_PTRS
        self.h = vp()
        if self.lib.pfe_create(0, C.byref(self.h)):
            raise RuntimeError("pfe_create failed in " + path)

    def _in(self, x, fr, sc):
        import torch

        self.lib.pfe_set_stream(self.h, torch.cuda.current_stream(0).cuda_stream or None)
        n, npart, nsub, L = x.shape
        return self.PfdIn(x.data_ptr(), fr.data_ptr(), sc.data_ptr(), npart, nsub, L, n)

    def _check(self, rc):
        if rc:
            raise RuntimeError(self.lib.pfe_last_error(self.h).decode())

    def dmprof(self, x, fr, sc, lyon8, status):
        pin = self._in(x, fr, sc)
        self._check(self.lib.pfe_pfd_dmprof(self.h, C.byref(pin), None, None, lyon8.data_ptr(),
                                            status.data_ptr(), self.flag))

    def bates22(self, x, fr, sc, out, status):
        pin = self._in(x, fr, sc)
        self._check(self.lib.pfe_pfd_bates22(self.h, C.byref(pin), out.data_ptr(), status.data_ptr(),
                                             self.flag))

    def close(self):
        self.lib.pfe_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x96x256:320,16x32x128:8192",
                    help="npart x nsub x proflen : n, comma-separated")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "pulsarfeatureextractor_amd", "lib",
                                                         "libpfe_parent.so"))
    ap.add_argument("--trace", action="store_true", help="(c) alone, three calls each, no timing")
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd._native import Engine
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    def pfd_f32_default_chunk(nsub, L, n):  # include/pfe.h: 1 GiB of part sums
        return min(n, max(1, (1 << 30) // (8 * nsub * L)))

    parent = None if args.trace else Parent(os.path.abspath(args.parent_lib))
    with Engine(0) as e:
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

            x32, tfr, tsc = tile(profs.astype(np.float32)), tile(fr), tile(sc)
            mk = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device="cuda")  # noqa: E731
            ly = {k: mk(n, 8) for k in "abc"}
            o22 = {k: mk(n, 22) for k in "abc"}
            st = {k: mk(n, dt=torch.int32) for k in "abc"}

            def c_dmprof():
                ly["c"] = e.pfd_dmprof(x32, tfr, tsc, profile=False, chis=False)["lyon8"]

            def c_bates22():
                e.pfd_bates22(x32, tfr, tsc, out=o22["c"], status=st["c"])

            if args.trace:
                for _ in range(3):
                    c_dmprof()
                    c_bates22()
                torch.cuda.synchronize()
                print(json.dumps({"shape": shape, "n": n, "trace": True,
                                  "partsum_bytes": n * nsub * L * (4 * npart + 8)}), flush=True)
                continue
            x64 = x32.double()
            quarter = max(1, pfd_f32_default_chunk(nsub, L, n) // 4)
            ways = {
                "dmprof": {"a": lambda: parent.dmprof(x64, tfr, tsc, ly["a"], st["a"]),
                           "b": lambda: parent.dmprof(x32.double(), tfr, tsc, ly["b"], st["b"]),
                           "c": c_dmprof},
                "bates22": {"a": lambda: parent.bates22(x64, tfr, tsc, o22["a"], st["a"]),
                            "b": lambda: parent.bates22(x32.double(), tfr, tsc, o22["b"], st["b"]),
                            "c": c_bates22},
            }
            res = {"shape": shape, "n": n, "rounds": args.rounds,
                   "f64_cube_bytes": n * npart * nsub * L * 8, "f32_cube_bytes": n * npart * nsub * L * 4,
                   "default_chunk": pfd_f32_default_chunk(nsub, L, n), "quarter_chunk": quarter}
            for call, w in ways.items():
                ms = {k: [] for k in "abcd"}
                for i in range(args.warmup + args.rounds):
                    t = {k: timed(w[k]) for k in "abc"}
                    with e.options(pfd_f32_chunk=quarter):
                        t["d"] = timed(w["c"])
                    if i >= args.warmup:
                        for k in "abcd":
                            ms[k].append(t[k])
                w["c"]()  # (d) ran last: leave (c)'s outputs for the comparison
                torch.cuda.synchronize()
                r = {k: stats(ms[k], n) for k in "abcd"}
                a, c = r["a"], r["c"]
                r["a_spread"] = round((a["max_ms"] - a["min_ms"]) / a["median_ms"], 4)
                r["c_over_a"] = round(c["median_ms"] / a["median_ms"], 4)
                r["c_over_b"] = round(c["median_ms"] / r["b"]["median_ms"], 4)
                r["d_over_c"] = round(r["d"]["median_ms"] / c["median_ms"], 4)
                r["c_faster_than_a_beyond_spread"] = bool(c["max_ms"] < a["min_ms"])
                got, want = (ly["c"], ly["a"]) if call == "dmprof" else (o22["c"], o22["a"])
                r["c_is_a_bits"] = bool(torch.equal(got.view(torch.int64), want.view(torch.int64)))
                res[call] = r
            print(json.dumps(res), flush=True)
            del x32, x64, tfr, tsc, ly, o22, st
            torch.cuda.empty_cache()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
