"""Time of one PFD score group against the whole chain at the bench shape: pfe_pfd_params4,
pfe_pfd_subband3, pfe_pfd_dmfit4 and pfe_pfd_bates22 on n folds of bench.py's synthetic block
(seed 20261019, tiled), device pointers, event-timed on the handle's stream.

    python tools/pfd_group_times.py [--n 32768] [--shape 16x32x128] [--steps 10] [--warmup 3]

Prints one JSON line: milliseconds per call (mean and min over the steps) for each entry point.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--shape", default="16x32x128")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    from pulsarfeatureextractor_amd import pfd
    from pulsarfeatureextractor_amd._native import Engine
    from pulsarfeatureextractor_amd.synth import pfd_fold_block

    shape = tuple(int(v) for v in args.shape.split("x"))
    blk = 1024
    ins = pfd.batch_inputs(pfd_fold_block(blk, shape, 20261019))
    reps = (args.n + blk - 1) // blk

    def tile(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t.repeat((reps,) + (1,) * (t.dim() - 1))[:args.n].contiguous()

    t = [tile(a) for a in ins]
    res = {"n": args.n, "shape": list(shape), "steps": args.steps, "unit": "ms per call"}
    with Engine(0) as e:
        for name, width in (("pfd_params4", 4), ("pfd_subband3", 3), ("pfd_dmfit4", 4),
                            ("pfd_bates22", 22)):
            fn = getattr(e, name)
            out = torch.empty((args.n, width), dtype=torch.float64, device="cuda")
            st = torch.empty((args.n,), dtype=torch.int32, device="cuda")
            ms = []
            for i in range(args.warmup + args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(*t, out=out, status=st)
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    ms.append(a.elapsed_time(b))
            res["pfe_" + name] = {"mean": round(float(np.mean(ms)), 4), "min": round(min(ms), 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
