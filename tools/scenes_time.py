#!/usr/bin/env python3
"""Scene batches against B contexts: for n in {100, 256, 1024, 2048} and B in {1, 16, 256, 2048} with
B * n <= 2^20 and k = 8 steps,
  batch     device time between two events around ONE nb_scenes_*_step_launch, both laws
  contexts  the only way the library offered before: B contexts' nb_step(k) / nb_step_boids(k) issued back to back, wall time to
            the last sync
median and min of --reps (20) runs after a warm-up, the four measurements of a shape taken in the same run in rotating order.
Prints ms and scene-steps/s.  scenes_time.py [--reps R] [--max-contexts C] [--sizes n,n,..] [--batches B,B,..]
(--max-contexts: shapes with more scenes than that time the batch only)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nenbody_amd as nb  # noqa: E402
from nenbody_amd import _lib  # noqa: E402

K = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-contexts", type=int, default=2048)
    ap.add_argument("--sizes", default="100,256,1024,2048")
    ap.add_argument("--batches", default="1,16,256,2048")
    args = ap.parse_args()
    import torch

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    print(f"{'n':>5} {'B':>5} {'law':>6} | {'batch ms med':>12} {'min':>8} {'scene-steps/s':>14} | {'contexts ms med':>15} {'min':>8} {'scene-steps/s':>14} | ratio")
    for n in (int(x) for x in args.sizes.split(",")):
        for batch in (int(x) for x in args.batches.split(",")):
            if batch * n > 1 << 20:
                continue
            states = [nb.init_state(n, 1234 + s) for s in range(batch)]
            rec = np.zeros((2, batch, n, 4), np.float32)
            rec[0, :, :, :3] = np.stack([p for p, _ in states])
            rec[1, :, :, :3] = np.stack([v for _, v in states])
            base = torch.from_numpy(rec).to(dev)
            work = base.clone()
            ctxs = [nb.Scene(p, v) for p, v in states] if batch <= args.max_contexts else []

            def batch_run(entry):
                def run():
                    work.copy_(base)                       # every run from the same state: the paths taken stay the same
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        _lib.check(entry(None, batch, n, K, work[0].data_ptr(), work[1].data_ptr(), stream.cuda_stream))
                        e1.record(stream)
                    e1.synchronize()
                    return e0.elapsed_time(e1)
                return run

            def ctx_run(step):
                def run():
                    t0 = time.perf_counter()
                    for sc in ctxs:
                        step(sc)
                    for sc in ctxs:
                        sc.sync()
                    return (time.perf_counter() - t0) * 1e3
                return run

            runs = {("nbody", "batch"): batch_run(lib.nb_scenes_nbody_step_launch), ("boids", "batch"): batch_run(lib.nb_scenes_boids_step_launch)}
            if ctxs:
                runs[("nbody", "contexts")] = ctx_run(lambda sc: sc.step_n(K))
                runs[("boids", "contexts")] = ctx_run(lambda sc: sc.step_boids_n(K))
            keys = list(runs)
            times = {key: [] for key in keys}
            for key in keys:                               # warm-up
                runs[key]()
                runs[key]()
            for r in range(args.reps):
                for i in range(len(keys)):
                    key = keys[(i + r) % len(keys)]
                    times[key].append(runs[key]())
            for sc in ctxs:
                sc.close()
            for law in ("nbody", "boids"):
                b = times[(law, "batch")]
                bm, bl = statistics.median(b), min(b)
                line = f"{n:5d} {batch:5d} {law:>6} | {bm:12.4f} {bl:8.4f} {batch * K / bm * 1e3:14.3e} | "
                if ctxs:
                    c = times[(law, "contexts")]
                    cm, cl = statistics.median(c), min(c)
                    line += f"{cm:15.4f} {cl:8.4f} {batch * K / cm * 1e3:14.3e} | {cm / bm:6.1f}"
                else:
                    line += f"{'-':>15} {'-':>8} {'-':>14} |      -"
                print(line, flush=True)


if __name__ == "__main__":
    main()
