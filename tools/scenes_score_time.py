#!/usr/bin/env python3
"""What scoring a scene batch on the device costs.

Table 1, for n in {100, 256, 1024, 2048} and B in {1, 16, 256}, device milliseconds between two events, median and min of --reps (20)
runs after a warm-up, the two measurements of a shape taken in the same run in rotating order, each from the same state:
  score     ONE nb_scenes_score_launch on caller memory
  gravity   ONE nb_scenes_nbody_step_launch with k = 1: the yardstick -- the same launch shape, the same O(n^2) walk over LDS
Table 2, at n = 100, B = 256, W = 1024, a policy (64, 32) per scene, wall milliseconds to the last result, median and min of
--rollouts (5) after a warm-up, in rotating order:
  device    step_policy_scored(8), then scores()
  host      eight times step_policy(1), positions() and velocities(), and the numpy restatement of the score (tests/score_restatement.py)
  download  the host side without its restatement: what the transfers and the waits alone cost
scenes_score_time.py [--reps R] [--rollouts R] [--sizes n,n,..] [--batches B,B,..]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nenbody_amd as nb  # noqa: E402
import score_restatement as Q  # noqa: E402
from nenbody_amd import _lib  # noqa: E402
from scenes_policy_time import policies  # noqa: E402

RADIUS_SQ = 4.0e4        # (the walk does the same work whatever the count)
GOAL = (0.0, 0.0, 0.0)
STEPS = 8


def rotate(runs, reps):
    keys = list(runs)
    times = {key: [] for key in keys}
    for key in keys:                                       # warm-up
        runs[key]()
        runs[key]()
    for r in range(reps):
        for i in range(len(keys)):
            key = keys[(i + r) % len(keys)]
            times[key].append(runs[key]())
    return times


def cell(t):
    return f"{statistics.median(t):9.4f} ({min(t):.4f})"


def table_one(args):
    import torch

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    sp = _lib.NbScoreParams(RADIUS_SQ, (ctypes.c_float * 3)(*GOAL))
    print(f"ms between two events, median (min) of {args.reps}")
    print(f"{'n':>5} {'B':>5} | {'score':>19} | {'gravity, k = 1':>19} | score / gravity")
    for n in (int(x) for x in args.sizes.split(",")):
        for batch in (int(x) for x in args.batches.split(",")):
            records = batch * n
            states = [nb.init_state(n, 1100 + s) for s in range(batch)]
            rec = np.zeros((2, records, 4), np.float32)
            rec[0, :, :3] = np.concatenate([p for p, _ in states])
            rec[1, :, :3] = np.concatenate([v for _, v in states])
            base = torch.from_numpy(rec).to(dev)
            work = base.clone()
            score = torch.zeros(batch * 4, dtype=torch.int64, device=dev)

            def timed(launch):
                def run():
                    work.copy_(base)                       # every run from the same state
                    score.zero_()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        launch()
                        e1.record(stream)
                    e1.synchronize()
                    return e0.elapsed_time(e1)
                return run

            def score_launch():
                _lib.check(lib.nb_scenes_score_launch(ctypes.byref(sp), batch, n, work[0].data_ptr(), work[1].data_ptr(), score.data_ptr(),
                                                      stream.cuda_stream))

            def gravity_launch():
                _lib.check(lib.nb_scenes_nbody_step_launch(None, batch, n, 1, work[0].data_ptr(), work[1].data_ptr(), stream.cuda_stream))

            t = rotate({"score": timed(score_launch), "gravity": timed(gravity_launch)}, args.reps)
            ratio = statistics.median(t["score"]) / statistics.median(t["gravity"])
            print(f"{n:5d} {batch:5d} | {cell(t['score']):>19} | {cell(t['gravity']):>19} | {ratio:6.2f}", flush=True)


def table_two(args):
    n, batch, width, shape = 100, 256, 1024, (64, 32)
    states = [nb.init_state(n, 1100 + s) for s in range(batch)]
    pos, vel = np.stack([p for p, _ in states]), np.stack([v for _, v in states])
    weights = policies(*shape, batch, np.random.default_rng(7))

    def rollout(form):
        def run():
            with nb.SceneBatch(pos, vel) as sb:
                sb.set_policy(weights, *shape, 0.5)
                sb.set_score(RADIUS_SQ, GOAL)
                sb.sync()
                t0 = time.perf_counter()
                if form == "device":
                    sb.step_policy_scored(STEPS, width)
                    records = sb.scores()
                else:
                    records = None
                    for _ in range(STEPS):
                        sb.step_policy(1, width)
                        p, v = sb.positions(), sb.velocities()
                        if form == "host":
                            records = Q.batch(p, v, RADIUS_SQ, GOAL, acc=records)
                t1 = time.perf_counter()
            run.records = records
            return (t1 - t0) * 1e3
        return run

    runs = {form: rollout(form) for form in ("device", "host", "download")}
    t = rotate(runs, args.rollouts)
    print(f"the two rollouts' records agree: {Q.same(runs['device'].records, runs['host'].records)}")
    print(f"n = {n}, B = {batch}, W = {width}, policy {shape}, {STEPS} steps; wall ms to the last result, median (min) of {args.rollouts}")
    for form in runs:
        print(f"{form:>9} | {cell(t[form]):>23}")
    print(f"host / device {statistics.median(t['host']) / statistics.median(t['device']):8.1f}, "
          f"download / device {statistics.median(t['download']) / statistics.median(t['device']):6.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rollouts", type=int, default=5)
    ap.add_argument("--sizes", default="100,256,1024,2048")
    ap.add_argument("--batches", default="1,16,256")
    args = ap.parse_args()
    table_one(args)
    table_two(args)


if __name__ == "__main__":
    main()
