#!/usr/bin/env python3
"""The scene batches' recurrent policy against their feedforward policy: for n in {100, 256} and B in
{1, 16, 256}, W = 1024, k = 4 steps, a policy per scene, at the shapes (F, H) = (64, 32) and (256, 64),
  recurrent    device time between two events around the k fused launches of nb_scenes_policy_recurrent_step_launch alone, the matrices
               left as they are, the record buffers alternating and the memory in place
  feedforward  the same with nb_scenes_policy_step_launch of the same (w1, b1, w2, b2): the yardstick, on the same state in the same run
  (1, 1)       the feedforward launch at (F, H) = (1, 1): feedforward - (1, 1) is the network's share of the step
median and min of --reps (20) runs after a warm-up, the measurements of a shape taken in the same run in rotating order.  The last
columns: recurrent - feedforward, the excess; the network's share; and the share x H / F, which is what the H further rows of the
chain should cost.
scenes_policy_recurrent_time.py [--reps R] [--sizes n,n,..] [--batches B,B,..] [--width W]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nenbody_amd as nb  # noqa: E402
from nenbody_amd import _lib  # noqa: E402

K = 4
SHAPES = ((64, 32), (256, 64))
LIMIT = 0.5
MEMORY_LIMIT = 1.0


def policies(features, hidden, count, rng):
    """(feedforward, recurrent) policies of the same (w1, b1, w2, b2): unit 0 reads the mean of the features, drives both outputs and
    feeds itself; the rest is small noise"""
    forward, recurrent = [], []
    for _ in range(count):
        w1 = rng.uniform(-1, 1, (features, hidden)) / features
        w1[:, 0] = rng.uniform(0.5, 1.5, features) / features
        wr = rng.uniform(-1, 1, (hidden, hidden)) / hidden
        wr[0, 0] = 0.7
        b1 = rng.uniform(-0.02, 0.02, hidden)
        w2 = rng.uniform(-2, 2, (2, hidden)) / hidden
        w2[:, 0] = rng.uniform(1, 2, 2)
        b2 = rng.uniform(-0.01, 0.01, 2)
        forward.append(nb.pack_policy(w1, b1, w2, b2))
        recurrent.append(nb.pack_policy_recurrent(w1, wr, b1, w2, b2))
    return np.stack(forward), np.stack(recurrent)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="100,256")
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--width", type=int, default=1024)
    args = ap.parse_args()
    import torch

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    width = args.width
    up = np.array([0, 0, 1], np.float32)
    cp = np.ascontiguousarray(nb.eye_constant(width), np.float32).reshape(16)
    rng = np.random.default_rng(7)
    print(f"W = {width}, k = {K}, a policy per scene; ms of the k fused launches, median (min) of {args.reps}")
    print(f"{'n':>5} {'B':>5} {'F,H':>7} | {'recurrent':>17} | {'feedforward':>17} | {'(1,1)':>17} | {'excess':>8} {'share':>8} {'share H/F':>9}")
    for n in (int(x) for x in args.sizes.split(",")):
        for batch in (int(x) for x in args.batches.split(",")):
            records = batch * n
            states = [nb.init_state(n, 1100 + s) for s in range(batch)]
            rec = np.zeros((2, records, 4), np.float32)
            rec[0, :, :3] = np.concatenate([p for p, _ in states])
            rec[1, :, :3] = np.concatenate([v for _, v in states])
            base = torch.from_numpy(rec).to(dev)
            work = [base.clone(), torch.empty_like(base)]
            cams = torch.empty((records, 16), dtype=torch.float32, device=dev)
            inst = torch.empty((records, 16), dtype=torch.float32, device=dev)
            one = torch.from_numpy(policies(1, 1, batch, rng)[0]).to(dev)

            def matrices():
                _lib.check(lib.nb_launch_instances(records, work[0][0].data_ptr(), work[0][1].data_ptr(), inst.data_ptr(), stream.cuda_stream))
                _lib.check(lib.nb_launch_cameras(records, work[0][0].data_ptr(), work[0][1].data_ptr(), up.ctypes.data, cp.ctypes.data,
                                                 cams.data_ptr(), stream.cuda_stream))

            def feedforward(shape, weights):
                def fused(cur):
                    _lib.check(lib.nb_scenes_policy_step_launch(None, batch, n, cams.data_ptr(), inst.data_ptr(), width, up.ctypes.data, shape[0],
                                                                shape[1], batch, weights.data_ptr(), LIMIT, work[cur][0].data_ptr(),
                                                                work[cur][1].data_ptr(), work[cur ^ 1][0].data_ptr(),
                                                                work[cur ^ 1][1].data_ptr(), stream.cuda_stream))
                return fused

            def recurrent(shape, weights, memory):
                def fused(cur):
                    _lib.check(lib.nb_scenes_policy_recurrent_step_launch(None, batch, n, cams.data_ptr(), inst.data_ptr(), width, up.ctypes.data,
                                                                          shape[0], shape[1], batch, weights.data_ptr(), LIMIT, MEMORY_LIMIT,
                                                                          work[cur][0].data_ptr(), work[cur][1].data_ptr(), memory.data_ptr(),
                                                                          work[cur ^ 1][0].data_ptr(), work[cur ^ 1][1].data_ptr(),
                                                                          memory.data_ptr(), stream.cuda_stream))
                return fused

            def device_run(fused, memory=None):
                def run():
                    work[0].copy_(base)                    # every run from the same state and an empty memory
                    if memory is not None:
                        memory.zero_()
                    with torch.cuda.stream(stream):
                        matrices()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        for s in range(K):
                            fused(s & 1)
                        e1.record(stream)
                    e1.synchronize()
                    return e0.elapsed_time(e1)
                return run

            for shape in SHAPES:
                fw, rc = (torch.from_numpy(w).to(dev) for w in policies(*shape, batch, rng))
                memory = torch.zeros((records, shape[1]), dtype=torch.float32, device=dev)
                runs = {"recurrent": device_run(recurrent(shape, rc, memory), memory), "feedforward": device_run(feedforward(shape, fw)),
                        "(1,1)": device_run(feedforward((1, 1), one))}
                keys = list(runs)
                times = {key: [] for key in keys}
                for key in keys:                           # warm-up
                    runs[key]()
                    runs[key]()
                for r in range(args.reps):
                    for i in range(len(keys)):
                        key = keys[(i + r) % len(keys)]
                        times[key].append(runs[key]())
                med = {key: statistics.median(times[key]) for key in keys}
                cell = lambda key: f"{med[key]:9.4f} ({min(times[key]):.4f})"
                share = med["feedforward"] - med["(1,1)"]
                print(f"{n:5d} {batch:5d} {shape[0]:3d},{shape[1]:3d} | " + " | ".join(f"{cell(key):>17}" for key in keys)
                      + f" | {med['recurrent'] - med['feedforward']:8.4f} {share:8.4f} {share * shape[1] / shape[0]:9.4f}", flush=True)


if __name__ == "__main__":
    main()
