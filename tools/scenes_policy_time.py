#!/usr/bin/env python3
"""The scene batches' neural policy against their gravity from located vision: for n in {100, 256, 1024} and
B in {1, 16, 256}, W = 1024, the reference's constants and k = 4 steps, a policy per scene,
  policy F,H   device time between two events around the k steps as nb_scenes_step_policy issues them -- per step nb_launch_instances
               and nb_launch_cameras over all bodies, then ONE nb_scenes_policy_step_launch, the record buffers alternating -- on
               caller memory, so that the events sit on the stream of the launches; at (F, H) = (64, 32) and at (1, 1)
  located      the same with nb_scenes_nbody_located_step_launch as the fused launch: the yardstick -- same raster, same launch shape
  fused        the k fused launches of each alone, the matrices left as they are
median and min of --reps (20) runs after a warm-up, the measurements of a shape taken in the same run in rotating order.  The
difference between (64, 32) and (1, 1) is the network's share.
scenes_policy_time.py [--reps R] [--sizes n,n,..] [--batches B,B,..] [--width W]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nenbody_amd as nb  # noqa: E402
from nenbody_amd import _lib  # noqa: E402

K = 4
SHAPES = ((64, 32), (1, 1))
LIMIT = 0.5


def policies(features, hidden, count, rng):
    """unit 0 reads the mean of the features and drives both outputs; the rest is small noise"""
    out = []
    for _ in range(count):
        w1 = rng.uniform(-1, 1, (features, hidden)) / features
        w1[:, 0] = rng.uniform(0.5, 1.5, features) / features
        b1 = rng.uniform(-0.02, 0.02, hidden)
        w2 = rng.uniform(-2, 2, (2, hidden)) / hidden
        w2[:, 0] = rng.uniform(1, 2, 2)
        out.append(nb.pack_policy(w1, b1, w2, rng.uniform(-0.01, 0.01, 2)))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="100,256,1024")
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
    names = [f"policy {f},{h}" for f, h in SHAPES] + ["located"]
    print(f"W = {width}, k = {K}, a policy per scene; ms, median (min) of {args.reps}; step = matrices + fused launch, fused = that launch alone")
    print(f"{'n':>5} {'B':>5} | " + " | ".join(f"{name + ' step':>19} {'fused':>17}" for name in names) + " | (64,32) / located, (64,32) - (1,1) fused")
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
            weights = {shape: torch.from_numpy(policies(*shape, batch, rng)).to(dev) for shape in SHAPES}

            def matrices(cur):
                _lib.check(lib.nb_launch_instances(records, work[cur][0].data_ptr(), work[cur][1].data_ptr(), inst.data_ptr(), stream.cuda_stream))
                _lib.check(lib.nb_launch_cameras(records, work[cur][0].data_ptr(), work[cur][1].data_ptr(), up.ctypes.data, cp.ctypes.data,
                                                 cams.data_ptr(), stream.cuda_stream))

            def policy(shape):
                def fused(cur):
                    _lib.check(lib.nb_scenes_policy_step_launch(None, batch, n, cams.data_ptr(), inst.data_ptr(), width, up.ctypes.data, shape[0],
                                                                shape[1], batch, weights[shape].data_ptr(), LIMIT, work[cur][0].data_ptr(),
                                                                work[cur][1].data_ptr(), work[cur ^ 1][0].data_ptr(),
                                                                work[cur ^ 1][1].data_ptr(), stream.cuda_stream))
                return fused

            def located(cur):
                _lib.check(lib.nb_scenes_nbody_located_step_launch(None, batch, n, cams.data_ptr(), inst.data_ptr(), up.ctypes.data, cp.ctypes.data,
                                                                   width, work[cur][0].data_ptr(), work[cur][1].data_ptr(),
                                                                   work[cur ^ 1][0].data_ptr(), work[cur ^ 1][1].data_ptr(),
                                                                   stream.cuda_stream))

            def device_run(fused, with_matrices):
                def run():
                    work[0].copy_(base)                    # every run from the same state
                    with torch.cuda.stream(stream):
                        matrices(0)                        # (the fused launches alone read these)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        for s in range(K):
                            if with_matrices:
                                matrices(s & 1)
                            fused(s & 1)
                        e1.record(stream)
                    e1.synchronize()
                    return e0.elapsed_time(e1)
                return run

            launches = [policy(shape) for shape in SHAPES] + [located]
            runs = {}
            for name, fused in zip(names, launches):
                runs[name + " step"] = device_run(fused, True)
                runs[name + " fused"] = device_run(fused, False)
            keys = list(runs)
            times = {key: [] for key in keys}
            for key in keys:                               # warm-up
                runs[key]()
                runs[key]()
            for r in range(args.reps):
                for i in range(len(keys)):
                    key = keys[(i + r) % len(keys)]
                    times[key].append(runs[key]())
            med = {key: statistics.median(times[key]) for key in keys}
            cell = lambda key: f"{med[key]:9.4f} ({min(times[key]):.4f})"
            line = f"{n:5d} {batch:5d} | " + " | ".join(f"{cell(name + ' step'):>19} {cell(name + ' fused'):>17}" for name in names)
            line += f" | {med[names[0] + ' step'] / med['located step']:6.2f} {med[names[0] + ' fused'] - med[names[1] + ' fused']:9.4f}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
