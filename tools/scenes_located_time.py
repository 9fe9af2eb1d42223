#!/usr/bin/env python3
"""The scene batches' gravity from located vision against B contexts: for n in {100, 256, 1024, 2048} and
B in {1, 16, 256}, W = 1024, the reference's constants and k = 4 steps,
  batch     device time between two events around the k steps as nb_scenes_step_nbody_located issues them -- per step
            nb_launch_instances and nb_launch_cameras over all bodies, then ONE nb_scenes_nbody_located_step_launch, the record
            buffers alternating -- on caller memory, so that the events sit on the stream of the launches
  fused     the k fused launches alone, the matrices left as they are
  matrices  the k nb_launch_instances + nb_launch_cameras alone
  contexts  the only way the library offered before: B contexts' nb_step_nbody_located(k) issued back to back, wall time to the last sync
median and min of --reps (20) runs after a warm-up, the measurements of a shape taken in the same run in rotating order.
scenes_located_time.py [--reps R] [--max-contexts C] [--sizes n,n,..] [--batches B,B,..] [--width W]
(--max-contexts: shapes with more scenes than that time the batch only)
One fold form is built (every lane forms its members' located points and quotients, lane 0 adds them in slot order), so there is
no second one to time."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nenbody_amd as nb  # noqa: E402
from nenbody_amd import _lib  # noqa: E402

K = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-contexts", type=int, default=256)
    ap.add_argument("--sizes", default="100,256,1024,2048")
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
    print(f"W = {width}, k = {K}; ms, median (min) of {args.reps}")
    print(f"{'n':>5} {'B':>5} | {'batch':>17} {'scene-steps/s':>13} | {'fused':>17} | {'matrices':>17} | {'contexts':>19} | ratio")
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
            ctxs = [nb.Scene(p, v) for p, v in states] if batch <= args.max_contexts else []

            def matrices(cur):
                _lib.check(lib.nb_launch_instances(records, work[cur][0].data_ptr(), work[cur][1].data_ptr(), inst.data_ptr(), stream.cuda_stream))
                _lib.check(lib.nb_launch_cameras(records, work[cur][0].data_ptr(), work[cur][1].data_ptr(), up.ctypes.data, cp.ctypes.data,
                                                 cams.data_ptr(), stream.cuda_stream))

            def fused(cur):
                _lib.check(lib.nb_scenes_nbody_located_step_launch(None, batch, n, cams.data_ptr(), inst.data_ptr(), up.ctypes.data, cp.ctypes.data,
                                                                   width, work[cur][0].data_ptr(), work[cur][1].data_ptr(),
                                                                   work[cur ^ 1][0].data_ptr(), work[cur ^ 1][1].data_ptr(),
                                                                   stream.cuda_stream))

            def device_run(with_matrices, with_fused):
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
                                matrices(s & 1 if with_fused else 0)
                            if with_fused:
                                fused(s & 1)
                        e1.record(stream)
                    e1.synchronize()
                    return e0.elapsed_time(e1)
                return run

            def ctx_run():
                t0 = time.perf_counter()
                for sc in ctxs:
                    sc.step_nbody_located_n(K, width=width)
                for sc in ctxs:
                    sc.sync()
                return (time.perf_counter() - t0) * 1e3

            runs = {"batch": device_run(True, True), "fused": device_run(False, True), "matrices": device_run(True, False)}
            if ctxs:
                runs["contexts"] = ctx_run
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
            cell = lambda key: f"{statistics.median(times[key]):9.4f} ({min(times[key]):.4f})"
            bm = statistics.median(times["batch"])
            line = f"{n:5d} {batch:5d} | {cell('batch'):>17} {batch * K / bm * 1e3:13.3e} | {cell('fused'):>17} | {cell('matrices'):>17} | "
            if ctxs:
                line += f"{cell('contexts'):>19} | {statistics.median(times['contexts']) / bm:6.1f}"
            else:
                line += f"{'-':>19} |      -"
            print(line, flush=True)


if __name__ == "__main__":
    main()
