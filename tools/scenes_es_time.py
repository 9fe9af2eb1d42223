#!/usr/bin/env python3
"""What an evolution-strategies generation on the device costs.

Table 1, per shape (B, F, H), device milliseconds between two events, median and min of --reps (20) runs after a warm-up, the
measurements of a shape taken in the same run in rotating order:
  perturb        ONE nb_scenes_es_perturb_launch: B * M floats written
  memset theta   hipMemsetAsync of the same B * M * 4 bytes: what merely writing the population costs
  rank+update    ONE nb_scenes_es_update_launch: the ranking workgroup, then the update
  rank           the same entry at (F, H) = (1, 1), M = 6: the ranking nearly alone
  memset out     hipMemsetAsync of the bytes that entry writes (ranks, fitnesses, report, mean)
Table 2, at n = 100, W = 1024, k = 8 and the same shapes, wall milliseconds per generation over --generations (10) generations in a
row ending in a wait, median and min of --reps runs after a warm-up, in rotating order:
  device     rewind; score_reset; es_perturb; step_policy_scored(k); es_update -- no wait inside
  host       the way without these entries, on the same context: a numpy draw (mirrored normals), set_policy, upload, score_reset,
             step_policy_scored(k), scores(), a numpy rank and update
  transfers  the host way's two uploads alone: set_policy and upload
scenes_es_time.py [--reps R] [--generations G] [--shapes B:F:H,B:F:H,..] [--bodies n]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nenbody_amd as nb  # noqa: E402
from nenbody_amd import _lib  # noqa: E402
from scenes_score_time import cell, rotate  # noqa: E402

RADIUS_SQ = 4.0e4
GOAL = (0.0, 0.0, 0.0)
COEF = (0.0, 0.0, 0.0, 0.0, -1.0, 0.0)
SIGMA, STEP, SEED = 0.05, 1e-9, 1234
STEPS, WIDTH = 8, 1024


def es_params(step=STEP):
    return _lib.NbEsParams(SIGMA, step, (ctypes.c_float * 6)(*COEF), SEED)


def table_one(args, shapes):
    import torch

    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ep = es_params()
    print(f"ms between two events, median (min) of {args.reps}")
    print(f"{'B':>5} {'F':>4} {'H':>3} {'M':>6} | {'perturb':>17} | {'memset theta':>17} | {'rank+update':>17} | {'rank (M = 6)':>17} | {'memset out':>17}")
    for batch, f, h in shapes:
        m = nb.policy_floats(f, h)
        rng = np.random.default_rng(3)
        mean = torch.from_numpy((rng.standard_normal(m) * 0.1).astype(np.float32)).to(dev)
        mean6 = torch.zeros(6, dtype=torch.float32, device=dev)
        theta = torch.empty(batch * m, dtype=torch.float32, device=dev)
        rec = np.zeros(batch, nb.SCORE_DTYPE)
        rec["goal2"] = rng.uniform(0, 100, batch).astype(np.float32)
        score = torch.from_numpy(rec.view(np.int64)).to(dev)
        out = torch.empty(2 * batch + 4 + m, dtype=torch.int32, device=dev)      # ranks, fitnesses, report, mean'
        p_rank, p_fit, p_rep, p_new = (out.data_ptr() + 4 * o for o in (0, batch, 2 * batch, 2 * batch + 4))

        def timed(launch):
            def run():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record(stream)
                    launch()
                    e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)
            return run

        def hip_ok(status):
            if status != 0:
                raise RuntimeError(f"hipMemsetAsync failed: {status}")

        runs = {
            "perturb": timed(lambda: _lib.check(lib.nb_scenes_es_perturb_launch(ctypes.byref(ep), f, h, 1, 0, batch, mean.data_ptr(), theta.data_ptr(),
                                                                                stream.cuda_stream))),
            "memset theta": timed(lambda: hip_ok(hip.hipMemsetAsync(theta.data_ptr(), 0, batch * m * 4, stream.cuda_stream))),
            "rank+update": timed(lambda: _lib.check(lib.nb_scenes_es_update_launch(ctypes.byref(ep), f, h, 1, batch, score.data_ptr(), mean.data_ptr(), p_new,
                                                                                   p_rank, p_fit, p_rep, stream.cuda_stream))),
            "rank": timed(lambda: _lib.check(lib.nb_scenes_es_update_launch(ctypes.byref(ep), 1, 1, 1, batch, score.data_ptr(), mean6.data_ptr(), p_new,
                                                                            p_rank, p_fit, p_rep, stream.cuda_stream))),
            "memset out": timed(lambda: hip_ok(hip.hipMemsetAsync(out.data_ptr(), 0, out.numel() * 4, stream.cuda_stream))),
        }
        t = rotate(runs, args.reps)
        print(f"{batch:5d} {f:4d} {h:3d} {m:6d} | " + " | ".join(f"{cell(t[key]):>17}" for key in runs), flush=True)


def table_two(args, shapes):
    n, gens = args.bodies, args.generations
    print(f"n = {n}, W = {WIDTH}, k = {STEPS}; wall ms per generation over {gens} generations, median (min) of {args.reps}")
    print(f"{'B':>5} {'F':>4} {'H':>3} | {'device':>19} | {'host':>19} | {'transfers':>19} | host - device")
    for batch, f, h in shapes:
        m = nb.policy_floats(f, h)
        states = [nb.init_state(n, 1100 + s) for s in range(batch)]
        pos, vel = np.stack([p for p, _ in states]), np.stack([v for _, v in states])
        mean0 = (np.random.default_rng(3).standard_normal(m) * 0.1).astype(np.float32)
        with nb.SceneBatch(pos, vel) as sb:
            sb.set_score(RADIUS_SQ, GOAL)
            sb.keep()
            lib, ctx = sb._lib, sb._ctx

            def device():
                sb.es_set(mean0, f, h, SIGMA, STEP, COEF, SEED, 0.5)
                sb.sync()
                t0 = time.perf_counter()
                for _ in range(gens):
                    sb.rewind()
                    sb.score_reset()
                    sb.es_perturb()
                    sb.step_policy_scored(STEPS, WIDTH)
                    sb.es_update()
                sb.sync()
                return (time.perf_counter() - t0) * 1e3 / gens

            def host(transfers_only=False):
                def run():
                    rng = np.random.default_rng(SEED)
                    mean = mean0.copy()
                    sb.sync()
                    t0, spent = time.perf_counter(), 0.0
                    for _ in range(gens):
                        half = rng.standard_normal(((batch + 1) // 2, m), dtype=np.float32)
                        eps = np.empty((batch, m), np.float32)
                        eps[0::2], eps[1::2] = half, -half[:batch // 2]
                        theta = mean[None] + np.float32(SIGMA) * eps
                        t1 = time.perf_counter()
                        sb.set_policy(theta, f, h, 0.5)
                        _lib.check(lib.nb_scenes_upload(ctx, pos.ctypes.data, vel.ctypes.data))
                        spent += time.perf_counter() - t1
                        if transfers_only:
                            continue
                        sb.score_reset()
                        sb.step_policy_scored(STEPS, WIDTH)
                        rec = sb.scores()
                        fitness = -rec["goal2"]
                        rank = np.empty(batch, np.int64)
                        rank[np.argsort(fitness, kind="stable")] = np.arange(batch)
                        mean = mean + np.float32(STEP) * ((2 * rank - (batch - 1)).astype(np.float32) @ eps)
                    return (spent if transfers_only else time.perf_counter() - t0) * 1e3 / gens
                return run

            t = rotate({"device": device, "host": host(), "transfers": host(True)}, args.reps)
        gap = statistics.median(t["host"]) - statistics.median(t["device"])
        print(f"{batch:5d} {f:4d} {h:3d} | {cell(t['device']):>19} | {cell(t['host']):>19} | {cell(t['transfers']):>19} | {gap:9.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--shapes", default="256:64:32,4096:256:64")
    ap.add_argument("--bodies", type=int, default=100)
    ap.add_argument("--tables", default="1,2")
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")]
    if "1" in args.tables.split(","):
        table_one(args, shapes)
    if "2" in args.tables.split(","):
        table_two(args, shapes)


if __name__ == "__main__":
    main()
