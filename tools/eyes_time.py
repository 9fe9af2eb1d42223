"""Per-call time of every entity's eye view: nb_launch_eyes on device tensors, every eye of the set, W = 1024,
at N = 100, 2 048, 16 384 and 131 072 (device time between two events), and Scene.eyes with its download at N = 100 and 2 048 (wall).
States: the reference's init (nb.init_state, seed 1234).

    python -u tools/eyes_time.py [N ...]
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import nenbody_amd as nb  # noqa: E402
from nenbody_amd import _lib  # noqa: E402

W = 1024


def launch_ms(n, reps):
    pos, vel = nb.init_state(n, 1234)
    with nb.Scene(pos, vel) as sc:
        cams = sc.cameras((0.0, 0.0, 1.0), nb.eye_constant(W))
        inst = sc.instances().copy()
    dev = torch.device("cuda", 0)
    ct = torch.from_numpy(cams.reshape(n, 16)).to(dev)
    it = torch.from_numpy(inst.reshape(n, 16)).to(dev)
    ids = torch.empty((n, W), dtype=torch.int32, device=dev)
    depth = torch.empty((n, W), dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream(dev)
    lib = _lib.load()

    def call():
        _lib.check(lib.nb_launch_eyes(n, 0, n, ct.data_ptr(), it.data_ptr(), W, 0, ids.data_ptr(), depth.data_ptr(), s.cuda_stream))

    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        call()
        b.record(s)
        b.synchronize()
        times.append(a.elapsed_time(b))
    filled = float((ids != -1).float().mean())
    del ids, depth
    torch.cuda.empty_cache()
    return times, filled


def scene_ms(n, reps):
    pos, vel = nb.init_state(n, 1234)
    with nb.Scene(pos, vel) as sc:
        sc.eyes(W)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            sc.eyes(W)
            times.append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [100, 2048, 16384, 131072]
    print(f"nb_launch_eyes, every eye, W = {W}: device ms per call (median / min of the reps), share of columns that see a body")
    for n in sizes:
        reps = 20 if n <= 16384 else 3
        t, filled = launch_ms(n, reps)
        edges = 3.0 * n * n
        print(f"  N = {n:6d}: {statistics.median(t):9.3f} / {min(t):9.3f} ms  ({reps} reps; {edges / min(t) / 1e6:7.2f} G eye-edges/s; "
              f"output {n * W * 8 / 2**20:.1f} MiB; filled {filled * 100:.1f} %)", flush=True)
    print("Scene.eyes (cameras + matrices + eyes + download of both rows), every eye: wall ms per call (median / min)")
    for n in (100, 2048):
        t = scene_ms(n, 20)
        print(f"  N = {n:6d}: {statistics.median(t):9.3f} / {min(t):9.3f} ms", flush=True)


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
