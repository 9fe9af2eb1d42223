"""Per-stage time of one located gravity step, every body of the set, W = 1024, state: the reference's init
(nb.init_state, seed 1234).  Device time between two events, median / min / max of the reps, the entries ALTERNATING inside every rep
(in an order that rotates from rep to rep) so that they share the device's state.  The stages through the stateless launches, on the
same tensors the step would chain:

  matrices  nb_launch_instances + nb_launch_cameras (the model matrices and the eye cameras of every body)
  rows      nb_launch_eyes, ids and depth (what the step runs)
  seen      nb_launch_seen with depth (count + list + nearest depths)
  located   nb_seen_located_launch (seen_rel alone, as the step runs it)
  fold      nb_nbody_located_step_launch over those rows
  otherrows with --other LIB.so (the parent commit's build, say): its nb_launch_eyes (ids + depth) on the same tensors
  otherstep its nb_step on a context of its own (one step + sync, wall): the unchanged-kernel check, beside
  step      this library's nb_step on a context of its own, the two alternating

then nb_step_nbody_located itself (Scene.step_nbody_located_n(k) + sync, wall per step), the batches chained on the context's stream:
with the library's batch (batch = 0: 2 047 eyes at W = 1024) and with the whole set as one batch.

    python -u tools/located_time.py [--other LIB.so] [N ...]          (default N: 100 2048 16384)
"""
import ctypes
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


def records(a, dev):
    r = np.zeros((len(a), 4), np.float32)
    r[:, :3] = a
    return torch.from_numpy(r).to(dev)


class Context:
    """a context of `lib` (this library or another build of it) holding the init state: nb_step on the current stream's device"""

    def __init__(self, lib, pos, vel):
        self.lib, self.ctx = lib, ctypes.c_void_p()
        if lib.nb_create(len(pos), 1, None, ctypes.byref(self.ctx)) != 0 or lib.nb_upload(self.ctx, pos.ctypes.data, vel.ctypes.data) != 0:
            raise RuntimeError("nb_create / nb_upload failed")

    def step(self):
        if self.lib.nb_step(self.ctx, 1) != 0:
            raise RuntimeError("nb_step failed")

    def close(self):
        self.lib.nb_sync(self.ctx)
        self.lib.nb_destroy(self.ctx)


def launch_ms(n, reps, other):
    pos, vel = nb.init_state(n, 1234)
    dev = torch.device("cuda", 0)
    tp, tv = records(pos, dev), records(vel, dev)
    op, ov = torch.empty_like(tp), torch.empty_like(tv)
    inst = torch.empty((n, 16), dtype=torch.float32, device=dev)
    cams = torch.empty((n, 16), dtype=torch.float32, device=dev)
    ids = torch.empty((n, W), dtype=torch.int32, device=dev)
    depth = torch.empty((n, W), dtype=torch.float32, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    lists = torch.empty((n, W), dtype=torch.int32, device=dev)
    ldepth = torch.empty((n, W), dtype=torch.float32, device=dev)
    rel = torch.empty((n, W, 4), dtype=torch.float32, device=dev)
    up = np.array([0, 0, 1], np.float32)
    cp = np.ascontiguousarray(nb.eye_constant(W))
    s = torch.cuda.current_stream(dev)
    lib = _lib.load()

    def matrices():
        _lib.check(lib.nb_launch_instances(n, tp.data_ptr(), tv.data_ptr(), inst.data_ptr(), s.cuda_stream))
        _lib.check(lib.nb_launch_cameras(n, tp.data_ptr(), tv.data_ptr(), up.ctypes.data, cp.ctypes.data, cams.data_ptr(), s.cuda_stream))

    def rows():
        _lib.check(lib.nb_launch_eyes(n, 0, n, cams.data_ptr(), inst.data_ptr(), W, 0, ids.data_ptr(), depth.data_ptr(), s.cuda_stream))

    def seen():
        _lib.check(lib.nb_launch_seen(n, W, ids.data_ptr(), depth.data_ptr(), cnt.data_ptr(), lists.data_ptr(), ldepth.data_ptr(), None,
                                      s.cuda_stream))

    def located():
        _lib.check(lib.nb_seen_located_launch(n, W, ids.data_ptr(), depth.data_ptr(), cnt.data_ptr(), lists.data_ptr(), ldepth.data_ptr(),
                                              tp.data_ptr(), tv.data_ptr(), up.ctypes.data, cp.ctypes.data, None, rel.data_ptr(), s.cuda_stream))

    def fold():
        _lib.check(lib.nb_nbody_located_step_launch(None, n, 0, n, tp.data_ptr(), tv.data_ptr(), cnt.data_ptr(), rel.data_ptr(), W,
                                                    op.data_ptr(), ov.data_ptr(), s.cuda_stream))

    def other_rows():
        rc = other.nb_launch_eyes(n, 0, n, cams.data_ptr(), inst.data_ptr(), W, 0, ids.data_ptr(), depth.data_ptr(), s.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"--other: nb_launch_eyes returned {rc}")

    # the order below is the step's: every stage finds its inputs in place, whichever entry the rotation starts with
    calls = [("matrices", matrices), ("rows", rows), ("seen", seen), ("located", located), ("fold", fold)]
    if other is not None:
        calls += [("otherrows", other_rows)]
    for _, call in calls:
        call()
    torch.cuda.synchronize()
    sizes = cnt.cpu().numpy()
    times = {name: [] for name, _ in calls}
    for r in range(reps):
        k = r % len(calls)
        for name, call in calls[k:] + calls[:k]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            call()
            b.record(s)
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return times, sizes


def nb_step_ms(n, reps, other):
    """nb_step of this library and of the other one, alternating, each on a context of its own: wall time of one step + sync after a
    warm-up step (the contexts run on streams of their own, which the events of this process cannot bracket)"""
    pos, vel = nb.init_state(n, 1234)
    libs = [("step", _lib.load())] + ([("otherstep", other)] if other is not None else [])
    ctxs = [(name, Context(lib, pos, vel)) for name, lib in libs]
    times = {name: [] for name, _ in ctxs}
    for _, c in ctxs:
        c.step()
        c.lib.nb_sync(c.ctx)
    for r in range(reps):
        k = r % len(ctxs)
        for name, c in ctxs[k:] + ctxs[:k]:
            t0 = time.perf_counter()
            c.step()
            c.lib.nb_sync(c.ctx)
            times[name].append((time.perf_counter() - t0) * 1e3)
    for _, c in ctxs:
        c.close()
    return times


def step_ms(n, k, reps, batch=0):
    pos, vel = nb.init_state(n, 1234)
    out = []
    with nb.Scene(pos, vel) as sc:          # warm-up: the kernels' code objects
        sc.step_nbody_located_n(1, batch=batch)
        sc.sync()
    for _ in range(reps):
        with nb.Scene(pos, vel) as sc:      # a fresh state every rep
            sc.located(count=1)             # (the context's rows and lists exist before the clock starts; the step grows them to its batch)
            t0 = time.perf_counter()
            sc.step_nbody_located_n(k, batch=batch)
            sc.sync()
            out.append((time.perf_counter() - t0) * 1e3 / k)
    return out


def bind_other(path):
    """nb_launch_eyes and the context entries nb_step needs of another build of the library, bound by hand (its other symbols may
    differ from this binding's)"""
    lib = ctypes.CDLL(path)
    c_u32, c_p = ctypes.c_uint32, ctypes.c_void_p
    lib.nb_launch_eyes.restype = ctypes.c_int
    lib.nb_launch_eyes.argtypes = [c_u32, c_u32, c_u32, c_p, c_p, c_u32, c_u32, c_p, c_p, c_p]
    for name in ("nb_create", "nb_upload", "nb_step", "nb_sync", "nb_destroy"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
    return lib


def main():
    args = sys.argv[1:]
    other = None
    if "--other" in args:
        i = args.index("--other")
        _lib.load()      # (first: this library's loader settles which HIP runtime the process holds)
        other = bind_other(args[i + 1])
        del args[i:i + 2]
    sizes = [int(a) for a in args] or [100, 2048, 16384]
    print(f"one located gravity step, every body, W = {W}: device ms per stage, median / min / max of the reps, the entries alternating")
    for n in sizes:
        reps = 20
        t, seen = launch_ms(n, reps, other)
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"  N = {n:6d} ({reps} reps; seen-set size mean {seen.mean():.1f}, max {seen.max()}, blind {int((seen == 0).sum())})")
        for name, v in t.items():
            print(f"    {name:9s} {med[name]:9.4f} / {min(v):9.4f} / {max(v):9.4f} ms", flush=True)
        print(f"    located = {med['located'] / med['seen']:.4f} of seen, located + fold = {(med['located'] + med['fold']) / med['rows']:.4f} of rows (medians); "
              f"the five stages together {sum(med[k] for k in ('matrices', 'rows', 'seen', 'located', 'fold')):.4f} ms")
        for name, v in nb_step_ms(n, reps, other).items():
            print(f"    nb_step ({name}), one step + sync, wall: {statistics.median(v):9.4f} / {min(v):9.4f} / {max(v):9.4f} ms", flush=True)
        for batch, what in ((0, "batch = 0"), (n, "one batch")):
            w = step_ms(n, 3, 5, batch)
            print(f"    nb_step_nbody_located, {what}, 3 steps + sync: {statistics.median(w):9.4f} / {min(w):9.4f} / {max(w):9.4f} ms per step (wall)",
                  flush=True)


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
