"""Per-call time of every entity's eye view, every eye of the set, W = 1024, states: the reference's init
(nb.init_state, seed 1234).  Device time between two events, median / min / max of the reps, the entries ALTERNATING inside every
rep (in an order that rotates from rep to rep) so that they share the device's state:

  eyes      nb_launch_eyes (ids + depth)
  colour    nb_launch_eyes_colour (ids + depth + rgba + bgra8, the reference's 20 x 20 skin, tests/golden/skin_rgba8.npy)
  msaa      nb_launch_eyes_msaa (ids8 + depth8 + rgba + bgra8: 8 samples per column, resolved; the same skin)
  other     nb_launch_eyes of a second build of the library (--other PATH: the parent commit's, say), timed TWICE per rep
            (other, other'): the difference between those two is the spread a build shows against itself
  othercol  nb_launch_eyes_colour of that second build: what msaa is measured against

then Scene.eyes and Scene.eyes_colour with their downloads at N = 100 and 2 048 (wall).

    python -u tools/eyes_time.py [--other LIB.so] [N ...]          (default N: 100 2048 16384 131072)
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
AGAIN = "other'"


def reference_skin():
    img = np.load(os.path.join(ROOT, "tests", "golden", "skin_rgba8.npy"))      # (missing: an error, the table names this skin)
    lin = np.empty(img.shape, np.float32)
    lin[..., :3] = nb.srgb_decode(img[..., :3])
    lin[..., 3] = img[..., 3].astype(np.float32) / np.float32(255)
    return lin


def launch_ms(n, reps, other):
    pos, vel = nb.init_state(n, 1234)
    with nb.Scene(pos, vel) as sc:
        cams = sc.cameras((0.0, 0.0, 1.0), nb.eye_constant(W))
        inst = sc.instances().copy()
    dev = torch.device("cuda", 0)
    ct = torch.from_numpy(cams.reshape(n, 16)).to(dev)
    it = torch.from_numpy(inst.reshape(n, 16)).to(dev)
    ids = torch.empty((n, W), dtype=torch.int32, device=dev)
    depth = torch.empty((n, W), dtype=torch.float32, device=dev)
    rgba = torch.empty((n, W, 4), dtype=torch.float32, device=dev)
    bgra8 = torch.empty((n, W), dtype=torch.int32, device=dev)
    ids8 = torch.empty((n, W, 8), dtype=torch.int32, device=dev)
    depth8 = torch.empty((n, W, 8), dtype=torch.float32, device=dev)
    skin = reference_skin()
    st = torch.from_numpy(skin).to(dev)
    th, tw = skin.shape[:2]
    s = torch.cuda.current_stream(dev)
    lib = _lib.load()

    def eyes():
        _lib.check(lib.nb_launch_eyes(n, 0, n, ct.data_ptr(), it.data_ptr(), W, 0, ids.data_ptr(), depth.data_ptr(), s.cuda_stream))

    def colour():
        _lib.check(lib.nb_launch_eyes_colour(n, 0, n, ct.data_ptr(), it.data_ptr(), W, 0, st.data_ptr(), tw, th,
                                             ids.data_ptr(), depth.data_ptr(), rgba.data_ptr(), bgra8.data_ptr(), s.cuda_stream))

    def msaa():
        _lib.check(lib.nb_launch_eyes_msaa(n, 0, n, ct.data_ptr(), it.data_ptr(), W, 0, st.data_ptr(), tw, th,
                                           ids8.data_ptr(), depth8.data_ptr(), rgba.data_ptr(), bgra8.data_ptr(), s.cuda_stream))

    def other_colour():
        rc = other.nb_launch_eyes_colour(n, 0, n, ct.data_ptr(), it.data_ptr(), W, 0, st.data_ptr(), tw, th,
                                         ids.data_ptr(), depth.data_ptr(), rgba.data_ptr(), bgra8.data_ptr(), s.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"--other: nb_launch_eyes_colour returned {rc}")

    def other_eyes():
        rc = other.nb_launch_eyes(n, 0, n, ct.data_ptr(), it.data_ptr(), W, 0, ids.data_ptr(), depth.data_ptr(), s.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"--other: nb_launch_eyes returned {rc}")

    calls = [("eyes", eyes), ("colour", colour), ("msaa", msaa)]
    if other is not None:
        calls = [("other", other_eyes), ("eyes", eyes), (AGAIN, other_eyes), ("colour", colour), ("othercol", other_colour), ("msaa", msaa)]
    for _, call in calls:
        call()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in calls}
    for r in range(reps):
        k = r % len(calls)      # the order rotates from rep to rep: every entry follows every other equally often
        for name, call in calls[k:] + calls[:k]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            call()
            b.record(s)
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    filled = float((ids != -1).float().mean())
    del ids, depth, rgba, bgra8, ids8, depth8
    torch.cuda.empty_cache()
    return times, filled


def scene_ms(n, reps):
    pos, vel = nb.init_state(n, 1234)
    out = {}
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(reference_skin())
        for name, call in (("Scene.eyes", sc.eyes), ("Scene.eyes_colour", sc.eyes_colour)):
            call(W)
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call(W)
                times.append((time.perf_counter() - t0) * 1e3)
            out[name] = times
    return out


def bind_other(path):
    """nb_launch_eyes and nb_launch_eyes_colour of another build of the library, bound by hand (its other symbols may differ from
    this binding's)"""
    lib = ctypes.CDLL(path)
    c_u32, c_p = ctypes.c_uint32, ctypes.c_void_p
    lib.nb_launch_eyes.restype = ctypes.c_int
    lib.nb_launch_eyes.argtypes = [c_u32, c_u32, c_u32, c_p, c_p, c_u32, c_u32, c_p, c_p, c_p]
    lib.nb_launch_eyes_colour.restype = ctypes.c_int
    lib.nb_launch_eyes_colour.argtypes = [c_u32, c_u32, c_u32, c_p, c_p, c_u32, c_u32, c_p, c_u32, c_u32, c_p, c_p, c_p, c_p, c_p]
    return lib


def main():
    args = sys.argv[1:]
    other = None
    if "--other" in args:
        i = args.index("--other")
        _lib.load()      # (first: this library's loader settles which HIP runtime the process holds)
        other = bind_other(args[i + 1])
        del args[i:i + 2]
    sizes = [int(a) for a in args] or [100, 2048, 16384, 131072]
    print(f"every eye, W = {W}: device ms per call, median / min / max of the reps, the entries alternating; "
          f"eyes writes 8 bytes per column, colour 28, msaa 84")
    for n in sizes:
        reps = 20 if n <= 16384 else 3
        t, filled = launch_ms(n, reps, other)
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"  N = {n:6d} ({reps} reps; filled {filled * 100:.1f} %; eyes writes {n * W * 8 / 2**20:.1f} MiB, colour {n * W * 28 / 2**20:.1f} MiB)")
        for name, v in t.items():
            print(f"    {name:8s} {med[name]:9.4f} / {min(v):9.4f} / {max(v):9.4f} ms", flush=True)
        print(f"    colour / eyes = {med['colour'] / med['eyes']:.3f} (median), {min(t['colour']) / min(t['eyes']):.3f} (min); "
              f"{3.0 * n * n / min(t['eyes']) / 1e6:7.2f} G eye-edges/s")
        base = "othercol" if other is not None else "colour"
        print(f"    msaa / {base} = {med['msaa'] / med[base]:.3f} (median), {min(t['msaa']) / min(t[base]):.3f} (min)")
        if other is not None:
            both = t["other"] + t[AGAIN]
            print(f"    eyes - other = {med['eyes'] - statistics.median(both):+.4f} ms (medians; other: both series together); the spread "
                  f"of the other build against itself: other' - other = {med[AGAIN] - med['other']:+.4f} ms (medians), "
                  f"its calls range over {max(both) - min(both):.4f} ms", flush=True)
    print("Scene.eyes / Scene.eyes_colour (cameras + matrices + kernel + download of every row), every eye: wall ms per call (median / min)")
    for n in (100, 2048):
        for name, t in scene_ms(n, 20).items():
            print(f"  N = {n:6d}: {name:17s} {statistics.median(t):9.3f} / {min(t):9.3f} ms", flush=True)


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
