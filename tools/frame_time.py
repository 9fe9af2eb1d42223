"""Per-call time of the scene camera's frame: nb_launch_frame with all four outputs at 1920 x 1080 through
the reference's scene camera above body 0, at height 990 (the reference's) and at height 120 (bodies eight times larger), states:
the reference's init (nb.init_state, seed 1234), the reference's 20 x 20 skin.  Device time between two events on one stream,
median / min / max of the reps (20; 3 at N = 131 072).  Up to N = 2 048 nb_launch_eyes_colour over every eye (W = 1024) is timed in
the same run, the calls ALTERNATING inside every rep in an order that rotates from rep to rep: the frame's bar is that call's median
at N = 2 048 (it writes as many pixels after 2 048 times the edge work).

Per N and height it also prints the covered pixels (counted on the device's ids) and the pixel writes (counted by the rule's
restatement, tests/frame_restatement.py, on the same camera and matrices), and the bytes each pass moves.  The three passes
separately are the kernel trace's: run

    rocprofv3 --kernel-trace --stats -- python tools/frame_time.py --once N [HEIGHT]

which launches the frame 20 times and nothing else; frame_clear_kernel, frame_edges_kernel and frame_resolve_kernel are its rows.

    python -u tools/frame_time.py [N ...]          (default N: 100 2048 16384 131072)
"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import nenbody_amd as nb  # noqa: E402
from nenbody_amd import _lib  # noqa: E402

EXTENT = (1920, 1080)
EYE_W = 1024


def reference_skin():
    img = np.load(os.path.join(ROOT, "tests", "golden", "skin_rgba8.npy"))      # (missing: an error, the table names this skin)
    lin = np.empty(img.shape, np.float32)
    lin[..., :3] = nb.srgb_decode(img[..., :3])
    lin[..., 3] = img[..., 3].astype(np.float32) / np.float32(255)
    return lin


class Setup:
    """device tensors of one state and one camera height, and the two calls on the current stream"""

    def __init__(self, n, height, with_eyes):
        W, H = EXTENT
        pos, vel = nb.init_state(n, 1234)
        with nb.Scene(pos, vel) as sc:
            self.cam = sc.scene_camera(EXTENT, height=height)
            self.inst = sc.instances().copy()
            cams = sc.cameras((0.0, 0.0, 1.0), nb.eye_constant(EYE_W)) if with_eyes else None
        self.n, self.dev = n, torch.device("cuda", 0)
        dev = self.dev
        self.ct = torch.from_numpy(self.cam.reshape(16).copy()).to(dev)
        self.it = torch.from_numpy(self.inst.reshape(n, 16)).to(dev)
        self.ids = torch.empty((H, W), dtype=torch.int32, device=dev)
        self.depth = torch.empty((H, W), dtype=torch.float32, device=dev)
        self.rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        self.bgra8 = torch.empty((H, W), dtype=torch.int32, device=dev)
        self.lib = _lib.load()
        self.scratch = torch.empty(self.lib.nb_frame_scratch_bytes(W, H) // 8, dtype=torch.int64, device=dev)
        skin = reference_skin()
        self.st = torch.from_numpy(skin).to(dev)
        self.th, self.tw = skin.shape[:2]
        self.s = torch.cuda.current_stream(dev)
        if with_eyes:
            self.ect = torch.from_numpy(cams.reshape(n, 16)).to(dev)
            self.eids = torch.empty((n, EYE_W), dtype=torch.int32, device=dev)
            self.edepth = torch.empty((n, EYE_W), dtype=torch.float32, device=dev)
            self.ergba = torch.empty((n, EYE_W, 4), dtype=torch.float32, device=dev)
            self.ebgra8 = torch.empty((n, EYE_W), dtype=torch.int32, device=dev)

    def frame(self):
        W, H = EXTENT
        _lib.check(self.lib.nb_launch_frame(self.n, self.ct.data_ptr(), self.it.data_ptr(), W, H, 0, self.st.data_ptr(), self.tw, self.th,
                                            self.scratch.data_ptr(), self.ids.data_ptr(), self.depth.data_ptr(), self.rgba.data_ptr(),
                                            self.bgra8.data_ptr(), self.s.cuda_stream))

    def eyes_colour(self):
        n = self.n
        _lib.check(self.lib.nb_launch_eyes_colour(n, 0, n, self.ect.data_ptr(), self.it.data_ptr(), EYE_W, 0, self.st.data_ptr(), self.tw,
                                                  self.th, self.eids.data_ptr(), self.edepth.data_ptr(), self.ergba.data_ptr(),
                                                  self.ebgra8.data_ptr(), self.s.cuda_stream))


def measure(setup, calls, reps):
    for _, call in calls:
        call()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in calls}
    for r in range(reps):
        k = r % len(calls)      # the order rotates from rep to rep: every entry follows every other equally often
        for name, call in calls[k:] + calls[:k]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(setup.s)
            call()
            b.record(setup.s)
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return times


def once(n, height):
    setup = Setup(n, height, False)
    for _ in range(20):
        setup.frame()
    torch.cuda.synchronize()
    print(f"N = {n}, height {height}: 20 frames launched")


def main():
    args = sys.argv[1:]
    if args and args[0] == "--once":
        once(int(args[1]), float(args[2]) if len(args) > 2 else 990.0)
        return
    import frame_restatement as FR

    W, H = EXTENT
    sizes = [int(a) for a in args] or [100, 2048, 16384, 131072]
    print(f"the frame at {W} x {H}, all four outputs: device ms per call, median / min / max of the reps; the clear pass writes "
          f"{W * H * 8 / 2**20:.1f} MiB of keys, the resolve pass reads them and writes {W * H * 28 / 2**20:.1f} MiB")
    for n in sizes:
        reps = 20 if n <= 16384 else 3
        for height in (990.0, 120.0):
            with_eyes = n <= 2048
            setup = Setup(n, height, with_eyes)
            calls = [("frame", setup.frame)] + ([("colour", setup.eyes_colour)] if with_eyes else [])
            t = measure(setup, calls, reps)
            covered = int((setup.ids != -1).sum())
            stats = {}
            FR.frame(setup.cam, setup.inst, W, H, stats=stats)
            assert stats["covered"] == covered, (stats["covered"], covered)
            print(f"  N = {n:6d}, height {height:5.0f} ({reps} reps): {covered} covered pixels, {stats['writes']} pixel writes over "
                  f"{stats['kept']} kept edges (longest {stats['longest']}); the edges pass reads {n * 64 / 2**20:.2f} MiB of matrices")
            for name, v in t.items():
                print(f"    {name:7s} {statistics.median(v):9.4f} / {min(v):9.4f} / {max(v):9.4f} ms", flush=True)
            if with_eyes:
                print(f"    frame / colour = {statistics.median(t['frame']) / statistics.median(t['colour']):.3f} (medians): "
                      f"nb_launch_eyes_colour over {n} eyes of {EYE_W} columns in the same run")
            del setup
            torch.cuda.empty_cache()


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
