"""Per-call time of the frame through 8 samples per pixel: nb_launch_frame_msaa against nb_launch_frame
from the same library, all four outputs each, at 1920 x 1080 through the reference's scene camera above body 0, at height 990 (the
reference's) and at height 120 (bodies eight times larger), states: the reference's init (nb.init_state, seed 1234), the reference's
20 x 20 skin.  Device time between two events on one stream; the two calls ALTERNATE inside every repetition in an order that
rotates from repetition to repetition; median / min of 20 repetitions, and the ratio of the medians.

Per N and height it also prints the covered samples and the pixels holding one (counted on the device's ids8).  The three passes
separately are the kernel trace's: run

    rocprofv3 --kernel-trace --stats -- python tools/frame_msaa_time.py --once N [HEIGHT]

which launches the 8-sample frame 20 times and nothing else; frame_clear_kernel, frame_msaa_edges_kernel and
frame_msaa_resolve_kernel are its rows.

    python -u tools/frame_msaa_time.py [N ...]          (default N: 100 2048 16384)
"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_time as FT  # noqa: E402  (puts the repository root on the path)
import torch  # noqa: E402

from nenbody_amd import _lib  # noqa: E402

EXTENT = FT.EXTENT
REPS = 20


class Setup(FT.Setup):
    """frame_time's tensors and its nb_launch_frame call, plus the sample outputs, the larger key plane and the 8-sample call"""

    def __init__(self, n, height):
        super().__init__(n, height, False)
        W, H = EXTENT
        self.ids8 = torch.empty((H, W, 8), dtype=torch.int32, device=self.dev)
        self.depth8 = torch.empty((H, W, 8), dtype=torch.float32, device=self.dev)
        self.scratch8 = torch.empty(self.lib.nb_frame_msaa_scratch_bytes(W, H) // 8, dtype=torch.int64, device=self.dev)

    def frame_msaa(self):
        W, H = EXTENT
        _lib.check(self.lib.nb_launch_frame_msaa(self.n, self.ct.data_ptr(), self.it.data_ptr(), W, H, 0, self.st.data_ptr(), self.tw,
                                                 self.th, self.scratch8.data_ptr(), self.ids8.data_ptr(), self.depth8.data_ptr(),
                                                 self.rgba.data_ptr(), self.bgra8.data_ptr(), self.s.cuda_stream))


def once(n, height):
    setup = Setup(n, height)
    for _ in range(20):
        setup.frame_msaa()
    torch.cuda.synchronize()
    print(f"N = {n}, height {height}: 20 frames of 8 samples per pixel launched")


def main():
    args = sys.argv[1:]
    if args and args[0] == "--once":
        once(int(args[1]), float(args[2]) if len(args) > 2 else 990.0)
        return
    W, H = EXTENT
    sizes = [int(a) for a in args] or [100, 2048, 16384]
    print(f"the frame at {W} x {H} through 8 samples per pixel against one, all four outputs each: device ms per call, median / min of "
          f"{REPS} repetitions; the clear pass writes {W * H * 64 / 2**20:.1f} MiB of keys (one sample: {W * H * 8 / 2**20:.1f}), the "
          f"resolve pass reads them and writes {W * H * 84 / 2**20:.1f} MiB ({W * H * 28 / 2**20:.1f})")
    for n in sizes:
        for height in (990.0, 120.0):
            setup = Setup(n, height)
            t = FT.measure(setup, [("msaa", setup.frame_msaa), ("frame", setup.frame)], REPS)
            covered = setup.ids8 != -1
            print(f"  N = {n:6d}, height {height:5.0f}: {int(covered.sum())} covered samples in {int(covered.any(-1).sum())} pixels "
                  f"({int((setup.ids != -1).sum())} pixels through one sample)")
            for name, v in t.items():
                print(f"    {name:6s} {statistics.median(v):9.4f} / {min(v):9.4f} ms", flush=True)
            print(f"    msaa / frame = {statistics.median(t['msaa']) / statistics.median(t['frame']):.2f} (medians)", flush=True)
            del setup
            torch.cuda.empty_cache()


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
