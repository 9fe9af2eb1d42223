"""GPU tests of the five launch forms of the eye rows and the scene camera's frame (nb_launch_eyes, nb_launch_eyes_colour,
nb_launch_eyes_msaa, nb_launch_frame, nb_launch_frame_msaa) on arbitrary caller matrices: the corpus of tests/hostile_matrices.py --
sheared, projective, overflowing, subnormal, infinite, NaN, degenerate, half-integer and duplicated model matrices under
orthographic, depth-pushed, perspective, random and zero-row cameras -- on torch device tensors and a stream of its own, every
output prefilled with a marker, every word against the numpy restatements of the rule.  What the corpus covers is asserted on the
CPU (tests/test_hostile_matrices_cpu.py), where the host-compiled copies of the same device functions agree with the restatements
on every word of it; what is compared here for the first time on such input is the device code: its compilation (a flushed
subnormal, a contracted multiply-add, a non-IEEE reciprocal would show), the hand-off to the wave, the LDS and global atomics, the
culls.

rgba is compared by its bits like the other outputs: the texture parameter is clamped to [0, 1] before anything is looked up (a
NaN becomes 0) and the corpus' skins are finite, so no NaN reaches a colour and there is no payload to disagree about.
"""
import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_restatement as R
import frame_restatement as FR
import hostile_matrices as HM

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = {"eyes": ("ids", "depth"), "eyes_colour": ("ids", "depth", "rgba", "bgra8"), "eyes_msaa": ("ids8", "depth8", "rgba", "bgra8"),
         "frame": ("ids", "depth", "rgba", "bgra8"), "frame_msaa": ("ids8", "depth8", "rgba", "bgra8")}


class Device:
    """the launch forms on caller-owned torch tensors and one stream that is not the default one"""

    def __init__(self, nb):
        import torch

        from nenbody_amd import _lib

        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.Stream(self.dev)
        torch.cuda.synchronize()

    def up(self, a, shape):
        return self.torch.from_numpy(np.ascontiguousarray(a, F).reshape(shape)).to(self.dev)

    def outs(self, view, cells):
        """the view's outputs, prefilled with the marker so that an unwritten word shows"""
        t, k = self.torch, (8,) if view.endswith("msaa") else ()
        o = [t.full(cells + k, HM.MARK, dtype=t.int32, device=self.dev), t.full(cells + k, float(HM.MARK), dtype=t.float32, device=self.dev)]
        if view != "eyes":
            o += [t.full(cells + (4,), float(HM.MARK), dtype=t.float32, device=self.dev), t.full(cells, HM.MARK, dtype=t.int32, device=self.dev)]
        return o

    def run(self, view, c, cams=None, width=None, extent=None, first=None, see_self=None):
        """one launch of `view` on case c (cameras, width / extent, first and see_self of the case unless given): the outputs as
        numpy arrays"""
        t, lib = self.torch, self.lib
        n = len(c["inst"])
        inst = self.up(c["inst"], (n, 16))
        skin = c["skin"]
        st = self.up(skin, skin.shape) if skin is not None else None
        sp, tw, th = (st.data_ptr(), skin.shape[1], skin.shape[0]) if skin is not None else (None, 0, 0)
        if view.startswith("eyes"):
            cams = c["cams"] if cams is None else cams
            width = c["width"] if width is None else width
            first = c["first"] if first is None else first
            flags = self._lib.NB_EYES_SEE_SELF if (c["see_self"] if see_self is None else see_self) else 0
            ct = self.up(cams, (len(cams), 16))
            o = self.outs(view, (len(cams), width))
            p = [x.data_ptr() for x in o]
            with t.cuda.stream(self.stream):
                if view == "eyes":
                    rc = lib.nb_launch_eyes(n, first, len(cams), ct.data_ptr(), inst.data_ptr(), width, flags, *p, self.stream.cuda_stream)
                else:
                    fn = lib.nb_launch_eyes_colour if view == "eyes_colour" else lib.nb_launch_eyes_msaa
                    rc = fn(n, first, len(cams), ct.data_ptr(), inst.data_ptr(), width, flags, sp, tw, th, *p, self.stream.cuda_stream)
        else:
            W, H = c["extent"] if extent is None else extent
            ct = self.up(c["cam"] if cams is None else cams, (16,))
            msaa = view == "frame_msaa"
            nbytes = lib.nb_frame_msaa_scratch_bytes(W, H) if msaa else lib.nb_frame_scratch_bytes(W, H)
            assert nbytes == W * H * (64 if msaa else 8)
            scratch = t.full((nbytes // 8,), HM.MARK, dtype=t.int64, device=self.dev)
            o = self.outs(view, (H, W))
            fn = lib.nb_launch_frame_msaa if msaa else lib.nb_launch_frame
            with t.cuda.stream(self.stream):
                rc = fn(n, ct.data_ptr(), inst.data_ptr(), W, H, 0, sp, tw, th, scratch.data_ptr(), *[x.data_ptr() for x in o], self.stream.cuda_stream)
        self._lib.check(rc)
        self.stream.synchronize()
        return tuple(x.cpu().numpy() for x in o)


@pytest.fixture(scope="module")
def device(nb):
    return Device(nb)


def assert_same(view, got, want, what):
    """every output as uint32 words; the message names how many words were compared and how many of them hold something"""
    assert len(got) == len(want) == len(NAMES[view])
    for name, g, w in zip(NAMES[view], got, want):
        assert g.shape == w.shape, f"{what}: {name} {g.shape} != {w.shape}"
        bad = HM.words(g) != HM.words(w)
        assert not bad.any(), (f"{view} {what}: {name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}: "
                               f"0x{HM.words(g)[bad][0]:08x} != 0x{HM.words(w)[bad][0]:08x}")
    print(f"{view} {what}: {sum(g.size for g in got)} words compared, {int((want[0] != R.NONE).sum())} of {want[0].size} ids non-empty")


# -- 1. every word of the corpus, view by view ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HM.EYE_NAMES_ONE)
def test_eyes(device, oracle, name):
    c = HM.case(oracle, name)
    assert_same("eyes", device.run("eyes", c), HM.expected("eyes_colour", c)[:2], name)


@pytest.mark.parametrize("name", HM.EYE_NAMES_ONE)
def test_eyes_colour(device, oracle, name):
    c = HM.case(oracle, name)
    assert_same("eyes_colour", device.run("eyes_colour", c), HM.expected("eyes_colour", c), name)


@pytest.mark.parametrize("name", HM.EYE_NAMES)
def test_eyes_msaa(device, oracle, name):
    c = HM.case(oracle, name)
    assert_same("eyes_msaa", device.run("eyes_msaa", c), HM.expected("eyes_msaa", c), name)


@pytest.mark.parametrize("name", HM.FRAME_NAMES)
def test_frame(device, oracle, name):
    c = HM.case(oracle, name)
    assert_same("frame", device.run("frame", c), HM.expected("frame", c), name)


@pytest.mark.parametrize("name", HM.FRAME_NAMES)
def test_frame_msaa(device, oracle, name):
    c = HM.case(oracle, name)
    assert_same("frame_msaa", device.run("frame_msaa", c), HM.expected("frame_msaa", c), name)


# -- 2. run to run: the order the atomics arrive in must not matter, least of all on the ties ----------------------------------------------
@pytest.mark.parametrize("view,name,other", [("eyes", "W65-self1", "W257-self0"), ("eyes_colour", "W65-self1", "W257-self0"),
                                             ("eyes_msaa", "W65-self1", "W2048-self1"), ("frame", "64x32-pushed", "3x128-zero_z"),
                                             ("frame_msaa", "64x32-pushed", "128x3-persp")])
def test_the_same_launch_twice_and_after_another_extent(device, oracle, view, name, other):
    c = HM.case(oracle, name)
    first = device.run(view, c)
    second = device.run(view, c)
    device.run(view, HM.case(oracle, other))
    third = device.run(view, c)
    for again, what in ((second, "the second launch"), (third, "after another extent")):
        for nm, a, b in zip(NAMES[view], first, again):
            assert (HM.words(a) == HM.words(b)).all(), f"{view} {name}: {nm} changed in {what}"
    dups = np.nonzero(c["cls"] == HM.CLASSES.index("duplicate"))[0]
    held = np.isin(first[0].view(np.uint32), [HM.duplicate_source(j) for j in dups])
    assert held.sum() >= 10 and not np.isin(first[0].view(np.uint32), dups).any()      # ties, held by the lower index every time


# -- 3. one row of the frame is the eye's colour row, beyond planar rigid data -----------------------------------------------------------------
def test_one_row_equals_eyes_colour_on_the_device(device, oracle):
    """The one-sample frame at H = 1 and the colour eye row on the same hostile matrices and camera.  The rule promises equal rows
    only where every clip y is +-0 (the frame clips and steps in y as well); so the restatements are asked first, and the device
    is held to equal rows on the cameras where they agree -- among them the orthographic camera with its y row zeroed."""
    agreed = covered = 0
    for name in ("W33-self1", "W64-self0", "W257-self0"):
        c = HM.case(oracle, name)
        W = c["width"]
        for e, cam in enumerate(c["cams"]):
            row = K.colour(cam[None], c["inst"], 0, W, True, c["skin"])
            frame = FR.frame(cam, c["inst"], W, 1, skin=c["skin"])
            if not all((HM.words(a) == HM.words(b.reshape(a.shape))).all() for a, b in zip(row, frame)):
                continue
            agreed += 1
            covered += int((row[0] != R.NONE).sum())
            got_row = device.run("eyes_colour", c, cams=cam[None], first=0, see_self=True)
            got_frame = device.run("frame", c, cams=cam, extent=(W, 1))
            for nm, a, b, w in zip(NAMES["frame"], got_row, got_frame, row):
                assert (HM.words(a) == HM.words(b.reshape(a.shape))).all(), f"{name} eye {e}: {nm}: the frame's row is not the eye's"
                assert (HM.words(a) == HM.words(w)).all(), f"{name} eye {e}: {nm}: not the restatement's"
    assert agreed >= 3 and covered >= 100, (agreed, covered)
