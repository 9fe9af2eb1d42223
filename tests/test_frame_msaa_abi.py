"""CPU tests of the argument checks of nb_frame_msaa / nb_launch_frame_msaa / nb_frame_msaa_scratch_bytes:
every rejected case returns NB_ERR_INVALID before anything touches a device."""
import numpy as np
import pytest

F = np.float32


def test_scratch_bytes(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    top = _lib.NB_FRAME_MSAA_MAX_DIM
    assert top == 2048
    assert lib.nb_frame_msaa_scratch_bytes(1, 1) == 64
    assert lib.nb_frame_msaa_scratch_bytes(1920, 1080) == 1920 * 1080 * 64 == 8 * lib.nb_frame_scratch_bytes(1920, 1080)
    assert lib.nb_frame_msaa_scratch_bytes(top, top) == 256 << 20
    assert lib.nb_frame_msaa_scratch_bytes(top, 1) == top * 64 and lib.nb_frame_msaa_scratch_bytes(3, top) == 3 * top * 64
    for w, h in ((0, 4), (4, 0), (top + 1, 4), (4, top + 1), (0, 0), (4096, 4096)):
        assert lib.nb_frame_msaa_scratch_bytes(w, h) == 0


def test_entry_points_validate_before_touching_the_device(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    buf = np.zeros(64, F)
    p = buf.ctypes.data
    assert lib.nb_frame_msaa(None, p, 4, 4, 0, None, None, None, p) == _lib.NB_ERR_INVALID
    assert "ctx is null" in _lib.last_error()
    fn = lib.nb_launch_frame_msaa
    big = _lib.NB_FRAME_MSAA_MAX_DIM + 1
    # 16-byte aligned, never dereferenced: the checks come first.  At 8 x 2: ids8 / depth8 512 bytes, rgba 256, bgra8 64, scratch 1024
    cam, inst, skin, scr, a, b, c, d = 0x100000, 0x200000, 0x300000, 0x380000, 0x400000, 0x500000, 0x600000, 0x700000

    def rc(n=4, cam=cam, inst=inst, width=8, height=2, flags=0, skin=skin, tw=4, th=4, scratch=scr, ids8=a, depth8=b, rgba=c, bgra8=d):
        return fn(n, cam, inst, width, height, flags, skin, tw, th, scratch, ids8, depth8, rgba, bgra8, None)

    bigskin = _lib.NB_EYES_MAX_SKIN + 1
    cases = {
        "width 0": dict(width=0), "height 0": dict(height=0), "width above the maximum": dict(width=big),
        "height above the maximum": dict(height=big), "nb_frame's maximum": dict(width=4096), "a flag": dict(flags=1),
        "flag bit 31": dict(flags=1 << 31), "no output": dict(ids8=None, depth8=None, rgba=None, bgra8=None),
        "ids8 = depth8": dict(depth8=a), "ids8 = rgba": dict(rgba=a), "ids8 = bgra8": dict(bgra8=a), "depth8 = rgba": dict(rgba=b),
        "depth8 = bgra8": dict(bgra8=b), "rgba = bgra8": dict(bgra8=c),
        "rgba over depth8": dict(depth8=c + 256 - 4), "bgra8 inside rgba": dict(bgra8=c + 64), "ids8 overlaps depth8": dict(depth8=a + 508),
        "depth8 inside ids8's eight words a pixel": dict(depth8=a + 64), "bgra8 in ids8's last word": dict(bgra8=a + 508),
        "ids8 over cam": dict(ids8=cam + 16), "depth8 over inst": dict(depth8=inst + 200), "rgba over inst end": dict(rgba=inst + 4 * 64 - 16),
        "bgra8 over skin": dict(bgra8=skin + 4 * 4 * 16 - 4), "rgba over skin": dict(rgba=skin + 16),
        "scratch over ids8": dict(scratch=a), "scratch over depth8 end": dict(scratch=b + 512 - 8), "scratch over rgba": dict(scratch=c + 16),
        "scratch over bgra8": dict(scratch=d - 8), "ids8 inside scratch": dict(ids8=scr + 1024 - 4),
        "ids8 behind nb_frame's share of the scratch": dict(ids8=scr + 128),
        "null cam": dict(cam=None), "null inst": dict(inst=None), "null scratch": dict(scratch=None),
        "misaligned cam": dict(cam=cam + 4), "misaligned inst": dict(inst=inst + 8), "misaligned skin": dict(skin=skin + 4),
        "misaligned rgba": dict(rgba=c + 8), "misaligned scratch": dict(scratch=scr + 4), "misaligned bgra8": dict(bgra8=d + 2),
        "misaligned ids8": dict(ids8=a + 1), "misaligned depth8": dict(depth8=b + 3),
        "tw 0": dict(tw=0), "th 0": dict(th=0), "tw above the maximum": dict(tw=bigskin), "th above the maximum": dict(th=bigskin),
    }
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
    assert "alias" in (rc(bgra8=a) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_FRAME_MSAA_MAX_DIM" in (rc(width=0) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_EYES_MAX_SKIN" in (rc(tw=bigskin) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "flags" in (rc(flags=1) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "all NULL" in (rc(ids8=None, depth8=None, rgba=None, bgra8=None) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert lib.nb_abi_version() == 2   # the change only adds symbols
    if lib.nb_device_count() == 0:
        # right up against each other is not an overlap; each output alone is enough; no skin: white; no bodies: no matrices
        top = _lib.NB_FRAME_MSAA_MAX_DIM
        for kw in (dict(), dict(depth8=a + 512), dict(bgra8=c + 256), dict(scratch=a + 512), dict(ids8=scr + 1024),
                   dict(depth8=None, rgba=None, bgra8=None), dict(ids8=None, rgba=None, bgra8=None), dict(ids8=None, depth8=None, bgra8=None),
                   dict(ids8=None, depth8=None, rgba=None), dict(width=top, height=1), dict(width=1, height=top),
                   dict(width=1, height=1), dict(skin=None, tw=0, th=0), dict(tw=_lib.NB_EYES_MAX_SKIN, th=1), dict(n=0, inst=None)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw
        with pytest.raises(nb.NbError):
            nb.Scene.new(4)
