"""CPU tests of the eye rows through 8 samples per column (nb_eyes_msaa / nb_launch_eyes_msaa):
the numpy restatement of the rule (tests/eyes_msaa_restatement.py) on the hand-checked lattice and against the one-sample rule, what
the GPU tests' inputs cover, and the new entry points' argument checks, which run before any device work.

A non-positive `den` in step 7 (an extrapolated t beyond the point where 1 / w crosses zero) is defined by the rule -- the clamps
of s make every outcome a number -- but is not reached by any input here or in tests/test_gpu_eyes_msaa.py, and none is
constructed."""
import os
import re

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_msaa_restatement as M
import eyes_restatement as R
from conftest import ROOT

F = np.float32
UP = np.array([0, 0, 1], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def init100(oracle):
    """N = 100, seed 1100, every eye, its own body not drawn: the restatement's outputs and statistics, the one-sample rule's rows,
    computed once and left unchanged"""
    pos, vel = oracle.init_state(100, 1100)
    cams = oracle.cameras(pos, vel, UP, R.eye_constant(oracle))
    inst = oracle.instances(pos, vel)
    stats = {}
    out = M.msaa(cams, inst, 0, 1024, False, stats=stats)
    return cams, inst, out, stats, K.colour(cams, inst, 0, 1024, False)


# -- the rule, restated ------------------------------------------------------------------------------------------------------------------
def test_exact_lattice_by_hand(oracle):
    """Body 0 spans xs in [511.5, 512.5) on every one of its edges (depth 0.5, w = 1): of column 511 it covers the samples with
    o_k >= 0.5 -- k = 0, 2, 6, 7 (9, 13, 11, 15 sixteenths) --, all of column 512, and of column 513 those with o_k < 0.5 --
    k = 1, 3, 4, 5.  Bodies 2 and 3 likewise on 514 .. 516 and 518 .. 520 (body 1 ties with body 0 and loses by index).
    One fragment per column, shaded at the centre: t = 0 on the first column (colour 0.5), t = 0.5 on the second (0.75), and t = 1
    on the third, whose centre 513.5 lies outside the span -- extrapolated: edge 0 has u = 0, v = s = 1, colour 1 - (0.25 + 0.25) =
    0.5.  A half column resolves four fragments of 0.5 and four clear samples: ((0.5 + 0.1) + ...) tree-summed, times 0.125 --
    0.3, 0.35, 0.4 in binary32 as the tree rounds them; a full column resolves eight equal values to that value exactly."""
    cams = np.repeat(R.lattice_camera()[None], 4, 0)
    stats = {}
    ids8, depth8, rgba, bgra8 = M.msaa(cams, oracle.instances(R.LATTICE_POS, R.LATTICE_VEL), 0, 1024, see_self=True, stats=stats)
    hi, lo = [0, 2, 6, 7], [1, 3, 4, 5]
    want_ids = np.full((1024, 8), R.NONE, np.uint32)
    want_rgba = np.tile(K.CLEAR, (1024, 1))
    want_bgra = np.full(1024, 0xFF597C95, np.uint32)
    half = np.array([0x3E99999A, 0x3EB33333, 0x3ECCCCCD, 0x3F800000], np.uint32).view(F)
    for c0, body in ((511, 0), (514, 2), (518, 3)):
        want_ids[c0, hi] = body
        want_ids[c0 + 1, :] = body
        want_ids[c0 + 2, lo] = body
        want_rgba[[c0, c0 + 2]] = half
        want_rgba[c0 + 1] = F([0.75, 0.75, 0.75, 1])
        want_bgra[[c0, c0 + 2]] = 0xFF95A0AA
        want_bgra[c0 + 1] = 0xFFE1E1E1
    want_depth = np.where(want_ids == R.NONE, F(1), F(0.5)).astype(F)
    for e in range(4):
        assert (ids8[e] == want_ids).all(), np.argwhere(ids8[e] != want_ids)[:4]
        assert (bits(depth8[e]) == bits(want_depth)).all()
        assert (bits(rgba[e]) == bits(want_rgba)).all(), np.argwhere(bits(rgba[e]) != bits(want_rgba))[:4]
        assert (bgra8[e] == want_bgra).all()
    # the half value is what binary32 makes of it: four times (0.5 + clear) in the tree, an eighth of it
    for ch in range(3):
        a = F(0.5) + K.CLEAR[ch]
        assert half[ch] == ((a + a) + (a + a)) * F(0.125)
    # per eye 3 bodies x 4 samples on the third column are extrapolated (t = 1); every fragment is edge 0's
    assert stats["extrapolated"] == 4 * 3 * 4 and (stats["edge"] == [4 * 3 * 16, 0, 0]).all()
    assert (stats["covered_hist"] == [4 * (1024 - 9), 0, 0, 0, 4 * 6, 0, 0, 0, 4 * 3]).all()
    assert stats["empty_centre"] == 4 * 3 and stats["two_bodies"] == 0


def test_columns_of_one_fragment_equal_the_one_sample_rule(oracle, init100):
    """where the eight samples have one (body, edge) and it is the one-sample winner's -- or all are empty and so is the centre --
    the resolve is eight equal values: rgba and bgra8 are eyes_colour's, bit for bit.  Alpha is 1.0f everywhere."""
    cams, inst, out, stats, one = init100
    ids8, _, rgba, bgra8 = out
    e8 = stats["edge8"]
    ei, ci = np.nonzero(one[0] != R.NONE)
    edge_c, _, _ = M.winning_fragments(cams, R.world_vertices(inst), ei, ci, ci.astype(F) + F(0.5), one[0][ei, ci].astype(np.int64),
                                       one[1][ei, ci].view(np.uint32), 1024, K.WHITE)
    centre_edge = np.full(one[0].shape, -1, np.int8)
    centre_edge[ei, ci] = edge_c
    q = (ids8 == ids8[..., :1]).all(-1) & (e8 == e8[..., :1]).all(-1) & (ids8[..., 0] == one[0]) & (e8[..., 0] == centre_edge)
    print("qualifying columns", int(q.sum()), "of", q.size)
    assert q.sum() >= 0.95 * q.size
    assert (bits(rgba)[q] == bits(one[2])[q]).all() and (bgra8[q] == one[3][q]).all()
    assert (bits(rgba[..., 3]) == 0x3F800000).all()
    assert (bgra8[~q] != one[3][~q]).any()              # and elsewhere the rows do differ: the resolve is not a no-op


def test_columns_of_one_fragment_at_257(oracle):
    pos, vel = oracle.init_state(257, 1257)
    cams = oracle.cameras(pos[:64], vel[:64], UP, R.eye_constant(oracle))
    inst = oracle.instances(pos, vel)
    stats = {}
    ids8, _, rgba, bgra8 = M.msaa(cams, inst, 0, 1024, False, stats=stats)
    one = K.colour(cams, inst, 0, 1024, False)
    e8 = stats["edge8"]
    ei, ci = np.nonzero(one[0] != R.NONE)
    edge_c, _, _ = M.winning_fragments(cams, R.world_vertices(inst), ei, ci, ci.astype(F) + F(0.5), one[0][ei, ci].astype(np.int64),
                                       one[1][ei, ci].view(np.uint32), 1024, K.WHITE)
    centre_edge = np.full(one[0].shape, -1, np.int8)
    centre_edge[ei, ci] = edge_c
    q = (ids8 == ids8[..., :1]).all(-1) & (e8 == e8[..., :1]).all(-1) & (ids8[..., 0] == one[0]) & (e8[..., 0] == centre_edge)
    assert q.sum() >= 0.9 * q.size
    assert (bits(rgba)[q] == bits(one[2])[q]).all() and (bgra8[q] == one[3][q]).all()


def test_coverage_of_the_gpu_cases(oracle, init100):
    """what the GPU tests rest on (tests/test_gpu_eyes_msaa.py uses these seeds), on the restatement; N = 100 seed 1100 measured
    208-239 columns per partial count, 488 columns fully covered by two bodies, 758 with an empty centre, 3 514 extrapolated
    samples and at least 26 410 samples per edge"""
    stats = init100[3]
    print({k: v for k, v in stats.items() if k != "edge8"})
    assert (stats["covered_hist"][1:8] >= 100).all(), stats["covered_hist"]
    assert stats["two_bodies_full"] >= 300
    assert stats["empty_centre"] >= 500
    assert stats["extrapolated"] >= 2000
    assert (stats["edge"] >= 10000).all(), stats["edge"]


@pytest.mark.parametrize("width,least", [(3, 500), (2048, 3000)])
def test_coverage_of_the_width_cases(oracle, width, least):
    """N = 257 seed 31: partly covered columns at the narrowest and the widest rows (545 and 3 751 measured)"""
    pos, vel = oracle.init_state(257, 31)
    cams = oracle.cameras(pos, vel, UP, R.eye_constant(oracle, width))
    stats = {}
    M.msaa(cams, oracle.instances(pos, vel), 0, width, False, stats=stats)
    assert stats["covered_hist"][1:8].sum() >= least, stats["covered_hist"]


# -- the entry points --------------------------------------------------------------------------------------------------------------------
def test_sample_offsets(nb):
    from nenbody_amd import _lib

    o = nb.eye_sample_offsets()
    assert o.dtype == np.float32 and (bits(o) == bits(M.OFFSETS)).all()
    assert (o * 16 == [9, 7, 13, 5, 3, 1, 11, 15]).all()
    assert _lib.load().nb_eyes_sample_offsets(None) == _lib.NB_ERR_INVALID
    assert _lib.NB_EYES_SAMPLES == 8 and _lib.NB_EYES_MSAA_MAX_WIDTH == 2048
    header = open(os.path.join(ROOT, "include", "nenbody.h")).read()
    assert "#define NB_EYES_SAMPLES 8u" in header and "#define NB_EYES_MSAA_MAX_WIDTH 2048u" in header


def test_msaa_entry_points_validate_before_touching_the_device(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    up, cp = np.array([0, 0, 1], F), np.zeros(16, F)
    buf = np.zeros(64, F)
    assert lib.nb_eyes_msaa(None, 0, 1, up.ctypes.data, cp.ctypes.data, 8, 0, None, None, buf.ctypes.data, None) == _lib.NB_ERR_INVALID
    assert "ctx is null" in _lib.last_error()
    fn = lib.nb_launch_eyes_msaa
    # 16-byte aligned, never dereferenced: the checks come first
    cams, inst, skin, a, b, c, d = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000

    def rc(n=4, first=0, count=2, cams=cams, inst=inst, width=8, flags=0, skin=skin, tw=4, th=4, ids8=a, depth8=b, rgba=c, bgra8=d):
        return fn(n, first, count, cams, inst, width, flags, skin, tw, th, ids8, depth8, rgba, bgra8, None)

    big = _lib.NB_EYES_MAX_SKIN + 1
    words8 = 2 * 8 * 8 * 4      # bytes of ids8 / depth8 at count 2, width 8
    cases = {
        "width 0": dict(width=0), "width above the maximum": dict(width=_lib.NB_EYES_MSAA_MAX_WIDTH + 1),
        "the one-sample maximum": dict(width=_lib.NB_EYES_MAX_WIDTH),
        "range past n": dict(first=3), "count past n": dict(count=5), "unknown flag": dict(flags=2), "flag bit 31": dict(flags=1 << 31),
        "no output at all": dict(ids8=None, depth8=None, rgba=None, bgra8=None),
        "ids8 = depth8": dict(depth8=a), "ids8 = bgra8": dict(bgra8=a), "depth8 = bgra8": dict(bgra8=b), "rgba = ids8": dict(ids8=c),
        "depth8 inside ids8's eight words a column": dict(depth8=a + words8 - 4), "bgra8 inside depth8": dict(bgra8=b + words8 - 4),
        "rgba over depth8": dict(depth8=c + 2 * 8 * 16 - 4), "bgra8 inside rgba": dict(bgra8=c + 64),
        "ids8 over cams": dict(ids8=cams + 16), "depth8 over inst": dict(depth8=inst + 200), "rgba over inst end": dict(rgba=inst + 4 * 64 - 16),
        "bgra8 over skin": dict(bgra8=skin + 4 * 4 * 16 - 4), "rgba over skin": dict(rgba=skin + 16),
        "null cams": dict(cams=None), "null inst": dict(inst=None), "misaligned cams": dict(cams=cams + 4),
        "misaligned inst": dict(inst=inst + 8), "misaligned skin": dict(skin=skin + 4), "misaligned rgba": dict(rgba=c + 8),
        "misaligned bgra8": dict(bgra8=d + 2), "misaligned ids8": dict(ids8=a + 1), "misaligned depth8": dict(depth8=b + 2),
        "tw 0": dict(tw=0), "th 0": dict(th=0), "tw above the maximum": dict(tw=big), "th above the maximum": dict(th=big),
    }
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
    assert "alias" in (rc(bgra8=a) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_EYES_MSAA_MAX_WIDTH" in (rc(width=2049) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_EYES_MAX_SKIN" in (rc(tw=big) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "all NULL" in (rc(ids8=None, depth8=None, rgba=None, bgra8=None) == _lib.NB_ERR_INVALID and _lib.last_error())
    # count = 0 is a no-op (no device needed)
    assert rc(count=0) == _lib.NB_OK and rc(count=0, first=4) == _lib.NB_OK
    # the ABI version stays: the change only adds symbols
    assert lib.nb_abi_version() == 2
    if lib.nb_device_count() == 0:
        # right up against each other is not an overlap; any output alone is enough; no skin: white
        for kw in (dict(), dict(depth8=a + words8), dict(bgra8=c + 2 * 8 * 16), dict(ids8=None, depth8=None, bgra8=None),
                   dict(ids8=None, depth8=None, rgba=None), dict(depth8=None, rgba=None, bgra8=None), dict(ids8=None, rgba=None, bgra8=None),
                   dict(flags=_lib.NB_EYES_SEE_SELF), dict(width=_lib.NB_EYES_MSAA_MAX_WIDTH), dict(width=1), dict(first=2),
                   dict(skin=None, tw=0, th=0), dict(tw=_lib.NB_EYES_MAX_SKIN, th=1)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw


def test_the_rust_shim_declares_the_msaa_entry_points():
    """integration/rust/scene.rs is text (no Rust toolchain here): the new symbols of the header are declared in its extern block
    with the header's argument counts, and Scene has eyes_msaa"""
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody.h")).read(), flags=re.S)
    for name in ("nb_eyes_sample_offsets", "nb_eyes_msaa"):
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)\s*->\s*c_int;" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    assert "pub fn eyes_msaa(" in text and "pub fn eye_sample_offsets(" in text


def test_the_header_points_at_the_msaa_entry():
    """the three sentences that said MSAA is not reproduced now name nb_eyes_msaa for the eyes; for the frame they stand"""
    header = open(os.path.join(ROOT, "include", "nenbody.h")).read()
    assert header.count("nb_eyes_msaa") >= 5
    assert "no MSAA resolve" in header           # nb_frame's
    for name in ("nb_eyes_sample_offsets", "nb_eyes_msaa", "nb_launch_eyes_msaa"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
