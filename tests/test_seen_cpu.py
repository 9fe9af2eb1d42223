"""CPU tests of the seen sets and the seen boids step: the numpy restatement (tests/seen_restatement.py)
against the plain boids restatement it must reduce to, on the exact lattice and on a hand-derived two-body case, its power to tell
the seen step from the plain one on the reference's initial state, and the new entry points' argument checks, which run before any
device work."""
import os
import re
import subprocess

import numpy as np
import pytest

import eyes_restatement as R
import np_restatement as NP
import seen_restatement as S
from conftest import ROOT

F = np.float32
UP = np.array([0, 0, 1], F)
EXE = os.path.join(ROOT, "build", "seen_check")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rows_of(oracle, pos, vel, width=1024):
    """the eye rows of every body of (pos, vel) by the numpy eye rule, cameras and matrices by the oracle"""
    cams = oracle.cameras(pos, vel, UP, R.eye_constant(oracle, width))
    return R.eyes(cams, oracle.instances(pos, vel), 0, width)


# -- the rule, restated ------------------------------------------------------------------------------------------------------------------
def test_an_all_true_mask_is_the_plain_boids_step(oracle):
    pos, vel = oracle.init_state(100, 1100)
    want = NP.boids_step(pos, vel)
    got = S.boids_seen_step(pos, vel, np.ones((100, 100), bool))
    assert (bits(got[0]) == bits(want[0])).all() and (bits(got[1]) == bits(want[1])).all()


def test_an_all_false_mask_stops_every_body(oracle):
    pos, vel = oracle.init_state(100, 1100)
    p, v = S.boids_seen_step(pos, vel, np.zeros((100, 100), bool))
    assert (bits(v) == 0).all()                      # +0, every component
    assert (bits(p) == bits(pos)).all()


def test_the_lattice_row(oracle):
    ids, depth = R.lattice_expectation()
    count, sids, sdepth, scols = S.seen(ids, depth)
    assert count == 3
    assert (sids[:3] == [0, 2, 3]).all() and (sids[3:] == S.NONE).all()
    assert (scols[:3] == [2, 2, 2]).all() and (scols[3:] == 0).all() and scols.sum() == (ids != R.NONE).sum()
    assert (sdepth[:3] == F(0.5)).all() and (bits(sdepth[3:]) == 0x3F800000).all()


def test_ids_compare_as_unsigned_numbers_and_depths_by_their_bits():
    ids = np.array([0x80000000, 5, S.NONE, 0xFFFFFFFE, 5, 0x80000000, 0], np.uint32)
    depth = np.array([0.5, 0.25, 1.0, 0.0, 1e-40, 0.75, 0x3F7FFFFF], np.float32)
    depth[6] = np.uint32(0x3F7FFFFF).view(F)
    count, sids, sdepth, scols = S.seen(ids, depth)
    assert count == 4 and (sids[:4] == [0, 5, 0x80000000, 0xFFFFFFFE]).all()
    assert (scols[:4] == [1, 2, 2, 1]).all()
    assert (bits(sdepth[:4]) == [0x3F7FFFFF, int(bits(F(1e-40))[0]), 0x3F000000, 0]).all()


def test_hand_case_two_bodies_in_binary32(oracle):
    """Bodies at (0,0,0) and (10,0,0), both heading +x, W = 1024, the reference's eye constant.  Eye 0 sees body 1's rear edge over
    columns 440 .. 583; eye 1 looks away from body 0 and sees nobody.  Body 0 then folds over body 1 alone: d2 = 100 < 1000, so the
    centre is (10, 0, 0) / 1; sqrt(100) = 10 is not below 5, so nothing repels; the velocities are equal, so the match is (1, 0, 0) / 1:
    v.x = (10 * 0.02f + 0 * 0.05f) + 1 * 0.5f, |v| < 1, x = v.x * 0.04f + 0.  Body 1 folds over nothing: velocity 0, position kept."""
    pos = np.array([[0, 0, 0], [10, 0, 0]], F)
    vel = np.array([[1, 0, 0], [1, 0, 0]], F)
    ids, depth = rows_of(oracle, pos, vel)
    assert (np.nonzero(ids[0] != R.NONE)[0] == np.arange(440, 584)).all() and (ids[0, 440:584] == 1).all()
    assert (ids[1] == R.NONE).all()
    count, sids, _, scols = S.seen_rows(ids, depth)
    assert (count == [1, 0]).all() and sids[0, 0] == 1 and scols[0, 0] == 144
    p, v = S.boids_seen_step(pos, vel, S.mask_of_rows(ids, 2))
    vx = (F(10) * F(0.02) + F(0) * F(0.05)) + F(1) * F(0.5)
    assert bits(vx) == 0x3F333333
    assert (bits(v[0]) == [0x3F333333, 0, 0]).all()
    assert (bits(p[0]) == [int(bits(vx * F(0.04) + F(0))[0]), 0, 0]).all()
    assert (bits(v[1]) == 0).all() and (bits(p[1]) == bits(F([10, 0, 0]))).all()


def test_the_reference_state_tells_the_seen_step_from_the_plain_one(oracle):
    """what the GPU tests rest on: at N = 100, seed 1100, some body is blind, most see someone, and the two steps differ"""
    pos, vel = oracle.init_state(100, 1100)
    ids, _ = rows_of(oracle, pos, vel)
    mask = S.mask_of_rows(ids, 100)
    assert not mask[np.arange(100), np.arange(100)].any()            # an eye does not see its own body
    sees = mask.sum(1)
    assert (sees == 0).sum() >= 1 and (sees > 0).sum() > 50, sees
    count = S.seen_rows(ids)[0]
    assert (count == sees).all()
    got = S.boids_seen_step(pos, vel, mask)
    plain = NP.boids_step(pos, vel)
    assert (bits(got[1]) != bits(plain[1])).any() and (bits(got[0]) != bits(plain[0])).any()
    blind = sees == 0
    assert (bits(got[1][blind]) == 0).all() and (bits(got[0][blind]) == bits(pos[blind])).all()


# -- the entry points --------------------------------------------------------------------------------------------------------------------
def test_launch_seen_validates_before_touching_the_device(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    fn = lib.nb_launch_seen
    # 4-byte aligned, never dereferenced: the checks come first.  count = 2, width = 8: rows and lists of 64 bytes, counts of 8
    ids, dep, cnt, a, b, c = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000

    def rc(count=2, width=8, ids=ids, depth=dep, seen_count=cnt, seen_ids=a, seen_depth=b, seen_cols=c):
        return fn(count, width, ids, depth, seen_count, seen_ids, seen_depth, seen_cols, None)

    big = _lib.NB_EYES_MAX_WIDTH + 1
    cases = {
        "null ids_rows": dict(ids=None), "null seen_count": dict(seen_count=None), "null seen_ids": dict(seen_ids=None),
        "all outputs null": dict(seen_count=None, seen_ids=None, seen_depth=None, seen_cols=None),
        "width 0": dict(width=0), "width above the maximum": dict(width=big),
        "seen_depth without depth_rows": dict(depth=None),
        "misaligned ids_rows": dict(ids=ids + 2), "misaligned depth_rows": dict(depth=dep + 1), "misaligned seen_count": dict(seen_count=cnt + 2),
        "misaligned seen_ids": dict(seen_ids=a + 1), "misaligned seen_depth": dict(seen_depth=b + 3), "misaligned seen_cols": dict(seen_cols=c + 2),
        "count = ids": dict(seen_ids=cnt), "count = depth": dict(seen_depth=cnt), "count = cols": dict(seen_cols=cnt),
        "ids = depth": dict(seen_depth=a), "ids = cols": dict(seen_cols=a), "depth = cols": dict(seen_cols=b),
        "count inside ids": dict(seen_count=a + 60), "ids over depth": dict(seen_depth=a + 60), "cols over ids": dict(seen_cols=a - 60),
        "depth over cols": dict(seen_depth=c + 32), "count over cols end": dict(seen_count=c + 60), "depth over count": dict(seen_depth=cnt - 60),
        "count over ids_rows": dict(seen_count=ids + 60), "ids over ids_rows": dict(seen_ids=ids + 4), "depth over ids_rows": dict(seen_depth=ids - 60),
        "cols over ids_rows": dict(seen_cols=ids), "count over depth_rows": dict(seen_count=dep), "ids over depth_rows": dict(seen_ids=dep + 60),
        "depth over depth_rows": dict(seen_depth=dep), "cols over depth_rows": dict(seen_cols=dep - 4),
    }
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
    assert "alias" in (rc(seen_cols=a) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "NB_EYES_MAX_WIDTH" in (rc(width=0) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "depth_rows" in (rc(depth=None) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert "4-byte" in (rc(seen_cols=c + 2) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert rc(count=0) == _lib.NB_OK                       # a no-op, with or without a device
    assert lib.nb_abi_version() == 2                       # the change only adds symbols
    if lib.nb_device_count() == 0:
        # right up against each other is not an overlap; the optional arguments may go
        for kw in (dict(), dict(seen_depth=a + 64), dict(seen_count=a - 8), dict(seen_ids=ids + 64), dict(depth=None, seen_depth=None),
                   dict(seen_cols=None), dict(seen_depth=None), dict(depth=None, seen_depth=None, seen_cols=None),
                   dict(width=_lib.NB_EYES_MAX_WIDTH, count=1), dict(width=1, count=1)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw


def test_launch_boids_seen_step_validates_before_touching_the_device(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    fn = lib.nb_launch_boids_seen_step
    pin, vin, pout, vout, cnt, lst = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000

    def rc(n=16, first=4, count=8, pos_in=pin, vel_in=vin, seen_count=cnt, seen_ids=lst, stride=32, pos_out=pout, vel_out=vout):
        return fn(None, n, first, count, pos_in, vel_in, seen_count, seen_ids, stride, pos_out, vel_out, None)

    cases = {
        "null pos_in": dict(pos_in=None), "null vel_in": dict(vel_in=None), "null pos_out": dict(pos_out=None), "null vel_out": dict(vel_out=None),
        "null seen_count": dict(seen_count=None), "null seen_ids": dict(seen_ids=None),
        "pos_out = pos_in": dict(pos_out=pin), "vel_out = vel_in": dict(vel_out=vin),
        "stride 0": dict(stride=0), "count 0": dict(count=0), "range past the set": dict(first=10, count=8),
        "misaligned seen_count": dict(seen_count=cnt + 2), "misaligned seen_ids": dict(seen_ids=lst + 1),
        "pos_out over seen_count": dict(seen_count=pout + 4 * 16), "pos_out over seen_ids": dict(seen_ids=pout + 4 * 16 - 8 * 32 * 4 + 4),
        "vel_out over seen_count": dict(seen_count=vout + 12 * 16 - 4), "vel_out over seen_ids": dict(seen_ids=vout + 8 * 16),
    }
    for what, kw in cases.items():
        assert rc(**kw) == _lib.NB_ERR_INVALID, what
    assert "lists" in (rc(seen_ids=vout + 8 * 16) == _lib.NB_ERR_INVALID and _lib.last_error())
    assert rc(n=1 << 24, first=0, count=8) == _lib.NB_ERR_UNSUPPORTED
    if lib.nb_device_count() == 0:
        # the records the launch does not write may hold the lists: only [first, first + count) is an output
        for kw in (dict(), dict(seen_count=pout), dict(seen_ids=vout + 12 * 16), dict(stride=1), dict(first=0, count=16)):
            assert rc(**kw) == _lib.NB_ERR_NO_DEVICE, kw


def test_the_context_entries_reject_a_null_context(nb):
    from nenbody_amd import _lib

    lib = _lib.load()
    buf = np.zeros(64, F)
    p = buf.ctypes.data
    assert lib.nb_eyes_seen(None, 0, 1, p, p, 8, 0, p, None, None, None) == _lib.NB_ERR_INVALID
    assert "nb_eyes_seen: ctx is null" in _lib.last_error()
    assert lib.nb_step_boids_seen(None, 1, None, p, p, 1024, 0) == _lib.NB_ERR_INVALID
    assert "nb_step_boids_seen: ctx is null" in _lib.last_error()
    if lib.nb_device_count() == 0:
        with pytest.raises(nb.NbError):
            nb.Scene.new(4)


def test_the_python_names_exist(nb):
    for name in ("seen", "step_boids_seen", "step_boids_seen_n"):
        assert callable(getattr(nb.Scene, name))
    from nenbody_amd import _lib

    for name in ("nb_launch_seen", "nb_eyes_seen", "nb_launch_boids_seen_step", "nb_step_boids_seen"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name)


def test_the_rust_shim_declares_the_seen_entry_points():
    """integration/rust/scene.rs is text (no Rust toolchain here): the context's seen symbols are declared in its extern block with
    the header's argument counts, and Scene has seen / step_boids_seen"""
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody.h")).read(), flags=re.S)
    for name in ("nb_eyes_seen", "nb_step_boids_seen"):
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)\s*->\s*c_int;" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for method in ("pub fn seen(", "pub fn step_boids_seen("):
        assert method in text, method


def build_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "nenbody_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "seen_check.cpp"), "-o", EXE, "-L", libdir, "-lnenbody_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)


def test_cpp_seen_host_compiles_and_refuses_to_run_without_a_gpu(nb, tmp_path):
    build_exe()
    from nenbody_amd import _lib

    have_device = _lib.load().nb_device_count() > 0
    r = subprocess.run([EXE, "16", "64", str(tmp_path / "out.bin")], capture_output=True, text=True)
    if have_device:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 10 and "no HIP device" in r.stderr     # NB_ERR_NO_DEVICE surfaced as nenbody::Error
