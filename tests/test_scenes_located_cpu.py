"""CPU tests of the scene batches' gravity from located vision: the premises the GPU tests rest on, checked
on the very rows of tests/scenes_located_cases.py through the numpy restatements of the eye rule, of the located sets and of the located
step; the header, the binding, the library, the C++ host and the Rust shim agree on the four entries; and what the entries refuse
without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import eyes_restatement as R
import located_restatement as L
import np_restatement as NP
import scenes_located_cases as K
from conftest import ROOT

F = np.float32
NAMES = ["nb_scenes_nbody_located_step_launch", "nb_scenes_located_launch", "nb_scenes_step_nbody_located", "nb_scenes_eyes_located"]
EXE = os.path.join(ROOT, "build", "scenes_located_check")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def located_of(oracle, pos, vel, width):
    """(rows of ids, rows of depth, (count, ids, depth, cols, col, rel)) of every body of one scene, by the numpy rules alone; cameras
    and matrices by the oracle"""
    cp = R.eye_constant(oracle, width)
    cams = oracle.cameras(pos, vel, K.UP, cp)
    ids, depth = R.eyes(cams, oracle.instances(pos, vel), 0, width, chunk=64)
    return ids, depth, L.located_of_rows(ids, depth, vel, K.UP, cp)


_checked = {}


def premises(oracle, seed, n, width, scale):
    """(blind bodies, bodies that see somebody, the largest set, members that are nearest at one depth on several columns, the located
    step differs from coasting, from nb_step's result)"""
    key = (seed, n, width, scale)
    if key not in _checked:
        pos, vel = K.batch(oracle, (seed, n, width, scale, 1))
        pos, vel = pos[0], vel[0]
        ids, depth, (count, sids, sdepth, _, col, rel) = located_of(oracle, pos, vel, width)
        assert not (ids == np.arange(n, dtype=np.uint32)[:, None]).any()         # an eye does not see its own body
        dbits = bits(depth)
        ties = 0
        for e in np.nonzero(count)[0]:
            for k in range(int(count[e])):
                hits = int(((ids[e] == sids[e, k]) & (dbits[e] == bits(sdepth[e, k:k + 1])[0])).sum())
                assert hits >= 1 and ids[e, col[e, k]] == sids[e, k]
                ties += hits > 1
        got = L.nbody_located_step(pos, vel, count, rel)
        coast = (vel + pos).astype(F)
        plain = NP.step(pos, vel)
        blind = count == 0
        assert (bits(got[1][blind]) == bits(vel[blind])).all() and (bits(got[0][blind]) == bits(coast[blind])).all()   # G3
        _checked[key] = (int(blind.sum()), int((count > 0).sum()), int(count.max()), int(ties),
                         bool((bits(got[0]) != bits(coast)).any() or (bits(got[1]) != bits(vel)).any()),
                         bool((bits(got[0]) != bits(plain[0])).any() or (bits(got[1]) != bits(plain[1])).any()))
    return _checked[key]


ROWS = sorted({row for row in K.ROWS if K.holds_premises(row)})


def test_the_rows_cover_what_the_issue_lists():
    assert sorted(K.SIZES) == [1, 2, 3, 63, 64, 65, 100, 128, 129, 257, 2048] and K.SIZES[2048][4] == 2
    assert sorted(K.WIDTHS) == [1, 63, 64, 65, 1000, 4096] and all(r[1] == 65 for r in K.WIDTHS.values())
    assert sorted(K.LISTS) == [(n, w) for n in (64, 100, 129) for w in (64, 1024)]
    assert K.FLOOR[1:] == (100, 1024, 1.0, 64)
    assert (K.PREMISE_MIN_N, K.PREMISE_MIN_WIDTH) == (63, 63)


@pytest.mark.parametrize("n", sorted({r[1] for r in ROWS}))
def test_every_scene_holds_the_premises(oracle, n):
    """every scene of a row: a blind body, most bodies see somebody, and the located step is neither coasting nor nb_step's result;
    every row: some eye has several members, and some member is nearest at one depth on several columns (L1's tie rule decides)"""
    rows = [r for r in ROWS if r[1] == n]
    assert rows
    for seed, _, width, scale, scenes in rows:
        most = ties = 0
        for s in range(scenes):
            blind, seeing, largest, tied, not_coast, not_plain = premises(oracle, seed + s, n, width, scale)
            assert blind >= 1 and seeing > n // 2 and not_coast and not_plain, (seed + s, n, width, scale, blind, seeing, not_coast, not_plain)
            most, ties = max(most, largest), ties + tied
        assert most > 1 and ties >= 1, (seed, n, width, scale, scenes, most, ties)


def test_the_hand_case_sits_in_a_scene_of_two(oracle):
    """DESIGN.md section 13's hand case as the GPU file places it in scene 1 of 3: eye 0 sees body 1 at column 440, eye 1 nobody"""
    pos, vel = np.array([[0, 0, 0], [10, 0, 0]], F), np.array([[1, 0, 0], [1, 0, 0]], F)
    _, _, (count, sids, _, _, col, rel) = located_of(oracle, pos, vel, 1024)
    assert (count == [1, 0]).all() and sids[0, 0] == 1 and col[0, 0] == 440
    assert (bits(rel[0, 0]) == [0x410FFFFE, 0x3F7CB3AE, 0, 0x410FFFFE]).all()
    p, v = L.nbody_located_step(pos, vel, count, rel)
    assert (bits(p[1]) == bits(F([11, 0, 0]))).all() and (bits(v[1]) == bits(vel[1])).all()


def test_premise_the_data_tells_leakage_from_isolation(oracle):
    """two scenes stepped as ONE set of 2 n bodies differ from the two stepped apart in some word of each scene: a kernel that let an
    eye see another scene's bodies would fail SL2's tests"""
    row = K.SIZES[100]
    pos, vel = K.batch(oracle, row, 2)
    n, width = row[1], row[2]
    apart = []
    for s in range(2):
        _, _, (count, _, _, _, _, rel) = located_of(oracle, pos[s], vel[s], width)
        apart.append(L.nbody_located_step(pos[s], vel[s], count, rel))
    p2, v2 = pos.reshape(2 * n, 3), vel.reshape(2 * n, 3)
    _, _, (count, _, _, _, _, rel) = located_of(oracle, p2, v2, width)
    together = L.nbody_located_step(p2, v2, count, rel)
    for s in range(2):
        rows = slice(s * n, (s + 1) * n)
        assert (bits(apart[s][0]) != bits(together[0][rows])).any() and (bits(apart[s][1]) != bits(together[1][rows])).any()


# -- the entries -------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody_scenes_located.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(nb):
    from nenbody_amd import _lib

    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert sorted(re.findall(r"\b(nb_[a-z_0-9]+)\s*\(", header)) == sorted(NAMES) == sorted(_lib.SCENES_LOCATED_PROTOTYPES)
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        assert len(_lib.SCENES_LOCATED_PROTOTYPES[name][1]) == c_args and hasattr(lib, name) and hasattr(_lib.load(), name), name
        assert not name.startswith("nb_launch_")
    main = open(os.path.join(ROOT, "include", "nenbody.h")).read()
    assert '#include "nenbody_scenes_located.h"' in main and int(re.search(r"#define NB_ABI_VERSION (\d+)", main).group(1)) == 2
    assert main.index("SL1") < main.index("SL5") < main.index('#include "nenbody_scenes_located.h"')   # the rule in front of the include
    for method in ("step_nbody_located", "located"):
        assert callable(getattr(nb.SceneBatch, method)), method


def test_the_rust_shim_declares_the_entry_points():
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = _header()
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for item in ("pub fn step_nbody_located(&mut self, k: u32, cp: &[[f32; 4]; 4], width: u32)", "pub fn located(&mut self, first_scene: u32"):
        assert item in text, item


def build_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "nenbody_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "scenes_located_check.cpp"), "-o", EXE, "-L", libdir, "-lnenbody_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)


def test_cpp_host_compiles_and_refuses_to_run_without_a_gpu(nb, tmp_path):
    build_exe()
    from nenbody_amd import _lib

    if _lib.load().nb_device_count() > 0:
        pytest.skip("a HIP device is present")
    r = subprocess.run([EXE, "3", "100", "1024", "2", str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 10 and "no HIP device" in r.stderr     # NB_ERR_NO_DEVICE surfaced as nenbody::Error


def test_the_entries_check_their_arguments_before_the_device(nb):
    """one refusal of each kind per entry; the full table with the texts is tests/test_scenes_located_api_messages.py"""
    from nenbody_amd import _lib

    lib = _lib.load()
    a = [0x10000000 + i * 0x4000000 for i in range(10)]           # fake device addresses, never dereferenced
    up = np.array([0, 0, 1], F)
    cp = np.zeros(16, F)
    cp[0], cp[5], cp[10], cp[11], cp[14] = 1.5, 1.5, -1.0001, -1.0, -1.0001
    flat = cp.copy()
    flat[11] = 0
    u, c, f = up.ctypes.data, cp.ctypes.data, flat.ctypes.data
    step, loc = lib.nb_scenes_nbody_located_step_launch, lib.nb_scenes_located_launch
    assert step(None, 3, 100, a[0], a[1], u, c, 1024, a[2], a[3], a[2], a[4], None) == _lib.NB_ERR_INVALID      # in place
    assert step(None, 3, 100, a[0], a[1], u, c, 4097, a[2], a[3], a[4], a[5], None) == _lib.NB_ERR_INVALID
    assert step(None, 3, 100, a[0], a[1], u, f, 1024, a[2], a[3], a[4], a[5], None) == _lib.NB_ERR_INVALID      # L6
    assert step(None, 1 << 17, 2048, a[0], a[1], u, c, 1024, a[2], a[3], a[4], a[5], None) == _lib.NB_ERR_UNSUPPORTED
    assert loc(3, 100, 0, 301, a[0], a[1], a[3], u, c, 1024, a[4], a[5], a[6], a[7], a[8], None) == _lib.NB_ERR_INVALID
    assert loc(3, 100, 0, 300, a[0], a[1], a[3], u, c, 1024, None, None, None, None, None, None) == _lib.NB_ERR_INVALID
    assert loc(3, 100, 0, 0, a[0], a[1], a[3], u, c, 1024, None, None, None, None, a[8], None) == _lib.NB_OK   # a checked no-op
    assert lib.nb_scenes_step_nbody_located(None, 1, None, None, 1024) == _lib.NB_ERR_INVALID
    assert lib.nb_scenes_eyes_located(None, 0, 1, None, None, 1024, None, None, None, None, None) == _lib.NB_ERR_INVALID
    with pytest.raises(ValueError):
        nb.SceneBatch.located(object(), first_scene=-1, scene_count=1)
