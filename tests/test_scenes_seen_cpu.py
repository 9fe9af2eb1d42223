"""CPU tests of the scene batches' seen boids step: the premises the GPU tests rest on, checked on the very
rows of tests/scenes_seen_cases.py through the numpy restatements of the eye rule and of the seen step; the header, the binding, the
library, the C++ host and the Rust shim agree on the four entries; and what the entries refuse without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import eyes_restatement as R
import np_restatement as NP
import scenes_seen_cases as K
import seen_restatement as S
from conftest import ROOT

F = np.float32
NAMES = ["nb_scenes_boids_seen_step_launch", "nb_scenes_seen_launch", "nb_scenes_step_boids_seen", "nb_scenes_eyes_seen"]
EXE = os.path.join(ROOT, "build", "scenes_seen_check")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mask_of(oracle, pos, vel, width):
    """what every body of one scene sees, by the numpy eye rule; cameras and matrices by the oracle"""
    cams = oracle.cameras(pos, vel, K.UP, R.eye_constant(oracle, width))
    ids, _ = R.eyes(cams, oracle.instances(pos, vel), 0, width, chunk=64)
    return S.mask_of_rows(ids, len(pos))


_checked = {}


def premises(oracle, seed, n, width, scale):
    """(blind bodies, bodies that see somebody, the seen step differs from the plain one in position and in velocity)"""
    key = (seed, n, width, scale)
    if key not in _checked:
        pos, vel = K.batch(oracle, (seed, n, width, scale, 1))
        pos, vel = pos[0], vel[0]
        mask = mask_of(oracle, pos, vel, width)
        assert not mask[np.arange(n), np.arange(n)].any()                 # an eye does not see its own body
        sees = mask.sum(1)
        got = S.boids_seen_step(pos, vel, mask)
        plain = NP.boids_step(pos, vel)
        blind = sees == 0
        assert (bits(got[1][blind]) == 0).all() and (bits(got[0][blind]) == bits(pos[blind])).all()
        _checked[key] = (int(blind.sum()), int((sees > 0).sum()),
                         bool((bits(got[0]) != bits(plain[0])).any() and (bits(got[1]) != bits(plain[1])).any()))
    return _checked[key]


ROWS = sorted({(seed + s, n, width, scale) for seed, n, width, scale, b in K.ROWS if K.holds_premises((seed, n, width, scale, b))
               for s in range(b)})


def test_the_rows_cover_what_the_issue_lists():
    assert sorted(K.SIZES) == [1, 2, 3, 63, 64, 65, 100, 128, 129, 257, 2048]
    assert sorted(K.WIDTHS) == [1, 63, 64, 65, 1000, 4096] and all(r[1] == 65 for r in K.WIDTHS.values())
    assert sorted(K.LISTS) == [(n, w) for n in (64, 100, 129) for w in (64, 1024)]
    assert K.FLOOR[1:] == (100, 1024, 1.0, 64)
    exempt = [r for r in K.ROWS if not K.holds_premises(r)]
    assert sorted({(r[1], r[2]) for r in exempt}) == [(1, 1024), (2, 1024), (3, 1024), (65, 1)]   # nothing else is let off


@pytest.mark.parametrize("n", sorted({r[1] for r in ROWS}))
def test_every_scene_has_a_blind_body_most_see_somebody_and_the_steps_differ(oracle, n):
    rows = [r for r in ROWS if r[1] == n]
    assert rows
    for seed, _, width, scale in rows:
        blind, seeing, differs = premises(oracle, seed, n, width, scale)
        assert blind >= 1 and seeing > n // 2 and differs, (seed, n, width, scale, blind, seeing, differs)


def test_the_known_row_is_the_design_tables(oracle):
    """DESIGN.md section 12's table: N = 100, seed 1100, W = 1024 has 9 blind bodies"""
    assert premises(oracle, 1100, 100, 1024, 1.0)[:2] == (9, 91)


@pytest.mark.parametrize("row", [K.SIZES[100], K.LISTS[(64, 64)]])
def test_premise_the_data_tells_leakage_from_isolation(oracle, row):
    """two scenes stepped as ONE set of 2 n bodies -- every eye seeing the other scene's bodies too -- differ from the two stepped
    apart in some word of each scene: a kernel that let an eye see, or a fold read, another scene's records would fail SV2's tests"""
    pos, vel = K.batch(oracle, row, 2)
    n, width = row[1], row[2]
    apart = [S.boids_seen_step(pos[s], vel[s], mask_of(oracle, pos[s], vel[s], width)) for s in range(2)]
    p2, v2 = pos.reshape(2 * n, 3), vel.reshape(2 * n, 3)
    together = S.boids_seen_step(p2, v2, mask_of(oracle, p2, v2, width))
    for s in range(2):
        rows = slice(s * n, (s + 1) * n)
        assert (bits(apart[s][0]) != bits(together[0][rows])).any() and (bits(apart[s][1]) != bits(together[1][rows])).any()


def test_the_hand_case_sits_in_a_scene_of_two(oracle):
    """DESIGN.md section 12's hand case as the GPU file places it in scene 1 of 3: body 0 takes v.x = 0.7f, body 1 stops"""
    pos, vel = np.array([[0, 0, 0], [10, 0, 0]], F), np.array([[1, 0, 0], [1, 0, 0]], F)
    mask = mask_of(oracle, pos, vel, 1024)
    assert (mask == [[False, True], [False, False]]).all()
    p, v = S.boids_seen_step(pos, vel, mask)
    assert (bits(v[0]) == [0x3F333333, 0, 0]).all() and (bits(v[1]) == 0).all() and (bits(p[1]) == bits(pos[1])).all()


# -- the entries -------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody_scenes_seen.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(nb):
    from nenbody_amd import _lib

    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert sorted(re.findall(r"\b(nb_[a-z_0-9]+)\s*\(", header)) == sorted(NAMES) == sorted(_lib.SCENES_SEEN_PROTOTYPES)
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        assert len(_lib.SCENES_SEEN_PROTOTYPES[name][1]) == c_args and hasattr(lib, name) and hasattr(_lib.load(), name), name
    main = open(os.path.join(ROOT, "include", "nenbody.h")).read()
    assert '#include "nenbody_scenes_seen.h"' in main and int(re.search(r"#define NB_ABI_VERSION (\d+)", main).group(1)) == 2
    for method in ("step_boids_seen", "seen"):
        assert callable(getattr(nb.SceneBatch, method)), method


def test_the_rust_shim_declares_the_entry_points():
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = _header()
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for item in ("pub fn step_boids_seen(&mut self, k: u32, cp: &[[f32; 4]; 4], width: u32)", "pub fn seen(&mut self, first_scene: u32"):
        assert item in text, item


def build_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "nenbody_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "scenes_seen_check.cpp"), "-o", EXE, "-L", libdir, "-lnenbody_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)


def test_cpp_host_compiles_and_refuses_to_run_without_a_gpu(nb, tmp_path):
    build_exe()
    from nenbody_amd import _lib

    if _lib.load().nb_device_count() > 0:
        pytest.skip("a HIP device is present")
    r = subprocess.run([EXE, "3", "100", "1024", "2", str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 10 and "no HIP device" in r.stderr     # NB_ERR_NO_DEVICE surfaced as nenbody::Error


def test_the_entries_check_their_arguments_before_the_device(nb):
    """one refusal of each kind per entry; the full table with the texts is tests/test_scenes_seen_api_messages.py"""
    from nenbody_amd import _lib

    lib = _lib.load()
    a = [0x10000000 + i * 0x4000000 for i in range(8)]            # fake device addresses, never dereferenced
    step, seen = lib.nb_scenes_boids_seen_step_launch, lib.nb_scenes_seen_launch
    assert step(None, 3, 100, a[0], a[1], 1024, a[2], a[3], a[2], a[4], None) == _lib.NB_ERR_INVALID      # in place
    assert step(None, 3, 100, a[0], a[1], 4097, a[2], a[3], a[4], a[5], None) == _lib.NB_ERR_INVALID
    assert step(None, 1 << 17, 2048, a[0], a[1], 1024, a[2], a[3], a[4], a[5], None) == _lib.NB_ERR_UNSUPPORTED
    assert seen(3, 100, 0, 301, a[0], a[1], 1024, a[2], a[3], None) == _lib.NB_ERR_INVALID
    assert seen(3, 100, 0, 300, a[0], a[1], 1024, None, None, None) == _lib.NB_ERR_INVALID
    assert seen(3, 100, 0, 0, a[0], a[1], 1024, a[2], None, None) == _lib.NB_OK                           # a checked no-op
    assert lib.nb_scenes_step_boids_seen(None, 1, None, None, None, 1024) == _lib.NB_ERR_INVALID
    assert lib.nb_scenes_eyes_seen(None, 0, 1, None, None, 1024, None, None) == _lib.NB_ERR_INVALID
    with pytest.raises(ValueError):
        nb.SceneBatch.seen(object(), first_scene=-1, scene_count=1)
