"""CPU tests of scene batches: the header, the binding, the library and the Rust shim agree on the entries;
the C++ host compiles and refuses to run without a GPU; the Python host refuses without one; and the premise of the GPU tests'
isolation checks -- on their data, stepping two scenes as one set differs from stepping them apart."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import scenes_restatement as R
from conftest import ROOT

NAMES = ["nb_scenes_nbody_step_launch", "nb_scenes_boids_step_launch", "nb_scenes_create", "nb_scenes_destroy", "nb_scenes_upload",
         "nb_scenes_step", "nb_scenes_step_boids", "nb_scenes_download", "nb_scenes_device_state", "nb_scenes_sync", "nb_scenes_steps",
         "nb_scenes_last_error"]
EXE = os.path.join(ROOT, "build", "scenes_check")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(nb):
    from nenbody_amd import _lib

    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == c_args and hasattr(lib, name), name
    assert sorted(n for n in _lib.PROTOTYPES if n.startswith("nb_scenes_")) == sorted(NAMES)
    assert int(re.search(r"#define NB_SCENES_MAX_BODIES (\d+)u", header).group(1)) == _lib.NB_SCENES_MAX_BODIES == 2048
    assert int(re.search(r"#define NB_ABI_VERSION (\d+)", header).group(1)) == 2
    for method in ("new", "step", "step_boids", "positions", "velocities", "instances", "device_state", "sync", "close", "__enter__",
                   "__exit__"):
        assert callable(getattr(nb.SceneBatch, method)), method
    assert isinstance(nb.SceneBatch.steps_done, property)


def test_no_new_name_looks_like_a_launch_or_scratch_entry():
    assert not [n for n in NAMES if n.startswith("nb_launch_") or "scratch_bytes" in n]


def test_the_rust_shim_declares_the_scene_batch_entry_points():
    """integration/rust/scene.rs is text (no Rust toolchain here): every scene-batch symbol is declared in its extern block with the
    header's argument count, and SceneBatch has the context's methods"""
    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = _header()
    for name in NAMES:
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for item in ("pub struct SceneBatch", "pub struct NbScenes", "pub fn step(&mut self, k: u32)", "pub fn step_boids(&mut self, k: u32)",
                 "pub fn download(", "pub fn device_state(", "pub fn sync(", "pub fn steps_done(", "impl Drop for SceneBatch",
                 "pub const NB_SCENES_MAX_BODIES: u32 = 2048;"):
        assert item in text, item


def build_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "nenbody_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "scenes_check.cpp"), "-o", EXE, "-L", libdir, "-lnenbody_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)


def test_cpp_host_compiles_and_refuses_to_run_without_a_gpu(nb, tmp_path):
    build_exe()
    from nenbody_amd import _lib

    if _lib.load().nb_device_count() > 0:
        pytest.skip("a HIP device is present")
    r = subprocess.run([EXE, "3", "100", "2", str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 10 and "no HIP device" in r.stderr     # NB_ERR_NO_DEVICE surfaced as nenbody::Error


def test_python_host_checks_shapes_and_refuses_without_a_gpu(nb):
    from nenbody_amd import _lib

    with pytest.raises(ValueError):
        nb.SceneBatch(np.zeros((3, 10, 2), np.float32), np.zeros((3, 10, 2), np.float32))
    with pytest.raises(ValueError):
        nb.SceneBatch(np.zeros((3, 10, 3), np.float32), np.zeros((3, 9, 3), np.float32))
    with pytest.raises(nb.NbError) as ei:
        nb.SceneBatch(np.zeros((3, 2049, 3), np.float32), np.zeros((3, 2049, 3), np.float32))
    assert ei.value.status == _lib.NB_ERR_INVALID and "nb_scenes_create: n must be 1 .. NB_SCENES_MAX_BODIES (2048)" in str(ei.value)
    with pytest.raises(nb.NbError) as ei:
        nb.SceneBatch.new(2, 10, 5, nb.default_params(mode=nb.NB_MODE_FAST))
    assert ei.value.status == _lib.NB_ERR_UNSUPPORTED and "STRICT only" in str(ei.value)
    if _lib.load().nb_device_count() == 0:
        with pytest.raises(nb.NbError) as ei:
            nb.SceneBatch.new(2, 10, 5)
        assert ei.value.status == _lib.NB_ERR_NO_DEVICE


@pytest.mark.parametrize("law", ["nbody", "boids"])
def test_premise_the_data_tells_leakage_from_isolation(oracle, law):
    """two scenes of the GPU tests' data stepped as ONE set of 2 n bodies differ from the per-scene result in some bit of every
    scene: a kernel that let one scene see another's records would fail the comparisons of tests/test_gpu_scenes.py"""
    import scenes_cases as K

    n = 100
    pos, vel = K.scenes(oracle, law, 2, n, seed=7)
    step = getattr(R, law)
    apart = step(oracle, pos, vel, 2)
    together = step(oracle, pos.reshape(1, 2 * n, 3), vel.reshape(1, 2 * n, 3), 2)
    for got, want in zip(apart, together):
        differs = (got.view(np.uint32) != want.reshape(2, n, 3).view(np.uint32)).any(axis=(1, 2))
        assert differs.all(), differs
    # and the restatement is per scene: scene 1 alone is scene 1 of the pair
    alone = step(oracle, pos[1:], vel[1:], 2)
    assert all((a.view(np.uint32) == b[1:].view(np.uint32)).all() for a, b in zip(alone, apart))
