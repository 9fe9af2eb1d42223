"""The frame through 8 samples per pixel through the C++ host mirror (Scene::frame_msaa of include/nenbody_scene.hpp): compiles
against the C ABI with plain g++, runs the host-only helpers and then fails loudly without a GPU (CPU test); on a GPU its four
outputs are the rule's, bit for bit (GPU test).  The Rust shim is text: its declarations are counted."""
import os
import subprocess

import numpy as np
import pytest

import frame_msaa_restatement as FM
import frame_restatement as FR
from conftest import ROOT

EXE = os.path.join(ROOT, "build", "frame_msaa_check")
F = np.float32


def build_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "nenbody_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "frame_msaa_check.cpp"), "-o", EXE, "-L", libdir, "-lnenbody_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)


def test_cpp_frame_msaa_host_compiles_and_refuses_to_run_without_a_gpu(nb, tmp_path):
    build_exe()
    from nenbody_amd import _lib

    have_device = _lib.load().nb_device_count() > 0
    r = subprocess.run([EXE, "-", "16", "-", "64", "32", "-", "0", "0", str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert "scratch ok" in r.stdout                                   # nb_frame_msaa_scratch_bytes and the offsets need no device
    if have_device:                                                   # (sixteen bodies at the origin through a NaN camera: a clear frame)
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 10 and "no HIP device" in r.stderr     # NB_ERR_NO_DEVICE surfaced as nenbody::Error


def test_the_rust_shim_declares_the_frame_msaa_entry_points():
    """integration/rust/scene.rs is text (no Rust toolchain here): the new symbols of the header are declared in its extern block
    with the header's argument counts, and Scene has frame_msaa"""
    import re

    text = open(os.path.join(ROOT, "integration", "rust", "scene.rs")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nenbody.h")).read(), flags=re.S)
    for name, ret in (("nb_frame_sample_offsets", "c_int"), ("nb_frame_msaa", "c_int"), ("nb_frame_msaa_scratch_bytes", "usize")):
        c_args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1).count(",") + 1
        m = re.search(r"fn %s\s*\(([^)]*)\)\s*->\s*%s;" % (name, ret), text)
        assert m, name
        assert m.group(1).strip().rstrip(",").count(",") + 1 == c_args, name
    for item in ("pub fn frame_msaa(", "pub fn frame_sample_offsets(", "pub struct FrameMsaa", "pub const NB_FRAME_MSAA_MAX_DIM: u32 = 2048;"):
        assert item in text, item


@pytest.mark.gpu
def test_cpp_frame_msaa_host_matches_the_rule(nb, oracle, tmp_path):
    """the "side" scene with a 7 x 5 skin: the camera Scene::camera_at forms is the oracle's, the frame is the rule's"""
    build_exe()
    pos, vel, cam, (W, H) = FR.scene(oracle, "side")
    skin = np.random.default_rng(11).uniform(-0.25, 1.5, (5, 7, 4)).astype(F)
    np.concatenate([pos.ravel(), vel.ravel()]).astype(F).tofile(tmp_path / "state.bin")
    cp = FR.frame_constant(oracle, (W, H))
    np.concatenate([F([-150, 0, 40]), F([1, 0, -0.25]), F([0, 0, 1]), np.ascontiguousarray(cp, F).ravel()]).tofile(tmp_path / "cam.bin")
    skin.tofile(tmp_path / "skin.bin")
    out = tmp_path / "out.bin"
    r = subprocess.run([EXE, str(tmp_path / "state.bin"), str(len(pos)), str(tmp_path / "cam.bin"), str(W), str(H), str(tmp_path / "skin.bin"),
                        "7", "5", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint32)
    cells = W * H
    got_cam, ids8, depth8, rgba, bgra8 = np.split(raw, [16, 16 + 8 * cells, 16 + 16 * cells, 16 + 20 * cells])
    assert (got_cam == np.ascontiguousarray(cam, F).view(np.uint32).ravel()).all()
    want = FM.frame_msaa(cam, oracle.instances(pos, vel), W, H, skin=skin)
    assert (ids8.reshape(H, W, 8) == want[0]).all() and (depth8.reshape(H, W, 8) == want[1].view(np.uint32)).all()
    assert (rgba.reshape(H, W, 4) == want[2].view(np.uint32)).all() and (bgra8.reshape(H, W) == want[3]).all()
    assert (want[0] != 0xFFFFFFFF).sum() > 2000
