"""The 8-sample eye rows through the C++ host mirror (Scene::eyes_msaa of include/nenbody_scene.hpp): compiles against the C ABI
with plain g++, runs the host-only sample offsets and then fails loudly without a GPU (CPU test); on a GPU its four outputs are the
rule's, bit for bit (GPU test)."""
import os
import subprocess

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_msaa_restatement as M
import eyes_restatement as R
from conftest import ROOT

EXE = os.path.join(ROOT, "build", "eyes_msaa_check")


def build_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "nenbody_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "eyes_msaa_check.cpp"), "-o", EXE, "-L", libdir, "-lnenbody_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)


def test_cpp_eyes_msaa_host_compiles_and_refuses_to_run_without_a_gpu(nb, tmp_path):
    build_exe()
    from nenbody_amd import _lib

    have_device = _lib.load().nb_device_count() > 0
    r = subprocess.run([EXE, "16", "64", "-", "0", "0", str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert "offsets ok" in r.stdout                                   # nb_eyes_sample_offsets needs no device
    if have_device:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 10 and "no HIP device" in r.stderr     # NB_ERR_NO_DEVICE surfaced as nenbody::Error


@pytest.mark.gpu
@pytest.mark.parametrize("n,width,skin", [(100, 1024, "reference"), (33, 257, "white")])
def test_cpp_eyes_msaa_host_matches_the_rule(nb, oracle, tmp_path, n, width, skin):
    build_exe()
    out = tmp_path / "out.bin"
    lin = None
    args = ["-", "0", "0"]
    if skin == "reference":
        lin = K.skin_from_srgb8(np.load(os.path.join(ROOT, "tests", "golden", "skin_rgba8.npy")))
        lin.tofile(tmp_path / "skin.bin")
        args = [str(tmp_path / "skin.bin"), "20", "20"]
    r = subprocess.run([EXE, str(n), str(width), *args, str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint32)
    cells = n * width
    ids8, depth8, rgba, bgra8, part = np.split(raw, [8 * cells, 16 * cells, 20 * cells, 21 * cells])
    pos, vel = oracle.init_state(n, 1234)
    cams = oracle.cameras(pos, vel, np.array([0, 0, 1], np.float32), R.eye_constant(oracle, width))
    inst = oracle.instances(pos, vel)
    want = M.msaa(cams, inst, 0, width, skin=lin)
    assert (ids8.reshape(n, width, 8) == want[0]).all() and (depth8.reshape(n, width, 8) == want[1].view(np.uint32)).all()
    assert (rgba.reshape(n, width, 4) == want[2].view(np.uint32)).all() and (bgra8.reshape(n, width) == want[3]).all()
    assert (want[0] != R.NONE).any()
    own = M.msaa(cams[n // 2:n // 2 + 1], inst, n // 2, width, see_self=True, skin=lin)
    assert (part == own[3][0]).all()
