"""The arithmetic of the eye kernels without a GPU: nb_eyes_msaa.inc's device functions, nb_eyes.inc's and the shared rule of
nb_raster.inc they all call, compiled for the host by g++ with -ffp-contract=off and driven sample by sample
(tests/cpp/eyes_msaa_host.cpp), against the numpy restatements of the rule, every word: the 8-sample rows, and the one-sample rows
(keys by eye_cover, colour by eye_shade) on the same cases.  What this cannot see is the kernels' own plumbing -- which lane takes
which sample, the LDS atomics, the launch -- which tests/test_gpu_eyes*.py cover on the device."""
import os
import subprocess

import numpy as np
import pytest

import eyes_colour_restatement as K
import eyes_msaa_restatement as M
import eyes_restatement as R
from conftest import ROOT

F = np.float32
UP = np.array([0, 0, 1], np.float32)
CSRC = os.path.join(ROOT, "nenbody_amd", "csrc")
BUILD = os.path.join(ROOT, "build", "eyes_msaa_host")


@pytest.fixture(scope="module")
def host():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "eyes_msaa_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "eyes_msaa_host.cpp"), "-o", exe], check=True)
    return exe


def run(exe, tmp_path, cams, inst, first, width, see_self, skin, one=False):
    cams.astype(F).tofile(tmp_path / "cams.bin")
    inst.astype(F).tofile(tmp_path / "inst.bin")
    th, tw = skin.shape[:2] if skin is not None else (0, 0)
    (skin if skin is not None else np.zeros(4, F)).astype(F).tofile(tmp_path / "skin.bin")
    E = len(cams)
    subprocess.run([exe, str(E), str(len(inst)), str(first), str(width), str(int(see_self)), str(tw), str(th), str(tmp_path / "cams.bin"),
                    str(tmp_path / "inst.bin"), str(tmp_path / "skin.bin"), str(tmp_path / "out.bin")] + (["one"] if one else []), check=True)
    raw = np.fromfile(tmp_path / "out.bin", np.uint32).reshape(E, -1)
    if one:
        return np.split(raw, [width, 2 * width, 6 * width], axis=1)[:2] + [raw[:, 2 * width:6 * width].reshape(E, width, 4), raw[:, 6 * width:]]
    a, b, c, d = np.split(raw, [8 * width, 16 * width, 20 * width], axis=1)
    return a.reshape(E, width, 8), b.reshape(E, width, 8), c.reshape(E, width, 4), d


def assert_same(got, want, what):
    assert len(got) == len(want) == 4
    for name, g, w in zip(("ids8", "depth8", "rgba", "bgra8"), got, want):
        bad = g != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"


def test_the_lattice(oracle, host, tmp_path):
    cams = np.repeat(R.lattice_camera()[None], 4, 0)
    inst = oracle.instances(R.LATTICE_POS, R.LATTICE_VEL)
    got = run(host, tmp_path, cams, inst, 0, 1024, True, None)
    assert_same(got, M.msaa(cams, inst, 0, 1024, True), "lattice")
    assert (got[0][0, 511] == [0, R.NONE, 0, R.NONE, R.NONE, R.NONE, 0, 0]).all() and got[3][0, 511] == 0xFF95A0AA


@pytest.mark.parametrize("see_self", [False, True])
def test_forty_eyes_of_a_hundred_bodies(oracle, host, tmp_path, see_self):
    pos, vel = oracle.init_state(100, 1100)
    skin = K.skin_from_srgb8(np.load(os.path.join(ROOT, "tests", "golden", "skin_rgba8.npy")))
    cams = oracle.cameras(pos[30:70], vel[30:70], UP, R.eye_constant(oracle))
    inst = oracle.instances(pos, vel)
    stats = {}
    want = M.msaa(cams, inst, 30, 1024, see_self, skin, stats=stats)
    assert stats["covered_hist"][1:8].min() >= 30 and stats["two_bodies"] >= 100 and stats["extrapolated"] >= 500, stats["covered_hist"]
    assert_same(run(host, tmp_path, cams, inst, 30, 1024, see_self, skin), want, f"N=100 see_self={see_self}")


@pytest.mark.parametrize("width", [1, 3, 2048])
def test_widths(oracle, host, tmp_path, width):
    pos, vel = oracle.init_state(257, 31)
    skin = np.random.default_rng(11).uniform(0, 1, (5, 7, 4)).astype(F)
    skin[0, 0, 0], skin[4, 6, 1] = 1.5, -0.25
    cams = oracle.cameras(pos[:24], vel[:24], UP, R.eye_constant(oracle, width))
    inst = oracle.instances(pos, vel)
    assert_same(run(host, tmp_path, cams, inst, 0, width, False, skin), M.msaa(cams, inst, 0, width, False, skin), f"W={width}")


# The one-sample rows through the same driver: eye_cover and eye_shade call the same nb_raster.inc functions as the 8-sample ones.

def test_the_lattice_one_sample(oracle, host, tmp_path):
    cams = np.repeat(R.lattice_camera()[None], 4, 0)
    inst = oracle.instances(R.LATTICE_POS, R.LATTICE_VEL)
    got = run(host, tmp_path, cams, inst, 0, 1024, True, None, one=True)
    assert_same(got, K.colour(cams, inst, 0, 1024, True), "lattice, one sample")
    ids, depth = R.lattice_expectation()
    assert (got[0] == ids).all() and (got[1] == depth.view(np.uint32)).all()


@pytest.mark.parametrize("see_self", [False, True])
def test_forty_eyes_of_a_hundred_bodies_one_sample(oracle, host, tmp_path, see_self):
    pos, vel = oracle.init_state(100, 1100)
    skin = K.skin_from_srgb8(np.load(os.path.join(ROOT, "tests", "golden", "skin_rgba8.npy")))
    cams = oracle.cameras(pos[30:70], vel[30:70], UP, R.eye_constant(oracle))
    inst = oracle.instances(pos, vel)
    want = K.colour(cams, inst, 30, 1024, see_self, skin)
    assert (want[0] != R.NONE).mean() > 0.05
    assert_same(run(host, tmp_path, cams, inst, 30, 1024, see_self, skin, one=True), want, f"N=100 see_self={see_self}, one sample")


@pytest.mark.parametrize("width", [1, 3, 2048])
def test_widths_one_sample(oracle, host, tmp_path, width):
    pos, vel = oracle.init_state(257, 31)
    skin = np.random.default_rng(11).uniform(0, 1, (5, 7, 4)).astype(F)
    skin[0, 0, 0], skin[4, 6, 1] = 1.5, -0.25
    cams = oracle.cameras(pos[:24], vel[:24], UP, R.eye_constant(oracle, width))
    inst = oracle.instances(pos, vel)
    assert_same(run(host, tmp_path, cams, inst, 0, width, False, skin, one=True), K.colour(cams, inst, 0, width, False, skin),
                f"W={width}, one sample")
