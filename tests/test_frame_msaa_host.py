"""The arithmetic of the frame kernels without a GPU: nb_frame_msaa.inc's device functions, nb_frame.inc's and the shared rule of
nb_raster.inc they all call, compiled for the host by g++ with -ffp-contract=off and driven sample by sample
(tests/cpp/frame_msaa_host.cpp), against the numpy restatements of the rule, every word: the 8-sample frame, and the one-sample
frame (keys by frame_cover, colour by frame_shade) on the same scenes.  What this cannot see is the kernels' own plumbing -- which
lane takes which sample, the atomics on the key plane, the launches -- which tests/test_gpu_frame*.py cover on the device."""
import os
import subprocess

import numpy as np
import pytest

import frame_msaa_restatement as FM
import frame_restatement as FR
from conftest import ROOT

F = np.float32
CSRC = os.path.join(ROOT, "nenbody_amd", "csrc")
BUILD = os.path.join(ROOT, "build", "frame_msaa_host")


@pytest.fixture(scope="module")
def host():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "frame_msaa_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-msse2", "-mfpmath=sse", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "frame_msaa_host.cpp"), "-o", exe], check=True)
    return exe


def run(exe, tmp_path, cam, inst, W, H, skin, one=False):
    np.ascontiguousarray(cam, F).tofile(tmp_path / "cam.bin")
    np.ascontiguousarray(inst, F).tofile(tmp_path / "inst.bin")
    th, tw = skin.shape[:2] if skin is not None else (0, 0)
    (skin if skin is not None else np.zeros(4, F)).astype(F).tofile(tmp_path / "skin.bin")
    subprocess.run([exe, str(len(inst)), str(W), str(H), str(tw), str(th), str(tmp_path / "cam.bin"), str(tmp_path / "inst.bin"),
                    str(tmp_path / "skin.bin"), str(tmp_path / "out.bin")] + (["one"] if one else []), check=True)
    raw = np.fromfile(tmp_path / "out.bin", np.uint32)
    if one:
        a, b, c, d = np.split(raw, [W * H, 2 * W * H, 6 * W * H])
        return a.reshape(H, W), b.reshape(H, W), c.reshape(H, W, 4), d.reshape(H, W)
    a, b, c, d = np.split(raw, [8 * W * H, 16 * W * H, 20 * W * H])
    return a.reshape(H, W, 8), b.reshape(H, W, 8), c.reshape(H, W, 4), d.reshape(H, W)


def assert_same(got, want, what):
    assert len(got) == len(want) == 4
    for name, g, w in zip(("ids8", "depth8", "rgba", "bgra8"), got, want):
        bad = g != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"


def test_the_hand_scene(oracle, host, tmp_path):
    inst = oracle.instances(np.array([[0.5, 0, 0]], F), np.array([[1, 0, 0]], F))
    cam = FR.ortho_camera(64, 32)
    got = run(host, tmp_path, cam, inst, 64, 32, None)
    assert_same(got, FM.frame_msaa(cam, inst, 64, 32), "hand scene")
    assert (got[0] != 0xFFFFFFFF).sum() == 38 and got[3][15, 31] == 0xFFDFDFDF and got[3][16, 31] == 0xFFE5E5E5


@pytest.mark.parametrize("name", ["side", "three"])
def test_the_scenes(oracle, host, tmp_path, name):
    pos, vel, cam, (W, H) = FR.scene(oracle, name)
    inst = oracle.instances(pos, vel)
    skin = None
    if name == "side":
        skin = np.random.default_rng(11).uniform(0, 1, (5, 7, 4)).astype(F)
        skin[0, 0, 0], skin[4, 6, 1] = 1.5, -0.25
    stats = {}
    want = FM.frame_msaa(cam, inst, W, H, skin=skin, stats=stats)
    assert stats["writes"] > 3000 and stats["two_bodies"] > 0 and (stats["edge"] > 0).all()
    assert_same(run(host, tmp_path, cam, inst, W, H, skin), want, name)


@pytest.mark.parametrize("extent", [(1, 1), (3, 2)])
def test_small_extents(oracle, host, tmp_path, extent):
    pos, vel = FR.spread_state(oracle, 257, 31, 30)
    cam = FR.camera(oracle, [0, 0, 150], [0, 0, -1], [1, 0, 0], FR.frame_constant(oracle, extent))
    inst = oracle.instances(pos, vel)
    skin = np.random.default_rng(3).uniform(0, 1, (3, 9, 4)).astype(F)
    want = FM.frame_msaa(cam, inst, extent[0], extent[1], skin=skin)
    assert (want[0] != 0xFFFFFFFF).any()
    assert_same(run(host, tmp_path, cam, inst, extent[0], extent[1], skin), want, f"{extent}")


# The one-sample frame through the same driver: frame_cover and frame_shade call the same nb_raster.inc functions as the 8-sample ones.

def test_the_hand_scene_one_sample(oracle, host, tmp_path):
    inst = oracle.instances(np.array([[0.5, 0, 0]], F), np.array([[1, 0, 0]], F))
    cam = FR.ortho_camera(64, 32)
    got = run(host, tmp_path, cam, inst, 64, 32, None, one=True)
    assert_same(got, FR.frame(cam, inst, 64, 32), "hand scene, one sample")
    assert (got[0] != 0xFFFFFFFF).any()


@pytest.mark.parametrize("name", ["side", "three"])
def test_the_scenes_one_sample(oracle, host, tmp_path, name):
    pos, vel, cam, (W, H) = FR.scene(oracle, name)
    inst = oracle.instances(pos, vel)
    skin = None
    if name == "side":
        skin = np.random.default_rng(11).uniform(0, 1, (5, 7, 4)).astype(F)
        skin[0, 0, 0], skin[4, 6, 1] = 1.5, -0.25
    stats = {}
    want = FR.frame(cam, inst, W, H, skin=skin, stats=stats)
    assert stats["writes"] > 300 and stats["covered"] > 0
    assert_same(run(host, tmp_path, cam, inst, W, H, skin, one=True), want, f"{name}, one sample")


@pytest.mark.parametrize("extent", [(1, 1), (3, 2)])
def test_small_extents_one_sample(oracle, host, tmp_path, extent):
    pos, vel = FR.spread_state(oracle, 257, 31, 30)
    cam = FR.camera(oracle, [0, 0, 150], [0, 0, -1], [1, 0, 0], FR.frame_constant(oracle, extent))
    inst = oracle.instances(pos, vel)
    skin = np.random.default_rng(3).uniform(0, 1, (3, 9, 4)).astype(F)
    want = FR.frame(cam, inst, extent[0], extent[1], skin=skin)
    assert (want[0] != 0xFFFFFFFF).any()
    assert_same(run(host, tmp_path, cam, inst, extent[0], extent[1], skin, one=True), want, f"{extent}, one sample")
