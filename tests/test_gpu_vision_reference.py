"""GPU tests of the eye rows, the seen sets and the frame against the binary64 geometric reference (tests/vision_reference.py) on the
cases of tests/vision_reference_cases.py: the device entries run on the uploaded (pos, vel), so cameras and model matrices are the
device's too, and every result is compared twice -- (a) with the reference: decided cells in full, ids exactly, depth and rgba
within their derived bounds, empty cells exactly; (b) bit for bit with the numpy restatements on these new cases, through the
comparison helpers of the files that hold each kernel to its restatement.  What the cases cover, that the restatements lie within
the bounds, and that the bounds reject mistakes the rule could hide is checked on the CPU, tests/test_vision_reference_cpu.py."""
import numpy as np
import pytest

import eyes_colour_restatement as K
import frame_restatement as FR
import seen_restatement as S
import test_gpu_eyes as TE
import test_gpu_eyes_colour as TC
import test_gpu_eyes_msaa as TM
import test_gpu_frame as TF
import test_gpu_seen as TS
import vision_reference as V
import vision_reference_cases as C

pytestmark = pytest.mark.gpu

F = np.float32
MSAA_CASES = [name for name, c in C.EYE_CASES.items() if c["width"] <= C.MSAA_MAX_WIDTH]


def scene_of(nb, oracle, name):
    """the case's Scene with its skin set, what every eye-row entry takes, and the restatement's helpers' arguments"""
    c = C.EYE_CASES[name]
    pos, vel = C.eye_state(oracle, name)
    sc = nb.Scene(pos, vel)
    given, _ = C.skin_of(c)
    sc.set_skin(given)
    call = dict(width=c["width"], up=c["up"], cp=C.eye_constant(nb, name), first=0, see_self=c["see_self"])
    want = dict(width=c["width"], cp=C.eye_constant(oracle, name), up=np.array(c["up"], F), see_self=c["see_self"])
    return sc, pos, vel, call, want, (K.skin_from_srgb8(given) if c["skin"] else None)


@pytest.mark.parametrize("name", list(C.EYE_CASES))
def test_eyes_and_eyes_colour(nb, oracle, name):
    sc, pos, vel, call, want, skin = scene_of(nb, oracle, name)
    rows = np.arange(C.eyes_of(name))
    with sc:
        plain = sc.eyes(count=len(rows), **call)
        got = sc.eyes_colour(count=len(rows), **call)
    ref = C.eye_reference(oracle, name)
    print(name, "eyes", V.compare(f"{name}: Scene.eyes", ref, *plain, labels=rows))
    print(name, "eyes_colour", V.compare(f"{name}: Scene.eyes_colour", ref, *got[:3], labels=rows))
    TE.assert_same(plain, TE.expect(oracle, pos, vel, rows, **want), f"{name}: Scene.eyes against the restatement")
    TC.assert_same(got, TC.expect(oracle, pos, vel, rows, skin=skin, **want), f"{name}: Scene.eyes_colour against the restatement")


@pytest.mark.parametrize("name", MSAA_CASES)
def test_eyes_msaa(nb, oracle, name):
    sc, pos, vel, call, want, skin = scene_of(nb, oracle, name)
    rows = np.arange(C.eyes_of(name, True))
    with sc:
        got = sc.eyes_msaa(count=len(rows), **call)
    ref = C.eye_reference(oracle, name, True)
    print(name, "eyes_msaa", V.compare(f"{name}: Scene.eyes_msaa", ref, *got[:3], labels=rows))
    TM.assert_same(got, TM.expect(oracle, pos, vel, rows, skin=skin, **want), f"{name}: Scene.eyes_msaa against the restatement")


@pytest.mark.parametrize("name", list(C.EYE_CASES))
def test_seen(nb, oracle, name):
    sc, pos, vel, call, want, _ = scene_of(nb, oracle, name)
    rows = np.arange(C.eyes_of(name))
    with sc:
        count, ids, depth, cols = sc.seen(count=len(rows), **call)
    print(name, "seen", V.compare_seen(f"{name}: Scene.seen", C.eye_reference(oracle, name), count, ids, depth, labels=rows))
    TS.assert_lists((count, ids, TS.bits(depth), cols), S.seen_rows(*TE.expect(oracle, pos, vel, rows, **want)),
                    f"{name}: Scene.seen against the restatement")


def frame_of(oracle, name):
    c = C.FRAME_CASES[name]
    pos, vel = C.frame_state(oracle)
    given, _ = C.skin_of(c)
    return c, pos, vel, given, (K.skin_from_srgb8(given) if c["skin"] else None)


@pytest.mark.parametrize("name", list(C.FRAME_CASES))
def test_camera_at_and_frame(nb, oracle, name):
    c, pos, vel, given, skin = frame_of(oracle, name)
    with nb.Scene(pos, vel) as sc:
        sc.set_skin(given)
        cam = sc.camera_at(c["eye"], c["direction"], c["up"], C.frame_constant(nb, name))
        got = sc.frame(cam, c["extent"])
    print(name, "frame", V.compare(f"{name}: Scene.frame", C.frame_reference(oracle, name), *got[:3], axes=("row", "column")))
    want_cam = FR.camera(oracle, c["eye"], c["direction"], c["up"], C.frame_constant(oracle, name))
    assert (TF.bits(cam) == TF.bits(want_cam)).all(), f"{name}: Scene.camera_at against the oracle's camera"
    TF.assert_same(got, FR.frame(want_cam, oracle.instances(pos, vel), *c["extent"], skin=skin), f"{name}: Scene.frame against the restatement")


def test_the_launch_forms(nb, oracle):
    """nb_launch_eyes_colour and nb_launch_frame on caller-owned device memory and a stream of their own, cameras and model matrices
    from the device: one eye case (3-D data, the far plane at 50, the reference's skin, 65 columns) and one frame case (oblique)"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    name = "n100_w65_lifted_far50_skin"
    sc, pos, vel, call, want, skin = scene_of(nb, oracle, name)
    n, e, w = len(pos), C.eyes_of(name), C.EYE_CASES[name]["width"]
    with sc:
        cams = torch.from_numpy(sc.cameras(call["up"], call["cp"])[:e].reshape(e, 16).copy()).to(dev)
        inst = torch.from_numpy(sc.instances().reshape(n, 16).copy()).to(dev)
    st = torch.from_numpy(skin).to(dev)
    out = [torch.full((e, w), 7, dtype=torch.int32, device=dev), torch.full((e, w), 7.0, dtype=torch.float32, device=dev),
           torch.full((e, w, 4), 7.0, dtype=torch.float32, device=dev), torch.full((e, w), 7, dtype=torch.int32, device=dev)]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        TC.launch(nb, n, 0, e, cams, inst, w, 0, st, *out, s)
    s.synchronize()
    got = (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy().view(np.uint32))
    print(name, "launch", V.compare(f"{name}: nb_launch_eyes_colour", C.eye_reference(oracle, name), *got[:3]))
    TC.assert_same(got, TC.expect(oracle, pos, vel, np.arange(e), skin=skin, **want), f"{name}: nb_launch_eyes_colour against the restatement")

    name = "oblique_96x64_skin"
    c, pos, vel, given, skin = frame_of(oracle, name)
    W, H = c["extent"]
    with nb.Scene(pos, vel) as sc:
        cam = sc.camera_at(c["eye"], c["direction"], c["up"], C.frame_constant(nb, name))
        inst_h = sc.instances().copy()
    ct = torch.from_numpy(np.ascontiguousarray(cam).reshape(16)).to(dev)
    it = torch.from_numpy(inst_h.reshape(len(pos), 16)).to(dev)
    st = torch.from_numpy(skin).to(dev)
    scratch = torch.empty(lib.nb_frame_scratch_bytes(W, H) // 8, dtype=torch.int64, device=dev)
    out = [torch.full((H, W), 7, dtype=torch.int32, device=dev), torch.full((H, W), 7.0, dtype=torch.float32, device=dev),
           torch.full((H, W, 4), 7.0, dtype=torch.float32, device=dev), torch.full((H, W), 7, dtype=torch.int32, device=dev)]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _lib.check(lib.nb_launch_frame(len(pos), ct.data_ptr(), it.data_ptr(), W, H, 0, st.data_ptr(), skin.shape[1], skin.shape[0],
                                       scratch.data_ptr(), *[t.data_ptr() for t in out], s.cuda_stream))
    s.synchronize()
    got = (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy().view(np.uint32))
    print(name, "launch", V.compare(f"{name}: nb_launch_frame", C.frame_reference(oracle, name), *got[:3], axes=("row", "column")))
    TF.assert_same(got, FR.frame(cam, oracle.instances(pos, vel), W, H, skin=skin), f"{name}: nb_launch_frame against the restatement")
