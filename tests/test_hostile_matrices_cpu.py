"""The corpus of arbitrary caller matrices (tests/hostile_matrices.py) without a GPU.

(a) What the corpus covers, from the numpy restatements alone: conditions on the inputs that tests/test_gpu_hostile_matrices.py rests
    on -- every drawing class on the screen, depths clamped to +0 and rejected at 1, edges dropped for w <= 0 and cut by each of the
    four boundaries, exact ties held by the lower index, spans and edges longer than a wave round, every edge index shading.
(b) The same corpus through the device functions compiled for the host (tests/cpp/eyes_msaa_host.cpp, tests/cpp/frame_msaa_host.cpp),
    one-sample and 8-sample mode, every word against the restatements; and through the same two stand-alone programs built with
    -fsanitize=address,undefined,float-cast-overflow: a float -> integer conversion of an out-of-range or NaN value, which g++ and
    the device may answer differently, stops them.
(c) The control arm: the drivers built to compute in x87 extended precision (products and sums no longer rounded to binary32 at
    each step, the way a contracted multiply-add is not) differ from the restatements somewhere in every view: the corpus can fail.
"""
import os
import subprocess

import numpy as np
import pytest

import eyes_restatement as R
import hostile_matrices as HM
from conftest import ROOT

F = np.float32
CSRC = os.path.join(ROOT, "nenbody_amd", "csrc")
BUILD = os.path.join(ROOT, "build", "hostile_matrices")
PLAIN = ["-O1", "-ffp-contract=off", "-msse2", "-mfpmath=sse"]
BUILDS = {
    "plain": PLAIN,
    "sanitized": PLAIN + ["-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"],
    "x87": ["-O1", "-ffp-contract=off", "-mfpmath=387"],
}
# the four views of the issue; the one-sample eye row stands for nb_launch_eyes and nb_launch_eyes_colour (the same keys)
VIEWS = ("eyes_colour", "eyes_msaa", "frame", "frame_msaa")


@pytest.fixture(scope="module")
def hosts():
    """the two drivers in the three builds: {(driver, build): path}"""
    os.makedirs(BUILD, exist_ok=True)
    out = {}
    for driver in ("eyes_msaa_host", "frame_msaa_host"):
        for build, flags in BUILDS.items():
            exe = os.path.join(BUILD, f"{driver}_{build}")
            subprocess.run(["g++", "-std=c++17"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", driver + ".cpp"), "-o", exe], check=True)
            out[driver, build] = exe
    return out


def cases_of(oracle, view):
    return [c for c in (HM.eye_cases(oracle) if view.startswith("eyes") else HM.frame_cases(oracle)) if view in c["views"]]


def run_host(exe, tmp_path, view, c):
    """the driver's four outputs as uint32 words, shaped as the restatement's"""
    skin = c["skin"]
    th, tw = skin.shape[:2] if skin is not None else (0, 0)
    (skin if skin is not None else np.zeros(4, F)).astype(F).tofile(tmp_path / "skin.bin")
    c["inst"].tofile(tmp_path / "inst.bin")
    one = ["one"] if view in ("eyes_colour", "frame") else []
    k = 1 if one else 8
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    if view.startswith("eyes"):
        c["cams"].tofile(tmp_path / "cams.bin")
        E, W = len(c["cams"]), c["width"]
        r = subprocess.run([exe, str(E), str(len(c["inst"])), str(c["first"]), str(W), str(int(c["see_self"])), str(tw), str(th),
                            str(tmp_path / "cams.bin"), str(tmp_path / "inst.bin"), str(tmp_path / "skin.bin"), str(tmp_path / "out.bin")] + one,
                           capture_output=True, text=True, env=env)
        assert r.returncode == 0, f"{view} {c['name']}: exit {r.returncode}\n{r.stderr[-3000:]}"
        raw = np.fromfile(tmp_path / "out.bin", np.uint32).reshape(E, -1)
        a, b, rg, bg = np.split(raw, [k * W, 2 * k * W, (2 * k + 4) * W], axis=1)
        shape = (E, W) if one else (E, W, 8)
        return a.reshape(shape), b.reshape(shape), rg.reshape(E, W, 4), bg
    W, H = c["extent"]
    np.ascontiguousarray(c["cam"], F).tofile(tmp_path / "cam.bin")
    r = subprocess.run([exe, str(len(c["inst"])), str(W), str(H), str(tw), str(th), str(tmp_path / "cam.bin"), str(tmp_path / "inst.bin"),
                        str(tmp_path / "skin.bin"), str(tmp_path / "out.bin")] + one, capture_output=True, text=True, env=env)
    assert r.returncode == 0, f"{view} {c['name']}: exit {r.returncode}\n{r.stderr[-3000:]}"
    raw = np.fromfile(tmp_path / "out.bin", np.uint32)
    a, b, rg, bg = np.split(raw, [k * W * H, 2 * k * W * H, (2 * k + 4) * W * H])
    shape = (H, W) if one else (H, W, 8)
    return a.reshape(shape), b.reshape(shape), rg.reshape(H, W, 4), bg.reshape(H, W)


def differing(got, want):
    """per output, the number of words that differ"""
    return [int((g != HM.words(w)).sum()) for g, w in zip(got, want)]


# -- (a) what the corpus covers ------------------------------------------------------------------------------------------------------------
def test_the_classes_interleave_and_the_duplicates_are_exact(oracle):
    for c in HM.eye_cases(oracle) + HM.frame_cases(oracle):
        assert (c["cls"] == np.arange(len(c["cls"])) % len(HM.CLASSES)).all()                   # every class within the first wave
        dups = np.nonzero(c["cls"] == HM.CLASSES.index("duplicate"))[0]
        for j in dups:
            src = HM.duplicate_source(j)
            assert src < j and HM.CLASSES[c["cls"][src]] in HM.DRAWING
            assert (HM.words(c["inst"][j]) == HM.words(c["inst"][src])).all()
    n300 = [c for c in HM.eye_cases(oracle) + HM.frame_cases(oracle) if len(c["inst"]) == HM.N]
    assert len(n300) >= 18
    c = HM.eye_cases(oracle)[0]
    assert len(c["cams"]) == HM.EYES and c["first"] == HM.FIRST
    assert {bool(e["see_self"]) for e in HM.eye_cases(oracle)} == {False, True}
    assert {e["skin"] is None for e in HM.eye_cases(oracle)} == {False, True} == {f["skin"] is None for f in HM.frame_cases(oracle)}


@pytest.mark.parametrize("view", VIEWS)
def test_coverage_of_the_corpus(oracle, view):
    """conditions on the inputs, summed over the cases of one view (what this corpus gives is in the comments)"""
    cases = cases_of(oracle, view)
    drawn = zero = 0
    wins = np.zeros(len(HM.CLASSES), np.int64)
    cut, edge = np.zeros(4, np.int64), np.zeros(3, np.int64)
    w_dropped = far = widest = longest_x = longest_y = 0
    for c in cases:
        ids, depth = HM.expected(view, c)[:2]
        st = HM.stats(view, c)
        on = ids != R.NONE
        drawn += int(on.sum())
        wins += np.bincount(c["cls"][ids[on]], minlength=len(HM.CLASSES))
        zero += int((HM.words(depth)[on] == 0).sum())
        cut += st["cut"]
        edge += st["edge"]
        w_dropped += st["w_dropped"]
        far += st["rejected_far"]
        widest = max(widest, st.get("widest", 0))
        longest_x, longest_y = max(longest_x, st.get("longest_x", 0)), max(longest_y, st.get("longest_y", 0))
    assert drawn >= 1000, drawn                               # 2 439 / 75 690 / 8 988 / 71 581 non-empty words
    for name in HM.DRAWING:
        assert wins[HM.CLASSES.index(name)] >= 1, (name, wins)
    assert wins[HM.CLASSES.index("duplicate")] == 0           # a duplicate never holds a pixel: its source ties and is lower
    assert zero >= 1                                          # the clamp to +0
    assert far >= 1                                           # a candidate rejected for d >= 1
    assert w_dropped >= 1                                     # an edge dropped for w <= 0 after the clip
    assert (cut >= 1).all(), cut                              # an edge cut by each of the four boundaries
    assert (edge >= 1).all(), edge                            # every edge index shades somewhere
    if view.startswith("eyes"):
        assert widest > 72, widest                            # an own-lane share and more than one round of the wave
    else:
        assert longest_x > 72 and longest_y > 72, (longest_x, longest_y)


@pytest.mark.parametrize("view,name", [("eyes_colour", "W65-self1"), ("eyes_msaa", "W65-self1"), ("frame", "64x32-pushed"),
                                       ("frame_msaa", "64x32-pushed")])
def test_a_duplicate_ties_with_its_source_and_the_lower_index_holds_the_pixel(oracle, view, name):
    """the higher index would have tied: with the sources taken out (NaN matrices) their duplicates hold the same words at the same
    depth bits, unless a body between the two ties as well"""
    c = HM.case(oracle, name)
    dups = np.nonzero(c["cls"] == HM.CLASSES.index("duplicate"))[0]
    src = np.array([HM.duplicate_source(j) for j in dups])
    ids, depth = HM.expected(view, c)[:2]
    without = c["inst"].copy()
    without[src] = np.nan
    ids2, depth2 = HM.restate(view, c, without)[:2]
    held = np.isin(ids, src)
    back = np.full(len(c["inst"]), -1, np.int64)
    back[src] = dups
    taken = held & (ids2 == back[np.where(held, ids, src[0])]) & (HM.words(depth) == HM.words(depth2))
    assert held.sum() >= 10 and taken.sum() >= 10, (int(held.sum()), int(taken.sum()))
    assert not np.isin(ids, dups).any()


# -- (b) the host-compiled device functions, plain and under the sanitizers ------------------------------------------------------------------
@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("name", HM.EYE_NAMES)
def test_the_eye_rows_through_the_host_driver(oracle, hosts, tmp_path, name, build):
    c = HM.case(oracle, name)
    for view in ("eyes_colour", "eyes_msaa"):
        if view in c["views"]:
            got = run_host(hosts["eyes_msaa_host", build], tmp_path, view, c)
            assert differing(got, HM.expected(view, c)) == [0, 0, 0, 0], (view, name, build)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("name", HM.FRAME_NAMES)
def test_the_frames_through_the_host_driver(oracle, hosts, tmp_path, name, build):
    c = HM.case(oracle, name)
    for view in ("frame", "frame_msaa"):
        got = run_host(hosts["frame_msaa_host", build], tmp_path, view, c)
        assert differing(got, HM.expected(view, c)) == [0, 0, 0, 0], (view, name, build)


# -- (c) the control arm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", VIEWS)
def test_the_extended_precision_build_differs_somewhere(oracle, hosts, tmp_path, view):
    """the same drivers computing in x87 registers: a step is no longer one binary32 operation (a product that overflows or goes
    subnormal in binary32 does neither there, a sum is rounded twice), and the corpus shows it in every view"""
    driver = "eyes_msaa_host" if view.startswith("eyes") else "frame_msaa_host"
    total = np.zeros(4, np.int64)
    for c in cases_of(oracle, view):
        total += differing(run_host(hosts[driver, "x87"], tmp_path, view, c), HM.expected(view, c))
    print(f"{view}: x87 build differs in {total.tolist()} words (ids, depth, rgba, bgra8)")
    assert total[0] >= 1 and total[1] >= 1 and total[2] >= 1, total
