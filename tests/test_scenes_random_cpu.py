"""What tests/test_gpu_scenes_random.py rests on, checked without a GPU on the very cases of tests/scenes_random_cases.py: the two
vision families are not vacuous -- a CAP on the cases in which nobody sees anybody and a floor on the cases with a scene in which most
bodies see somebody, evaluated with the numpy restatements alone --, and every law's default cases reach every workgroup size, both
sides of every line its launcher draws and its hostile kinds."""
import os

import numpy as np
import pytest

import scenes_guard_cases as GK
import scenes_random_cases as C

DEFAULT = 36          # the premises are those of the default cases, whatever NB_RANDOM_CASES says


def test_the_default_and_the_soak_knob():
    assert C.CASES == DEFAULT or "NB_RANDOM_CASES" in os.environ
    a, b = C.case("seen", 3), C.case("seen", 3)
    assert a["line"] == b["line"] and (a["pos"].view(np.uint32) == b["pos"].view(np.uint32)).all()       # seeded
    assert C.case("nbody", 3)["line"] != C.case("nbody", 4)["line"]


@pytest.mark.parametrize("law", ["seen", "located"])
def test_the_vision_cases_are_not_vacuous(oracle, law):
    vacuous, rich = [], []
    for i in range(DEFAULT):
        c = C.case(law, i)
        pos, vel, lists = C.vision_expected(oracle, law, i)
        count = lists[0]                                               # (B, n): what every body sees in the first step
        assert count.shape == (c["batch"], c["n"]) and pos.shape == vel.shape == (c["batch"], c["n"], 3)
        if not count.any():
            vacuous.append(i)
        if any((count[s] > 0).mean() > 0.5 and count[s].max() > 1 for s in range(c["batch"])):
            rich.append(i)
    assert len(vacuous) <= DEFAULT // 4, f"{law}: nobody sees anybody in cases {vacuous}"
    assert len(rich) >= DEFAULT // 4, f"{law}: most bodies see somebody, and some eye several, only in cases {rich}"


@pytest.mark.parametrize("law", ["nbody", "boids"])
def test_the_whole_set_cases_reach_every_workgroup_and_every_kind(law):
    cases = [C.case(law, i) for i in range(DEFAULT)]
    assert all(c["n"] in C.SIZES and c["batch"] in (1, 2, 5) and 1 <= c["k"] <= 3 for c in cases)
    assert {(GK.lanes(c["n"]), c["n"] > 1024) for c in cases} == {(64, False), (128, False), (256, False), (512, False), (1024, False), (1024, True)}
    assert {c["k"] for c in cases} == {1, 2, 3} and {c["batch"] for c in cases} == {1, 2, 5}
    kinds = [[C.scene_kind(p) for p in c["pos"]] for c in cases]
    flat = [k for ks in kinds for k in ks]
    assert any("high" in k for k in flat) and any("low" in k for k in flat)                       # both sides of the guard
    assert any("planar" in k for k in flat) and any("planar" not in k for k in flat)
    typical = [float(np.median(np.abs(p))) for c in cases for p in c["pos"]]
    assert min(typical) < 1e-3 and max(typical) > 1e4                                             # scales 1e-3 .. 1e5
    # one launch holds flagged and unflagged, planar and 3-D scenes
    assert any(any("high" in k for k in ks) and any("high" not in k for k in ks) for ks in kinds)
    assert any(any("planar" in k for k in ks) and any("planar" not in k for k in ks) for ks in kinds)
    for c in cases:
        assert c["pos"].dtype == c["vel"].dtype == np.float32 and c["pos"].shape == (c["batch"], c["n"], 3)


@pytest.mark.parametrize("law", ["seen", "located"])
def test_the_vision_cases_reach_both_sides_of_every_line(law):
    cases = [C.case(law, i) for i in range(DEFAULT)]
    assert all(c["n"] in C.VISION_SIZES and c["width"] in C.VISION_WIDTHS and c["batch"] in (1, 2, 4) and c["k"] in (1, 2) for c in cases)
    sizes, widths = {c["n"] for c in cases}, {c["width"] for c in cases}
    # one wave per eye up to 128 bodies, four above; a second pass over the bodies above 64 and above 256
    assert all(any(lo < n <= hi for n in sizes) for lo, hi in ((0, 64), (64, 128), (128, 256), (256, 2048)))
    assert any(w < 64 for w in widths) and 64 in widths and any(w > 64 for w in widths) and {1, 1024} <= widths
    assert {c["k"] for c in cases} == {1, 2} and {tuple(c["up"]) for c in cases} == {tuple(np.float32(u)) for u in C.VISION_UPS}
    kinds = {k.split(" +-")[0] for c in cases for k in c["kinds"]}
    assert kinds == set(C.VISION_KINDS)                              # "zero velocities" is these laws' hostile kind: NaN cameras
    zero = [c for c in cases if any(k.startswith("zero velocities") for k in c["kinds"])]
    assert all((~c["vel"].any(axis=2)).any() for c in zero)
    assert len({tuple(sorted(c["consts"].items())) for c in cases}) >= (2 if law == "located" else 10)
    assert any(len(set(c["kinds"])) > 1 for c in cases)              # scenes of several kinds in one launch
