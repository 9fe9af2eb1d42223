"""STRICT's divide guard in scenes_nbody_kernel (nb_scenes.inc), where a missed flag or a corner must show.  Bit-exact throughout.

The kernel is a launch shape of STRICT with flag logic of its own (tests/scenes_guard_cases.py says which, and builds the data).
Every batch goes through nb_scenes_nbody_step_launch between two guard scenes of NaN records (test_gpu_scenes.launch) and is
compared word for word with scenes_restatement.nbody -- the C oracle scene by scene -- under the case's constants:

  * corner batches: coordinates on the corners of {0} U [2^a, 2^b] under gc.CORNER_CONSTANTS at every workgroup size; one step is all
    ladder (fold_tile_strict<..., U, 1> with U = 8, and U = 4 at 1 024 lanes), the second hands over to '/';
  * outlier batches: one coordinate of 2^64, -2^70 or 2^100 at every place a flag can be forgotten, one scene per place.  The
    reference is finite on every scene (tests/test_scenes_guard_cpu.py), so one NaN in the device's result is a missed flag;
  * velocity batches: the outlier in the velocity, so that the flag arises in the record step 1 writes;
  * the grid-stride batch: outlier scenes and clean scenes taking turns in one workgroup.
A failure names the shape, the constants or the place, the scene and the body.

What is sharp: the outlier, velocity and grid-stride batches -- builds of the kernel with one wave's word not read, the per-step words
not rewritten or a lane's second body not flagged per step each failed them at every shape they touch.  The corner batches hold the
ladder itself at the extreme exponents; their second step is NOT a witness for a forgotten flag (the same builds passed them: a
coordinate that leaves the range without overflowing d still gets the reference's bits on this data)."""
import numpy as np
import pytest

import guard_corners as gc
import scenes_guard_cases as K
import scenes_restatement as R
from seen_cases import same_words
from test_gpu_scenes import launch

pytestmark = pytest.mark.gpu

_references = {}


def reference(key, make):
    """oracle results, computed once per case and never written to"""
    if key not in _references:
        out = make()
        for a in out:
            a.setflags(write=False)
        _references[key] = out
    return _references[key]


def assert_batch(got, want, what, where=None):
    """every word of every scene; `where`: {scene: text} naming what the scene holds"""
    for g, w, name in zip(got, want, ("positions", "velocities")):
        batch, n = w.shape[:2]
        ok, rows = same_words(g[:, :, :3].reshape(batch * n, 3), w.reshape(batch * n, 3))
        if not ok:
            bad = [divmod(int(r), n) for r in rows]
            scenes = sorted({s for s, _ in bad})
            held = "; ".join(f"scene {s}: {(where or {}).get(s, 'clean')}" for s in scenes[:4])
            raise AssertionError(f"{what}: {name} of {len(rows)} of {batch * n} bodies differ, first (scene, body) {bad[:6]} ({held})")


def corner_reference(oracle, case, n, k):
    def make():
        pos, vel = K.corner_batch(case, n)
        return R.nbody(oracle, pos, vel, k, **K.corner_constants(case))
    return reference(("corner", case, n, k), make)


# ---- corner batches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", K.corner_grid(), ids=K.corner_id)
def test_corner_batches_bit_exact(nb, oracle, item):
    case, n = item
    pos, vel = K.corner_batch(case, n)
    for k in K.corner_steps(case):
        got = launch(nb, "nbody", pos, vel, k, K.corner_params(nb, case))
        assert_batch(got, corner_reference(oracle, case, n, k), f"n={n} (G, bias)={case} seeds={K.corner_seeds(case)} k={k}")


@pytest.mark.parametrize("case", [gc.CORNER_CONSTANTS[4], gc.CORNER_CONSTANTS[8]], ids=gc.corner_id)
@pytest.mark.parametrize("n", [300, 1537])
def test_corner_batches_one_launch_of_two_steps_is_two_launches_of_one(nb, oracle, case, n):
    """the second step's flags come from LDS words in one launch and from the records read back in two: the same bits, the reference's"""
    pos, vel = K.corner_batch(case, n)
    once = launch(nb, "nbody", pos, vel, 2, K.corner_params(nb, case))
    twice = launch(nb, "nbody", pos, vel, 1, K.corner_params(nb, case), launches=2)
    want = corner_reference(oracle, case, n, 2)
    assert_batch(once, want, f"n={n} (G, bias)={case}: one launch of k=2")
    assert_batch(twice, want, f"n={n} (G, bias)={case}: two launches of k=1")
    for a, b in zip(once, twice):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()


# ---- outlier and velocity batches -----------------------------------------------------------------------------------------------------
def place_texts(where, kind):
    return {s: f"{kind} {'xyz'[c]} of body {body} = {'-' if v < 0 else ''}2^{int(np.log2(abs(v)))}" for s, body, v, c in where}


@pytest.mark.parametrize("n", K.SHAPES)
def test_one_outlier_at_every_place_bit_exact(nb, oracle, n):
    pos, vel, where = K.outlier_batch(oracle, n)
    want = reference(("outlier", n), lambda: R.nbody(oracle, pos, vel, K.OUTLIER_STEPS))
    got = launch(nb, "nbody", pos, vel, K.OUTLIER_STEPS)
    assert_batch(got, want, f"n={n}, one outlier per scene", place_texts(where, "position"))
    for g, w in zip(got, want):                                          # the clean scenes around them, said apart
        assert (g[[0, -1], :, :3].view(np.uint32) == w[[0, -1]].view(np.uint32)).all()


@pytest.mark.parametrize("n", K.SHAPES)
def test_one_velocity_outlier_at_every_place_flags_mid_launch(nb, oracle, n):
    pos, vel, where = K.velocity_batch(oracle, n)
    want = reference(("velocity", n), lambda: R.nbody(oracle, pos, vel, K.VELOCITY_STEPS))
    got = launch(nb, "nbody", pos, vel, K.VELOCITY_STEPS)
    assert_batch(got, want, f"n={n}, one velocity outlier per scene", place_texts(where, "velocity"))
    for g, w in zip(got, want):
        assert (g[[0, -1], :, :3].view(np.uint32) == w[[0, -1]].view(np.uint32)).all()


# ---- the grid-stride loop -------------------------------------------------------------------------------------------------------------
def test_outlier_and_clean_scenes_take_turns_in_one_workgroup(nb, oracle):
    pos, vel, where = K.grid_stride_batch(oracle)
    want = R.nbody(oracle, pos, vel, K.GRID_STEPS)
    got = launch(nb, "nbody", pos, vel, K.GRID_STEPS)
    assert_batch(got, want, f"{len(pos)} scenes of {K.GRID_N}", place_texts(where, "position"))


# ---- the context ----------------------------------------------------------------------------------------------------------------------
def test_context_steps_an_outlier_batch_and_a_corner_batch(nb, oracle):
    """SceneBatch: the outlier batch of 300 bodies in two calls of one step, and a corner batch under its constants in one call of two"""
    pos, vel, where = K.outlier_batch(oracle, 300)
    want = reference(("outlier", 300), lambda: R.nbody(oracle, pos, vel, K.OUTLIER_STEPS))
    assert K.OUTLIER_STEPS == 2
    with nb.SceneBatch(pos, vel) as sb:
        sb.step(1)
        sb.step(1)
        got = sb.positions(), sb.velocities()
    assert_batch(got, want, "SceneBatch, n=300, one outlier per scene", place_texts(where, "position"))
    case, n = gc.CORNER_CONSTANTS[4], 1537
    pos, vel = K.corner_batch(case, n)
    with nb.SceneBatch(pos, vel, K.corner_params(nb, case)) as sb:
        sb.step(2)
        got = sb.positions(), sb.velocities()
    assert_batch(got, corner_reference(oracle, case, n, 2), f"SceneBatch, n={n} (G, bias)={case}")
