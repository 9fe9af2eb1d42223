"""STRICT's divide guard on the device, where a missed flag or a corner must show.  Bit-exact throughout: no tolerances.

Family A -- corners inside the guard.  Every launch shape restates the shared-reciprocal ladder for itself (pair_strict, the j-packed
pair2_strict of the tiled and producer/consumer forms, the rows of the scalar-load form, the block chain's copy); here each meets
coordinates on the corners of {0} U [2^a, 2^b], where d, n = dx*G and q = n/d reach the extreme exponents the guard admits
(tests/guard_corners.py; the attained exponents are asserted in tests/test_guard_corners_cpu.py).  The first step is all ladder; by
the second some bodies have left the range, so it runs the hand-over to '/'.

Family B -- one outlier at a time.  One coordinate of one body is 2^64, -2^70 or 2^100, at the places a flag can be forgotten: a
workgroup's own first and last body, a tile's first and last record, the ragged last tile.  dx*dx overflows, d = +inf; '/' gives
+/-0, the ladder gives fma(-inf, rcp(inf) = 0, 1) = NaN.  The reference's result is finite on every case (CPU file), so the
comparison is plain and one NaN is a missed flag.  The value x component grid is thinned as guard_corners.outlier_cases says.

Family C -- FAST with an overflowing pair: two such bodies, every FAST form, the binary64 bounds of test_gpu_fast_binary64 unchanged.
"""
import numpy as np
import pytest

import guard_corners as gc
from test_gpu_fast_binary64 import FORMS, check_bodies, fast_step_velocities
from test_gpu_parity import _sharded_step_on_one_gpu, assert_bits_equal

pytestmark = pytest.mark.gpu

_references = {}


def reference(oracle, key, make):
    """oracle results shared by the forms: computed once per case, never written to"""
    if key not in _references:
        out = make()
        for a in out:
            for x in a:
                x.setflags(write=False)
        _references[key] = out
    return _references[key]


def strict_params(nb, G, bias, dt=gc.CORNER_DT):
    params = nb.default_params()
    params.dt, params.G, params.bias = float(dt), float(G), float(bias)
    return params


def consts(G, bias, dt=gc.CORNER_DT):
    return np.float32(dt), np.float32(G), np.float32(bias)


# ---- family A ---------------------------------------------------------------------------------------------------------------------
def corner_case(oracle, case):
    """((pos, vel), (p1, v1), (p2, v2)): the data of a pair of constants and the reference after one and two steps"""
    def make():
        G, bias = case
        a, b = gc.guard(G, bias)[:2]
        pos, vel = gc.corner_state(gc.CORNER_N, a, b, seed=gc.CORNER_CONSTANTS.index(case))
        return (pos, vel), oracle.run(pos, vel, 1, *consts(G, bias)), oracle.run(pos, vel, 2, *consts(G, bias))
    return reference(oracle, ("corner", case), make)


@pytest.mark.parametrize("case", gc.CORNER_CONSTANTS, ids=gc.corner_id)
@pytest.mark.parametrize("form", gc.STRICT_FORMS, ids=str)
def test_strict_on_the_guards_corners_bit_exact(nb, oracle, monkeypatch, form, case):
    (pos, vel), (p_ref, v_ref), _ = corner_case(oracle, case)
    gc.apply(monkeypatch, form, strict_params(nb, *case), len(pos), [len(pos)])
    with nb.Scene(pos, vel, strict_params(nb, *case)) as sc:
        sc.step_n(1)
        p, v = sc.state()
    assert_bits_equal(v, v_ref, f"velocities, form {form}, (G, bias) = {case}")
    assert_bits_equal(p, p_ref, f"positions, form {form}, (G, bias) = {case}")


@pytest.mark.parametrize("case", gc.CORNER_TWO_STEPS, ids=gc.corner_id)
@pytest.mark.parametrize("form", gc.STRICT_FORMS, ids=str)
def test_strict_second_step_from_the_corners_hands_over_bit_exact(nb, oracle, monkeypatch, form, case):
    (pos, vel), _, (p_ref, v_ref) = corner_case(oracle, case)
    gc.apply(monkeypatch, form, strict_params(nb, *case), len(pos), [len(pos)])
    with nb.Scene(pos, vel, strict_params(nb, *case)) as sc:
        sc.step_n(2)
        p, v = sc.state()
    assert_bits_equal(v, v_ref, f"velocities, form {form}, (G, bias) = {case}")
    assert_bits_equal(p, p_ref, f"positions, form {form}, (G, bias) = {case}")


@pytest.mark.parametrize("case", [gc.CORNER_CONSTANTS[0], (0.3, 2.0 ** -100)], ids=gc.corner_id)
@pytest.mark.parametrize("parts", [[(0, 1), (1, 255), (256, 1281)], [(0, 769), (769, 768)]], ids=["1+255+1281", "769+768"])
@pytest.mark.parametrize("form", ["default", 1, 16, "pc14", "bc", "sl"], ids=str)
def test_strict_shards_on_the_guards_corners_bit_exact(nb, oracle, monkeypatch, form, parts, case):
    (pos, vel), (p1, v1), (p2, v2) = corner_case(oracle, case)
    assert sum(count for _, count in parts) == len(pos)
    gc.apply(monkeypatch, form, strict_params(nb, *case), len(pos), [count for _, count in parts])
    for steps, p_ref, v_ref in ((1, p1, v1), (2, p2, v2)):
        p, v = _sharded_step_on_one_gpu(nb, pos.copy(), vel.copy(), parts, strict_params(nb, *case), steps)
        assert_bits_equal(v, v_ref, f"velocities after {steps}, form {form}, parts {parts}, (G, bias) = {case}")
        assert_bits_equal(p, p_ref, f"positions after {steps}, form {form}, parts {parts}, (G, bias) = {case}")


# ---- family B ---------------------------------------------------------------------------------------------------------------------
def outlier_id(case):
    index, value, component, planar = case[:4]
    return f"body{index}_{'xyz'[component]}{'+-'[value < 0]}2p{int(np.log2(abs(value)))}{'_planar' if planar else ''}"


def outlier_case(oracle, index, value, component, planar, steps):
    def make():
        pos, vel = gc.outlier_state(oracle, index, value, component, planar)
        return (pos, vel), oracle.run(pos, vel, steps)
    return reference(oracle, ("outlier", index, value, component, planar, steps), make)


@pytest.mark.parametrize("case", gc.outlier_cases(), ids=outlier_id)
@pytest.mark.parametrize("form", gc.STRICT_FORMS, ids=str)
def test_strict_one_outlier_bit_exact(nb, oracle, monkeypatch, form, case):
    (pos, vel), (p_ref, v_ref) = outlier_case(oracle, *case, gc.OUTLIER_STEPS)
    gc.apply(monkeypatch, form, nb.default_params(), len(pos), [len(pos)])
    with nb.Scene(pos, vel) as sc:
        sc.step_n(gc.OUTLIER_STEPS)
        p, v = sc.state()
    assert_bits_equal(v, v_ref, f"velocities, form {form}, {outlier_id(case)}")
    assert_bits_equal(p, p_ref, f"positions, form {form}, {outlier_id(case)}")


@pytest.mark.parametrize("case", gc.outlier_shard_cases(), ids=lambda c: f"{c[0]}_{outlier_id(c[2:5] + (False,))}")
@pytest.mark.parametrize("form", gc.STRICT_FORMS, ids=str)
def test_strict_one_outlier_in_shards_bit_exact(nb, oracle, monkeypatch, form, case):
    name, parts, index, value, component, steps = case
    (pos, vel), (p_ref, v_ref) = outlier_case(oracle, index, value, component, False, steps)
    gc.apply(monkeypatch, form, nb.default_params(), len(pos), [count for _, count in parts])
    p, v = _sharded_step_on_one_gpu(nb, pos.copy(), vel.copy(), parts, nb.default_params(), steps)
    own = np.concatenate([np.arange(first, first + count) for first, count in parts])
    assert_bits_equal(v, v_ref[own], f"velocities, form {form}, {name}")
    assert_bits_equal(p[own], p_ref[own], f"positions, form {form}, {name}")


# ---- family C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_fast_with_an_overflowing_pair_within_the_binary64_bound(nb, oracle, monkeypatch, form):
    pos, vel, dt, G, bias = gc.fast_overflow_state()
    v = fast_step_velocities(nb, monkeypatch, form, pos, vel, dt, G, bias)
    check_bodies(f"{form}: two bodies at 2^64 and -2^70", pos, vel, v, dt, G, bias, oracle)
