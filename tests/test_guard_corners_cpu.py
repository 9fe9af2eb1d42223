"""What tests/test_gpu_guard_corners.py rests on, checked without a GPU: the restated guard against the recorded plan table, the
corner data against the extremes it claims to reach, and the reference's results on every case finite -- so that the GPU tests
may compare bits plainly and a NaN there is the device's own."""
import os
import struct

import numpy as np
import pytest

import guard_corners as gc
from conftest import GOLDEN_DIR


def f32(h):
    return struct.unpack("<f", struct.pack("<I", int(h, 16)))[0]


def recorded_guards():
    """{(G word, bias word): (lo, hi, ieee)} of every STRICT line of the plan table that plans, without the knob that forces '/'"""
    out = {}
    with open(os.path.join(GOLDEN_DIR, "plan_table.txt")) as f:
        for line in f:
            case, results = line.rstrip("\n").split(" => ")
            d = dict(t.split("=", 1) for t in case.split())
            if d["mode"] != "0" or "NB_STRICT_FORCE_IEEE" in d or not results.startswith("rc=0 "):
                continue
            r = dict(t.split("=", 1) for t in results.split(" plan=")[0].split()[1:])
            words = (int(r["lo"], 16), int(r["hi"], 16), int(r.get("ieee", "0")))
            assert out.setdefault((d["G"], d["bias"]), words) == words, line
    return out


def test_the_restated_guard_gives_the_plan_tables_words():
    rec = recorded_guards()
    assert len(rec) == 17 and sum(w[2] for w in rec.values()) == 10
    for (G, bias), words in rec.items():
        assert gc.guard_words(f32(G), f32(bias)) == words, (G, bias)
        gd = gc.guard(f32(G), f32(bias))
        assert (gd is None) == (words[2] == 1)
        if gd is not None:
            a, b, g, c, dmax = gd
            assert 2.0 ** g <= abs(f32(G)) < 2.0 ** (g + 1) and 2.0 ** c <= f32(bias) < 2.0 ** (c + 1) and -120 <= a < b == gc.B


def test_every_form_of_the_lanes_fixture_is_carried():
    assert gc.STRICT_FORMS[:11] == [1, "1np", 2, 4, 8, 16, "pc8", "pc14", "pc14np", "bc", "sl"] and gc.STRICT_FORMS[11:] == ["sl2", "sl3", "default"]
    assert gc.form_env("sl3") == {"NB_STRICT_SL": "3", "NB_STRICT_BC": "0"} and gc.form_env("sl") == {"NB_STRICT_SL": "1", "NB_STRICT_BC": "0"}
    assert gc.form_env("pc14np") == {"NB_STRICT_NO_PACKED": "1", "NB_STRICT_PC": "14"} and gc.form_env("default") == {}


def test_every_pinned_form_plans_its_kernel_at_the_tests_sizes(nb, monkeypatch):
    """without a device: the knobs of every form but "default" decide the kernel for the whole sets and every shard of the GPU tests"""
    shard_counts = {count for case in gc.outlier_shard_cases() for _, count in case[1]}
    for form in gc.STRICT_FORMS:
        gc.apply(monkeypatch, form, nb.default_params(), gc.CORNER_N, [gc.CORNER_N, 1, 255, 1281, 769, 768])
        gc.apply(monkeypatch, form, nb.default_params(), gc.OUTLIER_N, [gc.OUTLIER_N] + sorted(shard_counts))
    assert {gc.form_kernel(f) for f in gc.STRICT_FORMS} == {None, "step_strict_kernel", "step_strict_pc_kernel", "step_strict_bc_kernel",
                                                            "step_strict_sl_kernel"}


# (d_lo, d_hi, n_lo, n_hi) each case must attain: d in [c, 2b+3] and n in [a-23+g, b+g+1], but for bias 2^61, where 3*2^42 + 2^61 < 2^62
ATTAINED = {
    (0.001, 1e-7): (-24, 43, -76, 11),
    (-0.001, 1e-7): (-24, 43, -76, 11),
    (0.001, 2.0 ** 61): (61, 61, -57, 11),
    (0.001, 2.0 ** -100): (-100, 43, -76, 11),
    (0.3, 2.0 ** -100): (-100, 43, -76, 19),
    (2.0 ** 30, 1.0): (0, 43, -76, 51),
    (-2.0, 3.0): (1, 43, -76, 22),
    (2.0 ** -60, 2.0 ** -20): (-20, 43, -76, -39),
    (2.0 ** -72, 2.0 ** -20): (-20, 43, -76, -51),
    (2.0 ** 100, 4.0): (2, 43, -43, 121),
}


@pytest.mark.parametrize("seed,case", list(enumerate(gc.CORNER_CONSTANTS)), ids=lambda x: gc.corner_id(x) if isinstance(x, tuple) else str(x))
def test_corner_data_is_in_range_reaches_the_extremes_and_stays_finite(oracle, seed, case):
    G, bias = case
    a, b, g, c, _ = gc.guard(G, bias)
    assert (0.3, 2.0 ** -100) != case or b + 2 + g - c == 120
    assert (2.0 ** -60, 2.0 ** -20) != case or a == 7
    pos, vel = gc.corner_state(gc.CORNER_N, a, b, seed)
    mag = np.abs(pos)
    assert ((mag == 0) | ((mag >= np.float32(2.0 ** a)) & (mag <= np.float32(2.0 ** b)))).all()
    assert (mag == 0).all(axis=1).any() and ((pos[:, 2] == 0) & (pos[:, 0] != 0)).any()
    assert len(np.unique(pos, axis=0)) < len(pos) - (mag == 0).all(axis=1).sum()   # coincident bodies besides those at the origin
    want = gc.expected_coverage(G, bias)
    assert want == ATTAINED[case]
    if bias != 2.0 ** 61:
        assert want == (c, 2 * b + 3, a - 23 + g, b + g + 1)
    assert gc.coverage(pos, G, bias) == want
    consts = (np.float32(gc.CORNER_DT), np.float32(G), np.float32(bias))
    p1, v1 = oracle.run(pos, vel, 1, *consts)
    assert np.isfinite(p1).all() and np.isfinite(v1).all()
    if case in gc.CORNER_TWO_STEPS:
        m1 = np.abs(p1)
        assert (~((m1 == 0) | ((m1 >= np.float32(2.0 ** a)) & (m1 <= np.float32(2.0 ** b))))).any()   # the second step hands over to '/'
        p2, v2 = oracle.run(pos, vel, 2, *consts)
        assert np.isfinite(p2).all() and np.isfinite(v2).all()


def test_the_outlier_values_leave_every_guard_and_overflow_the_square():
    for value in gc.OUTLIER_VALUES:
        v = np.float32(value)
        with np.errstate(over="ignore"):
            assert np.isfinite(v) and np.isinf(v * v) and abs(value) >= 2.0 ** 64 > 2.0 ** gc.B


def assert_reference_finite_and_outlier_still(oracle, pos, vel, index, steps):
    for k in range(1, steps + 1):
        p, v = oracle.run(pos, vel, k)
        assert np.isfinite(p).all() and np.isfinite(v).all(), k
        assert (v[index].view(np.uint32) == vel[index].view(np.uint32)).all()   # every term of the outlier's own sum is +/-0


def test_the_reference_is_finite_on_every_outlier_case(oracle):
    cases = gc.outlier_cases()
    assert len(cases) == 28
    assert {(c[0], c[1]) for c in cases if not c[3]} == {(i, v) for i in gc.OUTLIER_INDICES for v in gc.OUTLIER_VALUES}
    assert {(c[0], c[2]) for c in cases if not c[3]} == {(i, k) for i in gc.OUTLIER_INDICES for k in (0, 2)}
    assert {c[0] for c in cases if c[3]} == set(gc.OUTLIER_INDICES)
    for index, value, component, planar in cases:
        pos, vel = gc.outlier_state(oracle, index, value, component, planar)
        assert planar == bool((pos[:, 2] == 0).all())
        assert_reference_finite_and_outlier_still(oracle, pos, vel, index, gc.OUTLIER_STEPS)
    for _, parts, index, value, component, steps in gc.outlier_shard_cases():
        pos, vel = gc.outlier_state(oracle, index, value, component)
        assert all(first + count <= len(pos) for first, count in parts)
        assert_reference_finite_and_outlier_still(oracle, pos, vel, index, steps)


def test_the_reference_alone_meets_the_fast_bounds_with_an_overflowing_pair(oracle):
    """Family C's premise: in binary64 the terms with the two far bodies are merely tiny, so check_bodies' bounds apply unchanged."""
    from test_gpu_fast_binary64 import check_bodies

    pos, vel, dt, G, bias = gc.fast_overflow_state()
    assert len(pos) == gc.FAST_N and sorted(np.abs(pos).max(axis=1))[-2:] == [2.0 ** 64, 2.0 ** 70]
    _, v_ref = oracle.step_range(pos, vel, 0, len(pos), dt, G, bias)
    check_bodies("the reference itself", pos, vel, v_ref, dt, G, bias, oracle)
