"""oracle.step_range_dv_cond_f64 (the binary64 yardstick of tests/test_gpu_fast_binary64.py) against a numpy float64 loop, and the
reference's own binary32 arithmetic (the oracle) inside the bound that file holds every FAST form to, on the same data."""
import numpy as np
import pytest

from test_gpu_fast_binary64 import U, hostile_case


def numpy_dv_cond(pos, first, count, dt, G, bias):
    p = pos.astype(np.float64)
    d = p[None, :, :] - p[first:first + count, None, :]
    r2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + float(bias)
    t = (d * float(G)) / r2[..., None]
    dv = np.zeros((count, 3))
    for j in range(len(pos)):       # index order, as the helper adds
        dv = dv + t[:, j]
    return dv * float(dt), np.abs(t).sum(axis=1)


@pytest.mark.parametrize("case", range(6))
def test_helper_equals_a_numpy_float64_loop(oracle, case):
    _, pos, _, dt, G, bias = hostile_case(case)
    pos = pos[:700]
    first, count = 50, 300
    dv, S = oracle.step_range_dv_cond_f64(pos, first, count, dt, G, bias)
    dv_np, S_np = numpy_dv_cond(pos, first, count, dt, G, bias)
    assert np.array_equal(dv, dv_np) and np.allclose(S, S_np, rtol=1e-12, atol=0)
    # threads split the bodies, never a sum: the same bits on one thread
    dv1, S1 = oracle.step_range_dv_cond_f64(pos, first, count, dt, G, bias, threads=1)
    assert np.array_equal(dv, dv1) and np.array_equal(S, S1)
    # the default constants are the binary32 roundings of the reference's
    assert np.array_equal(oracle.step_range_dv_cond_f64(pos, 0, 5)[0],
                          oracle.step_range_dv_f64(pos, 0, 5, float(oracle.DT), float(oracle.G), float(oracle.BIAS)))


@pytest.mark.parametrize("case", range(12))
def test_reference_arithmetic_meets_the_bound(oracle, case):
    what, pos, vel, dt, G, bias = hostile_case(case)
    n = len(pos)
    dv64, S = oracle.step_range_dv_cond_f64(pos, 0, n, dt, G, bias)
    _, v = oracle.run(pos, vel, 1, dt, G, bias)
    v_true = vel.astype(np.float64) + dv64
    err = np.abs(v.astype(np.float64) - v_true)
    ulp = np.spacing(np.maximum(np.abs(v_true), np.abs(v)).astype(np.float32)).astype(np.float64)
    bound = abs(float(dt)) * (n + 16) * U * S + ulp
    assert (err <= bound).all(), f"{what}: {(err > bound).sum()} components beyond the bound"
