"""FAST per body against binary64, on data built to hurt: every body, every component, a bound derived from the arithmetic.

For body i and component k let t_ij be the exact terms ((p_j - p_i) G) / (|p_j - p_i|^2 + bias) of the binary32 snapshot with the
binary32 constants, a64 = sum_j t_ij and S_i = sum_j |t_ij| (oracle.step_range_dv_cond_f64).  Any binary32 form of the step obeys

    |v^ - (v0 + dt a64)| <= |dt| (n + 16) u S_i + ulp(v),        u = 2^-24

  * summation: any tree of n terms in binary32 is off by at most gamma_(n-1) sum |t^_ij| <= (n - 1) u S_i (1 + O(nu))
    [Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2]; the ring's received sums and the slices'
    partial sums are subtrees of such a tree;
  * each term carries at most ~12 roundings of its own: d (1), the three fused squares into r^2 (2 from d, 3 adds), v_rcp_f32
    (1 ulp = 2u), the shared reciprocal's product and back-multiplication (2 + the rcp of the product, 2u), d * inv (1) -- 12 u;
  * the sum's product with G (1) and dt (1): 2 u S_i;
  * (n - 1) + 12 + 2 < n + 16 leaves a margin for the O(u^2) terms; the final rounding of v0 + dt a is at most half an ulp of v.
The oracle's own sequential binary32 sum (the reference's arithmetic) meets the same bound: tests/test_oracle_cond_f64.py.

Sharper, on the same bodies: FAST may be further from binary64 than the reference's arithmetic by at most C u |dt| S_i (+ ulp(v)),
C = 64: every form sums at most a few hundred terms per partial sum in a fixed tree before adding partial sums; the reference's
sequential sum is itself up to (n - 1) u S_i away, so FAST's own error mostly hides inside it.

NB_RANDOM_CASES=N widens the cases (as in test_gpu_random_differential.py).
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("NB_RANDOM_CASES", "12"))
U = 2.0 ** -24
C_SHARP = 64


def hostile_case(seed):
    """(description, pos, vel, dt, G, bias) of one seeded case, n <= 8 192; every n a multiple of 2 048 so that the pairs form (blocks
    of 512) and the ring at four ranks can take it too"""
    from test_gpu_random_differential import random_state

    rng = np.random.default_rng(seed)
    n = int(rng.choice([2048, 4096, 8192]))
    family = ["random_state", "cluster_in_cloud", "ulp_pairs", "coincident", "collinear", "outliers"][seed % 6]
    if family == "random_state":
        pos, vel = random_state(rng, n)
    else:
        pos = rng.uniform(-100, 100, (n, 3)).astype(np.float32)
        vel = rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
        if family == "cluster_in_cloud":       # a 1e-3 cluster inside a 1e2 cloud
            m = n // 4
            pos[:m] = (rng.uniform(-1e-3, 1e-3, (m, 3)) + pos[0]).astype(np.float32)
        elif family == "ulp_pairs":            # pairs one ulp apart: their terms dominate S_i
            k = n // 16
            src = rng.choice(n, k, replace=False)
            dst = (src + n // 2) % n
            pos[dst] = np.nextafter(pos[src], np.float32(np.inf))
        elif family == "coincident":
            pos[rng.integers(0, n, n // 2)] = pos[rng.integers(0, n, n // 2)]
        elif family == "collinear":
            t = rng.uniform(-50, 50, n).astype(np.float32)
            pos = (np.float32([0.3, -0.7, 0.2])[None, :] * t[:, None]).astype(np.float32)
        elif family == "outliers":             # far outside every range the fast paths assume
            pos[rng.integers(0, n, 4)] *= np.float32(1e9)
            pos[rng.integers(0, n, 3)] *= np.float32(1e-30)
    dt = np.float32(rng.choice([0.1, 0.01, 1.0]))
    G = np.float32(rng.choice([0.001, 1.0, -0.05, -2.0]))
    bias = np.float32(rng.choice([1e-7, 1e-3, 2.0, 1e-30, 2.0 ** 61]))
    return f"seed={seed} family={family} n={n} dt={dt!r} G={G!r} bias={bias!r}", pos, vel, dt, G, bias


def check_bodies(what, pos, vel, v_got, dt, G, bias, oracle, c=C_SHARP, first=0):
    """Both bounds for the bodies [first, first + len(v_got)); returns (largest FAST error in units of u |dt| S, the same beyond the
    reference's own error)"""
    count = len(v_got)
    dv64, S = oracle.step_range_dv_cond_f64(pos, first, count, dt, G, bias)
    v_true = vel[first:first + count].astype(np.float64) + dv64
    _, v_ref = oracle.step_range(pos, vel[first:first + count], first, count, dt, G, bias)
    n = len(pos)
    got = v_got.astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(v_true), np.abs(got)).astype(np.float32)).astype(np.float64)
    unit = U * abs(float(dt)) * S
    err = np.abs(got - v_true)
    err_ref = np.abs(v_ref.astype(np.float64) - v_true)
    assert np.isfinite(got).all(), f"{what}: non-finite velocities"
    bad = err > (n + 16) * unit + ulp
    assert not bad.any(), f"{what}: {bad.sum()} components beyond |dt| (n + 16) u S; first body {first + np.argwhere(bad)[0][0]}"
    bad = err > err_ref + c * unit + ulp
    assert not bad.any(), (f"{what}: {bad.sum()} components beyond the reference's error + {c} u |dt| S; worst "
                           f"{float(((err - err_ref - ulp) / np.where(unit > 0, unit, np.inf)).max()):.1f}")
    with np.errstate(divide="ignore", invalid="ignore"):
        r1 = np.where(unit > 0, np.maximum(err - ulp, 0) / unit, 0)
        r2 = np.where(unit > 0, np.maximum(err - err_ref - ulp, 0) / unit, 0)
    return float(r1.max()), float(r2.max())


FORMS = {   # name: environment, tile
    "default": ({}, 0),
    "lds_groups": ({"NB_FAST_WAVES": "0", "NB_FAST_GROUPS": "2", "NB_FAST_IB": "2", "NB_FAST_SLICES": "3"}, 512),
    "wave": ({"NB_FAST_WAVES": "8", "NB_FAST_IB": "4", "NB_FAST_SLICES": "5"}, 256),
    "scalar_load": ({"NB_FAST_SL": "1", "NB_FAST_IB": "2", "NB_FAST_SLICES": "4"}, 0),
    "pairs_np2_w4": ({"NB_FAST_PAIRS": "1", "NB_FAST_PAIRS_NP": "2", "NB_FAST_PAIRS_W": "4"}, 0),
    "pairs_np4_w2_chunk": ({"NB_FAST_PAIRS": "1", "NB_FAST_PAIRS_NP": "4", "NB_FAST_PAIRS_W": "2", "NB_FAST_PAIRS_CHUNK": "1024"}, 0),
    "phases": ({}, 0),
    "ring": ({"NB_RING": "1"}, 0),
    "ring_phases": ({"NB_RING": "1"}, 0),
}


def fast_step_velocities(nb, monkeypatch, form, pos, vel, dt, G, bias):
    """the velocities after one FAST step taken through `form` (an entry of FORMS)"""
    from nenbody_amd import _lib

    env, tile = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params = nb.default_params(mode=nb.NB_MODE_FAST, tile=tile)
    params.dt, params.G, params.bias = float(dt), float(G), float(bias)
    n = len(pos)
    if form.startswith("pairs"):
        assert _lib.planned_kernels(params, n, n)[0] == "step_fast_pairs_kernel"
    if form.startswith("ring"):
        from test_gpu_ring import ring_steps_on_one_gpu

        _, v = ring_steps_on_one_gpu(nb, pos, vel, 4, params, 1, phases=form == "ring_phases")
    elif form == "phases":
        import torch

        lib = _lib.load()
        dev = torch.device("cuda", 0)
        cur = torch.zeros((n, 4), dtype=torch.float32)
        cur[:, :3] = torch.from_numpy(pos)
        cur = cur.to(dev)
        nxt = torch.zeros_like(cur)
        vt = torch.zeros((n, 4), dtype=torch.float32)
        vt[:, :3] = torch.from_numpy(vel)
        vt = vt.to(dev)
        j_lo, j_hi = n // 4, n // 2
        sb = lib.nb_scratch_bytes_phased(ctypes.byref(params), n, n, j_lo, j_hi)
        scratch = torch.empty((sb,), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for phase in (_lib.NB_PHASE_RANGE, _lib.NB_PHASE_REST):
            _lib.check(lib.nb_launch_step_phase(ctypes.byref(params), n, 0, n, j_lo, j_hi, phase, cur.data_ptr(), nxt.data_ptr(),
                                               vt.data_ptr(), scratch.data_ptr(), sb, stream))
        torch.cuda.synchronize()
        v = vt[:, :3].cpu().numpy()
    else:
        with nb.Scene(pos, vel, params) as sc:
            sc.step_n(1)
            _, v = sc.state()
    return v


@pytest.mark.parametrize("case", range(CASES))
@pytest.mark.parametrize("form", list(FORMS))
def test_fast_every_body_within_the_binary64_bound(nb, oracle, monkeypatch, capsys, form, case):
    what, pos, vel, dt, G, bias = hostile_case(case)
    what = f"{form}: {what}"
    n = len(pos)
    v = fast_step_velocities(nb, monkeypatch, form, pos, vel, dt, G, bias)
    r1, r2 = check_bodies(what, pos, vel, v, dt, G, bias, oracle)
    with capsys.disabled():
        print(f"\n  {what}: max error {r1:.2f} u|dt|S (bound n + 16 = {n + 16}), beyond the reference's {r2:.2f} (bound {C_SHARP})")
