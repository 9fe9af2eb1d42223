"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle and the golden vectors.

Bar: STRICT is bit-identical to the oracle (the reference's binary32 arithmetic) for any N, any K, any
sharding.  FAST is held to stated tolerances over short horizons (the system is chaotic after ~300 steps
at N=1024: SURVEY.md section 0, sixth finding -- no reassociated fp32 kernel can track it further).
north_star tolerance: |delta r| < 1e-4 after 1 000 steps; STRICT meets it with |delta r| = 0.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu


def matrices_equal(got, ref):
    """model matrices (main.rs:437-439) word for word: since round 4 the device computes the angle, its sine and cosine as the host's
    libm does (nenbody_amd/csrc/nb_libm.h); NaN entries (non-finite velocities) compare equal whatever their payload"""
    g, r = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    return g.shape == r.shape and bool(((g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r))).all())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what=""):
    g, r = bits(got), bits(ref)
    if not (g == r).all():
        bad = np.argwhere(g != r)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} words differ; first at {bad[0]}: "
                             f"{np.asarray(got).ravel()[np.ravel_multi_index(tuple(bad[0]), g.shape)]!r} vs "
                             f"{np.asarray(ref).ravel()[np.ravel_multi_index(tuple(bad[0]), r.shape)]!r}")


def state3d(oracle, n, seed):
    pos, vel = oracle.init_state(n, seed)
    rng = np.random.default_rng(seed)
    pos[:, 2] = rng.uniform(-100, 100, n).astype(np.float32)
    vel[:, 2] = rng.uniform(0, 0.1, n).astype(np.float32)
    return pos, vel


# ---------------------------------------------------------------------------------------------------------
# STRICT: bit-exact
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[1, "1np", 2, 4, 8, 16, "pc8", "pc14", "pc14np", "bc", "sl"], ids=lambda s: f"lanes{s}")
def lanes(request, monkeypatch):
    """STRICT launch shape: lanes per body (1 = plain, >1 = j-parallel) or "pc" = producer/consumer form; "1np" = one
    lane per body with planar tiles folded component-packed instead of j-packed (NB_STRICT_NO_PACKED=1).
    All of them keep the reference's summation order.  By default the library picks one from the shard size;
    the tests pin every value."""
    if request.param == "bc":                                    # block-chain form (nb_nbody_bc.inc)
        monkeypatch.setenv("NB_STRICT_BC", "1")
    elif request.param == "sl":                                  # scalar-load form (nb_nbody_sl.inc): what whole sets take
        monkeypatch.setenv("NB_STRICT_SL", "1")
        monkeypatch.setenv("NB_STRICT_BC", "0")
    elif request.param == "1np":
        monkeypatch.setenv("NB_STRICT_PC", "0")
        monkeypatch.setenv("NB_STRICT_LANES", "1")
        monkeypatch.setenv("NB_STRICT_NO_PACKED", "1")
    elif str(request.param).startswith("pc"):
        if request.param.endswith("np"):                         # component-packed producers instead of j-packed ones
            monkeypatch.setenv("NB_STRICT_NO_PACKED", "1")
        monkeypatch.setenv("NB_STRICT_PC", request.param[2:].replace("np", ""))   # producers per workgroup: 8 or 14
    else:
        monkeypatch.setenv("NB_STRICT_PC", "0")
        monkeypatch.setenv("NB_STRICT_LANES", str(request.param))
    return request.param


@pytest.mark.parametrize("n", [1, 2, 3, 15, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 1025, 2049])
def test_strict_ragged_sizes_bit_exact(nb, oracle, lanes, n):
    pos, vel = state3d(oracle, n, seed=n)
    with nb.Scene(pos, vel) as sc:
        sc.step_n(3)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 3)
    assert_bits_equal(p, p_ref, f"positions n={n}")
    assert_bits_equal(v, v_ref, f"velocities n={n}")


@pytest.mark.parametrize("n", [5, 300, 1026])
def test_strict_planar_ragged_sizes_bit_exact(nb, oracle, lanes, n):
    """z = 0, vz = 0 (the reference's own initial state): the planar shortcut must not change a bit."""
    pos, vel = oracle.init_state(n, seed=n + 1)
    with nb.Scene(pos, vel) as sc:
        sc.step_n(4)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 4)
    assert_bits_equal(p, p_ref, f"positions n={n}")
    assert_bits_equal(v, v_ref, f"velocities n={n}")


def test_strict_mixed_planar_and_3d_tiles_bit_exact(nb, oracle, lanes):
    """Only some tiles are planar: z != 0 for bodies 600..899 only, and the workgroups owning them."""
    n = 2500
    pos, vel = oracle.init_state(n, seed=123)
    pos[600:900, 2] = np.linspace(-5, 5, 300, dtype=np.float32)
    with nb.Scene(pos, vel) as sc:
        sc.step_n(3)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 3)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)


def test_force_3d_switch_gives_the_same_bits(nb, oracle, monkeypatch):
    pos, vel = oracle.init_state(3000, seed=7)
    outs = []
    for f3d in ("0", "1"):
        monkeypatch.setenv("NB_FORCE_3D", f3d)
        for mode in (nb.NB_MODE_STRICT, nb.NB_MODE_FAST):
            with nb.Scene(pos, vel, nb.default_params(mode=mode)) as sc:
                sc.step_n(3)
                outs.append(sc.state())
    assert_bits_equal(outs[0][0], outs[2][0], "STRICT planar vs 3-D path")
    assert_bits_equal(outs[1][0], outs[3][0], "FAST planar vs 3-D path")
    assert_bits_equal(outs[1][1], outs[3][1], "FAST planar vs 3-D path (vel)")


@pytest.mark.parametrize("tile", [256, 512, 1024])
def test_strict_every_tile_size_bit_exact(nb, oracle, tile):
    pos, vel = state3d(oracle, 3000, seed=tile)
    with nb.Scene(pos, vel, nb.default_params(tile=tile)) as sc:
        sc.step_n(2)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 2)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)


@pytest.mark.parametrize("force_lanes", [None, 1, 4, "pc8", "pc14"])
def test_strict_golden_n16_and_n1024(nb, monkeypatch, force_lanes):
    if str(force_lanes).startswith("pc"):
        monkeypatch.setenv("NB_STRICT_PC", force_lanes[2:])
    elif force_lanes is not None:
        monkeypatch.setenv("NB_STRICT_PC", "0")
        monkeypatch.setenv("NB_STRICT_LANES", str(force_lanes))
    g = np.load(os.path.join(GOLDEN_DIR, "nbody_golden.npz"))
    seed = int(g["seed"][0])
    pos, vel = nb.init_state(16, seed)
    assert_bits_equal(pos, g["n16_init_pos"])
    with nb.Scene(pos, vel) as sc:
        sc.step_n(1)
        assert_bits_equal(sc.positions(), g["n16_k1_pos"])
        sc.step_n(9)
        assert_bits_equal(sc.positions(), g["n16_k10_pos"])
        assert_bits_equal(sc.velocities(), g["n16_k10_vel"])
        assert matrices_equal(sc.instances(), g["n16_k10_inst"])
    pos, vel = nb.init_state(1024, seed)
    with nb.Scene(pos, vel) as sc:
        done = 0
        for k in (1, 10, 100, 1000):   # north_star: positions after 1 000 steps, |dr| < 1e-4 -- here exactly 0
            sc.step_n(k - done)
            done = k
            assert_bits_equal(sc.positions(), g[f"n1024_k{k}_pos"], f"n1024 k={k} pos")
            assert_bits_equal(sc.velocities(), g[f"n1024_k{k}_vel"], f"n1024 k={k} vel")
        assert matrices_equal(sc.instances(), g["n1024_k1000_inst"])


def test_strict_config2_n16384_vs_oracle_and_golden(nb, oracle):
    """BASELINE config 2: N=16 384, one GPU, checked against the CPU path."""
    g = np.load(os.path.join(GOLDEN_DIR, "nbody_golden.npz"))
    pos, vel = nb.init_state(16384, int(g["seed"][0]))
    with nb.Scene(pos, vel) as sc:
        sc.step_n(5)
        p, v = sc.state()
    idx = g["n16384_k5_sample_idx"]
    assert_bits_equal(p[idx], g["n16384_k5_sample_pos"])
    assert_bits_equal(v[idx], g["n16384_k5_sample_vel"])
    assert np.bitwise_xor.reduce(bits(p).ravel()) == g["n16384_k5_xor"][0]
    assert np.bitwise_xor.reduce(bits(v).ravel()) == g["n16384_k5_xor"][1]
    p_ref, v_ref = oracle.run(pos, vel, 5)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)


def test_strict_config2_n16384_long_horizons_vs_golden(nb):
    """BASELINE config 2 at the horizons SURVEY.md section 8d names: K = 100 and K = 1 000 (north_star: positions after
    1 000 steps within 1e-4 -- here every bit of every body, through the XOR of all bit patterns)."""
    g = np.load(os.path.join(GOLDEN_DIR, "nbody_golden_c2.npz"))
    pos, vel = nb.init_state(16384, int(g["seed"][0]))
    with nb.Scene(pos, vel) as sc:
        done = 0
        for k in (100, 1000):
            sc.step_n(k - done)
            done = k
            p, v = sc.state()
            idx = g[f"n16384_k{k}_sample_idx"]
            assert_bits_equal(p[idx], g[f"n16384_k{k}_sample_pos"], f"k={k} sampled positions")
            assert_bits_equal(v[idx], g[f"n16384_k{k}_sample_vel"], f"k={k} sampled velocities")
            assert np.bitwise_xor.reduce(bits(p).ravel()) == g[f"n16384_k{k}_xor"][0], f"k={k}: some position bit differs"
            assert np.bitwise_xor.reduce(bits(v).ravel()) == g[f"n16384_k{k}_xor"][1], f"k={k}: some velocity bit differs"


def test_config2_as_written_lds_tile_256(nb, monkeypatch):
    """BASELINE config 2 literally: "N=16 384 bodies, fp32, 1xMI355X, LDS tile=256, tolerance check vs CPU" -- the one-lane-per-
    body STRICT kernel staging 256-record tiles through LDS (params.tile = 256; the library's own choice for this size would be
    the block chain, which has no LDS tile), K = 5 against the golden XOR of every bit; FAST at its default tile of 256."""
    g = np.load(os.path.join(GOLDEN_DIR, "nbody_golden.npz"))
    pos, vel = nb.init_state(16384, int(g["seed"][0]))
    monkeypatch.setenv("NB_STRICT_BC", "0")
    monkeypatch.setenv("NB_STRICT_PC", "0")
    monkeypatch.setenv("NB_STRICT_LANES", "1")
    from nenbody_amd import _lib
    assert _lib.planned_kernels(nb.default_params(tile=256), 16384, 16384) == ["step_strict_kernel"]   # the LDS-tiled kernel
    with nb.Scene(pos, vel, nb.default_params(tile=256)) as sc:
        sc.step_n(5)
        p, v = sc.state()
    idx = g["n16384_k5_sample_idx"]
    assert_bits_equal(p[idx], g["n16384_k5_sample_pos"])
    assert_bits_equal(v[idx], g["n16384_k5_sample_vel"])
    assert np.bitwise_xor.reduce(bits(p).ravel()) == g["n16384_k5_xor"][0]
    assert np.bitwise_xor.reduce(bits(v).ravel()) == g["n16384_k5_xor"][1]
    fast = nb.default_params(mode=nb.NB_MODE_FAST, tile=256)
    assert _lib.planned_kernels(fast, 16384, 16384)[0] == "step_fast_wave_kernel"
    with nb.Scene(pos, vel, fast) as sc:
        sc.step_n(5)
        pf, vf = sc.state()
    assert np.abs(pf[idx] - g["n16384_k5_sample_pos"]).max() < 1e-4      # north_star's |dr| bound, at K = 5
    assert np.abs(vf[idx] - g["n16384_k5_sample_vel"]).max() < 1e-5


def _checksums(p, v):
    pu, vu = bits(p).ravel(), bits(v).ravel()
    return (np.array([np.bitwise_xor.reduce(pu), np.bitwise_xor.reduce(vu)], dtype=np.uint32),
            np.array([pu.sum(dtype=np.uint64) & 0xFFFFFFFF, vu.sum(dtype=np.uint64) & 0xFFFFFFFF], dtype=np.uint32))


def test_headline_size_through_1000_steps_vs_golden(nb):
    """The north_star's acceptance line, literally: N = 131 072 (BASELINE config 3, the size bench.py times), the reference's
    initial distributions and constants, 1 000 steps, positions against the CPU path to |dr| < 1e-4 -- here |dr| = 0: after
    EVERY one of the 1 000 steps the XOR and the wrapping sum of all position and velocity bit patterns equal the oracle's
    (tests/golden/nbody_golden_c3.npz, written by make_golden.py --c3), and 64 sampled bodies equal it word for word at
    K = 1, 40 (the cloud has collapsed), 100 and 1 000.  The data-dependent paths of the kernel (per-tile planarity and range
    flags, hence ladder or IEEE divide) see the whole evolution, not only the initial uniform square."""
    g = np.load(os.path.join(GOLDEN_DIR, "nbody_golden_c3.npz"))
    n = 131072
    pos, vel = nb.init_state(n, int(g["seed"][0]))
    idx = g["n131072_sample_idx"]
    xors, sums, steps = g["n131072_xor"], g["n131072_sum"], g["n131072_steps"]
    assert len(steps) == 1000 and steps[0] == 1 and steps[-1] == 1000
    with nb.Scene(pos, vel) as sc:
        for k in steps:
            sc.step_n(1)
            p, v = sc.state()
            x, s_ = _checksums(p, v)
            assert (x == xors[k - 1]).all() and (s_ == sums[k - 1]).all(), f"step {k}: the state differs from the oracle's"
            if f"n131072_k{k}_sample_pos" in g.files:
                assert_bits_equal(p[idx], g[f"n131072_k{k}_sample_pos"], f"k={k} sampled positions")
                assert_bits_equal(v[idx], g[f"n131072_k{k}_sample_vel"], f"k={k} sampled velocities")
                assert int(np.count_nonzero(p[:, 2]) + np.count_nonzero(v[:, 2])) == int(g[f"n131072_k{k}_nonplanar"][0])


def test_headline_size_fast_drift_curve(nb, oracle, capsys):
    """FAST at the headline size against STRICT (= the oracle, bit for bit: the test above) step by step through the collapse:
    what is asserted is what is true, and the curve is printed.  One step: at most two ulps of a coordinate.  From the second
    step on the WORST body is off by millimetres: 131 072 bodies in a 200 x 200 square have pairs a few 1e-4 apart, where the
    softened 1/r law (bias = 1e-7) is at its steepest -- a one-ulp difference in a position (7.6e-6) changes such a pair's force
    by percents, in any arithmetic that is not the reference's bit for bit.  The bulk stays within the north_star's 1e-4 for the
    free fall; nothing tracks the reference to 1 000 steps but STRICT, which is what STRICT is for.

    That explanation is TESTED here, two ways:
    (a) sensitivity, not error: STRICT itself, restarted from its own state after step 1 with ONE coordinate of ONE body of the
        closest pair moved by one ulp, leaves unperturbed STRICT as fast as FAST does (max |dr| at steps 2..10 at least half of
        FAST's; measured: the same curve to two digits); with one coordinate of EVERY body moved by one ulp it ends up ten times
        further out by step 10;
    (b) on the 64 bodies where FAST is furthest from STRICT after step 2, FAST's second step is no further from the same sum
        carried in binary64 over ITS OWN step-1 snapshot than STRICT's second step is from the binary64 sum over its snapshot:
        what differs is the input (by an ulp), not the quality of the arithmetic."""
    from scipy.spatial import cKDTree

    n = 131072
    pos, vel = nb.init_state(n, 1234)
    fastp = nb.default_params(mode=nb.NB_MODE_FAST)
    with nb.Scene(pos, vel) as ref:
        ref.step_n(1)
        p1, v1 = ref.state()
    # the closest pair of the state after step 1; nudge the coordinate along which the two are furthest apart
    tree = cKDTree(p1[:, :2].astype(np.float64))
    dist, nbr = tree.query(p1[:, :2].astype(np.float64), k=2)
    a = int(np.argmin(dist[:, 1]))
    b = int(nbr[a, 1])
    axis = int(np.argmax(np.abs(p1[a, :2] - p1[b, :2])))
    one = p1.copy()
    one[a, axis] = np.nextafter(one[a, axis], np.float32(np.inf), dtype=np.float32)
    rng = np.random.default_rng(5)
    every = p1.copy()
    up = rng.random(n) < 0.5
    every[:, 0] = np.where(up, np.nextafter(p1[:, 0], np.float32(np.inf), dtype=np.float32), np.nextafter(p1[:, 0], np.float32(-np.inf), dtype=np.float32))
    curve, state2 = [], {}
    with nb.Scene(pos, vel) as ref, nb.Scene(pos, vel, fastp) as fast, nb.Scene(one, v1) as nudged, nb.Scene(every, v1) as shaken:
        for k in range(1, 61):
            ref.step_n(1)
            fast.step_n(1)
            if k >= 2:
                nudged.step_n(1)
                shaken.step_n(1)
            if k == 1:
                state2["fast1"] = fast.state()
            if k <= 10 or k % 10 == 0:
                (pr, vr), (pf, vf) = ref.state(), fast.state()
                dr = np.abs(pf.astype(np.float64) - pr).max(axis=1)
                row = [k, float(dr.max()), float(np.quantile(dr, 0.999)), float(np.median(dr)), 0.0, 0.0]
                if 2 <= k <= 10:
                    row[4] = float(np.abs(nudged.state()[0].astype(np.float64) - pr).max())
                    row[5] = float(np.abs(shaken.state()[0].astype(np.float64) - pr).max())
                if k == 2:
                    state2.update(ref2=(pr, vr), fast2=(pf, vf), dr=dr)
                curve.append(tuple(row))
    with capsys.disabled():
        print("\n  FAST vs STRICT at N = 131072, |dr| by step (max / 99.9 % / median): " +
              ", ".join(f"{k}: {a_:.1e} / {b_:.1e} / {c:.1e}" for k, a_, b_, c, _, _ in curve))
        print(f"  STRICT restarted after step 1 with one coordinate of body {a} (closest pair {a}-{b}, {dist[a, 1]:.2e} apart) one ulp off, and with "
              "x of every body one ulp off: max |dr| against unperturbed STRICT by step (one body / every body / FAST): " +
              ", ".join(f"{k}: {o:.1e} / {e:.1e} / {a_:.1e}" for k, a_, _, _, o, e in curve if 2 <= k <= 10))
    d = {row[0]: row[1:] for row in curve}
    assert d[1][0] < 2e-5                   # one step: at most a couple of ulps of a coordinate of magnitude 100 (7.6e-6 each)
    assert d[10][2] < 1e-4, curve           # the typical body is inside the north_star's bound through the free fall
    # (a) STRICT nudged by one ulp diverges as fast as FAST does
    for k in range(2, 11):
        assert d[k][3] >= 0.5 * d[k][0], f"step {k}: one body of the closest pair one ulp off {d[k][3]:.2e} against FAST's {d[k][0]:.2e}"
    # (measured: 1.4e-3 / 2.7e-3 / 4.1e-3 ... 1.2e-2 against FAST's 1.3e-3 / 2.7e-3 / 4.0e-3 ... 1.3e-2 -- FAST's worst body IS that pair.  With
    # x of EVERY body one ulp off the pair's separation happens to change less at first -- 2.6e-4 at step 2 -- and other pairs take
    # over: 1.2e-2 at step 5, 1.7e-1 at step 10, ten times FAST's.)
    assert d[10][4] >= 0.5 * d[10][0], f"step 10: every body one ulp off {d[10][4]:.2e} against FAST's {d[10][0]:.2e}"
    # (b) FAST's second step on its own snapshot is as close to the binary64 sum as STRICT's on its own
    worst = np.argsort(state2["dr"])[-64:]
    c = [float(np.float32(x)) for x in (0.1, 0.001, 0.0000001)]
    pf1, vf1 = state2["fast1"]
    (_, vr2), (_, vf2) = state2["ref2"], state2["fast2"]
    dv64_ref = np.concatenate([oracle.step_range_dv_f64(p1, int(i), 1, *c) for i in worst])
    dv64_fast = np.concatenate([oracle.step_range_dv_f64(pf1, int(i), 1, *c) for i in worst])
    err_ref = np.abs(vr2[worst].astype(np.float64) - (v1[worst].astype(np.float64) + dv64_ref)).max(axis=1)
    err_fast = np.abs(vf2[worst].astype(np.float64) - (vf1[worst].astype(np.float64) + dv64_fast)).max(axis=1)
    ulp_v = float(np.spacing(np.float32(np.abs(vr2[worst]).max())))
    with capsys.disabled():
        print(f"  the 64 bodies furthest apart after step 2 (|dr| {state2['dr'][worst].min():.1e} .. {state2['dr'][worst].max():.1e}): second step against "
              f"the binary64 sum over the mode's own snapshot, max |dv error|: STRICT {err_ref.max():.2e}, FAST {err_fast.max():.2e} (ulp of v {ulp_v:.1e})")
    assert err_fast.max() <= err_ref.max() + ulp_v
    assert (err_fast <= err_ref + ulp_v + 2e-5 * np.abs(dv64_ref).max(axis=1)).all()


def test_headline_size_fast_is_deterministic_and_finite_through_the_collapse(nb):
    """FAST at the headline size (the pairs form: 2 016 workgroups whose b-side sums meet in LDS, rows added in index order):
    two runs of 100 steps give the same bits after every tenth step -- no sum depends on which workgroup finished first --, and
    no body goes non-finite while the cloud collapses and rebounds (step ~40)."""
    n = 131072
    pos, vel = nb.init_state(n, 1234)
    fast = nb.default_params(mode=nb.NB_MODE_FAST)
    from nenbody_amd import _lib
    assert _lib.planned_kernels(fast, n, n)[0] == "step_fast_pairs_kernel"
    with nb.Scene(pos, vel, fast) as a, nb.Scene(pos, vel, fast) as b:
        for k in range(10):
            a.step_n(10)
            b.step_n(10)
            (pa, va), (pb, vb) = a.state(), b.state()
            assert_bits_equal(pa, pb, f"step {10 * (k + 1)}: positions differ between two runs")
            assert_bits_equal(va, vb, f"step {10 * (k + 1)}: velocities differ between two runs")
            assert np.isfinite(pa).all() and np.isfinite(va).all(), f"step {10 * (k + 1)}"


def test_strict_ieee_fallback_path_bit_exact(nb, oracle, lanes, monkeypatch):
    """The guarded '/' path (taken when coordinates leave the range where the shared-reciprocal ladder is
    proven exact) must give the same bits; force it for every tile."""
    pos, vel = state3d(oracle, 1500, seed=77)
    monkeypatch.setenv("NB_STRICT_FORCE_IEEE", "1")
    with nb.Scene(pos, vel) as sc:
        sc.step_n(3)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 3)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)


def test_strict_extreme_coordinates_bit_exact(nb, oracle, lanes):
    """Data that trips the per-tile range guard: tiny, huge, subnormal-producing and coincident coordinates,
    mixed into ordinary ones so that some tiles take the ladder and others the IEEE path."""
    n = 2048
    pos, vel = state3d(oracle, n, seed=5)
    pos[5] = [1e-30, -3e-25, 0.0]          # |x| far below the ladder's lower bound
    pos[6] = [1e-30, -3e-25, 1e-38]        # nearly coincident with body 5: dx underflows, subnormal products
    pos[700] = [3e7, -2e7, 1e7]            # above the upper bound: r^2 ~ 1e15
    pos[701] = pos[700]                    # exactly coincident pair
    pos[1500] = [1e-45, 1e-44, -1e-45]     # subnormal coordinates
    pos[2047] = [-2e6, 5e-12, 1.5e6]
    with nb.Scene(pos, vel) as sc:
        sc.step_n(2)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 2)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)


def test_strict_nonfinite_input_propagates_like_the_reference(nb, oracle, lanes):
    pos, vel = state3d(oracle, 300, seed=9)
    pos[17, 0] = np.inf
    pos[200, 1] = np.nan
    with nb.Scene(pos, vel) as sc:
        sc.step_n(1)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 1)
    assert (np.isnan(p) == np.isnan(p_ref)).all() and (np.isnan(v) == np.isnan(v_ref)).all()
    ok = ~np.isnan(p_ref)
    assert (bits(p)[ok] == bits(p_ref)[ok]).all()


def test_strict_nondefault_constants_bit_exact(nb, oracle, lanes):
    pos, vel = state3d(oracle, 700, seed=21)
    for dt, g_, bias in [(0.05, 0.5, 0.01), (1.0, -0.001, 1e-3), (0.1, 1e-30, 1e-7), (0.1, 0.001, 0.0)]:
        params = nb.default_params()
        params.dt, params.G, params.bias = dt, g_, bias
        if bias == 0.0:
            pos2 = pos.copy()      # bias 0: the self term is 0/0 = NaN in the reference; keep the comparison NaN-aware
        else:
            pos2 = pos
        with nb.Scene(pos2, vel, params) as sc:
            sc.step_n(2)
            p, v = sc.state()
        p_ref, v_ref = oracle.run(pos2, vel, 2, np.float32(dt), np.float32(g_), np.float32(bias))
        assert (np.isnan(p) == np.isnan(p_ref)).all()
        ok = ~np.isnan(p_ref)
        assert (bits(p)[ok] == bits(p_ref)[ok]).all(), (dt, g_, bias)
        okv = ~np.isnan(v_ref)
        assert (bits(v)[okv] == bits(v_ref)[okv]).all(), (dt, g_, bias)


def test_strict_is_deterministic(nb, oracle):
    pos, vel = state3d(oracle, 5000, seed=31)
    outs = []
    for _ in range(2):
        with nb.Scene(pos, vel) as sc:
            sc.step_n(4)
            outs.append(sc.state())
    assert_bits_equal(outs[0][0], outs[1][0])
    assert_bits_equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------------------------------------------------
# launch API / sharding (one process, several index ranges): what each rank of a multi-GPU job runs
# ---------------------------------------------------------------------------------------------------------
def _oracle_bodies(oracle, pos, vel, idx, consts):
    """(binary64 velocity change, the reference's binary32 new velocity) of scattered bodies, one step against `pos`: the
    oracle's scalar loops body by body on a thread pool (ctypes releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor

    def one(i):
        i = int(i)
        return oracle.step_range_dv_f64(pos, i, 1, *consts)[0], oracle.step_range(pos, vel[i:i + 1], i, 1)[1][0]

    with ThreadPoolExecutor(max_workers=oracle.ncores()) as pool:
        out = list(pool.map(one, idx))
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], np.float32)


def _sharded_step_on_one_gpu(nb, pos, vel, parts, params, steps):
    import torch

    from nenbody_amd.dist import HipBackend

    be = HipBackend()
    n = len(pos)
    dev = torch.device("cuda", 0)
    cur = torch.zeros((n, 4), dtype=torch.float32)
    cur[:, :3] = torch.from_numpy(pos)
    cur = cur.to(dev)
    nxt = torch.zeros_like(cur)
    vels = []
    for first, count in parts:
        vr = torch.zeros((count, 4), dtype=torch.float32)
        vr[:, :3] = torch.from_numpy(vel[first:first + count])
        vels.append(vr.to(dev))
    for _ in range(steps):
        for (first, count), vr in zip(parts, vels):
            sb = be.scratch_bytes(params, n, count)
            scratch = torch.empty((sb,), dtype=torch.uint8, device=dev) if sb else None
            be.step(params, n, first, count, cur, nxt, vr, scratch)
        cur, nxt = nxt, cur
    torch.cuda.synchronize()
    v = np.concatenate([vr[:, :3].cpu().numpy() for vr in vels])
    return cur[:, :3].cpu().numpy(), v


@pytest.mark.parametrize("parts", [[(0, 1000)], [(0, 500), (500, 500)], [(0, 1), (1, 255), (256, 257), (513, 487)]])
def test_strict_sharded_launch_equals_unsharded(nb, oracle, lanes, parts):
    pos, vel = state3d(oracle, 1000, seed=11)
    p, v = _sharded_step_on_one_gpu(nb, pos, vel, parts, nb.default_params(), 3)
    p_ref, v_ref = oracle.run(pos, vel, 3)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)


def test_sharded_scene_world_of_one_on_gpu(nb, oracle):
    pos, vel = state3d(oracle, 777, seed=13)
    sc = nb.ShardedScene(pos, vel)
    sc.step_n(3)
    sc.sync()
    p_ref, v_ref, inst_ref = oracle.run(pos, vel, 3, want_instances=True)
    assert_bits_equal(sc.positions(), p_ref)
    assert_bits_equal(sc.velocities(), v_ref)
    assert matrices_equal(sc.local_instances(), inst_ref)


# ---------------------------------------------------------------------------------------------------------
# full BASELINE size, N = 131 072: size-independent properties + an oracle check on sampled bodies
# ---------------------------------------------------------------------------------------------------------
def test_strict_full_size_sampled_bodies_vs_oracle_and_shard_invariance(nb, oracle):
    n = 131072
    pos, vel = nb.init_state(n, 1234)
    with nb.Scene(pos, vel) as sc:
        sc.step_n(1)
        p, v = sc.state()
    # (1) 320 bodies spread over first/last/middle workgroups, each folded over all 131 072 j's by the oracle
    idx = np.unique(np.concatenate([np.arange(0, 64), np.arange(n - 64, n), np.linspace(64, n - 65, 192).astype(np.int64)]))
    for i in idx:
        p_ref, v_ref = oracle.step_range(pos, vel[i:i + 1], int(i), 1)
        assert (bits(p[i]) == bits(p_ref[0])).all() and (bits(v[i]) == bits(v_ref[0])).all(), f"body {i}"
    # (2) antisymmetry of the pair force: the total acceleration cancels to rounding
    a = (v.astype(np.float64) - vel.astype(np.float64)) / 0.1
    assert np.abs(a.sum(axis=0)).max() < 1e-2 * np.abs(a).sum(axis=0).max()
    # (3) planar input stays planar, exactly (z = 0, vz = 0 is a fixed point of the reference's arithmetic)
    assert (p[:, 2] == 0).all() and (v[:, 2] == 0).all()
    # (4) an 8-way index-range sharding of the same step gives the same bits
    parts = nb.partition(n, 8)
    p8, v8 = _sharded_step_on_one_gpu(nb, pos, vel, parts, nb.default_params(), 1)
    assert_bits_equal(p8, p)
    assert_bits_equal(v8, v)


def test_config5_size_one_million_bodies_sampled(nb, oracle):
    """BASELINE config 5 size, N = 1 048 576: one FAST and one STRICT step; sampled bodies folded over all j by the oracle."""
    n = 1 << 20
    pos, vel = nb.init_state(n, 1234)
    idx = np.unique(np.concatenate([np.arange(0, 8), np.arange(n - 8, n), np.linspace(8, n - 9, 48).astype(np.int64)]))
    with nb.Scene(pos, vel) as sc:
        sc.step_n(1)
        p, v = sc.state()
    with nb.Scene(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST)) as sc:
        sc.step_n(1)
        pf, vf = sc.state()
    acc = 0.0
    for i in idx:
        p_ref, v_ref = oracle.step_range(pos, vel[i:i + 1], int(i), 1)
        assert (bits(p[i]) == bits(p_ref[0])).all() and (bits(v[i]) == bits(v_ref[0])).all(), f"STRICT body {i}"
        acc = max(acc, float(np.abs(v_ref[0] - vel[i]).max()))
        # a million-term binary32 sum: FAST's reassociated partial sums and the reference's sequential sum each carry
        # ~1e-5 relative rounding error of their own, so the tolerance is 1e-4 of the step's velocity change here
        assert np.abs(vf[i] - v_ref[0]).max() <= 1e-4 * float(np.abs(v_ref[0] - vel[i]).max()) + 1e-9, f"FAST body {i}"
    assert acc > 0


# BASELINE configs 4 and 5: the launch shapes every rank of the 2-, 4- and 8-GPU jobs issues -- (first, count) of
# nenbody_amd.dist.partition, first != 0 for all but rank 0, the library's own choice of kernel form, slices and bodies per
# thread for that count -- run one after another on the one GPU and assembled into the step.
_REF_STEP = {}


def _unsharded_reference_step(nb, n, mode):
    """one whole-set step on the GPU (STRICT and FAST), cached across the parametrised cases"""
    key = (n, mode)
    if key not in _REF_STEP:
        pos, vel = nb.init_state(n, 1234)
        with nb.Scene(pos, vel, nb.default_params(mode=mode)) as sc:
            sc.step_n(1)
            _REF_STEP[key] = sc.state()
    return _REF_STEP[key]


@pytest.mark.parametrize("n,world", [(131072, 2), (131072, 4), (131072, 8), (1 << 20, 2), (1 << 20, 4), (1 << 20, 8)],
                         ids=lambda x: str(x))
def test_every_rank_shape_of_configs_4_and_5_vs_oracle(nb, oracle, n, world):
    pos, vel = nb.init_state(n, 1234)
    parts = nb.partition(n, world)
    assert all(c == n // world for _, c in parts) and [f for f, _ in parts][1] == n // world
    # STRICT: all ranks' launches == the unsharded step, bit for bit, every body ...
    p1, v1 = _unsharded_reference_step(nb, n, nb.NB_MODE_STRICT)
    ps, vs = _sharded_step_on_one_gpu(nb, pos, vel, parts, nb.default_params(), 1)
    assert_bits_equal(ps, p1, f"STRICT positions, {world} ranks vs 1")
    assert_bits_equal(vs, v1, f"STRICT velocities, {world} ranks vs 1")
    # ... and == the oracle on bodies of EVERY rank: first, last and six inside each range (>= 64 bodies at 8 ranks)
    idx = np.unique(np.concatenate([np.concatenate([[f, f + c - 1], np.linspace(f + 1, f + c - 2, 6).astype(np.int64)])
                                    for f, c in parts]))
    v_ref = np.empty((len(idx), 3), np.float32)
    for k, i in enumerate(idx):
        p_ref, vr = oracle.step_range(pos, vel[i:i + 1], int(i), 1)
        v_ref[k] = vr[0]
        assert (bits(ps[i]) == bits(p_ref[0])).all() and (bits(vs[i]) == bits(vr[0])).all(), f"STRICT body {i}"
    # FAST, the library's own slices / bodies per thread for this count: against the reference's arithmetic AND against
    # the same sum carried in binary64.  The reference's sequential binary32 sum of n terms carries a rounding error of its
    # own (~sqrt(n) half-ulps of a sum that is ~n*G/R); FAST's partial sums carry less.  So FAST is held to (a) the stated
    # per-step tolerance against the oracle, widened at n = 2^20 to 1e-4 of the velocity change, and (b) -- the evidence
    # for that widening -- being no further from the binary64 sum than the reference's own arithmetic is.
    pf, vf = _sharded_step_on_one_gpu(nb, pos, vel, parts, nb.default_params(mode=nb.NB_MODE_FAST), 1)
    pf1, vf1 = _unsharded_reference_step(nb, n, nb.NB_MODE_FAST)
    c = [float(np.float32(x)) for x in (0.1, 0.001, 0.0000001)]
    dv64 = np.concatenate([oracle.step_range_dv_f64(pos, int(i), 1, *c) for i in idx])
    v_true = vel[idx].astype(np.float64) + dv64
    scale = np.abs(dv64).max()
    err_ref = np.abs(v_ref.astype(np.float64) - v_true).max(axis=1)
    err_fast = np.abs(vf[idx].astype(np.float64) - v_true).max(axis=1)
    ulp_v = float(np.spacing(np.float32(np.abs(v_true).max())))      # the final rounding of v = v + a*dt, common to both
    msg = (f"n={n} ranks={world}: max |v - v64| / max|dv|: reference binary32 {err_ref.max() / scale:.2e}, FAST "
           f"{err_fast.max() / scale:.2e}; max |FAST - reference| / max|dv| {np.abs(vf[idx] - v_ref).max() / scale:.2e}")
    print(msg)
    assert err_fast.max() <= err_ref.max() + ulp_v, msg
    assert (err_fast <= err_ref + 2e-5 * scale + ulp_v).all(), msg
    tol = 2e-5 if n <= 131072 else 1e-4
    assert np.abs(vf[idx] - v_ref).max() <= tol * scale + ulp_v, msg
    # sharding FAST changes the chunk boundaries, not the law: over ALL bodies the ranks' launches stay within tolerance of the
    # whole-set launch.  A body with a neighbour at r ~ 1e-4 (there are a few among 2^20 bodies in a 200 x 200 box) has one
    # term G*dt/r ~ 1 in its sum: every later addition then rounds at that magnitude, in the reference's sequential sum as
    # in any other order, so two orders differ by ~1e-4 for such a body -- hence a bound on the bulk (99.9 %) at FAST's
    # stated tolerance and a looser one on the worst body.
    ulp_p = float(np.spacing(np.float32(np.abs(pf1).max())))          # the final rounding of p = v + p
    dv_all = np.abs(vf - vf1).max(axis=1)
    # (both are binary32 sums with their own rounding error -- a whole-set launch at 2^20 bodies does not split j at all and
    # carries a sequential sum's error, like the reference -- so the two may differ by twice the tolerance against the oracle)
    # The evidence for that factor, on the bodies that need it: the 2 048 bodies on which the two FAST launches
    # differ most plus 2 048 evenly spaced ones, each against the same sum in binary64 and against the reference's own binary32
    # arithmetic -- neither FAST launch may be further from the binary64 sum than the reference is (plus FAST's stated per-step
    # tolerance, which covers bodies on which the reference's error happens to cancel).
    tail = np.argsort(dv_all)[-2048:]
    chosen = np.unique(np.concatenate([tail, np.linspace(0, n - 1, 2048).astype(np.int64)]))
    dv64_t, v_ref_t = _oracle_bodies(oracle, pos, vel, chosen, c)
    v_true_t = vel[chosen].astype(np.float64) + dv64_t
    err_ref_t = np.abs(v_ref_t.astype(np.float64) - v_true_t).max(axis=1)
    err_sh_t = np.abs(vf[chosen].astype(np.float64) - v_true_t).max(axis=1)
    err_one_t = np.abs(vf1[chosen].astype(np.float64) - v_true_t).max(axis=1)
    in_tail = np.isin(chosen, tail)
    msg2 = (msg + f"; {len(chosen)} bodies (2 048 with the largest sharded-vs-whole difference, up to {dv_all.max() / scale:.2e}): "
            f"max |v - v64| / max|dv| on the tail: reference {err_ref_t[in_tail].max() / scale:.2e}, FAST sharded "
            f"{err_sh_t[in_tail].max() / scale:.2e}, FAST whole set {err_one_t[in_tail].max() / scale:.2e}; medians "
            f"{np.median(err_ref_t) / scale:.2e} / {np.median(err_sh_t) / scale:.2e} / {np.median(err_one_t) / scale:.2e}")
    print(msg2)
    for name, err in (("sharded", err_sh_t), ("whole-set", err_one_t)):
        assert err.max() <= err_ref_t.max() + ulp_v, f"FAST {name}: " + msg2
        worst = int(np.argmax(err - err_ref_t))
        assert (err <= err_ref_t + 2e-5 * scale + ulp_v).all(), (f"FAST {name}, body {chosen[worst]}: {err[worst] / scale:.2e} against the "
                                                                   f"reference's {err_ref_t[worst] / scale:.2e}; " + msg2)
    assert np.quantile(dv_all, 0.999) <= 2 * tol * scale + ulp_v and dv_all.max() <= 1e-3 * scale, msg2
    assert np.abs(pf - pf1).max() <= dv_all.max() + ulp_p, msg2


def test_shards_of_a_four_million_body_set_vs_oracle(nb, oracle):
    """Index arithmetic past 2^22: ragged shards of a 4 194 341-body set through the launch API -- a block-chain shard near the
    front, a one-lane-per-body shard that ends at the last body, the boids controller on a producer/consumer shard and on a
    chain-split shard -- against the oracle on sampled bodies (first, last, inside), STRICT and boids bit for bit."""
    import torch

    from nenbody_amd.dist import HipBackend

    n = (1 << 22) + 37
    pos, vel = nb.init_state(n, 4242)
    parts = [(5, 4099), (n - 70001, 70001)]
    ps, vs = _sharded_step_on_one_gpu(nb, pos, vel, parts, nb.default_params(), 1)
    off = 0
    for first, count in parts:
        for i in sorted({first, first + 1, first + count // 3, first + count - 2, first + count - 1}):
            p_ref, v_ref = oracle.step_range(pos, vel[i:i + 1], int(i), 1)
            assert (bits(ps[i]) == bits(p_ref[0])).all(), f"STRICT position of body {i} (shard {first}+{count})"
            assert (bits(vs[off + i - first]) == bits(v_ref[0])).all(), f"STRICT velocity of body {i} (shard {first}+{count})"
        off += count
    # FAST on the same shards.  At 4e6 terms the reference's own sequential binary32 sum is ~1e-3 of the velocity change away
    # from the sum carried in binary64, so FAST is held to being no further from THAT sum than the reference's arithmetic is
    # (plus its stated per-step tolerance), as in the 2^20-body test above.
    pf, vf = _sharded_step_on_one_gpu(nb, pos, vel, parts, nb.default_params(mode=nb.NB_MODE_FAST), 1)
    c = [float(np.float32(x)) for x in (0.1, 0.001, 0.0000001)]
    off = 0
    for first, count in parts:
        idx = np.array(sorted({first, first + count // 2, first + count - 1}))
        refs = np.concatenate([oracle.step_range(pos, vel[i:i + 1], int(i), 1)[1] for i in idx])
        dv64 = np.concatenate([oracle.step_range_dv_f64(pos, int(i), 1, *c) for i in idx])
        v_true = vel[idx].astype(np.float64) + dv64
        scale = np.abs(dv64).max()
        err_ref = np.abs(refs.astype(np.float64) - v_true).max()
        err_fast = np.abs(vf[off + idx - first].astype(np.float64) - v_true).max()
        assert err_fast <= err_ref + 2e-5 * scale, f"FAST shard {first}+{count}: {err_fast / scale:.2e} against the reference's {err_ref / scale:.2e}"
        off += count
    # boids: a producer/consumer shard and a chain-split shard
    be, dev = HipBackend(), torch.device("cuda", 0)

    def rec(a):
        t = torch.zeros((n, 4))
        t[:, :3] = torch.from_numpy(a)
        return t.to(dev)

    pin, vin = rec(pos), rec(vel)
    pout, vout = torch.zeros_like(pin), torch.zeros_like(vin)
    bp, obp = nb.default_boids_params(), oracle.boids_params()
    for first, count in ((11, 5000), (n - 50000, 50000)):
        be.boids_step(bp, n, first, count, pin, vin, pout, vout)
        torch.cuda.synchronize()
        for i in sorted({first, first + count // 2, first + count - 1}):
            p_ref, v_ref = oracle.boids_step_range(pos, vel, int(i), 1, obp)
            got_p, got_v = pout[i, :3].cpu().numpy(), vout[i, :3].cpu().numpy()
            assert (bits(got_p) == bits(p_ref[0])).all() and (bits(got_v) == bits(v_ref[0])).all(), f"boids body {i} (shard {first}+{count})"


def test_fast_full_size_close_to_strict_and_shard_consistent(nb):
    n = 131072
    pos, vel = nb.init_state(n, 1234)
    with nb.Scene(pos, vel) as sc:
        sc.step_n(1)
        p_s, v_s = sc.state()
    with nb.Scene(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST)) as sc:
        sc.step_n(1)
        p_f, v_f = sc.state()
    acc = np.abs(v_s - vel).max()
    assert np.abs(v_f - v_s).max() <= 2e-5 * acc + 1e-9      # per-step relative force error, tolerance 2e-5 of the largest
    assert np.abs(p_f - p_s).max() <= 1e-4                    # north_star's |dr| bound, one step
    parts = nb.partition(n, 8)
    p8, v8 = _sharded_step_on_one_gpu(nb, pos, vel, parts, nb.default_params(mode=nb.NB_MODE_FAST), 1)
    assert np.abs(p8 - p_s).max() <= 1e-4 and np.abs(v8 - v_s).max() <= 2e-5 * acc + 1e-9


# ---------------------------------------------------------------------------------------------------------
# FAST: stated tolerances
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,tol_r", [(1024, 1, 1e-6), (1024, 10, 1e-5), (1024, 100, 1e-4), (16384, 3, 1e-4), (1000, 10, 1e-5)])
def test_fast_within_tolerance_of_oracle(nb, oracle, n, k, tol_r):
    """|delta r| bound of north_star (1e-4) over horizons where a reassociated fp32 sum can meet it."""
    pos, vel = oracle.init_state(n, 1234)
    with nb.Scene(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST)) as sc:
        sc.step_n(k)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, k)
    dr = np.linalg.norm(p.astype(np.float64) - p_ref.astype(np.float64), axis=1).max()
    assert dr < tol_r, f"max |dr| = {dr:.3e} after {k} steps"


@pytest.mark.parametrize("ib,groups,slices,tile", [(1, 1, 1, 256), (2, 1, 1, 512), (4, 1, 1, 1024), (1, 1, 4, 256), (2, 1, 7, 512),
                                                   (4, 1, 64, 256), (1, 2, 1, 256), (2, 2, 3, 512), (4, 2, 1, 256), (1, 4, 1, 512),
                                                   (2, 4, 2, 256), (4, 4, 1, 512), (4, 4, 5, 256), (4, 4, 16, 512)])
def test_fast_every_launch_shape(nb, oracle, monkeypatch, ib, groups, slices, tile):
    """bodies per lane x 256-lane groups per workgroup (each folding its own j chunk, combined in LDS) x grid.y slices
    (combined through memory) x tile: every built shape, ragged sizes included"""
    monkeypatch.setenv("NB_FAST_IB", str(ib))
    monkeypatch.setenv("NB_FAST_GROUPS", str(groups))
    monkeypatch.setenv("NB_FAST_SLICES", str(slices))
    n = 5000
    pos, vel = state3d(oracle, n, seed=ib * 100 + slices)
    with nb.Scene(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST, tile=tile)) as sc:
        sc.step_n(1)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 1)
    acc = np.abs(v_ref - vel).max()
    assert np.abs(v - v_ref).max() <= 2e-5 * acc + 1e-9
    assert np.abs(p - p_ref).max() <= 1e-5


@pytest.mark.parametrize("ib,waves,slices,tile", [(1, 1, 1, 256), (1, 4, 3, 256), (1, 16, 1, 256), (2, 8, 1, 256), (2, 16, 2, 512), (4, 4, 5, 256),
                                                  (4, 8, 1, 256), (4, 16, 1, 256), (4, 16, 2, 512), (2, 4, 64, 256)])
def test_fast_wave_form_every_launch_shape(nb, oracle, monkeypatch, ib, waves, slices, tile):
    """the barrier-free FAST form (step_fast_wave_kernel): `waves` waves per workgroup share 64*ib bodies, stage their own
    tiles and fold one j chunk each; sums meet in LDS in wave order, grid.y slices through memory"""
    monkeypatch.setenv("NB_FAST_IB", str(ib))
    monkeypatch.setenv("NB_FAST_WAVES", str(waves))
    monkeypatch.setenv("NB_FAST_SLICES", str(slices))
    for n in (5000, 64 * ib, 777):
        pos, vel = state3d(oracle, n, seed=ib * 100 + slices + waves)
        if n == 777:
            pos[:, 2] = 0          # the planar form of the fold
            vel[:, 2] = 0
        fast = nb.default_params(mode=nb.NB_MODE_FAST, tile=tile)
        outs = []
        for _ in range(2):
            with nb.Scene(pos, vel, fast) as sc:
                sc.step_n(2)
                outs.append(sc.state())
        assert_bits_equal(outs[0][0], outs[1][0], "run-to-run determinism")
        assert_bits_equal(outs[0][1], outs[1][1], "run-to-run determinism (velocities)")
        p, v = outs[0]
        p_ref, v_ref = oracle.run(pos, vel, 2)
        acc = np.abs(v_ref - vel).max()
        assert np.abs(v - v_ref).max() <= 4e-5 * acc + float(np.spacing(np.abs(v_ref).max())), f"n={n}"
        assert np.abs(p - p_ref).max() <= 2e-5, f"n={n}"


@pytest.mark.parametrize("ib,slices", [(1, 1), (2, 1), (4, 1), (1, 3), (2, 5), (4, 2), (4, 64)])
def test_fast_scalar_load_form_every_launch_shape(nb, oracle, monkeypatch, ib, slices):
    """FAST through scalar loads (step_fast_sl_kernel, what sets of 4 096 bodies and more run): ragged sizes (ranges that
    start and end anywhere in a 16-record request, sets smaller than one request), planar and 3-D data, with and without the
    shared reciprocal, a huge-coordinate set that must not share; deterministic run to run."""
    monkeypatch.setenv("NB_FAST_SL", "1")
    monkeypatch.setenv("NB_FAST_IB", str(ib))
    monkeypatch.setenv("NB_FAST_SLICES", str(slices))
    fast = nb.default_params(mode=nb.NB_MODE_FAST)
    from nenbody_amd import _lib
    assert _lib.planned_kernels(fast, 777, 777)[0] == "step_fast_sl_kernel"
    for n, planar, no_share in ((5000, False, "0"), (64 * ib, False, "0"), (777, True, "0"), (1, True, "0"), (15, False, "0"), (17, True, "1"),
                                (4099, True, "0"), (2049, False, "1")):
        monkeypatch.setenv("NB_FAST_NO_SHARE", no_share)
        pos, vel = state3d(oracle, n, seed=ib * 100 + slices + n)
        if planar:
            pos[:, 2] = 0
            vel[:, 2] = 0
        outs = []
        for _ in range(2):
            with nb.Scene(pos, vel, fast) as sc:
                sc.step_n(2)
                outs.append(sc.state())
        assert_bits_equal(outs[0][0], outs[1][0], "run-to-run determinism")
        assert_bits_equal(outs[0][1], outs[1][1], "run-to-run determinism (velocities)")
        p, v = outs[0]
        p_ref, v_ref = oracle.run(pos, vel, 2)
        acc = np.abs(v_ref - vel).max()
        assert np.abs(v - v_ref).max() <= 4e-5 * acc + float(np.spacing(np.abs(v_ref).max())), f"n={n}"
        assert np.abs(p - p_ref).max() <= 2e-5, f"n={n}"
    # coordinates of 2^28 and more: the product of two r^2 would overflow; the step's flag must switch sharing off (same bits as forced off)
    monkeypatch.setenv("NB_FAST_IB", "2")
    pos, vel = state3d(oracle, 3000, seed=91)
    pos[5::64] = np.array([3.0e9, -2.5e9, 1.0e9], np.float32) * (1 + np.arange(len(pos[5::64]), dtype=np.float32)[:, None] / 64)
    got = []
    for no_share in ("1", "0"):
        monkeypatch.setenv("NB_FAST_NO_SHARE", no_share)
        with nb.Scene(pos, vel, fast) as sc:
            sc.step_n(1)
            got.append(sc.state())
    assert np.isfinite(got[0][0]).all() and np.isfinite(got[0][1]).all()
    assert_bits_equal(got[1][0], got[0][0], "huge coordinates must take the unshared form")
    assert_bits_equal(got[1][1], got[0][1], "huge coordinates must take the unshared form (velocities)")
    # through the launch API: shards with first != 0 and ragged counts against the whole-set launch of the same form
    n = 6000
    pos, vel = state3d(oracle, n, seed=7)
    monkeypatch.setenv("NB_FAST_NO_SHARE", "0")
    monkeypatch.setenv("NB_FAST_SLICES", "1")          # one chunk per wave x 8 waves, the same chunks for every shard: the same sums
    pw, vw = _sharded_step_on_one_gpu(nb, pos, vel, [(0, n)], fast, 1)
    ps, vs = _sharded_step_on_one_gpu(nb, pos, vel, [(0, 1), (1, 2047), (2048, 3000), (5048, 952)], fast, 1)
    assert_bits_equal(ps, pw, "FAST scalar-load form: shards == whole set (same chunks, same order)")
    assert_bits_equal(vs, vw, "FAST scalar-load form: shards == whole set (velocities)")


@pytest.mark.parametrize("n,w,chunk", [(256, 8, 0), (512, 1, 0), (512, 8, 0), (2048, 2, 0), (2304, 8, 0), (2304, 4, 0), (4096, 1, 0), (4096, 8, 0),
                                       (6400, 8, 0), (6400, 2, 0), (8192, 4, 0), (32768, 0, 0),
                                       (4096, 1, 1024), (6400, 2, 2048), (6400, 1, 256), (8192, 4, 2048), (7168, 8, 4096), (32768, 4, 8192),
                                       # eight bodies per lane (blocks of 512): -w
                                       (512, -1, 0), (1024, -4, 0), (4096, -2, 0), (6656, -4, 0), (8192, -4, 4096), (7168, -2, 2048), (7168, -1, 512)])
def test_fast_pairs_form(nb, oracle, monkeypatch, n, w, chunk):
    """the FAST pairs form (step_fast_pairs_kernel, nb_nbody_sym.inc; what whole sets of 32 768 to 262 144 bodies run): every
    unordered pair evaluated once and credited to both bodies -- the a-side in registers, the b-side in sums that rotate through
    the wave (DPP) and meet in LDS in a fixed order; superblocks against themselves folded the ordered way
    (pairs_diag_kernel); rows added in order (pairs_integrate_kernel).  Every workgroup width w (superblocks of 256 w bodies;
    0 = the plan's own choice; negative: eight bodies per lane instead of four, superblocks of 512 |w|); sizes with one superblock (no pairs kernel at all), whole superblocks, and a last superblock of
    one block (2 304 = 9 blocks, 6 400 = 25); sets walked in chunks (what sets above 262 144 bodies do, at test sizes); planar, 3-D and mixed data, coordinates too large for the shared reciprocal.
    Within FAST's tolerance of the oracle, deterministic from run to run, and within that tolerance of the ordered fold."""
    from nenbody_amd import _lib

    monkeypatch.setenv("NB_FAST_PAIRS", "1")
    monkeypatch.setenv("NB_FAST_PAIRS_NP", "4" if w < 0 else "2")   # bodies per lane: eight (blocks of 512) or four (256)
    w = abs(w)
    if w:
        monkeypatch.setenv("NB_FAST_PAIRS_W", str(w))
    if chunk:   # the two-level walk of sets above 262 144 bodies, at test sizes: tiles of one or two chunks, a ragged last chunk
        monkeypatch.setenv("NB_FAST_PAIRS_CHUNK", str(chunk))
        assert "pairs_accumulate_kernel" in _lib.planned_kernels(nb.default_params(mode=nb.NB_MODE_FAST), n, n)
    assert _lib.planned_kernels(nb.default_params(mode=nb.NB_MODE_FAST), n, n)[0] == "step_fast_pairs_kernel"
    fast = nb.default_params(mode=nb.NB_MODE_FAST)
    for flavour in ("3d", "planar", "mixed", "big"):
        if n > 8192 and flavour != "planar":
            continue
        pos, vel = state3d(oracle, n, seed=n + len(flavour))
        if flavour == "planar":
            pos[:, 2] = 0
            vel[:, 2] = 0
        elif flavour == "mixed":
            pos[:, 2] = 0
            pos[n // 3:n // 3 + 100, 2] = np.linspace(-3, 3, 100, dtype=np.float32)
        elif flavour == "big":
            pos[7] = [3.0e9, -2.5e9, 1.0e9]
            pos[n - 5] = [-4.0e9, 1.0, 7.0e9]
        k = 1 if n > 8192 else 2
        outs = []
        for _ in range(2):
            with nb.Scene(pos, vel, fast) as sc:
                sc.step_n(k)
                outs.append(sc.state())
        assert_bits_equal(outs[0][0], outs[1][0], f"{flavour}: run-to-run determinism")
        assert_bits_equal(outs[0][1], outs[1][1], f"{flavour}: run-to-run determinism (velocities)")
        p, v = outs[0]
        if n > 8192:
            idx = np.unique(np.concatenate([[0, n - 1], np.linspace(0, n - 1, 60).astype(np.int64)]))
            v_ref = np.concatenate([oracle.step_range(pos, vel[i:i + 1], int(i), 1)[1] for i in idx])
            acc = np.abs(v_ref - vel[idx]).max()
            assert np.abs(v[idx] - v_ref).max() <= 4e-5 * acc + float(np.spacing(np.abs(v_ref).max())), flavour
            continue
        p_ref, v_ref = oracle.run(pos, vel, k)
        assert np.isfinite(p).all() and np.isfinite(v).all(), flavour
        acc = np.abs(v_ref - vel).max()
        tol = 4e-5 * acc + float(np.spacing(np.abs(v_ref).max()))
        assert np.abs(v - v_ref).max() <= tol, f"{flavour}: {np.abs(v - v_ref).max():.3e} > {tol:.3e}"
        assert np.abs(p - p_ref).max() <= 4e-5 * acc + float(np.spacing(np.abs(p_ref).max())), flavour
    if n <= 8192:   # the same data through the ordered fold: the two must agree to FAST's tolerance
        monkeypatch.setenv("NB_FAST_PAIRS", "0")
        with nb.Scene(pos, vel, fast) as sc:
            sc.step_n(k)
            p0, v0 = sc.state()
        assert np.abs(v0 - v).max() <= 2 * tol


@pytest.mark.parametrize("waves", [0, 8])
@pytest.mark.parametrize("n,first,count,j_lo,j_hi", [(6000, 0, 6000, 0, 750), (6000, 1500, 750, 1500, 2250), (6000, 5250, 750, 5250, 6000),
                                                     (5001, 1000, 333, 0, 0), (5001, 0, 5001, 0, 5001), (131072, 16384, 16384, 16384, 32768)])
def test_fast_step_in_two_phases_equals_one_call(nb, oracle, monkeypatch, waves, n, first, count, j_lo, j_hi):
    """nb_launch_step_phase: NB_PHASE_RANGE folds records [j_lo, j_hi) (a rank's own slot, present before the all-gather lands),
    NB_PHASE_REST the rest of the set + every partial sum in a fixed order + the integration.  Same law, another order of
    additions: within FAST's tolerance of the one-call step and of the oracle; deterministic; STRICT refuses."""
    import torch

    from nenbody_amd import _lib

    if waves:
        monkeypatch.setenv("NB_FAST_WAVES", str(waves))
    lib = _lib.load()
    pos, vel = state3d(oracle, n, seed=n + first)
    dev = torch.device("cuda", 0)
    cur = torch.zeros((n, 4), dtype=torch.float32)
    cur[:, :3] = torch.from_numpy(pos)
    cur = cur.to(dev)
    fast = nb.default_params(mode=nb.NB_MODE_FAST)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def phased():
        nxt = torch.zeros_like(cur)
        v = torch.zeros((count, 4), dtype=torch.float32)
        v[:, :3] = torch.from_numpy(vel[first:first + count])
        v = v.to(dev)
        sb = lib.nb_scratch_bytes_phased(ctypes.byref(fast), n, count, j_lo, j_hi)
        assert sb >= 2 * count * 16
        scratch = torch.empty((sb,), dtype=torch.uint8, device=dev)
        for phase in (_lib.NB_PHASE_RANGE, _lib.NB_PHASE_REST):
            _lib.check(lib.nb_launch_step_phase(ctypes.byref(fast), n, first, count, j_lo, j_hi, phase, cur.data_ptr(), nxt.data_ptr(),
                                               v.data_ptr(), scratch.data_ptr(), sb, stream))
        torch.cuda.synchronize()
        return nxt[first:first + count, :3].cpu().numpy(), v[:, :3].cpu().numpy()

    p2, v2 = phased()
    p2b, v2b = phased()
    assert_bits_equal(p2, p2b, "run-to-run determinism")
    assert_bits_equal(v2, v2b, "run-to-run determinism (velocities)")
    idx = np.unique(np.concatenate([[0, count - 1], np.linspace(0, count - 1, 24).astype(np.int64)]))
    scale = 0.0
    for i in idx:
        p_ref, v_ref = oracle.step_range(pos, vel[first + i:first + i + 1], int(first + i), 1)
        scale = max(scale, float(np.abs(v_ref[0] - vel[first + i]).max()))
    for i in idx:
        p_ref, v_ref = oracle.step_range(pos, vel[first + i:first + i + 1], int(first + i), 1)
        assert np.abs(v2[i] - v_ref[0]).max() <= 4e-5 * scale + 1e-9, f"body {first + i}"
        assert np.abs(p2[i] - p_ref[0]).max() <= 4e-5 * scale + 1e-5, f"body {first + i}"
    strict = nb.default_params()
    assert lib.nb_scratch_bytes_phased(ctypes.byref(strict), n, count, j_lo, j_hi) == 0
    rc = lib.nb_launch_step_phase(ctypes.byref(strict), n, first, count, j_lo, j_hi, 0, cur.data_ptr(), cur.data_ptr() + 16, cur.data_ptr(),
                                  cur.data_ptr(), 1 << 30, stream)
    assert rc == _lib.NB_ERR_UNSUPPORTED and "order" in _lib.last_error()


def test_fast_shared_reciprocal_guard(nb, oracle, monkeypatch):
    """FAST takes two reciprocals from one v_rcp_f32 (1/a = b * rcp(a*b)) where the product cannot leave binary32's normal
    range.  Huge coordinates, and a bias outside [2^-60, 2^60], must fall back to one reciprocal per pair: same bits as with
    sharing switched off (unguarded, the product of two r^2 ~ 1e19 overflows and both pairs silently contribute 0)."""
    monkeypatch.setenv("NB_FAST_IB", "2")     # sets this small would take one body per lane, which has no pair to share with
    n = 3000
    pos, vel = state3d(oracle, n, seed=91)
    # |c| >= 2^28: r^2 ~ 1e19, the product of two of them overflows.  One such body in every 64 records, so that EVERY tile
    # (and every wave's own bodies) must fall back -- the other tiles would legitimately differ between the two settings
    pos[5::64] = np.array([3.0e9, -2.5e9, 1.0e9], np.float32) * (1 + np.arange(len(pos[5::64]), dtype=np.float32)[:, None] / 64)
    fast = nb.default_params(mode=nb.NB_MODE_FAST)

    def run(no_share):
        monkeypatch.setenv("NB_FAST_NO_SHARE", "1" if no_share else "0")
        with nb.Scene(pos, vel, fast) as sc:
            sc.step_n(1)
            return sc.state()

    p0, v0 = run(True)
    p1, v1 = run(False)
    assert np.isfinite(p0).all() and np.isfinite(v0).all()
    assert_bits_equal(p1, p0, "tiles with huge coordinates must take the unshared form")
    assert_bits_equal(v1, v0, "tiles with huge coordinates must take the unshared form (velocities)")
    # a bias the product form cannot take: the host switches sharing off, so both settings give the same bits
    tiny = nb.default_params(mode=nb.NB_MODE_FAST)
    tiny.bias = 1e-30
    pos2, vel2 = state3d(oracle, 2000, seed=92)
    outs = []
    for no_share in ("1", "0"):
        monkeypatch.setenv("NB_FAST_NO_SHARE", no_share)
        with nb.Scene(pos2, vel2, tiny) as sc:
            sc.step_n(2)
            outs.append(sc.state())
    assert_bits_equal(outs[0][0], outs[1][0], "bias below 2^-60")
    # and on ordinary data the two forms agree to a few ulp of the force
    monkeypatch.setenv("NB_FAST_NO_SHARE", "1")
    with nb.Scene(pos2, vel2, fast) as sc:
        sc.step_n(1)
        pa, va = sc.state()
    monkeypatch.setenv("NB_FAST_NO_SHARE", "0")
    with nb.Scene(pos2, vel2, fast) as sc:
        sc.step_n(1)
        pb, vb = sc.state()
    assert (va.view(np.uint32) != vb.view(np.uint32)).any(), "the shared form was not taken on ordinary data"
    dv = np.abs(va - vb).max()
    assert dv <= 1e-6 * np.abs(va - vel2).max() + 1.5e-8, dv   # + two ulp of a velocity of 0.1, where the sums are rounded into


def test_fast_is_deterministic(nb, oracle, monkeypatch):
    monkeypatch.setenv("NB_FAST_SLICES", "8")
    pos, vel = state3d(oracle, 4096, seed=41)
    outs = []
    for _ in range(2):
        with nb.Scene(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST)) as sc:
            sc.step_n(3)
            outs.append(sc.state())
    assert_bits_equal(outs[0][0], outs[1][0])


# ---------------------------------------------------------------------------------------------------------
# the reference's operator interface
# ---------------------------------------------------------------------------------------------------------
def test_update_instance_nbody_matches_reference_semantics(nb, oracle):
    n = 300
    pos, vel = state3d(oracle, n, seed=51)
    p_ref, v_ref, inst_ref = oracle.run(pos, vel, 1, want_instances=True)
    positions, velocities = pos.copy(), vel.copy()
    old_p, old_v = np.zeros_like(pos), np.zeros_like(vel)
    inst = np.zeros((n, 4, 4), np.float32)
    nb.update_instance_nbody(inst, positions, old_p, velocities, old_v)
    assert_bits_equal(old_p, pos)          # main.rs:415
    assert_bits_equal(old_v, vel)          # main.rs:416
    assert_bits_equal(positions, p_ref)
    assert_bits_equal(velocities, v_ref)
    assert matrices_equal(inst, inst_ref)
    assert (inst[:, 3, :3] == positions).all()       # translation column is the new position, exactly


@pytest.mark.parametrize("zero_copy", ["1", "0"], ids=["kernels-touch-pinned-host-memory", "staged-by-dma-copies"])
@pytest.mark.parametrize("n", [100, 2048, 5000])
def test_small_set_transfers_both_ways(nb, oracle, monkeypatch, zero_copy, n):
    """Sets of up to 16 384 bodies cross the bus through one pinned buffer; by default the pack / unpack kernels read and write
    it through the bus themselves, NB_DROPIN_ZERO_COPY=0 stages it with a DMA copy each way.  Same results either way, in the
    drop-in calls (n-body over frames, boids) and in Scene's upload / step / download."""
    monkeypatch.setenv("NB_DROPIN_ZERO_COPY", zero_copy)
    pos, vel = state3d(oracle, n, seed=300 + n)
    p_ref, v_ref, inst_ref = oracle.run(pos, vel, 2, want_instances=True)
    p, v = pos.copy(), vel.copy()
    op, ov, inst = np.zeros_like(p), np.zeros_like(v), np.zeros((n, 4, 4), np.float32)
    for _ in range(2):
        nb.update_instance_nbody(inst, p, op, v, ov)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)
    assert matrices_equal(inst, inst_ref)
    pb, vb = pos.copy(), vel.copy()
    nb.update_instance_boids(inst, pb, op, vb, ov)
    pb_ref, vb_ref = oracle.boids_run(pos, vel, 1)
    assert_bits_equal(pb, pb_ref)
    assert_bits_equal(vb, vb_ref)
    with nb.Scene(pos, vel) as sc:
        sc.step()
        sc.step()
        assert_bits_equal(sc.positions(), p_ref)
        assert_bits_equal(sc.velocities(), v_ref)
        assert matrices_equal(sc.instances(), inst_ref)


@pytest.mark.parametrize("n,m", [(200, 50), (20000, 70)])   # both transfer paths of the drop-in call (small / large sets)
def test_update_instance_nbody_zip_truncation(nb, oracle, n, m):
    """instances shorter than positions: only that many bodies move, the fold still sees everyone (main.rs:420-425)."""
    pos, vel = state3d(oracle, n, seed=52)
    p_ref, v_ref = oracle.step_range(pos, vel[:m], 0, m)
    positions, velocities = pos.copy(), vel.copy()
    inst = np.zeros((m, 4, 4), np.float32)
    nb.update_instance_nbody(inst, positions, np.zeros_like(pos), velocities, np.zeros_like(vel))
    assert_bits_equal(positions[:m], p_ref)
    assert_bits_equal(velocities[:m], v_ref)
    assert_bits_equal(positions[m:], pos[m:])
    assert_bits_equal(velocities[m:], vel[m:])


def test_update_instance_nbody_short_velocity_slice(nb, oracle):
    """velocities shorter than positions: the zip stops there (main.rs:420-423); old_velocities is never read by the
    n-body fold, so this is legal in the reference."""
    n, m = 180, 33
    pos, vel = state3d(oracle, n, seed=54)
    p_ref, v_ref = oracle.step_range(pos, vel[:m], 0, m)
    positions, velocities = pos.copy(), vel[:m].copy()
    inst = np.full((n, 4, 4), 7, np.float32)
    nb.update_instance_nbody(inst, positions, np.zeros_like(pos), velocities, np.zeros_like(velocities))
    assert_bits_equal(positions[:m], p_ref)
    assert_bits_equal(velocities, v_ref)
    assert_bits_equal(positions[m:], pos[m:])
    assert (inst[m:] == 7).all() and (inst[:m, 3, :3] == positions[:m]).all()


def test_update_instance_nbody_called_every_frame(nb, oracle):
    """The call-site shape of main.rs:925-931: the same Vecs every frame.  The library keeps its device context between
    calls and must rebuild it when the body count or the constants change."""
    from nenbody_amd import _lib

    for n, frames, params in ((256, 4, None), (700, 2, None), (700, 2, nb.default_params(mode=nb.NB_MODE_STRICT, tile=256)),
                              (5000, 2, None), (17000, 2, None), (256, 1, None)):   # 5 000: block-chain kernel + one-copy round trip
        pos, vel = state3d(oracle, n, seed=60 + n)
        positions, velocities = pos.copy(), vel.copy()
        old_p, old_v = np.zeros_like(pos), np.zeros_like(vel)
        inst = np.zeros((n, 4, 4), np.float32)
        for _ in range(frames):
            nb.update_instance_nbody(inst, positions, old_p, velocities, old_v, params)
        p_ref, v_ref = oracle.run(pos, vel, frames)
        assert_bits_equal(positions, p_ref, f"n={n}")
        assert_bits_equal(velocities, v_ref, f"n={n}")
    # non-default constants reach the kernel
    n = 128
    pos, vel = state3d(oracle, n, seed=77)
    prm = _lib.default_params()
    prm.dt, prm.G, prm.bias = 0.05, 0.01, 1e-3
    positions, velocities = pos.copy(), vel.copy()
    nb.update_instance_nbody(np.zeros((n, 4, 4), np.float32), positions, np.zeros_like(pos), velocities, np.zeros_like(vel), prm)
    p_ref, v_ref = oracle.run(pos, vel, 1, dt=0.05, g=0.01, bias=1e-3)
    assert_bits_equal(positions, p_ref)
    assert_bits_equal(velocities, v_ref)
    nb.update_release()
    nb.update_release()  # idempotent
    nb.update_instance_nbody(np.zeros((n, 4, 4), np.float32), positions, np.zeros_like(pos), velocities, np.zeros_like(vel), prm)
    p_ref, v_ref = oracle.run(p_ref, v_ref, 1, dt=0.05, g=0.01, bias=1e-3)
    assert_bits_equal(positions, p_ref)


@pytest.mark.parametrize("n", [1, 100, 255, 256, 257, 1000, 2048, 2049])
def test_small_set_dropin_waits_on_the_word_the_export_kernel_writes(nb, oracle, monkeypatch, n):
    """Up to 2 048 bodies the drop-in calls (and Scene's download) do not wait on the stream: the export kernel's LAST workgroup writes
    a sequence number behind the results in the mapped host buffer once every workgroup's stores are home, and the host polls that
    word (nb_api.hip: wait_export; ~4 us per call, tools/ubench_sync.hip).  Held here: the results are the stream-wait path's bits
    (NB_DROPIN_POLL=0) frame after frame -- sets of one workgroup and of several, one past the line -- for both controllers and
    Scene.step, and a long run of calls (the word's sequence, the counter left at zero, the periodic stream wait) stays exact."""
    pos, vel = state3d(oracle, n, seed=900 + n)
    frames = 6
    got = {}
    for poll in ("0", "1"):
        monkeypatch.setenv("NB_DROPIN_POLL", poll)
        positions, velocities = pos.copy(), vel.copy()
        old_p, old_v = np.zeros_like(pos), np.zeros_like(vel)
        inst = np.zeros((n, 4, 4), np.float32)
        for _ in range(frames):
            nb.update_instance_nbody(inst, positions, old_p, velocities, old_v)
        pb, vb, instb = positions.copy(), velocities.copy(), np.zeros((n, 4, 4), np.float32)
        for _ in range(2):
            nb.update_instance_boids(instb, pb, old_p, vb, old_v)
        with nb.Scene(pos, vel) as sc:
            for _ in range(3):
                sc.step()          # one step + download of positions, velocities and matrices
            ps, vs, ins = sc.positions().copy(), sc.velocities().copy(), sc.instances().copy()
        got[poll] = (positions, velocities, inst.copy(), pb, vb, instb, ps, vs, ins)
        nb.update_release()
    for a, b in zip(got["0"], got["1"]):
        assert_bits_equal(a, b)
    p_ref, v_ref = oracle.run(pos, vel, frames)
    assert_bits_equal(got["1"][0], p_ref)
    assert_bits_equal(got["1"][1], v_ref)
    if n == 100:   # the reference's default entity_count: 2 500 consecutive frames against the oracle's
        monkeypatch.setenv("NB_DROPIN_POLL", "1")
        positions, velocities = pos.copy(), vel.copy()
        old_p, old_v = np.zeros_like(pos), np.zeros_like(vel)
        inst = np.zeros((n, 4, 4), np.float32)
        for _ in range(2500):
            nb.update_instance_nbody(inst, positions, old_p, velocities, old_v)
        p_ref, v_ref, inst_ref = oracle.run(pos, vel, 2500, want_instances=True)
        assert_bits_equal(positions, p_ref)
        assert_bits_equal(velocities, v_ref)
        assert matrices_equal(inst, inst_ref)


def test_small_set_dropin_poll_backs_off_after_a_timeout(nb, oracle, monkeypatch):
    """The polled wait is adaptive: with a poll budget of ZERO every polled call times out at once, falls back to the
    stream wait, re-zeroes the export counter and keeps the next 64, 128, ... calls of the context off the word altogether
    (NB_DROPIN_POLL_BUDGET_US: the knob only the tests throw).  300 frames mix timed-out polls and held-off calls: every frame must
    still be the oracle's, and when the budget is given back the word is polled again and still right."""
    n = 100
    pos, vel = state3d(oracle, n, seed=77)
    monkeypatch.setenv("NB_DROPIN_POLL", "1")
    monkeypatch.setenv("NB_DROPIN_POLL_BUDGET_US", "0")
    positions, velocities = pos.copy(), vel.copy()
    old_p, old_v = np.zeros_like(pos), np.zeros_like(vel)
    inst = np.zeros((n, 4, 4), np.float32)
    for _ in range(300):
        nb.update_instance_nbody(inst, positions, old_p, velocities, old_v)
    p_ref, v_ref = oracle.run(pos, vel, 300)
    assert_bits_equal(positions, p_ref)
    assert_bits_equal(velocities, v_ref)
    monkeypatch.delenv("NB_DROPIN_POLL_BUDGET_US")
    for _ in range(200):   # (the hold-off of the last timeout runs out inside these calls)
        nb.update_instance_nbody(inst, positions, old_p, velocities, old_v)
    p_ref, v_ref, inst_ref = oracle.run(pos, vel, 500, want_instances=True)
    assert_bits_equal(positions, p_ref)
    assert_bits_equal(velocities, v_ref)
    assert matrices_equal(inst, inst_ref)
    nb.update_release()


def test_scene_step_refreshes_host_mirrors(nb, oracle):
    pos, vel = state3d(oracle, 100, seed=53)
    with nb.Scene.from_state(pos, vel) as sc:
        sc.step()
        p1, v1, i1 = sc._positions.copy(), sc._velocities.copy(), sc._instances.copy()
        assert sc.steps_done == 1
    p_ref, v_ref, inst_ref = oracle.run(pos, vel, 1, want_instances=True)
    assert_bits_equal(p1, p_ref)
    assert_bits_equal(v1, v_ref)
    assert matrices_equal(i1, inst_ref)


def test_instances_edge_cases(nb, oracle):
    pos = np.array([[1, 2, 3], [0, 0, 0], [-5, 1e6, -1e-6], [7, 7, 7]], np.float32)
    vel = np.array([[0, 0, 0], [-1, 0, 0], [0, -2, 5], [1e-20, 1e-20, 0]], np.float32)   # atan2(0,0)=0; heading -x; -y
    import torch

    from nenbody_amd.dist import HipBackend

    dev = torch.device("cuda", 0)
    pr = torch.zeros((4, 4)); pr[:, :3] = torch.from_numpy(pos)
    vr = torch.zeros((4, 4)); vr[:, :3] = torch.from_numpy(vel)
    inst = torch.zeros((4, 16), device=dev)
    HipBackend().instances(4, pr.to(dev), vr.to(dev), inst)
    torch.cuda.synchronize()
    got = inst.cpu().numpy().reshape(4, 4, 4)
    ref = oracle.instances(pos, vel)
    assert matrices_equal(got, ref)
    assert (got[:, 3, :3] == pos).all() and (got[:, 3, 3] == 1).all() and (got[:, 2] == [0, 0, 1, 0]).all()


# ---------------------------------------------------------------------------------------------------------
# several ranks on the one GPU of this box (gloo, positions gathered through the host): the real multi-rank
# control flow with the real HIP kernels.  RCCL itself needs one GPU per rank and is the driver's to run.
# ---------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, n, k, mode, out_dir, overlap=False, boids_split=False, state=None, schedule=None, nbody=None):
    """one rank of a ShardedScene world on the one GPU: k n-body steps; or with `schedule` ((what, k) or (what, k, boids constants
    as a dict)) those steps, boids through step_boids(split=boids_split), on state = (pos, vel) with n-body constants `nbody`
    ({dt, G, bias}), the state after every entry saved as pos_<i>, vel_<i>"""
    import sys

    from conftest import ROOT

    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import nenbody_amd

        torch.cuda.set_device(0)
        if state is None:
            pos, vel = nenbody_amd.init_state(n, 99)
            pos[:, 2] = np.linspace(-50, 50, n, dtype=np.float32)
        else:
            pos, vel = state
        params = nenbody_amd.default_params(mode=mode)
        for name, value in (nbody or {}).items():
            setattr(params, name, value)
        sc = nenbody_amd.ShardedScene(pos, vel, params, overlap=overlap)
        assert sc.overlap == (overlap and mode == nenbody_amd.NB_MODE_FAST)
        every = {}
        for i, (what, steps, *consts) in enumerate(schedule or (("nbody", k),)):
            if what == "nbody":
                sc.step_n(steps)
            else:
                bp = nenbody_amd.default_boids_params()
                for name, value in (consts[0] if consts else {}).items():
                    setattr(bp, name, value)
                for _ in range(steps):
                    sc.step_boids(bp, split=boids_split)
                scratch = getattr(sc, "_boids_partial", None)
                if boids_split and scratch is not None:   # the split form's scratch: its size and the step's flag word at its end
                    nbytes = scratch.numel()
                    every[f"scratch_{i}"] = nbytes
                    every[f"flags_{i}"] = int(scratch[nbytes - 64:nbytes - 60].cpu().numpy().view(np.uint32)[0])
            sc.sync()
            every[f"pos_{i}"], every[f"vel_{i}"] = sc.positions(), sc.velocities()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), pos=sc.positions(), vel=sc.velocities(), **every)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 4096), (3, 1000)])
def test_multirank_on_one_gpu_strict_equals_oracle(tmp_path, nb, oracle, world, n):
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    k = 3
    mp.spawn(_rank_worker, args=(world, port, n, k, nb.NB_MODE_STRICT, str(tmp_path)), nprocs=world, join=True)
    pos, vel = nb.init_state(n, 99)
    pos[:, 2] = np.linspace(-50, 50, n, dtype=np.float32)
    p_ref, v_ref = oracle.run(pos, vel, k)
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        assert_bits_equal(got["pos"], p_ref, f"rank {r} positions")
        assert_bits_equal(got["vel"], v_ref, f"rank {r} velocities")


@pytest.mark.parametrize("world,n", [(2, 4096), (3, 1000), (3, 20000)])
def test_multirank_on_one_gpu_fast_with_overlapped_exchange(tmp_path, nb, oracle, world, n):
    """FAST with overlap=True, real kernels, 2-3 ranks sharing the GPU (gloo exchange): every step folds the rank's own slot
    first (NB_PHASE_RANGE), then the rest after the exchange (NB_PHASE_REST).  Within FAST's tolerance of the oracle on every
    rank.  (No performance claim: the overlap needs one GPU per rank and RCCL to show.)"""
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    k = 3
    mp.spawn(_rank_worker, args=(world, port, n, k, nb.NB_MODE_FAST, str(tmp_path), True), nprocs=world, join=True)
    pos, vel = nb.init_state(n, 99)
    pos[:, 2] = np.linspace(-50, 50, n, dtype=np.float32)
    p_ref, v_ref = oracle.run(pos, vel, k)
    acc = np.abs(v_ref - vel).max()
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        assert np.abs(got["vel"] - v_ref).max() <= 4e-5 * acc + 1e-9, f"rank {r}"
        assert np.abs(got["pos"] - p_ref).max() <= 2e-5, f"rank {r}"


def _peers_worker(rank, world, port, n, k, mode, out_dir, what):
    import sys

    from conftest import ROOT

    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import nenbody_amd

        torch.cuda.set_device(0)
        if what.startswith("ring"):
            os.environ["NB_RING"] = "1"       # (sets this small keep the ordered fold by themselves)
            nenbody_amd.reload_env()
        pos, vel = nenbody_amd.init_state(n, 99)
        p = nenbody_amd.default_params(mode=mode)
        if what == "choose":   # the collectives (here: gloo through the host) against the pulls, timed; the state must come back
            sc = nenbody_amd.ShardedScene(pos, vel, p)
            sc.step()
            before = (sc.positions().copy(), sc.velocities().copy())
            chosen = sc.choose_exchange(steps=2, warm=1)
            assert chosen in ("peers", "collective") and set(sc.exchange_times) == {"peers", "collective"} and sc.exchange == chosen
            # (the report describes the exchange kept; the collectives were verified first, on their own)
            assert sc.exchange_report["all_gather"] == ("peers" if chosen == "peers" else "in_place") and sc.exchange_report["verified"]
            assert sc.exchange_report["collective"] == {"all_gather": "in_place", "ring_exchange": None}, sc.exchange_report
            assert (sc.positions() == before[0]).all() and (sc.velocities() == before[1]).all()
            sc.step_n(k - 1)
        elif what in ("ring_lossy", "ring_stale"):   # rank 0's pulls lose a record / deliver only the first time (a stale cache: the SECOND
            # pattern round catches it): every rank goes back to the collectives for both exchanges
            sc = nenbody_amd.ShardedScene(pos, vel, p, exchange="peers", ring=True)
            nenbody_amd.load().nb_diag_peers_lossy(1 if what == "ring_lossy" else 2)
            try:
                rep = sc.verify_exchanges()
            finally:
                nenbody_amd.load().nb_diag_peers_lossy(0)
            assert rep["all_gather"] == "in_place" and rep["ring_exchange"] == "grouped" and sc.exchange == "collective" and sc.partners, rep
            sc.step_n(k)
        else:
            sc = nenbody_amd.ShardedScene(pos, vel, p, exchange="peers", ring=True if what.startswith("ring") else None,
                                          ring_overlap=what == "ring_overlap", overlap=what == "overlap")
            assert sc.exchange == "peers"
            rep = sc.verify_exchanges()
            assert rep["all_gather"] == "peers" and rep["ring_exchange"] == ("peers" if sc.partners else None) and sc.exchange == "peers", rep
            real = dist.all_gather_into_tensor
            calls = []
            dist.all_gather_into_tensor = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
            sc.step_n(k)
            sc.sync()
            dist.all_gather_into_tensor = real
            assert not calls, "a step went through the collective"
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), pos=sc.positions(), vel=sc.velocities())
        sc.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,what", [(2, 4096, "strict"), (3, 1000, "strict"), (3, 20000, "overlap"), (4, 16384, "ring"), (4, 16384, "ring_overlap"),
                                          (2, 8192, "ring_overlap"), (3, 4096, "choose"), (4, 16384, "ring_lossy"), (4, 16384, "ring_stale")])
def test_sharded_scene_pulls_its_exchanges_over_ipc(tmp_path, nb, oracle, world, n, what):
    """ShardedScene(exchange="peers"): the all-gather and the pairs form's second exchange as pulls over IPC-mapped buffers, ordered by
    stream value waits (nb_peers_*), between PROCESSES sharing the one GPU; torch.distributed only carries the handles.  Every step
    is checked not to touch a collective; STRICT (a ragged world too) bit-identical to the oracle, the FAST forms -- ordered fold with
    the pull behind the own slot's fold, the pairs form in sequence and in phases -- at FAST's tolerance; verify_exchanges reports the
    pulls verified; choose_exchange times them against the collectives and puts the state back; pulls made lossy on one rank, or whole
    the first time only (nb_diag_peers_lossy 1 / 2), send every rank back to the collectives."""
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    k = 3
    mode = nb.NB_MODE_STRICT if what in ("strict", "choose") else nb.NB_MODE_FAST
    mp.spawn(_peers_worker, args=(world, port, n, k, mode, str(tmp_path), what), nprocs=world, join=True)
    pos, vel = nb.init_state(n, 99)
    p_ref, v_ref = oracle.run(pos, vel, k)
    acc = np.abs(v_ref - vel).max()
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        if mode == nb.NB_MODE_STRICT:
            assert_bits_equal(got["pos"], p_ref, f"rank {r} positions")
            assert_bits_equal(got["vel"], v_ref, f"rank {r} velocities")
        else:
            assert np.abs(got["vel"] - v_ref).max() <= 4e-5 * acc + 1e-9, f"rank {r}"
            assert np.abs(got["pos"] - p_ref).max() <= 2e-5, f"rank {r}"


def _rccl_world_of_one(rank, port, n, k, out_dir):
    import sys

    from conftest import ROOT

    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        import nenbody_amd

        pos, vel = nenbody_amd.init_state(n, 5)
        sc = nenbody_amd.ShardedScene(pos, vel)
        assert dist.get_backend() == "nccl"
        for _ in range(k):
            sc.step()
            sc._all_gather_slots(sc.pos[sc.cur])  # the exchange bench.py --gpus N runs, here with one contributor
            sc.step_boids()
            sc._all_gather_slots(sc.velfull[sc.cur])
        sc.sync()
        np.savez(os.path.join(out_dir, "rccl.npz"), pos=sc.positions(), vel=sc.velocities())
    finally:
        dist.destroy_process_group()


def test_rccl_in_place_all_gather_world_of_one(tmp_path, nb, oracle):
    """The RCCL leg itself (backend "nccl", send buffer = this rank's slot of the receive buffer) with the one rank this
    box can give it: the collective must run on torch's stream between the kernels and leave the replica untouched."""
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    n, k = 3000, 2
    mp.spawn(_rccl_world_of_one, args=(port, n, k, str(tmp_path)), nprocs=1, join=True)
    pos, vel = nb.init_state(n, 5)
    for _ in range(k):
        pos, vel = oracle.run(pos, vel, 1)
        pos, vel = oracle.boids_run(pos, vel, 1)
    got = np.load(os.path.join(str(tmp_path), "rccl.npz"))
    assert_bits_equal(got["pos"], pos, "positions")
    assert_bits_equal(got["vel"], vel, "velocities")


# ---------------------------------------------------------------------------------------------------------
# the STRICT division ladder itself, against the IEEE divide, over the whole guarded exponent rectangle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g_,bias", [(0.001, 1e-7), (0.5, 0.01), (-2.0, 3.0), (1e-6, 1e-12)])
def test_strict_division_ladder_equals_ieee_divide(nb, g_, bias):
    """2^37 (1.4e11) random (numerator, denominator) pairs per parameter set, structured mantissas included: the shared-reciprocal
    ladder STRICT uses inside the range guard must reproduce the correctly rounded quotient every time."""
    from nenbody_amd import _lib

    p = nb.default_params()
    p.G, p.bias = g_, bias
    bad = ctypes.c_uint64(123)
    pair = np.zeros(2, np.float32)
    rc = _lib.load().nb_selftest_divide(ctypes.byref(p), 1 << 37, 2024, ctypes.byref(bad), pair.ctypes.data)
    assert rc == 0, _lib.last_error()
    assert bad.value == 0, f"{bad.value} mismatches, e.g. n={pair[0]!r} d={pair[1]!r}"


def test_strict_division_ladder_is_exact_for_every_pair_of_significands(nb):
    """The proof STRICT's arithmetic rests on: with normal intermediates the ladder's result depends on the two 24-bit
    significands only, and here ALL 2^23 x 2^23 of them are compared with the IEEE divide (7.0e13 pairs; under a minute)."""
    from nenbody_amd import _lib

    lib = _lib.load()
    bad = ctypes.c_uint64(123)
    pair = np.zeros(2, np.float32)
    rc = lib.nb_selftest_ladder(0, 1 << 23, ctypes.byref(bad), pair.ctypes.data)
    assert rc == 0, _lib.last_error()
    assert bad.value == 0, f"{bad.value} mismatches, e.g. n={pair[0]!r} d={pair[1]!r}"


def test_rcp_commutes_with_scaling_over_the_whole_normal_range(nb):
    """The one step of the ladder that is not IEEE arithmetic: v_rcp_f32(m * 2^k) == v_rcp_f32(m) * 2^-k for every significand."""
    from nenbody_amd import _lib

    lib = _lib.load()
    bad = ctypes.c_uint64(123)
    assert lib.nb_selftest_rcp_scaling(-125, 125, ctypes.byref(bad)) == 0, _lib.last_error()
    assert bad.value == 0
    assert lib.nb_selftest_rcp_scaling(-126, 0, ctypes.byref(bad)) == _lib.NB_ERR_INVALID


def test_ladder_enumeration_can_fail(nb, monkeypatch):
    """Control arm: the same steps on the UNREFINED reciprocal differ from '/' for some significands, and the run reports them."""
    from nenbody_amd import _lib

    lib = _lib.load()
    monkeypatch.setenv("NB_SELFTEST_CONTROL", "1")
    bad = ctypes.c_uint64(0)
    pair = np.zeros(2, np.float32)
    # the last 2^16 denominator significands (mantissas near 2) hold most of the failures
    assert lib.nb_selftest_ladder((1 << 23) - (1 << 16), 1 << 16, ctypes.byref(bad), pair.ctypes.data) == 0, _lib.last_error()
    assert bad.value > 0 and 1.0 <= pair[0] < 2.0 and 1.0 <= pair[1] < 2.0
    assert np.float32(pair[0]) / np.float32(pair[1]) != 0  # a usable counter-example came back
    assert lib.nb_selftest_ladder(1 << 23, 1, ctypes.byref(bad), None) == _lib.NB_ERR_INVALID
    assert lib.nb_selftest_ladder(0, 0, ctypes.byref(bad), None) == _lib.NB_ERR_INVALID


def test_division_selftest_can_fail(nb, monkeypatch):
    """Control arm: comparing the uncorrected product n * (1/d) with the IEEE quotient must report mismatches (a few
    percent of the draws are one ulp off) -- i.e. the self-test is able to fail."""
    from nenbody_amd import _lib

    monkeypatch.setenv("NB_SELFTEST_CONTROL", "1")
    bad = ctypes.c_uint64(0)
    pair = np.zeros(2, np.float32)
    pairs = 1 << 30
    rc = _lib.load().nb_selftest_divide(None, pairs, 7, ctypes.byref(bad), pair.ctypes.data)
    assert rc == 0, _lib.last_error()
    assert 0.001 * pairs < bad.value < 0.6 * pairs
    assert np.isfinite(np.float32(pair[0]) / np.float32(pair[1]))


def test_selftest_refuses_parameters_without_a_guarded_range(nb):
    from nenbody_amd import _lib

    p = nb.default_params()
    p.bias = 0.0            # no softening: d can be 0 -> STRICT always uses the IEEE divide
    bad = ctypes.c_uint64(0)
    assert _lib.load().nb_selftest_divide(ctypes.byref(p), 1024, 1, ctypes.byref(bad), None) == _lib.NB_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------
# the block chain's give-up path is an ERROR at the ABI, never NaN with NB_OK
# ---------------------------------------------------------------------------------------------------------
def test_block_chain_give_up_is_reported_as_an_error(nb, oracle, monkeypatch):
    """A wave of the block-chain kernel that exhausts its polls stops waiting (so the grid drains) and poisons its
    workgroup's outputs; the library must then fail the next call that waits for the device with NB_ERR_STATE.
    NB_BC_SPIN_BUDGET=1 (one poll per wait) forces it.  Afterwards the same process runs the same set correctly."""
    from nenbody_amd import _lib

    n = 8192
    pos, vel = oracle.init_state(n, seed=77)
    monkeypatch.setenv("NB_STRICT_BC", "1")
    monkeypatch.setenv("NB_BC_SPIN_BUDGET", "1")
    with nb.Scene(pos, vel) as sc:
        sc.step_n(1)
        with pytest.raises(nb.NbError) as e:
            sc.sync()
        assert e.value.status == _lib.NB_ERR_STATE and "gave up" in str(e.value)
        sc.sync()  # reported once; the word is cleared
    with nb.Scene(pos, vel) as sc:  # the download path reports it too
        sc.step_n(1)
        with pytest.raises(nb.NbError) as e:
            sc.state()
        assert e.value.status == _lib.NB_ERR_STATE
    # the one-call drop-in: the status word rides home in its transfer buffer (written there by the unpack kernel, or staged)
    for zero_copy in ("1", "0"):
        monkeypatch.setenv("NB_DROPIN_ZERO_COPY", zero_copy)
        p, v = pos.copy(), vel.copy()
        with pytest.raises(nb.NbError) as e:
            nb.update_instance_nbody(np.zeros((n, 4, 4), np.float32), p, np.zeros_like(p), v, np.zeros_like(v))
        assert e.value.status == _lib.NB_ERR_STATE, zero_copy
    monkeypatch.delenv("NB_DROPIN_ZERO_COPY")
    nb.update_release()
    # launch API: nb_launch_status
    import torch

    sh = nb.ShardedScene(pos, vel, world=1, rank=0)
    sh.step()
    with pytest.raises(nb.NbError) as e:
        sh.sync()
    assert e.value.status == _lib.NB_ERR_STATE
    sh.sync()
    del sh
    torch.cuda.synchronize()
    monkeypatch.delenv("NB_BC_SPIN_BUDGET")
    with nb.Scene(pos, vel) as sc:
        sc.step_n(2)
        sc.sync()
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 2)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)


def test_block_chain_ieee_fallback_in_the_same_kernel(nb, oracle, monkeypatch):
    """The IEEE-divide form of the block chain is a function call inside the one kernel: data that leaves the ladder's
    proven range (a coordinate of 2^21, an infinity) must select it and give the oracle's bits, for own and foreign bodies."""
    n = 6000
    pos, vel = state3d(oracle, n, seed=5)
    pos[17, 0] = np.float32(2.0 ** 21)      # outside [2^-43, 2^20]
    pos[4000, 1] = np.float32(-3.0e-30)     # tiny, outside the range too
    monkeypatch.setenv("NB_STRICT_BC", "1")
    with nb.Scene(pos, vel) as sc:
        sc.step_n(2)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 2)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)


def test_roctx_ranges_do_not_change_results(nb, oracle, monkeypatch):
    """NB_ROCTX=1 brackets the step loops with roctx ranges (dlopen of the roctx library at first use): same bits."""
    monkeypatch.setenv("NB_ROCTX", "1")
    pos, vel = state3d(oracle, 700, seed=3)
    with nb.Scene(pos, vel) as sc:
        sc.step_n(3)
        p, v = sc.state()
    p_ref, v_ref = oracle.run(pos, vel, 3)
    assert_bits_equal(p, p_ref)
    assert_bits_equal(v, v_ref)
    with nb.NativeShard(pos, vel) as sh:
        sh.step(2)
        assert_bits_equal(sh.positions(), oracle.run(pos, vel, 2)[0])


def test_valu_rate_streams_are_sane(nb):
    """nb_selftest_valu_rate: the three yardsticks bench.py prints (pure fma, the folds' mix as plain instructions, the same mix
    as packed instructions) are positive, below the spec lane rate, and ordered as measured: fma < mix <= packed mix."""
    lib = nb.load()
    rates, clocks = [], []
    for mix in (0, 1, 2, 3, 4):
        r, mhz = ctypes.c_double(), ctypes.c_double()
        assert lib.nb_selftest_valu_rate(mix, 0.02, ctypes.byref(r), ctypes.byref(mhz)) == 0
        rates.append(r.value)
        clocks.append(mhz.value)
    spec = 256 * 128 * 2.4e9          # lanes x clock: 7.9e13 lane-operations/s
    assert all(1e13 < x < 1.05 * spec for x in rates), rates
    assert rates[0] < rates[1] <= 1.2 * rates[2] and rates[2] > 0.9 * rates[1], rates
    # the clock each stream was stamped at (s_memtime against the 100 MHz s_memrealtime): a shader clock, at most the 2.4 GHz peak
    assert all(900.0 < c < 2500.0 for c in clocks), clocks
    # source registers of their own per chain (3) and the VOP2 form (4) issue about 1.5 times as fast as the stream whose eight
    # chains share two sources (0): the 3.4 cycles per instruction of that stream were an operand-bank effect
    assert rates[3] > 1.25 * rates[0] and rates[4] > 1.25 * rates[0], rates


def test_step_clock_of_the_headline_kernels(nb):
    """nb_diag_step_clock: the clock the part holds under step_strict_kernel and step_fast_wave_kernel at the headline size,
    from stamps inside the kernel; the stamped step's results are untouched (the stamps go to a buffer of their own)."""
    lib = nb.load()
    for mode in (nb.NB_MODE_STRICT, nb.NB_MODE_FAST):
        mhz, cyc, ms = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        p = nb.default_params(mode=mode)
        assert lib.nb_diag_step_clock(ctypes.byref(p), 131072, 0.1, ctypes.byref(mhz), ctypes.byref(cyc), ctypes.byref(ms)) == 0, nb._lib.last_error()
        assert 900.0 < mhz.value < 2500.0 and 0.5 < ms.value < 30.0
        # a wave's lifetime in cycles / the clock cannot exceed the kernel's duration
        assert cyc.value / (mhz.value * 1e3) <= ms.value * 1.02


@pytest.mark.parametrize("mode_fast,tile,n,kernel", [(True, 0, 1024, "step_fast_wave_kernel"), (True, 0, 4096, "step_fast_sl_kernel"),
                                                    (True, 0, 32768, "step_fast_pairs_kernel"), (False, 256, 57408, "step_strict_kernel"),
                                                    (False, 0, 1536, "step_strict_bc_kernel")])
def test_step_clock_of_the_other_stamped_forms(nb, mode_fast, tile, n, kernel):
    """nb_diag_step_clock on the smallest shape that reaches each stamped form the headline test does not: its stamped launch is the
    plan's own dispatch with the stamps set (nb_plan.h: visit_launch).  No clock or time bound at these sizes: the part does not ramp
    on microsecond kernels.  The block chain (n = 1 536, STRICT) carries no stamps and is still refused.

    No workgroup of the two smallest steps runs for the 20 us (2 000 ticks of the 100 MHz counter) that clock_from_stamps asks of a
    workgroup where it has the choice; those steps are timed from every workgroup the counter saw run.  Before that rule the call
    answered NB_ERR_STATE, "no workgroup ran long enough to time", for FAST sets of 1 024, 4 096 and 8 192 bodies, with the planner in
    nb_api.hip as with it in nb_plan.h; the shapes that were timed then give what they gave (measured on one MI355X, before / after
    the planner moved: 32 768 FAST, pairs: 2 330.4 / 2 329.8 MHz, 161 784 / 161 920 cycles, 0.150 ms; 57 408 STRICT tiled: 2 383.1 /
    2 383.2 MHz, 4 185 744 / 4 185 776 cycles, 1.774 ms)."""
    lib = nb.load()
    p = nb.default_params(mode=nb.NB_MODE_FAST if mode_fast else nb.NB_MODE_STRICT, tile=tile)
    assert nb._lib.planned_kernels(p, n, n)[0] == kernel
    mhz, cyc, ms = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    rc = lib.nb_diag_step_clock(ctypes.byref(p), n, 0.05, ctypes.byref(mhz), ctypes.byref(cyc), ctypes.byref(ms))
    if kernel == "step_strict_bc_kernel":
        assert rc == nb._lib.NB_ERR_UNSUPPORTED
        assert nb._lib.last_error() == ("nb_diag_step_clock: only the whole-set kernels carry stamps (STRICT one lane per body, FAST wave and pairs "
                                        "forms)")
        return
    assert rc == 0, nb._lib.last_error()
    for v in (mhz.value, cyc.value, ms.value):
        assert np.isfinite(v) and v > 0, (kernel, mhz.value, cyc.value, ms.value)


def test_perf_floor_of_the_whole_set_kernels(nb, capsys):
    """What the headline rests on, as a TIME (the ISA side is tests/test_isa_guard.py): N = 131 072, each
    controller stepped for >= 100 ms first (the part ramps its clock after an idle gap), then 40 steps against the wall clock
    with one wait at the end -- launches are asynchronous and back to back, so the wall time is the device time.  Floors 10 %
    over the slowest device seen in rounds 3-4: STRICT 6.0 ms per step, FAST 1.95, boids 5.0; one rank's share of an 8-rank FAST
    step in the pairs form (fold + finish, no exchange) 0.27.
    Those tight floors are asserted only with NB_PERF_FLOORS=1 (the builder's profiling runs: tools/collect_profiles.sh sets it): a
    correctness suite must not go red on a shared, power-capped or differently clocked part.  The default run holds
    every figure to 1.6 x its floor -- what falling back to another kernel form would break, not what a slow clock would -- and
    prints the times; the ISA guard (tests/test_isa_guard.py) is the regression tripwire that needs no clock."""
    import os
    import time

    import torch

    from nenbody_amd.dist import HipBackend

    n = 131072
    pos, vel = nb.init_state(n, 1234)
    got = {}
    for name, mode, floor in (("strict", nb.NB_MODE_STRICT, 6.0), ("fast", nb.NB_MODE_FAST, 1.95), ("boids", None, 5.0)):
        with nb.Scene(pos, vel, nb.default_params(mode=mode if mode is not None else nb.NB_MODE_STRICT)) as sc:
            step = sc.step_boids_n if mode is None else sc.step_n
            step(70 if name == "fast" else 25)
            sc.sync()
            t0 = time.perf_counter()
            step(40)
            sc.sync()
            got[name] = ((time.perf_counter() - t0) / 40 * 1e3, floor)
    be, dev = HipBackend(), torch.device("cuda", 0)
    fast = nb.default_params(mode=nb.NB_MODE_FAST)
    S = n // 8
    cur = torch.zeros((n, 4), device=dev)
    cur[:, :3] = torch.from_numpy(pos).to(dev)
    nxt, v4 = torch.zeros_like(cur), torch.zeros((S, 4), device=dev)
    D = be.ring_partners(fast, n, 0, S)
    sums, recv = torch.zeros(((D + 1) * S, 4), device=dev), torch.zeros((D * S, 4), device=dev)
    scratch = torch.empty((be.ring_scratch_bytes(fast, n, 0, S),), dtype=torch.uint8, device=dev)

    def share(k):
        for _ in range(k):
            be.ring_fold(fast, n, 0, S, cur, sums, scratch)
            be.ring_finish(fast, n, 0, S, cur, nxt, v4, sums, recv)
        torch.cuda.synchronize()

    share(400)
    t0 = time.perf_counter()
    share(100)
    got["fast, one of 8 ranks (pairs form)"] = ((time.perf_counter() - t0) / 100 * 1e3, 0.27)
    with capsys.disabled():
        print("\n  ms per step at N = 131072: " + ", ".join(f"{k} {v:.3f} (floor {f})" for k, (v, f) in got.items()))
    slack = 1.0 if os.environ.get("NB_PERF_FLOORS") == "1" else 1.6
    for k, (v, f) in got.items():
        assert v <= f * slack, f"{k}: {v:.3f} ms per step, floor {f} x {slack}"


def test_the_product_library_refuses_the_legacy_forms_by_name(nb, oracle):
    """The product library holds the launch shapes its own plan reaches; a shape only a diagnostic knob can name (here the
    producer/consumer STRICT form and the workgroup-tile FAST form of round 1) is answered with NB_ERR_UNSUPPORTED and a message that
    says where it lives -- never with another kernel.  (The knob is set behind the fixture's back: the fixture would bind the legacy
    build.)"""
    from nenbody_amd import _lib

    assert _lib.load().nb_diag_legacy_forms() == 0, "the default binding must be the product library"
    pos, vel = oracle.init_state(4096, 3)
    for knob, value, mode in (("NB_STRICT_PC", "14", nb.NB_MODE_STRICT), ("NB_FAST_WAVES", "0", nb.NB_MODE_FAST)):
        os.environ[knob] = value
        nb.reload_env()
        try:
            with pytest.raises(nb.NbError) as e:
                with nb.Scene(pos, vel, nb.default_params(mode=mode)) as sc:
                    sc.step_n(1)
                    sc.sync()
            assert e.value.status == _lib.NB_ERR_UNSUPPORTED and "legacy" in str(e.value)
        finally:
            del os.environ[knob]
            nb.reload_env()
    with nb.Scene(pos, vel) as sc:   # ... and the library is none the worse for it
        sc.step_n(2)
        p, _ = sc.state()
    assert_bits_equal(p, oracle.run(pos, vel, 2)[0])


def test_contexts_on_concurrent_host_threads(nb, oracle):
    """A context is single-owner (`Scene: Send`, not `Sync`), but DIFFERENT contexts may be driven from
    different host threads at the same time -- each has its own stream, plans are cached per thread, the last error is
    thread-local -- and the launch API may be called from several threads too.  Four threads, four sets of different sizes and
    arithmetic (block chain, j-parallel, FAST, boids), stepping concurrently: every result is the oracle's."""
    import threading

    cases = [(4096, "strict"), (700, "strict"), (3000, "boids"), (2500, "fast"), (5000, "strict"), (1800, "boids")]
    results, errors = {}, []

    def work(idx, n, kind):
        try:
            pos, vel = oracle.init_state(n, seed=900 + idx)
            for _ in range(3):                     # several contexts per thread, one after another
                if kind == "boids":
                    with nb.Scene(pos, vel) as sc:
                        sc.step_boids_n(3)
                        results[idx] = sc.state()
                else:
                    mode = nb.NB_MODE_FAST if kind == "fast" else nb.NB_MODE_STRICT
                    with nb.Scene(pos, vel, nb.default_params(mode=mode)) as sc:
                        sc.step_n(3)
                        results[idx] = sc.state()
        except Exception as e:  # pragma: no cover
            errors.append((idx, repr(e)))

    threads = [threading.Thread(target=work, args=(i, n, k)) for i, (n, k) in enumerate(cases)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, (n, kind) in enumerate(cases):
        pos, vel = oracle.init_state(n, seed=900 + i)
        p, v = results[i]
        if kind == "boids":
            p_ref, v_ref = oracle.boids_run(pos, vel, 3)
        else:
            p_ref, v_ref = oracle.run(pos, vel, 3)
        if kind == "fast":
            assert np.abs(p - p_ref).max() < 1e-4, (i, n)
        else:
            assert_bits_equal(p, p_ref, f"thread {i}: {kind} n={n}")
            assert_bits_equal(v, v_ref, f"thread {i}: {kind} n={n}")
