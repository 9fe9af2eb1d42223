"""The exact boids lattice (tests/boids_lattice.py) on the CPU: its expectation is what the reference's arithmetic gives, in the
reference's order and in the split form's orders (slices, rows, the rule-3 total), and its builder and certifier refuse what would
be inexact.  A control arm shows a corruption the split form's tolerance criteria let through and the lattice flags."""
import numpy as np
import pytest

from boids_lattice import (F32_EXACT, KINDS, Consts, assert_exact, bounds, boids_lattice, exact, expected, finish, flag_word, on_lattice,
                           quantum, rule3_bound, schedule_consts, schedule_state, shortcut, split_shape, sqrt_threshold, vlim, wrong_bodies)
from boids_split import assert_sampled_close, close_to_the_reference, headline_sample

F = np.float32
ODD_RADII = [("rule_1_distance", np.inf), ("rule_2_distance", 0.0), ("rule_3_distance", -1.0), ("rule_1_distance", np.nan),
             ("rule_2_distance", np.nan), ("rule_3_distance", np.inf), ("rule_3_distance", 0.0)]


def assert_same(p, v, p_exp, v_exp, what):
    bad = wrong_bodies(p, v, p_exp, v_exp)
    assert len(bad) == 0, f"{what}: {len(bad)} bodies differ, first {bad[:8].tolist()}"


@pytest.mark.parametrize("n", [1, 2, 257, 1500, 5000])
@pytest.mark.parametrize("kind", list(KINDS))
def test_expectation_is_the_oracle_and_the_restatement(oracle, kind, n):
    import np_restatement

    for seed in (0, 1, 2) if n <= 1500 else (3,):
        pos, vel, cs = boids_lattice(n, seed, kind)
        p, v, d = expected(pos, vel, cs, detail=True)
        pr, vr = oracle.boids_run(pos, vel, 1, cs.oracle(oracle))
        assert_same(p, v, pr, vr, f"oracle, {kind} n={n} seed={seed}")
        if n <= 1500:
            pn, vn = np_restatement.boids_step(pos, vel, *(F(x) for _, x in cs.items()))
            assert_same(p, v, pn, vn, f"np_restatement, {kind} n={n} seed={seed}")
        if n >= 257:   # the clamp of main.rs:516-518 fires for some bodies and not for others
            assert 0 < d["clamped"].sum() < n, f"{kind} n={n}: {d['clamped'].sum()} clamped"


def test_the_kinds_are_what_they_say():
    n = 3000
    for kind in KINDS:
        pos, vel, cs = boids_lattice(n, 7, kind)
        assert len(np.unique(pos, axis=0)) < n // 4 and len(np.unique(vel, axis=0)) < n // 4, f"{kind}: many bodies per site"
        planar = (pos[:, 2] == 0) & (vel[:, 2] == 0)
        assert planar.all() == (kind == "planar"), kind
        if kind == "mixed":   # whole planar 1 024-record blocks (planar tiles) among 3-D ones
            assert planar[1024:2048].all() and not planar[:1024].all() and not planar[2048:].all()
        word = flag_word(pos, vel, cs)
        assert shortcut(word, cs) == (kind in ("planar", "3d", "mixed", "rule3_holds")), kind
    pos, vel, cs = boids_lattice(n, 7, "rule3_edge")
    lim = float(vlim(cs))
    over = np.abs(vel) > lim
    assert over.sum() == 1 and np.abs(vel[over])[0] == (np.floor(lim / 2 ** -6) + 1) * 2 ** -6
    _, _, d = expected(pos, vel, cs, detail=True)
    assert (d["vcnt"] == n - 1).all()           # rule 3 still holds for every pair: only the path differs
    pos, vel, cs = boids_lattice(n, 7, "rule3_cuts")
    _, _, d = expected(pos, vel, cs, detail=True)
    assert (d["vcnt"] < n - 1).mean() > 0.9
    pos, vel, cs = boids_lattice(n, 7, "ties")     # ties on every radius occur between bodies
    P = np.unique(pos, axis=0)
    d2 = (((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)).astype(F)
    assert (d2 == F(cs.rule_1_distance)).any() and (np.sqrt(d2) == F(cs.rule_2_distance)).any()
    W = np.unique(vel, axis=0)
    e = W[:, None, :] - W[None, :, :]
    sq = e * e
    assert (np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]) == F(cs.rule_3_distance)).any()


@pytest.mark.parametrize("kind", ["3d", "rule3_cuts", "ties"])
def test_expectation_with_other_constants(oracle, kind):
    n = 1200
    pos, vel, cs = boids_lattice(n, 4, kind)
    variants = [cs.with_(dt=0.1, rule_1_scale=0.3, rule_2_scale=0.2, rule_3_scale=0.75), cs.with_(dt=2.0 ** -3, rule_1_scale=-0.5)]
    variants += [cs.with_(**{k: v}) for k, v in ODD_RADII]
    for c in variants:
        p, v = expected(pos, vel, c)
        pr, vr = oracle.boids_run(pos, vel, 1, c.oracle(oracle))
        assert_same(p, v, pr, vr, f"{kind} {c}")


@pytest.mark.parametrize("n,R,V,kind,consts", [
    (131072, 63, 63, "planar", None),
    (131072, 63, 63, "rule3_cuts", None),
    (1 << 20, 7, 7, "3d", Consts(rule_2_distance=1.5, rule_2_scale=2.0 ** -9)),
], ids=["131072-planar", "131072-rule3-cuts", "2^20-3d"])
def test_expectation_at_the_headline_sizes_on_sampled_bodies(oracle, nb_partition, n, R, V, kind, consts):
    """every 8-rank share's first, last and middle body, and bodies at ties and on both sides of the clamp, against the oracle"""
    pos, vel, cs = boids_lattice(n, 5, kind, R=R, V=V, consts=consts)
    p, v, d = expected(pos, vel, cs, detail=True)
    assert 0 < d["clamped"].sum() < n
    rng = np.random.default_rng(0)
    idx = [i for f, c in nb_partition(n, 8) for i in (f, f + c - 1, f + c // 2)]
    idx += list(rng.choice(np.flatnonzero(d["clamped"]), 4)) + list(rng.choice(np.flatnonzero(~d["clamped"]), 4))
    ob = cs.oracle(oracle)
    for i in sorted(set(int(i) for i in idx)):
        pr, vr = oracle.boids_step_range(pos, vel, i, 1, ob)
        assert_same(p[i:i + 1], v[i:i + 1], pr, vr, f"body {i}")


@pytest.fixture
def nb_partition():
    """nenbody_amd.partition restated without loading the HIP library: the library's own (first, count) of every rank"""
    import nenbody_amd.dist as dist

    return dist.partition


# -- the split form's orders, emulated -------------------------------------------------------------------------------------------
def split_emulation(pos, vel, bp, slices, chunk, use_total, rng=None):
    """the split form's arithmetic in numpy binary32: every slice [k chunk, (k+1) chunk) folded in index order (rng: a random
    order), its rows added in slice order (rng: a random order), and -- use_total -- rule 3 as the total of all velocities (in
    boids_prep_kernel's and boids_combine_kernel's order: four records per lane, a tree over 256 lanes per 1 024 records, the
    groups strided over 256 threads and a tree; rng: a random order) minus the body's own, count n - 1"""
    n = len(pos)
    f = lambda k: F(getattr(bp, k))
    rows = []
    for k in range(slices):
        js = np.arange(k * chunk, min((k + 1) * chunk, n))
        if rng is not None:
            js = rng.permutation(js)
        acc = [np.zeros((n, 3), F) for _ in range(3)]
        cnt, vcnt = np.zeros(n, F), np.zeros(n, F)
        idx = np.arange(n)
        for j in js:
            d = pos[j][None, :] - pos
            sq = d * d
            d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
            ne = idx != j
            with np.errstate(invalid="ignore"):
                p1 = (d2 < f("rule_1_distance")) & ne
                p2 = (np.sqrt(d2) < f("rule_2_distance")) & ne
                e = vel[j][None, :] - vel
                se = e * e
                p3 = (np.sqrt((se[:, 0] + se[:, 1]) + se[:, 2]) < f("rule_3_distance")) & ne
            acc[0] = np.where(p1[:, None], acc[0] + pos[j], acc[0])
            cnt = np.where(p1, cnt + F(1), cnt)
            acc[1] = np.where(p2[:, None], acc[1] + (pos - pos[j]), acc[1])
            if not use_total:
                acc[2] = np.where(p3[:, None], acc[2] + vel[j], acc[2])
                vcnt = np.where(p3, vcnt + F(1), vcnt)
        rows.append((acc, cnt, vcnt))
    order = rng.permutation(slices) if rng is not None else range(slices)
    c, r, m = (np.zeros((n, 3), F) for _ in range(3))
    cnt, vcnt = np.zeros(n, F), np.zeros(n, F)
    for k in order:
        (a0, a1, a2), c0, v0 = rows[k]
        c, r, m, cnt, vcnt = c + a0, r + a1, m + a2, cnt + c0, vcnt + v0
    if use_total:
        if rng is not None:
            tot = np.zeros(3, F)
            for j in rng.permutation(n):
                tot = tot + vel[j]
        else:
            groups = []
            for g in range(0, n, 1024):
                lane = np.zeros((256, 3), F)
                for k in range(4):
                    js = g + np.arange(256) + 256 * k
                    ok = js < n
                    lane[ok] = lane[ok] + vel[js[ok]]
                w = 128
                while w:
                    lane[:w] = lane[:w] + lane[w:2 * w]
                    w //= 2
                groups.append(lane[0])
            t = np.zeros((256, 3), F)
            for g0 in range(0, len(groups), 256):
                for th, gv in enumerate(groups[g0:g0 + 256]):
                    t[th] = t[th] + gv
            w = 128
            while w:
                t[:w] = t[:w] + t[w:2 * w]
                w //= 2
            tot = t[0]
        m = (tot[None, :] - vel).astype(F)
        vcnt = np.full(n, F(n - 1))
    p, v, _ = finish(c, r, m, cnt, vcnt, pos, bp)
    return p, v


@pytest.mark.parametrize("kind", ["planar", "mixed", "rule3_holds", "rule3_edge", "rule3_cuts", "ties"])
@pytest.mark.parametrize("n,tile,knob", [(300, 256, None), (1500, 256, 1), (1500, 256, 2), (1500, 512, 3), (1500, 256, 7), (1500, 256, 64)])
def test_split_form_orders_equal_the_expectation(kind, n, tile, knob):
    pos, vel, cs = boids_lattice(n, n + tile, kind)
    p_exp, v_exp = expected(pos, vel, cs)
    slices, chunk = split_shape(n, n, tile, knob)
    use_total = shortcut(flag_word(pos, vel, cs), cs)
    p, v = split_emulation(pos, vel, cs, slices, chunk, use_total)
    assert_same(p, v, p_exp, v_exp, f"{kind} n={n} slices={slices} total={use_total}")
    p, v = split_emulation(pos, vel, cs, slices, chunk, use_total, rng=np.random.default_rng(n))
    assert_same(p, v, p_exp, v_exp, f"shuffled: {kind} n={n} slices={slices} total={use_total}")


def test_split_form_orders_round_off_the_lattice(oracle):
    """the same emulation on a state the certifier rejects: the orders give other bits (what the lattice guards against is real)"""
    pos, vel = oracle.init_state(1500, 3)
    pos *= F(0.2)
    assert not exact(pos, vel)
    cs = Consts()
    slices, chunk = split_shape(1500, 1500, 256, 3)
    p, v = split_emulation(pos, vel, cs, slices, chunk, True)
    pr, vr = oracle.boids_run(pos, vel, 1)
    assert len(wrong_bodies(p, v, pr, vr)) > 100


def test_split_shape_restatement():
    assert split_shape(131072, 16384, 1024) == (8, 16384)
    assert split_shape(1, 1, 1024) == (1, 1024)
    assert split_shape(3000, 3000, 256, 7) == (6, 512)           # 12 tiles, 2 per slice: no empty slice
    assert split_shape(20000, 20000, 256, 64) == (40, 512)       # 79 tiles, at most 64 slices, no empty slice
    assert split_shape(1 << 20, 1 << 19, 1024) == (1, 1 << 20)
    for n in (1, 255, 257, 1023, 1025, 3000, 20000):
        for tile in (256, 512, 1024):
            for knob in (None, 0, 1, 2, 3, 7, 64, 1000):
                sl, ch = split_shape(n, n, tile, knob)
                assert 1 <= sl <= 64 and ch % tile == 0 and (sl - 1) * ch < n <= sl * ch


def test_thresholds_restated():
    assert sqrt_threshold(-1.0) == -1 and sqrt_threshold(np.nan) == -1 and sqrt_threshold(0.0) == -1
    assert np.sqrt(sqrt_threshold(5.0)) < F(5) and not np.sqrt(np.nextafter(sqrt_threshold(5.0), F(99))) < F(5)
    lim = vlim(Consts(rule_3_distance=1.0))
    assert 0.28 < lim < 0.29 and rule3_bound(F(-1)) == -1 and vlim(Consts(rule_3_distance=0.0)) == -1
    assert not shortcut(0, Consts(rule_3_distance=np.nan)) and not shortcut(0, Consts(), force=4) and shortcut(0, Consts())


# -- refusals --------------------------------------------------------------------------------------------------------------------
def test_certifier_refuses_one_quantum_past_each_bound():
    n = 4
    # rule 2: sum |p| + n max|p| = 2^24 - 1 quanta passes, 2^24 fails
    total = lambda p: int(np.abs(p[:, 0]).astype(np.int64).sum() + n * np.abs(p[:, 0]).max())
    pos = np.zeros((n, 3), F)
    a = (F32_EXACT - 1) // (n + 1)
    pos[0, 0] = a                                                  # sum a, n max = n a
    pos[1, 0] = F32_EXACT - 1 - (n + 1) * a                        # below a: raises the sum only
    assert total(pos) == F32_EXACT - 1 and quantum(pos) == 1.0
    vel = np.zeros((n, 3), F)
    assert exact(pos, vel)
    pos[1, 0] += 1
    assert total(pos) == F32_EXACT and not exact(pos, vel)
    with pytest.raises(ValueError, match="rule2"):
        assert_exact(pos, vel)
    # rule 3: sum |v| in quanta of qv
    qv = 2.0 ** -6
    pos = np.zeros((n, 3), F)
    vel = np.zeros((n, 3), F)
    vel[:, 2] = F((F32_EXACT // n) * qv)                            # 2^22 quanta each: sum = 2^24
    vel[0, 2] = F((F32_EXACT // n - 1) * qv)                        # ... - 1; qv stays 2^-6 (an odd multiple)
    assert quantum(vel) == qv and bounds(pos, vel)[2]["rule3"].max() == F32_EXACT - 1 and exact(pos, vel)
    vel[0, 2] = F((F32_EXACT // n + 1) * qv)
    assert bounds(pos, vel)[2]["rule3"].max() == F32_EXACT + 1 and not exact(pos, vel)
    with pytest.raises(ValueError, match="rule3"):
        assert_exact(pos, vel)
    # rule 1 (sum |p|) is below the rule-2 bound whenever a position is nonzero: it can only be the one to fail with it
    _, _, b = bounds(pos + F(1), vel)
    assert (b["rule1"] < b["rule2"]).all()


def test_certifier_refuses_a_position_off_the_quantum():
    pos, vel, cs = boids_lattice(131072, 1, "planar")
    assert exact(pos, vel) and quantum(pos) == 1.0
    on_lattice(pos, vel, 1.0, 2.0 ** -6)
    bad = pos.copy()
    bad[777, 1] += F(2.0 ** -4)                                    # one coordinate a sixteenth off the integer lattice
    with pytest.raises(ValueError, match="qp"):
        on_lattice(bad, vel, 1.0, 2.0 ** -6)
    assert quantum(bad) == 2.0 ** -4 and not exact(bad, vel)      # the quantum falls: 16 x the quanta, far past 2^24
    badv = vel.copy()
    badv[5, 0] += F(2.0 ** -12)
    with pytest.raises(ValueError, match="qv"):
        on_lattice(pos, badv, 1.0, 2.0 ** -6)
    nonfinite = pos.copy()
    nonfinite[3, 0] = np.inf
    assert not exact(nonfinite, vel)


def test_builder_refuses_what_would_be_inexact():
    """the sizes that matter fit (131 072 bodies within +-63, 2^20 within +-7); a box that does not is refused, not built"""
    boids_lattice(131072, 0, "3d", R=63, V=63)
    with pytest.raises(ValueError, match="rule2"):
        boids_lattice(131072, 0, "3d", R=200, V=63)
    boids_lattice(1 << 20, 0, "3d", R=7, V=7)
    with pytest.raises(ValueError, match="rule2"):
        boids_lattice(1 << 20, 0, "3d", R=16, V=7)
    with pytest.raises(ValueError, match="rule3"):
        boids_lattice(1 << 20, 0, "3d", R=7, V=40)
    with pytest.raises(ValueError):
        boids_lattice(100, 0, "3d", qp=0.3)
    with pytest.raises(ValueError):
        boids_lattice(100, 0, "nonsense")
    with pytest.raises(ValueError):
        boids_lattice(0, 0, "3d")


def test_schedule_stays_on_the_lattice(oracle):
    """boids (schedule_consts) -> n-body with dt = 0 -> boids: every state exact, the n-body step is p + v (main.rs:434-436)"""
    for n in (1, 2, 1000, 2000):
        pos, vel, A, B = schedule_state(n, n)
        p1, v1 = expected(pos, vel, A)
        pr, vr = oracle.boids_run(pos, vel, 1, A.oracle(oracle))
        assert_same(p1, v1, pr, vr, f"n={n} boids")
        assert_exact(p1, v1)
        p2, v2 = oracle.run(p1, v1, 1, dt=F(0))
        assert_same(p2, v2, (p1 + v1).astype(F), v1, f"n={n} n-body, dt = 0")
        assert_exact(p2, v2)
        if n <= 1000:
            p3, v3 = expected(p2, v2, B)
            pr, vr = oracle.boids_run(p2, v2, 1, B.oracle(oracle))
            assert_same(p3, v3, pr, vr, f"n={n} boids after n-body")
    assert schedule_consts().rule_1_distance < 1


# -- control arm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [1, 3])
def test_control_arm_one_dropped_neighbour(oracle, nb_partition, rule):
    """20 000 bodies: one rule-1 (or rule-3) neighbour dropped from one body's sum and count, as a kernel could.  The split form's
    tolerance criteria pass it -- test_native_shard_boids_split_form's 1e-4 max|v|, close_to_the_reference and the headline test's
    sampled check -- and the lattice flags exactly that body."""
    n = 20000
    pos, vel, cs = boids_lattice(n, 9, "planar")
    p_exp, v_exp, d = expected(pos, vel, cs, detail=True)
    rng = np.random.default_rng(rule)
    idx = headline_sample(nb_partition(n, 8))
    i = int(rng.choice(np.setdiff1d(np.arange(n), idx)))
    # the neighbour whose loss moves body i least (but moves it): a neighbour near the body's mean
    if rule == 1:
        dd = pos - pos[i]
        nbr = np.flatnonzero((((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]) < F(cs.rule_1_distance)) & (np.arange(n) != i))
        mean = d["c"][i] / d["cnt"][i]
        j = nbr[np.argmin(np.abs(pos[nbr] - mean).sum(axis=1) + 1e9 * (pos[nbr] == mean).all(axis=1))]
        c, cnt = d["c"].copy(), d["cnt"].copy()
        c[i] = c[i] - pos[j]
        cnt[i] -= 1
        p, v, _ = finish(c, d["r"], d["m"], cnt, d["vcnt"], pos, cs)
    else:
        assert (d["vcnt"] == n - 1).all()
        mean = d["m"][i] / d["vcnt"][i]
        nbr = np.setdiff1d(np.arange(n), [i])
        j = nbr[np.argmin(np.abs(vel[nbr] - mean).sum(axis=1) + 1e9 * (vel[nbr] == mean).all(axis=1))]
        m, vcnt = d["m"].copy(), d["vcnt"].copy()
        m[i] = m[i] - vel[j]
        vcnt[i] -= 1
        p, v, _ = finish(d["c"], d["r"], m, d["cnt"], vcnt, pos, cs)
    assert wrong_bodies(p, v, p_exp, v_exp).tolist() == [i]
    # test_native_shard_boids_split_form's criterion
    assert np.abs(v - v_exp).max() <= 1e-4 * np.abs(v_exp).max() and np.abs(p - p_exp).max() <= 1e-4
    # close_to_the_reference (the tolerance half; its binary64 half samples bodies where the two differ most -- body i -- and
    # holds it no further from the binary64 sums than the reference plus four ulps, which one neighbour in 20 000 also meets)
    close_to_the_reference(v, v_exp, p, p_exp, f"rule {rule}")
    # the headline test's sampled check: body i is not among its bodies, so every sampled body is the reference's
    assert i not in set(idx.tolist())
    refs = [(p_exp[k:k + 1], v_exp[k:k + 1]) for k in idx]
    assert_sampled_close(p, v, pos, vel, idx, refs, cs)
