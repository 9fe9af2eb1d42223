"""The exact lattice (tests/exact_lattice.py) on the CPU: its closed form is what the reference's arithmetic gives, in the reference's
order and in any other, and it refuses parameters that would make it inexact.  A control arm shows what it catches that FAST's
global tolerance (|v - v_ref| <= 2e-5 max|dv| + ulp) lets through, and the sharded scene's orchestration is held to it bit for bit
over two steps on every rank."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT
from exact_lattice import KINDS, assert_exact, lattice, wrong_bodies

SCALES = [1.0, 2.0 ** -20, 2.0 ** 29, 2.0 ** 31]
F = np.float32


def terms(lat, idx, p=None):
    """(len(idx), n, 3) binary32 terms (d * G) / (|d|^2 + bias) of bodies idx against every body, as main.rs:428-430 rounds them
    (positions p; default: the lattice's start)"""
    p = lat.pos if p is None else p
    d = p[None, :, :] - p[idx][:, None, :]
    sq = d * d
    r2 = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + lat.bias
    return (d * lat.G) / r2[..., None]


def integrate(lat, acc, p=None, v=None):
    p = lat.pos if p is None else p
    v = ((lat.vel if v is None else v) + acc * lat.dt).astype(F)
    return (v + p).astype(F), v


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"2^{int(np.log2(s))}")
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("steps", [1, 2])
def test_closed_form_is_the_oracle_and_the_restatement(oracle, kind, scale, steps):
    import np_restatement

    lat = lattice(257, seed=steps, kind=kind, scale=scale, steps=steps)
    p, v = oracle.run(lat.pos, lat.vel, steps, *lat.consts)
    assert_exact(lat, p, v, "oracle.run")
    p, v = lat.pos, lat.vel
    for _ in range(steps):
        p, v = np_restatement.step(p, v, *lat.consts)
    assert_exact(lat, p, v, "np_restatement")


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"2^{int(np.log2(s))}")
@pytest.mark.parametrize("kind", list(KINDS))
def test_closed_form_in_any_order_of_additions(kind, scale):
    """numpy binary32 sums of every body's terms shuffled, pairwise (np.sum's tree) and reversed: the same bits"""
    lat = lattice(300, seed=5, kind=kind, scale=scale)
    t = terms(lat, np.arange(len(lat.pos)))
    rng = np.random.default_rng(1)
    for order in ("pairwise", "reversed", "shuffled"):
        if order == "pairwise":
            acc = t.sum(axis=1, dtype=F)
        else:
            acc = np.zeros((len(lat.pos), 3), F)
            js = np.arange(len(lat.pos))[::-1] if order == "reversed" else rng.permutation(len(lat.pos))
            for j in js:
                acc = (acc + t[:, j]).astype(F)
        p, v = integrate(lat, acc)
        assert_exact(lat, p, v, order)


@pytest.mark.parametrize("opts", [dict(runs=64), dict(runs=100, empty=(1,)), dict(skew=(20, 1, 1, 1)), dict(empty=(0, 2)),
                                  dict(G0=2.0 ** -5, dt=-2.0 ** -2), dict(G0=2.0 ** 2, dt=2.0 ** -6, scale=2.0 ** -3)], ids=str)
@pytest.mark.parametrize("steps", [1, 2])
def test_options_stay_exact(oracle, opts, steps):
    lat = lattice(1000, seed=3, steps=steps, **opts)
    p, v = oracle.run(lat.pos, lat.vel, steps, *lat.consts)
    assert_exact(lat, p, v, str(opts))
    if "empty" in opts:
        assert all(lat.counts[t] == 0 for t in opts["empty"])
    if "runs" in opts:
        r = opts["runs"]
        assert all(len(set(lat.site[i:i + r])) == 1 for i in range(0, 1000, r))


def test_constants_are_the_design_not_the_reference():
    lat = lattice(10, kind="tetra", scale=2.0 ** 5, G0=-2.0 ** -3, dt=2.0 ** -1)
    assert lat.G == F(-2.0 ** 7) and lat.bias == F(2.0 ** 11) and lat.dt == F(0.5)
    lat = lattice(10, kind="line", scale=2.0 ** 5)
    assert lat.bias == F(2.0 ** 10)
    # tetra: no body in the plane z = 0 (a 3-D tile everywhere); tetra_mixed: both kinds of site
    assert (lattice(400, kind="tetra").pos[:, 2] != 0).all()
    z = lattice(400, kind="tetra_mixed").pos[:, 2]
    assert (z == 0).any() and (z != 0).any()
    assert (lattice(400, kind="planar").pos[:, 2] == 0).all() and (lattice(400, kind="line").pos[:, 2] == 0).all()


def test_refuses_what_would_be_inexact():
    with pytest.raises(ValueError, match="normal range"):
        lattice(16, scale=2.0 ** -60)                 # G = G0 s^2 is subnormal
    with pytest.raises(ValueError, match="power of two"):
        lattice(16, G0=0.001)
    with pytest.raises(ValueError, match="power of two"):
        lattice(16, scale=3.0)
    with pytest.raises(ValueError, match="must differ"):
        lattice(16, G0=2.0 ** -1, dt=2.0 ** -1)
    with pytest.raises(ValueError, match="2\\^24"):
        lattice(1 << 24)
    with pytest.raises(ValueError, match="not exact"):
        lattice(16, vmax=1 << 26)
    with pytest.raises(ValueError, match="not exact"):   # a large set whose sums of velocity units outgrow the grid
        lattice(4194304, G0=2.0 ** 4, dt=2.0 ** -1, scale=1.0, skew=(50, 1, 1, 1))
    # the headline parameters leave a margin the helper reports
    lat = lattice(4194304 + 256, seed=1, G0=2.0 ** -3, dt=2.0 ** -1, steps=2)
    assert 1 <= lat.margin_bits < 4


def test_control_arm_one_dropped_and_one_doubled_pair_at_the_headline_size():
    """n = 131 072: a FAST-like sum (numpy binary32, pairwise tree) with one cross-site pair dropped and another counted twice.  The
    lattice flags exactly those four bodies; FAST's existing criterion |v - v_ref| <= 2e-5 max|dv| + ulp passes the same result."""
    n = 131072
    lat = lattice(n, seed=11, kind="tetra", G0=2.0 ** -3, dt=2.0 ** -1)
    rep = np.array([int(np.flatnonzero(lat.site == t)[0]) for t in range(4)])
    acc_site = terms(lat, rep).sum(axis=1, dtype=F)               # the same for every body of a site (all exact)
    acc = acc_site[lat.site].copy()
    p, v = integrate(lat, acc)
    assert_exact(lat, p, v, "uncorrupted")
    rng = np.random.default_rng(2)
    i, j, k, l = rng.choice(n, 4, replace=False)
    while lat.site[i] == lat.site[j] or lat.site[k] == lat.site[l]:
        i, j, k, l = rng.choice(n, 4, replace=False)
    t = terms(lat, np.array([i, j, k, l]))
    acc[i] = acc[i] - t[0, j]            # pair (i, j) dropped: both bodies lose their halves
    acc[j] = acc[j] - t[1, i]
    acc[k] = acc[k] + t[2, l]            # pair (k, l) doubled
    acc[l] = acc[l] + t[3, k]
    p, v = integrate(lat, acc)
    assert sorted(wrong_bodies(lat, p, v).tolist()) == sorted(int(x) for x in (i, j, k, l))
    scale = float(np.abs(lat.v_exp - lat.vel).max())
    ulp = float(np.spacing(np.float32(np.abs(lat.v_exp).max())))
    err = float(np.abs(v - lat.v_exp).max())
    assert 0 < err <= 2e-5 * scale + ulp, "the old criterion was expected to pass this corruption (the gap this file closes)"


# -- the permuted two-step lattice: the first step carries every site onto another, so the second step's terms are not the first's --
SWAPS = {"tetra": (1, 2, 3, 0), "tetra_mixed": (2, 3, 0, 1), "planar": (1, 0), "line": (1, 0)}   # tetra_mixed: the layers change places
PERMUTED_OPTS = {"random": {}, "runs": dict(runs=64), "skew": dict(skew=(5, 1, 3, 1)), "empty": dict(empty=(3,))}


def _opts(kind, name):
    opts = dict(PERMUTED_OPTS[name])
    if "skew" in opts and len(KINDS[kind][0]) == 2:
        opts["skew"] = (5, 1)
    return opts


def _two_site_kind_with_an_empty_site(kind, name):
    return name == "empty" and len(KINDS[kind][0]) == 2


@pytest.mark.parametrize("opt", list(PERMUTED_OPTS))
@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"2^{int(np.log2(s))}")
@pytest.mark.parametrize("kind", list(KINDS))
def test_permuted_closed_form_is_the_oracle_and_the_restatement(oracle, kind, scale, opt):
    import np_restatement

    if _two_site_kind_with_an_empty_site(kind, opt):   # one occupied site: nothing moves it relative to another (refused below)
        with pytest.raises(ValueError, match="keep their acceleration"):
            lattice(257, seed=2, kind=kind, scale=scale, steps=2, permute=SWAPS[kind], empty=(1,))
        return
    lat = lattice(257, seed=2, kind=kind, scale=scale, steps=2, permute=SWAPS[kind], **_opts(kind, opt))
    assert lat.permute == SWAPS[kind] and (lat.K2 != lat.K).any(axis=1)[lat.counts > 0].all()
    p, v = oracle.run(lat.pos, lat.vel, 1, *lat.consts)
    assert (p.view(np.uint32) == lat.p_mid.view(np.uint32)).all() and (v.view(np.uint32) == lat.v_mid.view(np.uint32)).all()
    p, v = oracle.run(p, v, 1, *lat.consts)
    assert_exact(lat, p, v, "oracle.run")
    p, v = lat.pos, lat.vel
    for _ in range(2):
        p, v = np_restatement.step(p, v, *lat.consts)
    assert_exact(lat, p, v, "np_restatement")
    # every site stands on another after the first step, shifted by the same w
    sites = np.array(KINDS[kind][0], np.float64) * lat.scale
    moved = lat.p_mid.astype(np.float64) - sites[np.array(SWAPS[kind])][lat.site]
    assert (moved == moved[0]).all()


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"2^{int(np.log2(s))}")
@pytest.mark.parametrize("kind", list(KINDS))
def test_permuted_closed_form_in_any_order_of_additions(kind, scale):
    """both steps of the permuted lattice, every body's terms summed pairwise, reversed and shuffled: the same bits after each"""
    lat = lattice(300, seed=5, kind=kind, scale=scale, steps=2, permute=SWAPS[kind])
    rng = np.random.default_rng(1)
    for order in ("pairwise", "reversed", "shuffled"):
        p, v = lat.pos, lat.vel
        for step in range(2):
            t = terms(lat, np.arange(len(p)), p)
            if order == "pairwise":
                acc = t.sum(axis=1, dtype=F)
            else:
                acc = np.zeros((len(p), 3), F)
                js = np.arange(len(p))[::-1] if order == "reversed" else rng.permutation(len(p))
                for j in js:
                    acc = (acc + t[:, j]).astype(F)
            p, v = integrate(lat, acc, p, v)
            if step == 0:
                assert (p == lat.p_mid).all() and (v == lat.v_mid).all(), order
        assert_exact(lat, p, v, order)


def test_permute_refusals():
    with pytest.raises(ValueError, match="needs steps=2"):
        lattice(64, steps=1, permute=(1, 2, 3, 0))
    for bad in ((1, 2, 3), (1, 2, 3, 3), (1, 2, 3, 4), (1.0, 2.0, 3.0, 0.0), (1, 0)):
        with pytest.raises(ValueError, match="not a permutation"):
            lattice(64, steps=2, permute=bad)
    with pytest.raises(ValueError, match="not a permutation"):
        lattice(64, kind="planar", steps=2, permute=(1, 0, 2))
    with pytest.raises(ValueError, match="in place"):
        lattice(64, steps=2, permute=(0, 1, 2, 3))
    with pytest.raises(ValueError, match=r"site\(s\) \[3\] in place"):
        lattice(64, steps=2, permute=(1, 2, 0, 3))
    lattice(64, steps=2, permute=(1, 0, 3, 2))
    # an empty site may stay where it is; an occupied one may not
    lattice(64, steps=2, permute=(1, 2, 0, 3), empty=(3,))
    with pytest.raises(ValueError, match="in place"):
        lattice(64, steps=2, permute=(1, 2, 0, 3), empty=(0,))
    # K'_t == K_t: on these lattices only where a single site is occupied (K = K' = 0) -- no translation carries two sites of a
    # simplex onto sites, so a permutation that keeps every acceleration of two or more occupied sites does not exist
    with pytest.raises(ValueError, match="keep their acceleration"):
        lattice(64, kind="line", steps=2, permute=(1, 0), empty=(0,))
    with pytest.raises(ValueError, match=r"site\(s\) \[2\] keep"):
        lattice(64, steps=2, permute=(1, 2, 3, 0), sites=np.full(64, 2))
    with pytest.raises(ValueError, match="not exact"):   # the range check covers the moved states too
        lattice(64, steps=2, permute=(1, 2, 3, 0), vmax=1 << 26)
    # without permute the two-step lattice is the translated one: K' = K
    lat = lattice(64, steps=2)
    assert lat.permute is None and (lat.K2 == lat.K).all()
    assert lattice(64).K2 is None


def test_permuted_lattice_keeps_its_margin_at_two_to_the_twenty():
    lat = lattice(1 << 20, seed=2, G0=2.0 ** -3, dt=2.0 ** -1, steps=2, permute=SWAPS["tetra"])
    assert lat.margin_bits >= 4
    assert lattice(131072, seed=2, G0=2.0 ** -3, dt=2.0 ** -1, steps=2, permute=SWAPS["tetra"]).margin_bits >= 7


def _accel(lat, p, idx, js=None):
    """binary32 accelerations of bodies idx from the positions p, over records js (all): pairwise sums, exact on the lattice"""
    t = terms(lat, idx, p)
    return (t if js is None else t[:, js]).sum(axis=1, dtype=F)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 29], ids=lambda s: f"2^{int(np.log2(s))}")
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("arm", ["stale_forces", "stale_own_slot"])
def test_control_arm_stale_records_pass_the_translated_lattice_and_fail_the_permuted(kind, scale, arm):
    """Rank r of 4 (300 bodies, random sites) takes a stale record into its second step: step 1's accelerations for its whole chunk
    (a stale received half or sums record), or the pairs inside its own slot from step 0's positions (the fused finish's own-slot planes
    of the wrong step, or its own slot read one step late).  The translated lattice reproduces the closed form anyway -- its second step
    has the first step's terms; the permuted lattice flags exactly the bodies whose closed form the stale record changes."""
    from nenbody_amd.dist import partition

    n, world, r = 300, 4, 2
    first, count = partition(n, world)[r]
    mine = np.arange(first, first + count)
    sites_u = np.array(KINDS[kind][0], np.int64)
    for permute in (None, SWAPS[kind]):
        lat = lattice(n, seed=9, kind=kind, scale=scale, steps=2, permute=permute)
        acc1 = _accel(lat, lat.pos, np.arange(n))
        p1, v1 = integrate(lat, acc1)
        assert (p1 == lat.p_mid).all() and (v1 == lat.v_mid).all()
        acc2 = _accel(lat, p1, np.arange(n))
        if arm == "stale_forces":
            acc2[mine] = acc1[mine]
            c = lat.counts
            K, K2 = lat.K, lat.K2
        else:
            others = np.setdiff1d(np.arange(n), mine)
            own = terms(lat, mine, lat.pos)[:, mine].sum(axis=1, dtype=F)       # the own slot's pairs at step 0's positions
            acc2[mine] = (_accel(lat, p1, mine, others) + own).astype(F)
            c = np.bincount(lat.site[mine], minlength=len(sites_u))            # the closed form of the own slot's pairs alone
            moved = sites_u[np.array(permute if permute else range(len(sites_u)))]
            K = (c[:, None, None] * (sites_u[:, None, :] - sites_u[None, :, :])).sum(axis=0)
            K2 = (c[:, None, None] * (moved[:, None, :] - moved[None, :, :])).sum(axis=0)
        p, v = integrate(lat, acc2, p1, v1)
        bad = wrong_bodies(lat, p, v)
        if permute is None:
            assert len(bad) == 0, f"{arm}: the translated lattice was expected to be blind to this"
        else:
            hit = mine[(K2 != K).any(axis=1)[lat.site[mine]]]
            assert len(hit) > count // 2
            assert bad.tolist() == hit.tolist(), f"{arm}: flagged {len(bad)} bodies, {len(hit)} expected"


# -- the sharded scene's orchestration on the two-step lattice (gloo on the CPU, tests/oracle_backend.py sums in numpy in any order) --
def _lattice_worker(rank, world, port, n, out_dir, overlap, ring, ring_overlap):
    import torch.distributed as dist

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import nenbody_amd
        from exact_lattice import lattice as make
        from oracle_backend import OracleBackend
        from test_exact_lattice import SWAPS

        for permute, name in ((None, ""), (SWAPS["tetra"], "permuted_")):   # the translated lattice, then the permuted one
            lat = make(n, seed=world, kind="tetra", scale=2.0 ** 3, steps=2, permute=permute)
            params = nenbody_amd.default_params(mode=nenbody_amd.NB_MODE_FAST)
            params.dt, params.G, params.bias = (float(c) for c in lat.consts)
            sc = nenbody_amd.ShardedScene(lat.pos, lat.vel, params, backend=OracleBackend(), device="cpu", overlap=overlap, ring=ring,
                                          ring_overlap=ring_overlap)
            assert (sc.partners > 0) == ring and sc.overlap == overlap and sc.ring_overlap == ring_overlap
            sc.step_n(2)
            np.savez(os.path.join(out_dir, f"{name}rank{rank}.npz"), pos=sc.positions(), vel=sc.local_velocities(), first=sc.first,
                     count=sc.count)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("form", ["ordered", "overlap", "ring", "ring_overlap"])
@pytest.mark.parametrize("world,n", [(2, 64), (3, 48), (4, 64), (8, 64)])
def test_sharded_scene_two_steps_on_the_lattice_bit_exact(tmp_path, form, world, n):
    from test_dist_gloo import _free_port

    if form == "overlap" and world == 8:
        n = 70                                           # the ordered fold takes ragged ranks too
    lat = lattice(n, seed=world, kind="tetra", scale=2.0 ** 3, steps=2)
    mp.spawn(_lattice_worker, args=(world, _free_port(), n, str(tmp_path), form == "overlap", form.startswith("ring"),
                                    form == "ring_overlap"), nprocs=world, join=True)
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        bad = np.flatnonzero((got["pos"].view(np.uint32) != lat.p_exp.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, f"{form}, rank {r} of {world}: {len(bad)} positions of the replica differ, first {bad[:1]}"
        assert_exact(lat, got["pos"][first:first + count], got["vel"], f"{form}, rank {r} of {world}: own bodies", first, count)
    # the permuted lattice (the second step's terms are not the first's: a stale record of either exchange shows)
    lat = lattice(n, seed=world, kind="tetra", scale=2.0 ** 3, steps=2, permute=SWAPS["tetra"])
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"permuted_rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        bad = np.flatnonzero((got["pos"].view(np.uint32) != lat.p_exp.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, f"{form}, permuted, rank {r} of {world}: {len(bad)} positions of the replica differ, first {bad[:1]}"
        assert_exact(lat, got["pos"][first:first + count], got["vel"], f"{form}, permuted, rank {r} of {world}: own bodies", first, count)
