"""Every launch form of the boids step against the C oracle, every bit of every body, at the smallest shapes where what the forms
share (nb_boids.inc: the own-body preamble, the tile stage, the per-tile header, the form ladder, the epilogue) can go wrong.

Forms (NB_BOIDS_PC): 1 producer/consumer, 2 / 3 one lane per body packed / plain, 4 / 5 chain split plain / packed; and the split
launch (nb_launch_boids_step_split) with one and three slices: to its tolerance off the lattice, bit for bit on it.
Sizes: 1; 65 (one workgroup, a ragged second wave); 600 (three workgroups of 256, at tile 256 a self tile and two foreign tiles
each); 1100 (three producer/consumer tiles of 512, the last of two chunks, 64 + 12 records); and 1100 as the shard (257, 600), whose
first body is a multiple of nothing.  Tiles 256 / 512 / 1024 where the form takes one (the chain split stages 512 or 1024).
Tile forms: NB_BOIDS_FORCE 0..7 on planar finite data, and `mixed`, whose 256-record tiles take the ladder's branches by their own
flags."""
import numpy as np
import pytest

from boids_lattice import Consts, boids_lattice, vlim, wrong_bodies
from boids_split import close_to_the_reference, split_step
from test_gpu_boids import assert_bits_equal, assert_bits_equal_nan_alike, cloud, mixed_tiles

pytestmark = pytest.mark.gpu

SHARDS = [(1, 0, 1), (65, 0, 65), (600, 0, 600), (1100, 0, 1100), (1100, 257, 600)]   # (n, first, count)
FORMS = [(1, 0)] + [(pc, t) for pc in (2, 3) for t in (256, 512, 1024)] + [(pc, t) for pc in (4, 5) for t in (512, 1024)]
FORM_NAMES = {1: "pc", 2: "lane-packed", 3: "lane", 4: "chain", 5: "chain-packed"}
R3 = 1.0                                          # a rule-3 radius that cuts: its bound is 1 / (2 sqrt 3) = 0.2887
NONFINITE, NONPLANAR, VELFAR = 1, 2, 4            # nb_boids.inc: kBoidsNonFinite, kBoidsNonPlanar, kBoidsVelFar

_cache = {}


def planar(oracle, n):
    """the reference's kind of state: z = 0, vz = 0, every record finite; with the default constants rule 3 holds everywhere"""
    if ("planar", n) not in _cache:
        pos, vel = oracle.init_state(n, seed=n + 3)
        pos *= np.float32(0.2)
        _cache["planar", n] = (pos, vel, oracle.boids_run(pos, vel, 1))
    return _cache["planar", n]


def mixed(oracle, n):
    """records 0 .. 512 (of 1100; scaled for other n) planar with velocities inside the rule-3 bound, .. 768 off the plane, .. 1024
    planar with velocities on both sides of the bound (the rule-3 test holds for some pairs and fails for others), the rest like the
    first but for one non-finite record: (pos, vel, reference with rule_3_distance = R3)"""
    if ("mixed", n) not in _cache:
        a, b, c = (k * n // 1100 for k in (512, 768, 1024))
        pos, vel = mixed_tiles(oracle, n, 99, (a, b), (a, (a + b) // 2), max(0, n - 6))
        rng = np.random.default_rng(n)
        vel[:, :2] = rng.uniform(-0.25, 0.25, (n, 2)).astype(np.float32)
        vel[b:c, :2] = rng.uniform(-0.9, 0.9, (c - b, 2)).astype(np.float32)
        obp = oracle.boids_params()
        obp.rule_3_distance = R3
        _cache["mixed", n] = (pos, vel, oracle.boids_run(pos, vel, 1, obp))
    return _cache["mixed", n]


def test_mixed_data_takes_each_ladder_branch_by_its_own_flags(nb, oracle):
    """at 1100 bodies and tile 256: the workgroup of bodies 0 .. 255 (clean itself) meets a clean tile (planar, rule 3 known to
    hold), a 3-D tile inside the bound, a planar tile outside it and a non-finite one; the workgroup of bodies 512 .. 767 (3-D)
    meets the tile outside the bound as 3-D with rule 3 tested"""
    pos, vel, (p_ref, v_ref) = mixed(oracle, 1100)
    # the non-finite record fails both position tests (d2 = inf) with everybody: the step leaves it alone non-finite
    assert np.isfinite(v_ref).all() and np.flatnonzero(~np.isfinite(p_ref).all(axis=1)).tolist() == [1094]
    bp = nb.default_boids_params()
    bp.rule_3_distance = R3
    lim = vlim(bp)
    assert 0.28 < lim < 0.29
    words = []
    for t in range(0, 1100, 256):
        p, v = pos[t:t + 256], vel[t:t + 256]
        words.append((0 if np.isfinite(p).all() and np.isfinite(v).all() else NONFINITE) | (NONPLANAR if (p[:, 2] != 0).any() or (v[:, 2] != 0).any() else 0)
                     | (VELFAR if not (np.abs(v) <= lim).all() else 0))
    assert words == [0, 0, NONPLANAR, VELFAR, NONFINITE]
    far = vel[768:1024]
    e = np.sqrt(((far[:, None, :] - far[None, :, :]) ** 2).sum(-1))
    assert (e < R3).any() and (e >= R3).any()


def launch(nb, bp, pos, vel, first, count):
    """one step of bodies [first, first + count) through the launch API; rows outside the shard must stay as they were"""
    import torch

    from nenbody_amd.dist import HipBackend

    n, dev = len(pos), torch.device("cuda", 0)

    def rec(a):
        t = torch.zeros((n, 4), dtype=torch.float32)
        t[:, :3] = torch.from_numpy(a)
        return t.to(dev)

    pin, vin = rec(pos), rec(vel)
    pout, vout = torch.full_like(pin, 7.0), torch.full_like(vin, 7.0)
    HipBackend().boids_step(bp, n, first, count, pin, vin, pout, vout)
    torch.cuda.synchronize()
    p, v = pout.cpu().numpy(), vout.cpu().numpy()
    outside = np.r_[0:first, first + count:n]
    assert (p[outside] == 7.0).all() and (v[outside] == 7.0).all(), "a row outside the shard was written"
    assert (p[first:first + count, 3] == 0).all() and (v[first:first + count, 3] == 0).all()
    return p[first:first + count, :3], v[first:first + count, :3]


@pytest.mark.parametrize("n,first,count", SHARDS, ids=[f"n{n}-first{f}-count{c}" for n, f, c in SHARDS])
@pytest.mark.parametrize("pc,tile", FORMS, ids=[f"{FORM_NAMES[pc]}-tile{t or 512}" for pc, t in FORMS])
def test_every_form_every_forced_tile_form_bit_exact(nb, oracle, monkeypatch, pc, tile, n, first, count):
    monkeypatch.setenv("NB_BOIDS_PC", str(pc))
    pos, vel, (p_ref, v_ref) = planar(oracle, n)
    sl = slice(first, first + count)
    for force in range(8):
        monkeypatch.setenv("NB_BOIDS_FORCE", str(force))
        p, v = launch(nb, nb.default_boids_params(tile=tile), pos, vel, first, count)
        assert_bits_equal(v, v_ref[sl], f"velocities, NB_BOIDS_FORCE={force}")
        assert_bits_equal(p, p_ref[sl], f"positions, NB_BOIDS_FORCE={force}")


@pytest.mark.parametrize("n,first,count", SHARDS, ids=[f"n{n}-first{f}-count{c}" for n, f, c in SHARDS])
@pytest.mark.parametrize("pc,tile", FORMS, ids=[f"{FORM_NAMES[pc]}-tile{t or 512}" for pc, t in FORMS])
def test_every_form_on_tiles_with_flags_of_their_own_bit_exact(nb, oracle, monkeypatch, pc, tile, n, first, count):
    monkeypatch.setenv("NB_BOIDS_PC", str(pc))
    pos, vel, (p_ref, v_ref) = mixed(oracle, n)
    bp = nb.default_boids_params(tile=tile)
    bp.rule_3_distance = R3
    sl = slice(first, first + count)
    p, v = launch(nb, bp, pos, vel, first, count)
    assert_bits_equal_nan_alike(p, v, p_ref[sl], v_ref[sl])


# -- the split launch: slices of the j range, the slices' sums added in slice order ---------------------------------------------
CUTS = Consts(rule_3_distance=16 * 2.0 ** -6)     # cuts between lattice velocities: rule 3 stays in the slices' loops
PARTS = {(1, 0, 1): [(0, 1)], (65, 0, 65): [(0, 65)], (600, 0, 600): [(0, 600)], (1100, 0, 1100): [(0, 1100)],
         (1100, 257, 600): [(0, 257), (257, 600), (857, 243)]}   # the shard among its neighbours: the whole set is checked


def lattice(oracle, n, kind, consts):
    key = ("lattice", n, kind, consts is None)
    if key not in _cache:
        pos, vel, cs = boids_lattice(n, 7 + n, kind, R=31, consts=consts)
        _cache[key] = (pos, vel, cs, oracle.boids_run(pos, vel, 1, cs.oracle(oracle)))
    return _cache[key]


@pytest.mark.parametrize("slices", ["1", "3"])
@pytest.mark.parametrize("tile", [256, 512, 1024])
@pytest.mark.parametrize("shard", SHARDS, ids=[f"n{n}-first{f}-count{c}" for n, f, c in SHARDS])
def test_split_launch_on_and_off_the_lattice(nb, oracle, monkeypatch, shard, tile, slices):
    monkeypatch.setenv("NB_BOIDS_SLICES", slices)
    n, parts = shard[0], PARTS[shard]
    for kind, consts in (("planar", None), ("3d", CUTS)):        # rule 3 from the step's total; rule 3 in the loops
        pos, vel, cs, (p_ref, v_ref) = lattice(oracle, n, kind, consts)
        p, v = split_step(nb, pos, vel, parts, cs.nb(nb, tile=tile))
        bad = wrong_bodies(p, v, p_ref, v_ref)
        assert len(bad) == 0, f"lattice, {kind}: {len(bad)} of {n} bodies differ, first {bad[:8].tolist()}"
    if ("cloud", n) not in _cache:
        pos, vel = cloud(oracle, n, seed=n + 1)
        _cache["cloud", n] = (pos, vel, oracle.boids_run(pos, vel, 1))
    pos, vel, (p_ref, v_ref) = _cache["cloud", n]
    bp = nb.default_boids_params(tile=tile)
    p, v = split_step(nb, pos, vel, parts, bp)
    close_to_the_reference(v, v_ref, p, p_ref, f"n={n} slices={slices} tile={tile}", (pos, vel, bp))
