"""GPU tests of the seen boids step where its rules cut and its lists are unsorted:
nb_launch_boids_seen_step on caller lists -- full lists against the C oracle over the whole-set kernels' hostile battery, partial
lists on data where each rule holds for some seen pairs and fails for others, and the header's list contract (list order, duplicates,
the clamp at `stride`, the slots behind the count) against the list-order restatement -- and the chained step Scene.step_boids_seen
under other constants, widths, its own batch split, a caller's camera constant, and mixed with the other steps.  Every comparison is
of every bit; a NaN of the reference must be met by a NaN.  tests/test_seen_lists_cpu.py checks on the same arrays that these inputs
can tell a wrong kernel from a right one."""
import numpy as np
import pytest

import seen_cases as K
import seen_restatement as S
from seen_cases import PAD
from test_gpu_boids import matrices_equal
from test_gpu_seen import bits, launch_boids_seen

pytestmark = pytest.mark.gpu

F = np.float32


def assert_launch(got, want, first, count, what):
    """rows [first, first + count) of the launch's outputs against (positions, velocities) of those bodies; w = 0 there, and every
    other record, the padding included, keeps its fill"""
    for g, w, name in zip(got, want, ("positions", "velocities")):
        ok, rows = K.same_words(g[first:first + count, :3], w)
        assert ok, f"{what}: {name} of {len(rows)} of {count} bodies differ, first {first + rows[:8]}"
        assert (g[first:first + count, 3] == 0).all(), f"{what}: {name}: w is not 0"
        rest = np.ones(len(g), bool)
        rest[first:first + count] = False
        assert (g[rest] == -7).all(), f"{what}: {name} written outside the range"


def launch(nb, pos, vel, cnt, lists, first=0, tile=0, **kw):
    return launch_boids_seen(len(pos), first, len(lists), pos, vel, cnt, lists, K.device_params(nb, tile=tile, **kw))


# -- (a) full lists: the C oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_full_lists_ragged_sizes_are_the_oracle_step(nb, oracle, n):
    pos, vel = K.cloud(oracle, n, seed=n)
    got = launch_boids_seen(n, 0, n, pos, vel, *K.full_lists(n, n))                      # params NULL: the defaults
    assert_launch(got, oracle.boids_run(pos, vel, 1), 0, n, f"n={n}")


@pytest.mark.parametrize("first,count", [(0, 1), (1, 255), (256, 257), (513, 487)])
def test_full_lists_ranges_are_the_oracle_range(nb, oracle, first, count):
    n = 1000
    pos, vel = K.cloud(oracle, n, seed=n)
    got = launch_boids_seen(n, first, count, pos, vel, *K.full_lists(count, n))
    assert_launch(got, oracle.boids_step_range(pos, vel, first, count), first, count, f"[{first}, {first + count})")


@pytest.mark.parametrize("name", K.FULL_LIST_CASES)
def test_full_lists_battery_is_the_oracle_step(nb, oracle, name):
    """radius boundaries, a rule-3 radius that cuts, radii 0, -1, NaN and +inf, subnormal and huge thresholds, d2 = +inf, and
    non-finite positions: the whole-set kernels' battery, here through the seen kernel's own three tests"""
    pos, vel, kw = K.full_list_case(oracle, name)
    n = len(pos)
    got = launch(nb, pos, vel, *K.full_lists(n, n), **kw)
    assert_launch(got, oracle.boids_run(pos, vel, 1, K.oracle_params(oracle, **kw)), 0, n, name)


# -- (b) partial lists where every rule cuts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_partial_lists_where_every_rule_cuts(nb, oracle, density):
    n = 800
    pos, vel = K.cut_cloud(oracle, n, 5)
    mask = K.bernoulli_mask(n, density, 5)
    got = launch(nb, pos, vel, *S.lists_of_mask(mask, n), **K.CUT)
    assert_launch(got, S.boids_seen_step(pos, vel, mask, **K.CUT), 0, n, f"density {density}")


# -- (c) the list contract ---------------------------------------------------------------------------------------------------------------
N_C, STRIDE_C = 300, 48


@pytest.fixture(scope="module")
def contract(oracle):
    """the order data, its variants, and the restatement's result for each, computed once"""
    pos, vel = K.cut_cloud(oracle, N_C, 9)
    variants = K.contract_variants(N_C, STRIDE_C, 9)
    want = {name: S.boids_seen_step_lists(pos, vel, cnt, lists, **K.CUT) for name, (cnt, lists) in variants.items()}
    return pos, vel, variants, want


@pytest.mark.parametrize("name", ["ascending", "permuted", "duplicate appended", "one entry repeated", "count above stride", "count zero",
                                  "valid ids behind the count", "own index and padding in the middle"])
def test_list_contract(nb, contract, name):
    pos, vel, variants, want = contract
    got = launch(nb, pos, vel, *variants[name], **K.CUT)
    assert_launch(got, want[name], 0, N_C, name)
    if name == "count zero":                                                             # the body stops: velocity +0, position kept
        assert (bits(got[1][:N_C, :3]) == 0).all() and (bits(got[0][:N_C, :3]) == bits(pos)).all()
    if name == "permuted":                                                               # a kernel that sorted its lists fails here
        differs = (bits(got[1][:N_C, :3]) != bits(want["ascending"][1])).any(1)
        assert differs.sum() >= N_C // 4, f"list order changes only {int(differs.sum())} of {N_C} bodies"


def test_list_contract_stride_one(nb, contract):
    pos, vel = contract[:2]
    cnt, lists = K.stride_one_lists(N_C, 4)
    assert_launch(launch(nb, pos, vel, cnt, lists, **K.CUT), S.boids_seen_step_lists(pos, vel, cnt, lists, **K.CUT), 0, N_C, "stride 1")


def test_list_contract_on_a_range(nb, contract):
    """row e of the lists is body first + e: own-index entries are the range's bodies', not the rows'"""
    pos, vel, variants, want = contract
    cnt, lists = variants["own index and padding in the middle"]
    first, count = 37, 100
    got = launch(nb, pos, vel, cnt[first:first + count], lists[first:first + count], first=first, **K.CUT)
    w = want["own index and padding in the middle"]
    assert_launch(got, (w[0][first:first + count], w[1][first:first + count]), first, count, "range")


# -- (d) overrides and determinism -------------------------------------------------------------------------------------------------------
def test_tile_and_form_overrides_and_a_second_launch_give_the_same_bits(nb, contract, monkeypatch):
    pos, vel, variants, want = contract
    cnt, lists = variants["permuted"]
    base = launch(nb, pos, vel, cnt, lists, **K.CUT)
    assert_launch(base, want["permuted"], 0, N_C, "base")
    again = launch(nb, pos, vel, cnt, lists, **K.CUT)
    assert (bits(again[0]) == bits(base[0])).all() and (bits(again[1]) == bits(base[1])).all()
    for tile in (256, 512, 1024):
        got = launch(nb, pos, vel, cnt, lists, tile=tile, **K.CUT)
        assert (bits(got[0]) == bits(base[0])).all() and (bits(got[1]) == bits(base[1])).all(), f"tile {tile}"
    for force, pc in (("1", "3"), ("4", "1"), ("6", "2"), ("2", "4"), ("7", "5")):      # the seen form ignores these
        monkeypatch.setenv("NB_BOIDS_FORCE", force)
        monkeypatch.setenv("NB_BOIDS_PC", pc)
        got = launch(nb, pos, vel, cnt, lists, **K.CUT)
        assert (bits(got[0]) == bits(base[0])).all() and (bits(got[1]) == bits(base[1])).all(), f"NB_BOIDS_FORCE={force} NB_BOIDS_PC={pc}"


# -- the chained step --------------------------------------------------------------------------------------------------------------------
def assert_step(nb, sc, what, consts, **kw):
    """one seen step of the Scene's current state under `consts` against the restatement under the same, the mask from Scene.eyes
    of that state: the mask"""
    p0, v0 = sc.state()
    ids, _ = sc.eyes(**{k: v for k, v in kw.items() if k in ("width", "cp")})
    mask = S.mask_of_rows(ids, sc.n)
    want = S.boids_seen_step(p0, v0, mask, **consts)
    done = sc.steps_done
    sc.step_boids_seen(K.device_params(nb, **consts), **kw)
    got = sc.state()
    for g, w, name in zip(got, want, ("positions", "velocities")):
        ok, rows = K.same_words(g, w)
        assert ok, f"{what}: {name} of {len(rows)} of {sc.n} bodies differ, first {rows[:8]}"
    assert sc.steps_done == done + 1
    return mask


def test_other_constants_three_steps_and_blind_bodies_stay_blind(nb, oracle):
    pos, vel = K.chain_state(oracle, 300, 41)
    with nb.Scene(pos, vel) as sc:
        blind = None
        for k in range(3):
            mask = assert_step(nb, sc, f"step {k}", K.CHAIN)
            now = mask.sum(1) == 0
            if blind is not None:
                assert now[blind].all()                                                  # a stopped body has no heading: it sees nobody
            blind = now if blind is None else blind | now
            p, v = sc.state()
            assert (bits(v[now]) == 0).all()
        assert blind.sum() >= 1 and (~blind).sum() > 150


@pytest.mark.parametrize("width", [1, 3, 65, 4096])
def test_other_constants_widths(nb, oracle, width):
    pos, vel = K.chain_state(oracle, 257, 31)
    with nb.Scene(pos, vel) as sc:
        assert_step(nb, sc, f"W={width}", K.CHAIN, width=width)


def test_the_library_splits_a_large_set_into_batches(nb, oracle):
    """width 4096: the default batch is (64 << 20) // (4096 * 8 + 4) = 2047 eyes, so 2100 bodies run as 2047 + 53"""
    n, width = 2100, 4096
    assert n > (64 << 20) // (width * 8 + 4)
    pos, vel = K.chain_state(oracle, n, 5)
    with nb.Scene(pos, vel) as sc:
        assert_step(nb, sc, "default batch", K.CHAIN, width=width)
        split = sc.state()
    with nb.Scene(pos, vel) as sc:
        sc.step_boids_seen(K.device_params(nb, **K.CHAIN), width=width, batch=n)
        whole = sc.state()
    assert (bits(split[0]) == bits(whole[0])).all() and (bits(split[1]) == bits(whole[1])).all()


def test_a_batch_of_one(nb, oracle):
    pos, vel = K.chain_state(oracle, 65, 65)
    with nb.Scene(pos, vel) as sc:
        assert_step(nb, sc, "batch 1", K.CHAIN, batch=1)


def test_seen_steps_mix_with_the_other_steps(nb, oracle):
    """the velocity buffers swap and the position buffers flip under the seen step; every other step must find the state there"""
    n, seed = 600, 77
    pos, vel = K.chain_state(oracle, n, 12)

    def check(sc, want, what):
        for g, w, name in zip(sc.state(), want, ("positions", "velocities")):
            ok, rows = K.same_words(g, w)
            assert ok, f"{what}: {name} of {len(rows)} bodies differ, first {rows[:8]}"

    def seen_step(sc, what):
        assert_step(nb, sc, what, K.CHAIN)
        p, v = sc.state()
        assert matrices_equal(sc.instances(), oracle.instances(p, v)), f"{what}: model matrices are not the new state's"
        return p, v

    with nb.Scene(pos, vel) as sc:
        sc.step_n(1)
        p, v = oracle.run(pos, vel, 1)
        check(sc, (p, v), "n-body step")
        p, v = seen_step(sc, "seen step after the n-body step")
        sc.step_boids_n(1)
        p, v = oracle.boids_run(p, v, 1)
        check(sc, (p, v), "boids step")
        p, v = seen_step(sc, "seen step after the boids step")
        assert sc.steps_done == 4
        sc.step_random(seed, 1)
        p, v = oracle.random_run(p, v, 1, seed, first_step=4)
        check(sc, (p, v), "random step")
        seen_step(sc, "seen step after the random step")
        assert sc.steps_done == 6


def test_a_caller_camera_constant_with_other_constants(nb, oracle):
    n = 300
    pos, vel = K.chain_state(oracle, n, 9)
    rng = np.random.default_rng(9)
    pos[:, 2] = rng.uniform(-10, 10, n).astype(F)
    vel[:, 2] = rng.uniform(-1.5, 1.5, n).astype(F)
    cp = oracle.camera_constant(30.0, 1.0, 1.0, 10000.0)
    with nb.Scene(pos, vel) as sc:
        mask = assert_step(nb, sc, "3-D, cp", K.CHAIN, cp=cp)
        _, v = sc.state()
    shares = K.predicate_shares(pos, vel, mask, **K.CHAIN)
    assert shares[3] > 100 and all(0.02 < s < 0.98 for s in shares[:3]), shares
    assert (v[:, 2] != 0).any()
