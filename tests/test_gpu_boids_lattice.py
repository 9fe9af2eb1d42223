"""The boids split form (nb_launch_boids_step_split, nb_shard_set_boids_split, ShardedScene.step_boids(split=True)) bit for bit on
every body of an exact lattice (tests/boids_lattice.py): there every sum is exact in any order, so the split form's reassociated
sums must give the reference's words.  Against the oracle up to 20 000 bodies, against the lattice's expectation above.  Where the
scratch is the caller's (split_step, ShardedScene) a test also reads back which path ran -- the flag word the prep kernel leaves at
the end of the scratch (the rule-3 shortcut or the in-loop test) -- and the slice count the scratch size implies, and checks both;
the native shard keeps its scratch to itself, so its tests check the bits and name the restated slices and path.  Every message
names share, slices and path."""
import os
import socket

import numpy as np
import pytest

from boids_lattice import (Consts, assert_exact, boids_lattice, expected, flag_word, schedule_state, shortcut, slices_from_scratch_bytes,
                           split_shape, wrong_bodies)
from boids_split import split_step
from nenbody_amd.dist import partition

pytestmark = pytest.mark.gpu

F = np.float32
ORACLE_MAX = 20000


def path_name(short):
    return "rule-3 shortcut (total minus own)" if short else "rule 3 in the loop"


def reference(oracle, pos, vel, cs):
    """the oracle's step where it is affordable (and the expectation must agree with it), else the expectation"""
    p_exp, v_exp = expected(pos, vel, cs)
    if len(pos) <= ORACLE_MAX:
        p_ref, v_ref = oracle.boids_run(pos, vel, 1, cs.oracle(oracle))
        assert len(wrong_bodies(p_exp, v_exp, p_ref, v_ref)) == 0, "the lattice's expectation is not the oracle's step"
        return p_ref, v_ref
    return p_exp, v_exp


def check_shares(p, v, p_ref, v_ref, info, pos, vel, cs, what, force=0, knob=None, tile=1024):
    """every body of every share bit for bit; the flag word and the slice count each share's launch used"""
    n = len(pos)
    word = flag_word(pos, vel, cs)
    short = shortcut(word, cs, force)
    for part in info:
        first, count = part["first"], part["count"]
        slices = slices_from_scratch_bytes(part["scratch_bytes"], n, count)
        share = f"{what}: share ({first}, {count}) of n={n}, {slices} slices, {path_name(short)}"
        assert part["flags"] == word, f"{share}: flag word {part['flags']:#x}, expected {word:#x}"
        assert slices == split_shape(n, count, tile, knob)[0], f"{share}: the library's slice count is not boids_split_shape's"
        sl = slice(first, first + count)
        bad = first + wrong_bodies(p[sl], v[sl], p_ref[sl], v_ref[sl])
        assert len(bad) == 0, (f"{share}: {len(bad)} of {count} bodies differ from the reference, first {bad[:8].tolist()}: "
                               f"v {v[bad[0]].tolist()} against {v_ref[bad[0]].tolist()}")


# -- 1. launch shapes through split_step: a covering design ---------------------------------------------------------------------
SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 3000, 20000]
SLICES = ["1", "2", "3", "7", "64", None]
TILES = [256, 512, 1024]
FORCES = [0, 1, 2, 4, 6, 7]
CUTS = Consts(rule_3_distance=16 * 2.0 ** -6)     # rule 3 cuts between lattice velocities (+-63 qv): the in-loop path


def size_class(n):
    return 0 if n <= 2 else 1 if n <= 257 else 2 if n <= 1025 else 3


def parts_for(n, c):
    forms = [[(0, n)], [(0, 1), (1, n - 1)] if n > 1 else [(0, n)], [(0, 1000), (1000, n - 1000)] if n > 1000 else [(0, n)]]
    if n >= 3:
        forms.append([(f, k) for f, k in partition(n, 3) if k])
    return forms[c % len(forms)]


def _design():
    """(n, NB_BOIDS_SLICES, tile, NB_BOIDS_FORCE, kind, cuts, k): planar, 3-D and mixed data each against every force value, on
    the shortcut (default rule_3_distance) and on the in-loop path (`cuts`: rule_3_distance = 16 qv) wherever the force value
    allows the shortcut at all (bit 4 forbids it); the lattice's other kinds (ties, the bound's edge, rule 3 held with a small
    radius) besides; mixed data only on sets of several tiles with whole planar tiles (3 000 and 20 000 bodies).  Sizes, slices
    and tiles are dealt round so that every value meets every size class."""
    rows = [(kind, force, cuts) for kind in ("planar", "3d", "mixed") for force in FORCES for cuts in ((False, True) if force & 4 == 0 else (True,))]
    rows += [("ties", f, False) for f in (0, 1, 4, 6, 7)] + [("rule3_edge", f, False) for f in (0, 2, 4, 6, 7)]
    rows += [("rule3_holds", f, False) for f in (0, 1, 2)] + [("rule3_cuts", f, False) for f in (1, 4, 6, 7)]
    classes = [[n for n in SIZES if size_class(n) == c] for c in range(4)]
    per_force, per_class, cases = {}, [0, 0, 0, 0], []
    for k, (kind, force, cuts) in enumerate(rows):
        if kind == "mixed":
            n = (3000, 20000)[k % 2]
        else:                                      # a force value's rows go round the size classes
            i = per_force[force] = per_force.get(force, -1) + 1
            n = classes[i % 4][(i // 4 + k) % len(classes[i % 4])]
        c = size_class(n)
        j = per_class[c]                           # a size class's rows go round the slice counts and the tiles
        per_class[c] += 1
        cases.append((n, SLICES[j % 6], TILES[(j + j // 6) % 3], force, kind, cuts, k))
    # the slice count's clamps at their limits: 127 tiles of 256 with 64 (and 100) slices asked for -> 64 slices of two tiles
    cases += [(32512, "64", 256, 0, "3d", False, len(cases)), (32512, "100", 256, 1, "planar", True, len(cases) + 1)]
    return cases


CASES = _design()


def case_state(n, kind, cuts, k):
    return boids_lattice(n, 100 + k, kind, R=31 if n <= 3000 else 63, consts=CUTS if cuts else None)


def _covers():
    """what the design misses: a knob value against a size class, a force value or a data kind against a rule-3 path (the path
    the flag word and the force value select), mixed data with force 0 and 1 on each path"""
    met = set()
    for n, sl, tile, force, kind, cuts, k in CASES:
        pos, vel, cs = case_state(min(n, 3000), kind, cuts, k)      # (the path does not depend on n above a few bodies)
        path = shortcut(flag_word(pos, vel, cs), cs, force)
        c = size_class(n)
        met |= {("slices", sl, c), ("tile", tile, c), ("force", force, c), ("force", force, path), ("data", kind, path)}
        if kind == "mixed":
            met.add(("mixed", force, path))
    need = {("slices", s, c) for s in SLICES for c in range(4)} | {("tile", t, c) for t in TILES for c in range(4)}
    need |= {("force", f, c) for f in FORCES for c in range(4)}
    need |= {("force", f, p) for f in FORCES for p in ((False, True) if f & 4 == 0 else (False,))}
    need |= {("data", d, p) for d in ("planar", "3d", "mixed") for p in (False, True)} | {("mixed", f, p) for f in (0, 1) for p in (False, True)}
    return need - met


def test_the_covering_design_covers():
    missing = _covers()
    assert not missing, f"the covering design misses {sorted(missing, key=str)[:8]}"
    assert max(split_shape(n, c, tile, sl)[0] for n, sl, tile, *_ in CASES for _, c in parts_for(n, 0)) == 64


@pytest.mark.parametrize("n,slices,tile,force,kind,cuts,k", CASES,
                         ids=[f"n{n}-sl{s or 'lib'}-t{t}-f{f}-{d}{'-cuts' if c else ''}" for n, s, t, f, d, c, _ in CASES])
def test_split_form_launch_shapes_bit_exact(nb, oracle, monkeypatch, n, slices, tile, force, kind, cuts, k):
    if slices is not None:
        monkeypatch.setenv("NB_BOIDS_SLICES", slices)
    monkeypatch.setenv("NB_BOIDS_FORCE", str(force))
    pos, vel, cs = case_state(n, kind, cuts, k)
    p_ref, v_ref = reference(oracle, pos, vel, cs)
    parts = parts_for(n, k)
    info = []
    p, v = split_step(nb, pos, vel, parts, cs.nb(nb, tile=tile), info)
    check_shares(p, v, p_ref, v_ref, info, pos, vel, cs,
                 f"{kind}{', r3 = 16 qv' if cuts else ''}, tile {tile}, NB_BOIDS_FORCE={force}, NB_BOIDS_SLICES={slices}",
                 force=force, knob=slices, tile=tile)


# -- 2. every rank's share at the headline sizes -------------------------------------------------------------------------------
HEADLINE = {
    "131072-planar": (131072, dict(kind="planar"), None),
    "131072-rule3-cuts": (131072, dict(kind="rule3_cuts"), None),
    "2^20-3d": (1 << 20, dict(kind="3d", R=7, V=7), Consts(rule_2_distance=1.5, rule_2_scale=2.0 ** -9)),
}


@pytest.mark.parametrize("name", list(HEADLINE))
def test_split_form_every_share_at_the_headline_sizes(nb, name):
    n, kw, consts = HEADLINE[name]
    pos, vel, cs = boids_lattice(n, 17, consts=consts, **kw)
    p_exp, v_exp, d = expected(pos, vel, cs, detail=True)
    assert 0 < d["clamped"].sum() < n
    for P in (2, 4, 8):
        parts = [(f, c) for f, c in nb.partition(n, P) if c]
        info = []
        p, v = split_step(nb, pos, vel, parts, cs.nb(nb), info)
        check_shares(p, v, p_exp, v_exp, info, pos, vel, cs, f"{name}, {P} ranks")


# -- 3. the hosts ---------------------------------------------------------------------------------------------------------------
def schedule_expectations(oracle, n, seed):
    """(pos, vel, schedule, [(p, v) after each entry]) of  boids(A) -> n-body (dt = 0) -> boids(B), every state exact.

    boids(A) changes every velocity, and the n-body step with dt = 0 keeps them (v + a * 0 = v) while it moves the positions: so
    boids(B) catches a velocity replica left over from before boids(A), and one that does not follow the n-body step's positions,
    but NOT a host that merely skips the rebuild after the n-body step (its replica would hold the same velocities)."""
    pos, vel, A, B = schedule_state(n, seed)
    p1, v1 = reference(oracle, pos, vel, A)
    p2, v2 = oracle.run(p1, v1, 1, dt=F(0))
    assert_exact(p2, v2)
    p3, v3 = reference(oracle, p2, v2, B)
    schedule = (("boids", 1, dict(A.items())), ("nbody", 1), ("boids", 1, dict(B.items())))
    return pos, vel, schedule, [(p1, v1), (p2, v2), (p3, v3)], (A, B)


def launch_tag(n, count, before, consts):
    """what a host's boids step launches for a share of `count` bodies, RESTATED (the library's own slices, no knobs; the path
    from the state) -- for the native shard, whose scratch no caller can read: names only, nothing checked"""
    if not consts:
        return ""
    cs = Consts(**consts[0])
    short = shortcut(flag_word(*before, cs), cs)
    return f", {split_shape(n, count, 1024)[0] if count else 0} slices, {path_name(short)}"


def check_host_launch(n, count, nbytes, word, before, cs, what):
    """a host's split launch, read back from its scratch: the flag word against the restatement, the slice count the scratch size
    implies against boids_split_shape's (the library's own slices); returns the two for the messages"""
    slices = slices_from_scratch_bytes(nbytes, n, count)
    short = shortcut(flag_word(*before, cs), cs)
    tag = f", {slices} slices, {path_name(short)}"
    assert word == flag_word(*before, cs), f"{what}{tag}: flag word {word:#x}, expected {flag_word(*before, cs):#x}"
    assert slices == split_shape(n, count, 1024)[0], f"{what}{tag}: the slice count is not boids_split_shape's"
    return tag


def assert_state(p, v, p_ref, v_ref, what):
    bad = wrong_bodies(p, v, p_ref, v_ref)
    assert len(bad) == 0, f"{what}: {len(bad)} bodies differ, first {bad[:8].tolist()}"


def assert_rows(a, ref, what, first=0):
    assert a.shape == ref.shape, f"{what}: shape {a.shape} against {ref.shape}"
    bad = first + np.flatnonzero((a.view(np.uint32) != np.ascontiguousarray(ref, F).view(np.uint32)).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} bodies differ, first {bad[:8].tolist()}"


@pytest.mark.parametrize("n", [1, 2000])
def test_sharded_scene_split_world_of_one(nb, oracle, n):
    from nenbody_amd.dist import HipBackend

    pos, vel, schedule, refs, (A, B) = schedule_expectations(oracle, n, 31)
    params = nb.default_params()
    params.dt = 0.0
    sc = nb.ShardedScene(pos, vel, params)
    states = [(pos, vel)] + refs
    for i, (what, k, *consts) in enumerate(schedule):
        if what == "nbody":
            sc.step_n(k)
        else:
            cs = Consts(**consts[0])
            sc.step_boids(cs.nb(nb), split=True)
        sc.sync()
        tag = f"ShardedScene(split=True), world 1, n={n}, step {i} ({what})"
        if what == "boids":
            nbytes = sc._boids_partial.numel()
            assert nbytes == HipBackend().boids_split_scratch_bytes(cs.nb(nb), n, n)
            word = int(sc._boids_partial[nbytes - 64:nbytes - 60].cpu().numpy().view(np.uint32)[0])
            tag += check_host_launch(n, n, nbytes, word, states[i], cs, tag)
        assert_state(sc.positions(), sc.velocities(), *refs[i], tag)


@pytest.mark.parametrize("n", [1, 2000])
def test_native_shard_split_world_of_one(nb, oracle, n):
    """the lattice twin of test_native_shard_boids_split_form: boids, an n-body step with dt = 0 (p + v: the state stays on the
    lattice; see schedule_expectations for what it does and does not prove about the velocity replica), boids -- every step bit
    for bit"""
    pos, vel, schedule, refs, _ = schedule_expectations(oracle, n, 37)
    params = nb.default_params()
    params.dt = 0.0
    with nb.NativeShard(pos, vel, params, boids_split=True) as sh:
        for i, (what, k, *consts) in enumerate(schedule):
            if what == "nbody":
                sh.step(k)
            else:
                sh.step_boids(k, Consts(**consts[0]).nb(nb))
            sh.sync()
            tag = f"NativeShard(boids_split=True), world 1, n={n}, step {i} ({what}){launch_tag(n, n, ([(pos, vel)] + refs)[i], consts)}"
            assert_state(sh.positions(), sh.local_velocities(), *refs[i], tag)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,n", [(2, 2000), (3, 1000), (3, 2)])
def test_native_shard_split_worlds_of_two_and_three(tmp_path, nb, oracle, world, n):
    """the native shard's split form with world > 1 (gloo through the host, processes sharing the GPU): every rank's replica of
    the positions and its velocities after every step; (3, 2) leaves one rank without bodies"""
    import torch.multiprocessing as mp

    pos, vel, schedule, refs, _ = schedule_expectations(oracle, n, 41 + world)
    mp.spawn(_native_entry, args=(world, _port(), n, nb.NB_MODE_STRICT, str(tmp_path), schedule, (pos, vel)), nprocs=world, join=True)
    covered = 0
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        assert (first, count) == nb.partition(n, world)[r]
        for i, (what, _, *consts) in enumerate(schedule):
            p_ref, v_ref = refs[i]
            tag = (f"NativeShard(boids_split=True), world {world}, rank {r} share ({first}, {count}) of n={n}, step {i} ({what})"
                   f"{launch_tag(n, count, ([(pos, vel)] + refs)[i], consts)}")
            assert_rows(got[f"pos_{i}"], p_ref, f"{tag}: positions (replica)")
            assert_rows(got[f"vel_{i}"], v_ref[first:first + count], f"{tag}: velocities", first)
        covered += count
    assert covered == n


def _native_entry(rank, world, port, n, mode, out_dir, schedule, state):
    from test_gpu_native_shard import _rank_worker

    _rank_worker(rank, world, port, n, mode, out_dir, schedule=schedule, boids_split=True, state=state, nbody=dict(dt=0.0))


@pytest.mark.parametrize("world,n", [(2, 2000), (3, 1000), (3, 2)])
def test_sharded_scene_split_worlds_of_two_and_three(tmp_path, nb, oracle, world, n):
    import torch.multiprocessing as mp

    pos, vel, schedule, refs, _ = schedule_expectations(oracle, n, 43 + world)
    mp.spawn(_scene_entry, args=(world, _port(), n, nb.NB_MODE_STRICT, str(tmp_path), schedule, (pos, vel)), nprocs=world, join=True)
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        first, count = nb.partition(n, world)[r]
        for i, (what, _, *consts) in enumerate(schedule):
            tag = f"ShardedScene(split=True), world {world}, rank {r} share ({first}, {count}) of n={n}, step {i} ({what})"
            if what == "boids" and count:
                tag += check_host_launch(n, count, int(got[f"scratch_{i}"]), int(got[f"flags_{i}"]), ([(pos, vel)] + refs)[i],
                                         Consts(**consts[0]), tag)
            elif what == "boids":
                assert f"scratch_{i}" not in got, f"{tag}: a rank without bodies allocated split scratch"
            assert_state(got[f"pos_{i}"], got[f"vel_{i}"], *refs[i], tag)


def _scene_entry(rank, world, port, n, mode, out_dir, schedule, state):
    from test_gpu_parity import _rank_worker

    _rank_worker(rank, world, port, n, 0, mode, out_dir, boids_split=True, state=state, schedule=schedule, nbody=dict(dt=0.0))
