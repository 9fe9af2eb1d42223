"""GPU tests of the seen sets and the seen boids step: the HIP kernels of nb_seen.inc against the numpy
restatement (tests/seen_restatement.py), every word of every list -- unused slots included -- and every bit of every body's
position and velocity, with the mask taken from Scene.eyes of the state before the step."""
import os
import subprocess

import numpy as np
import pytest

import eyes_restatement as R
import seen_restatement as S
from conftest import ROOT
from seen_cases import PAD   # NaN records behind n_total: an out-of-set entry that were read would show as a NaN, not as a fault

pytestmark = pytest.mark.gpu

F = np.float32
NONE = S.NONE
UP = np.array([0, 0, 1], F)
FILL = 0x07070707        # what the outputs hold before a launch: every word must be written


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# -- crafted rows through nb_launch_seen -------------------------------------------------------------------------------------------------
def crafted_rows(width, seed=0):
    """one row per pattern: (ids (E, W) uint32, depth (E, W) float32)"""
    rng = np.random.default_rng(1000 * width + seed)
    c = np.arange(width)
    rows = []
    pool = rng.integers(0, 50, width).astype(np.uint32)                       # a few ids, many columns each, a third of them empty
    pool[rng.random(width) < 0.33] = NONE
    rows.append((pool, rng.random(width, dtype=F)))
    rows.append((np.full(width, NONE, np.uint32), np.ones(width, F)))          # an all-empty row
    rows.append((np.full(width, 77, np.uint32), rng.random(width, dtype=F)))   # one id everywhere
    rows.append((((width - 1 - c) * 3 + 1).astype(np.uint32), rng.random(width, dtype=F)))   # width distinct ids, descending
    rows.append((np.where(c % 2 == 0, 9, 4).astype(np.uint32), np.where(c % 2 == 0, F(0.25), F(0.75)).astype(F)))   # two ids alternating
    ext = np.array([0, 0x80000000, 0xFFFFFFFE, NONE], np.uint32)[rng.integers(0, 4, width)]   # ids at and above 2^31 are ordinary ids
    rows.append((ext, rng.random(width, dtype=F)))
    edge = np.array([0, 1, 0x3F7FFFFF, 0x00400000, 0x3F000000], np.uint32)[rng.integers(0, 5, width)]   # +0, subnormals, the last below 1
    rows.append((rng.integers(0, 3, width).astype(np.uint32), edge.view(F)))
    wild = rng.integers(0, 2 ** 32, width, dtype=np.uint64).astype(np.uint32)               # a caller's row: any bit pattern as a depth
    rows.append((rng.integers(0, 7, width).astype(np.uint32), wild.view(F)))
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def launch_seen(ids, depth, want_depth=True, want_cols=True):
    """nb_launch_seen on torch tensors and a stream of its own: (count, ids, depth or None, cols or None) as numpy arrays"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    e, w = ids.shape
    t_ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32)).to(dev)
    t_depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int32)).to(dev) if depth is not None else None
    o_count = torch.full((e,), FILL, dtype=torch.int32, device=dev)
    o_ids = torch.full((e, w), FILL, dtype=torch.int32, device=dev)
    o_depth = torch.full((e, w), FILL, dtype=torch.int32, device=dev) if want_depth else None
    o_cols = torch.full((e, w), FILL, dtype=torch.int32, device=dev) if want_cols else None
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        _lib.check(lib.nb_launch_seen(e, w, t_ids.data_ptr(), t_depth.data_ptr() if t_depth is not None else None, o_count.data_ptr(),
                                      o_ids.data_ptr(), o_depth.data_ptr() if want_depth else None,
                                      o_cols.data_ptr() if want_cols else None, s.cuda_stream))
    s.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)
    return host(o_count), host(o_ids), host(o_depth), host(o_cols)


def assert_lists(got, want, what, depth=True, cols=True):
    gc, gi, gd, gl = got
    wc, wi, wd, wl = want
    assert (gc == wc).all(), f"{what}: counts differ in rows {np.nonzero(gc != wc)[0][:8]}"
    assert (gi == wi).all(), f"{what}: ids differ, first at {np.argwhere(gi != wi)[0]}"
    if depth:
        assert (gd == bits(wd)).all(), f"{what}: depths differ, first at {np.argwhere(gd != bits(wd))[0]}"
    if cols:
        assert (gl == wl).all(), f"{what}: cols differ, first at {np.argwhere(gl != wl)[0]}"


@pytest.mark.parametrize("width", [1, 3, 63, 64, 65, 1000, 1024, 4095, 4096])
def test_crafted_rows_every_word(nb, width):
    ids, depth = crafted_rows(width)
    want = S.seen_rows(ids, depth)
    assert_lists(launch_seen(ids, depth), want, f"W={width}")
    assert want[0][3] == width and want[0][1] == 0                    # the descending row fills its list, the empty row has none
    assert (want[3].sum(1) == (ids != NONE).sum(1)).all()             # S4: the counts add up to the non-empty columns


@pytest.mark.parametrize("width", [3, 65, 1024])
def test_without_depth_rows_and_without_optional_outputs(nb, width):
    ids, depth = crafted_rows(width, 1)
    want = S.seen_rows(ids, None)
    assert_lists(launch_seen(ids, None, want_depth=False), want, "no depth rows", depth=False)
    assert_lists(launch_seen(ids, None, want_depth=False, want_cols=False), want, "ids alone", depth=False, cols=False)
    assert_lists(launch_seen(ids, depth, want_cols=False), S.seen_rows(ids, depth), "no cols", cols=False)


@pytest.mark.parametrize("count,width", [(1, 65), (2, 65), (300, 65), (2100, 3), (2100, 65)])
def test_many_eyes_in_one_launch(nb, count, width):
    """300 rows, and 2100: more than the 2048 workgroups a launch has at most, so some workgroups take a second eye"""
    rng = np.random.default_rng(count + width)
    ids = rng.integers(0, 40, (count, width)).astype(np.uint32)
    ids[rng.random((count, width)) < 0.4] = NONE
    depth = rng.random((count, width), dtype=F)
    assert_lists(launch_seen(ids, depth), S.seen_rows(ids, depth), f"count={count}")


# -- Scene.seen against seen() of Scene.eyes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 100, 257])
def test_scene_seen_is_the_seen_set_of_scene_eyes(nb, oracle, n):
    pos, vel = oracle.init_state(n, 1000 + n)
    with nb.Scene(pos, vel) as sc:
        for see_self in (False, True):
            ids, depth = sc.eyes(see_self=see_self)
            got = sc.seen(see_self=see_self)
            assert_lists((got[0], got[1], bits(got[2]), got[3]), S.seen_rows(ids, depth), f"N={n} see_self={see_self}")
            if see_self and n >= 100:
                assert ((got[1] == np.arange(n, dtype=np.uint32)[:, None]).sum(1) <= 1).all()
    if n >= 100:
        assert (got[0] > 0).mean() > 0.5


@pytest.mark.parametrize("width", [1, 3, 1024, 4096])
def test_scene_seen_widths(nb, oracle, width):
    pos, vel = oracle.init_state(257, 31)
    with nb.Scene(pos, vel) as sc:
        ids, depth = sc.eyes(width=width)
        got = sc.seen(width=width)
    assert_lists((got[0], got[1], bits(got[2]), got[3]), S.seen_rows(ids, depth), f"W={width}")


def test_scene_seen_subsets(nb, oracle):
    pos, vel = oracle.init_state(100, 12)
    with nb.Scene(pos, vel) as sc:
        for first, count in ((5, 10), (99, 1), (40, 0)):
            ids, depth = sc.eyes(first=first, count=count)
            got = sc.seen(first=first, count=count)
            assert got[0].shape == (count,) and got[1].shape == (count, 1024)
            if count:
                assert_lists((got[0], got[1], bits(got[2]), got[3]), S.seen_rows(ids, depth), f"first={first} count={count}")


def test_context_entries_validate_their_arguments(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    pos, vel = oracle.init_state(8, 1)
    buf = np.zeros(8 * 64 + 64, np.uint32)
    p, up, cp = buf.ctypes.data, UP.ctypes.data, np.ascontiguousarray(nb.eye_constant(64)).ctypes.data
    big = _lib.NB_EYES_MAX_WIDTH + 1
    with nb.Scene(pos, vel) as sc:
        ctx = sc._ctx
        for args in ((0, 8, None, cp, 64, 0, p, None, None, None), (0, 8, up, None, 64, 0, p, None, None, None),
                     (0, 8, up, cp, 0, 0, p, None, None, None), (0, 8, up, cp, big, 0, p, None, None, None),
                     (0, 8, up, cp, 64, 2, p, None, None, None), (4, 8, up, cp, 64, 0, p, None, None, None),
                     (0, 8, up, cp, 64, 0, None, None, None, None), (0, 1, up, cp, 64, 0, None, p, p, None)):
            assert lib.nb_eyes_seen(ctx, *args) == _lib.NB_ERR_INVALID, args
        for args in ((1, None, None, cp, 64, 0), (1, None, up, None, 64, 0), (1, None, up, cp, 0, 0), (1, None, up, cp, big, 0)):
            assert lib.nb_step_boids_seen(ctx, *args) == _lib.NB_ERR_INVALID, args
        assert lib.nb_eyes_seen(ctx, 0, 8, up, cp, 64, 0, p, None, None, None) == _lib.NB_OK      # one output is enough


# -- the step ----------------------------------------------------------------------------------------------------------------------------
def assert_step(sc, what, **kw):
    """one seen step of the Scene's current state against the restatement, the mask from Scene.eyes of that state"""
    p0, v0 = sc.state()
    ids, _ = sc.eyes(**{k: v for k, v in kw.items() if k in ("width", "cp")})
    mask = S.mask_of_rows(ids, sc.n)
    want_p, want_v = S.boids_seen_step(p0, v0, mask)
    sc.step_boids_seen(**kw)
    p1, v1 = sc.state()
    bad = (bits(p1) != bits(want_p)).any(1) | (bits(v1) != bits(want_v)).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {sc.n} bodies differ, first {np.nonzero(bad)[0][:8]}"
    assert (bits(sc.positions()) == bits(p1)).all()                  # the mirrors were refreshed
    return mask


@pytest.mark.parametrize("n", [1, 2, 3, 100, 257, 2048])
def test_one_step_every_bit(nb, oracle, n):
    pos, vel = oracle.init_state(n, 1000 + n if n != 2048 else 5)
    with nb.Scene(pos, vel) as sc:
        mask = assert_step(sc, f"N={n}")
        assert sc.steps_done == 1
    if n >= 100:
        sees = mask.sum(1)
        assert (sees == 0).any() and (sees > 0).mean() > 0.5          # the step differs from the plain one (tests/test_seen_cpu.py)


def test_three_consecutive_steps(nb, oracle):
    pos, vel = oracle.init_state(257, 1257)
    with nb.Scene(pos, vel) as sc:
        for k in range(3):
            assert_step(sc, f"step {k}")


def test_three_dimensional_data(nb, oracle):
    n = 300
    pos, vel = oracle.init_state(n, 9)
    rng = np.random.default_rng(9)
    pos[:, 2] = rng.uniform(-30, 30, n).astype(F)
    vel[:, 2] = rng.uniform(-0.05, 0.05, n).astype(F)
    cp = oracle.camera_constant(30.0, 1.0, 1.0, 10000.0)
    with nb.Scene(pos, vel) as sc:
        mask = assert_step(sc, "3-D", cp=cp)
        assert mask.sum() > 100
        _, v = sc.state()
    assert (v[:, 2] != 0).any()


def test_every_batch_size_gives_the_same_bits(nb, oracle):
    pos, vel = oracle.init_state(257, 1257)
    got = []
    for batch in (0, 64, 257, 1000):
        with nb.Scene(pos, vel) as sc:
            if batch == 0:
                assert_step(sc, "batch 0")
            else:
                sc.step_boids_seen(batch=batch)
            got.append(sc.state())
    for p, v in got[1:]:
        assert (bits(p) == bits(got[0][0])).all() and (bits(v) == bits(got[0][1])).all()


def test_hand_case(nb):
    """tests/test_seen_cpu.py derives it: body 0 sees body 1 and takes v.x = 0.7f, body 1 sees nobody and stops"""
    pos = np.array([[0, 0, 0], [10, 0, 0]], F)
    vel = np.array([[1, 0, 0], [1, 0, 0]], F)
    with nb.Scene(pos, vel) as sc:
        count, ids, depth, cols = sc.seen()
        assert (count == [1, 0]).all() and ids[0, 0] == 1 and cols[0, 0] == 144 and (ids[0, 1:] == NONE).all() and (ids[1] == NONE).all()
        sc.step_boids_seen()
        p, v = sc.state()
    vx = (F(10) * F(0.02) + F(0) * F(0.05)) + F(1) * F(0.5)
    assert (bits(v[0]) == [0x3F333333, 0, 0]).all() and bits(p[0])[0] == bits(vx * F(0.04) + F(0))[0] and (bits(p[0])[1:] == 0).all()
    assert (bits(v[1]) == 0).all() and (bits(p[1]) == bits(F([10, 0, 0]))).all()


def test_two_calls_give_identical_bits(nb, oracle):
    pos, vel = oracle.init_state(2048, 21)
    got = []
    for _ in range(2):
        with nb.Scene(pos, vel) as sc:
            lists = sc.seen()
            sc.step_boids_seen_n(2)
            got.append((lists, sc.state()))
    (la, (pa, va)), (lb, (pb, vb)) = got
    assert all((bits(x) == bits(y)).all() if x.dtype == F else (x == y).all() for x, y in zip(la, lb))
    assert (bits(pa) == bits(pb)).all() and (bits(va) == bits(vb)).all()


# -- nb_launch_boids_seen_step with caller lists -----------------------------------------------------------------------------------------
def caller_lists(n, stride, rng):
    """ascending lists without duplicates (so that list order is index order) that hold the body's own index and n itself"""
    count = np.zeros(n, np.uint32)
    lists = np.full((n, stride), NONE, np.uint32)
    for e in range(n):
        pick = np.unique(np.concatenate([rng.choice(n, rng.integers(0, stride - 2), replace=False), [e, n]]).astype(np.uint32))
        count[e] = len(pick)
        lists[e, :len(pick)] = pick
    return count, lists


def launch_boids_seen(n_total, first, count, pos, vel, cnt, lists, params=None):
    """the launch on tensors with PAD extra records of NaNs behind n_total: (pos_out, vel_out) (n_total + PAD, 4) float32, every
    word -7 before the launch; ``params``: an NbBoidsParams, None for the defaults"""
    import ctypes

    import torch

    from nenbody_amd import _lib

    dev = torch.device("cuda", 0)

    def rec(a):
        r = np.full((n_total + PAD, 4), np.nan, F)
        r[:n_total, :3] = a
        r[:n_total, 3] = 0
        return torch.from_numpy(r).to(dev)

    tp, tv = rec(pos), rec(vel)
    op = torch.full((n_total + PAD, 4), -7.0, dtype=torch.float32, device=dev)
    ov = torch.full((n_total + PAD, 4), -7.0, dtype=torch.float32, device=dev)
    tc = torch.from_numpy(np.ascontiguousarray(cnt, np.uint32).view(np.int32)).to(dev)
    tl = torch.from_numpy(np.ascontiguousarray(lists, np.uint32).view(np.int32)).to(dev)
    assert tc.numel() == count and tl.numel() == count * lists.shape[1]      # the kernel reads this many words, no more
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        _lib.check(_lib.load().nb_launch_boids_seen_step(ctypes.byref(params) if params is not None else None, n_total, first, count,
                                                         tp.data_ptr(), tv.data_ptr(), tc.data_ptr(), tl.data_ptr(), lists.shape[1],
                                                         op.data_ptr(), ov.data_ptr(), s.cuda_stream))
    s.synchronize()
    return op.cpu().numpy(), ov.cpu().numpy()


def test_caller_lists_own_index_and_entries_outside_the_set(nb, oracle):
    n, stride = 70, 16
    pos, vel = oracle.init_state(n, 70)
    cnt, lists = caller_lists(n, stride, np.random.default_rng(70))
    assert (lists == np.arange(n, dtype=np.uint32)[:, None]).any(1).all() and (lists == n).any(1).all()
    want_p, want_v = S.boids_seen_step(pos, vel, S.mask_of_lists(cnt, lists, n))
    gp, gv = launch_boids_seen(n, 0, n, pos, vel, cnt, lists)
    assert (bits(gp[:n, :3]) == bits(want_p)).all() and (bits(gv[:n, :3]) == bits(want_v)).all()   # a NaN would show a missing guard
    assert (gp[:n, 3] == 0).all() and (gv[:n, 3] == 0).all() and (gp[n:] == -7).all() and (gv[n:] == -7).all()


@pytest.mark.parametrize("first,count", [(0, 1), (5, 10), (69, 1), (13, 57)])
def test_caller_lists_subsets_write_only_their_range(nb, oracle, first, count):
    n, stride = 70, 16
    pos, vel = oracle.init_state(n, 70)
    cnt, lists = caller_lists(n, stride, np.random.default_rng(71))
    want_p, want_v = S.boids_seen_step(pos, vel, S.mask_of_lists(cnt, lists, n))
    rows = slice(first, first + count)
    gp, gv = launch_boids_seen(n, first, count, pos, vel, cnt[rows].copy(), lists[rows])    # row e of the lists is body first + e
    assert (bits(gp[rows, :3]) == bits(want_p[rows])).all() and (bits(gv[rows, :3]) == bits(want_v[rows])).all()
    rest = np.ones(n + PAD, bool)
    rest[rows] = False
    assert (gp[rest] == -7).all() and (gv[rest] == -7).all()


# -- the C++ host ------------------------------------------------------------------------------------------------------------------------
def test_cpp_seen_host_matches_the_restatement(nb, oracle, tmp_path):
    import test_seen_cpu as C

    C.build_exe()
    n, width = 100, 1024
    out = tmp_path / "out.bin"
    r = subprocess.run([C.EXE, str(n), str(width), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint32)
    cells = n * width
    count, ids, depth, cols, p, v = np.split(raw, [n, n + cells, n + 2 * cells, n + 3 * cells, n + 3 * cells + 3 * n])
    pos, vel = oracle.init_state(n, 1234)
    rows = R.eyes(oracle.cameras(pos, vel, UP, R.eye_constant(oracle, width)), oracle.instances(pos, vel), 0, width)
    want = S.seen_rows(*rows)
    assert_lists((count, ids.reshape(n, width), depth.reshape(n, width), cols.reshape(n, width)), want, "C++ lists")
    want_p, want_v = S.boids_seen_step(pos, vel, S.mask_of_rows(rows[0], n))
    assert (p.reshape(n, 3) == bits(want_p)).all() and (v.reshape(n, 3) == bits(want_v)).all()
