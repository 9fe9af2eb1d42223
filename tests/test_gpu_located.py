"""GPU tests of the located seen sets and the vision-only gravity step: the HIP kernels of nb_located.inc
against the numpy restatement (tests/located_restatement.py), every word of every output -- unused slots included -- and every bit of
every body's position and velocity, with the rows taken from Scene.eyes of the state before the step."""
import ctypes
import subprocess

import numpy as np
import pytest

import eyes_restatement as R
import located_restatement as L
import seen_restatement as S

pytestmark = pytest.mark.gpu

F = np.float32
NONE = L.NONE
UP = np.array([0, 0, 1], F)
FILL = 0x07070707        # what the outputs hold before a launch: every word must be written
PAD = 3                  # NaN records behind n_total, -7 behind the outputs: nothing outside the range is read or written


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# -- crafted rows through nb_launch_seen -> nb_seen_located_launch ---------------------------------------------------------------------------
def crafted_rows(width, seed=0):
    """one row per pattern: (ids (E, W) uint32, depth (E, W) float32 in [0, 1])"""
    rng = np.random.default_rng(1000 * width + seed)
    c = np.arange(width)
    few = (rng.integers(1, 5, width) * F(0.125)).astype(F)                     # four depths: the nearest occurs on several columns
    rows = []
    pool = rng.integers(0, 50, width).astype(np.uint32)                       # a few ids, many columns each, a third of them empty
    pool[rng.random(width) < 0.33] = NONE
    rows.append((pool, rng.random(width, dtype=F)))
    rows.append((np.full(width, NONE, np.uint32), np.ones(width, F)))          # an empty row
    rows.append((np.full(width, 77, np.uint32), rng.random(width, dtype=F)))   # one member on every column
    rows.append((np.full(width, 78, np.uint32), few))                          # ... its nearest depth on many of them
    rows.append((((width - 1 - c) * 3 + 1).astype(np.uint32), rng.random(width, dtype=F)))   # width distinct members, descending
    rows.append((rng.integers(0, 6, width).astype(np.uint32), few))            # equal nearest depth on several columns
    ext = np.array([0, 0x80000000, 0x80000001, 0xFFFFFFFE, NONE], np.uint32)[rng.integers(0, 5, width)]   # ids at and above 2^31
    rows.append((ext, few))
    edge = np.array([0, 1, 0x3F7FFFFF, 0x00400000, 0x3F000000, 0x3F800000], np.uint32)[rng.integers(0, 6, width)]   # +0, subnormals, 1 - ulp, 1
    rows.append((rng.integers(0, 3, width).astype(np.uint32), edge.view(F)))
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def directions(count, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(count, 3)).astype(F)
    d[::3, 2] = 0                                                              # planar headings among them
    d[np.abs(d).sum(1) == 0] = F(1)
    return d


def records(a, dev, pad=0, fill=0.0):
    import torch

    r = np.full((len(a) + pad, 4), np.nan, F)
    r[:len(a), :3] = a
    r[:len(a), 3] = fill
    return torch.from_numpy(r).to(dev)


def launch_located(ids, depth, dirs, cp, up=UP, want_col=True, lists=None):
    """nb_launch_seen (unless ``lists`` = (count, ids, depth) are given) then nb_seen_located_launch on torch tensors and a stream of
    its own: (count, seen_ids, seen_depth bits, col or None, rel bits (E, W, 4)) as numpy arrays"""
    import torch

    from nenbody_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    e, w = ids.shape
    dev_u32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    t_ids, t_depth = dev_u32(ids), dev_u32(np.ascontiguousarray(depth, F))
    if lists is None:
        o_count = torch.full((e,), FILL, dtype=torch.int32, device=dev)
        o_ids = torch.full((e, w), FILL, dtype=torch.int32, device=dev)
        o_depth = torch.full((e, w), FILL, dtype=torch.int32, device=dev)
    else:
        o_count, o_ids, o_depth = dev_u32(np.asarray(lists[0], np.uint32)), dev_u32(np.asarray(lists[1], np.uint32)), dev_u32(np.ascontiguousarray(lists[2], F))
    t_eyes = torch.full((e, 4), float("nan"), dtype=torch.float32, device=dev)     # the eye's own position does not enter
    t_dirs = records(dirs, dev)
    o_col = torch.full((e, w), FILL, dtype=torch.int32, device=dev) if want_col else None
    o_rel = torch.full((e, w, 4), FILL, dtype=torch.int32, device=dev)
    upv, cpm = np.ascontiguousarray(up, F).reshape(3), np.ascontiguousarray(cp, F).reshape(16)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        if lists is None:
            _lib.check(lib.nb_launch_seen(e, w, t_ids.data_ptr(), t_depth.data_ptr(), o_count.data_ptr(), o_ids.data_ptr(), o_depth.data_ptr(), None,
                                          s.cuda_stream))
        _lib.check(lib.nb_seen_located_launch(e, w, t_ids.data_ptr(), t_depth.data_ptr(), o_count.data_ptr(), o_ids.data_ptr(), o_depth.data_ptr(),
                                              t_eyes.data_ptr(), t_dirs.data_ptr(), upv.ctypes.data, cpm.ctypes.data,
                                              o_col.data_ptr() if want_col else None, o_rel.data_ptr(), s.cuda_stream))
    s.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)
    return host(o_count), host(o_ids), host(o_depth), host(o_col), host(o_rel)


def assert_located(got, want, what, col=True):
    """got: (count, ids, depth bits, col, rel bits) of a launch; want: located_of_rows' six arrays"""
    gc, gi, gd, gcol, grel = got
    wc, wi, wd, _, wcol, wrel = want
    assert (gc == wc).all() and (gi == wi).all() and (gd == bits(wd)).all(), f"{what}: the lists differ"
    if col:
        assert (gcol == wcol).all(), f"{what}: columns differ, first at {np.argwhere(gcol != wcol)[0]}"
    assert (grel == bits(wrel)).all(), f"{what}: seen_rel differs, first at {np.argwhere(grel != bits(wrel))[0]}"


@pytest.mark.parametrize("width", [1, 3, 63, 64, 65, 1000, 1024, 4095, 4096])
def test_crafted_rows_every_word(nb, width):
    ids, depth = crafted_rows(width)
    dirs = directions(len(ids), width)
    cp = nb.eye_constant(width)
    want = L.located_of_rows(ids, depth, dirs, UP, cp)
    assert_located(launch_located(ids, depth, dirs, cp), want, f"W={width}")
    count, col = want[0], want[4]
    assert count[1] == 0 and count[2] == 1 and count[4] == width and (col[1] == NONE).all()       # the empty row, one member, W members
    assert col[2, 0] == np.argmin(bits(depth[2])) and (np.sort(col[4]) == np.arange(width)).all()  # the lowest nearest column; one column each
    used = np.arange(width)[None, :] < count[:, None]
    assert (col[used] != NONE).all() and (col[~used] == NONE).all()
    if width >= 63:
        assert ((depth[3] == F(0.125)).sum() > 1) and col[3, 0] == np.nonzero(depth[3] == F(0.125))[0][0]     # L1's tie: the lowest column
        assert (want[1][6, :count[6]] >= 0x80000000).sum() >= 2


@pytest.mark.parametrize("width", [3, 65, 1024])
def test_without_seen_col_and_with_another_up(nb, width):
    ids, depth = crafted_rows(width, 1)
    dirs = directions(len(ids), width + 1)
    cp = nb.camera_constant(30.0, 1.0, 1.0, 10000.0)
    up = np.array([0.25, -0.5, 1.0], F)
    want = L.located_of_rows(ids, depth, dirs, up, cp)
    assert_located(launch_located(ids, depth, dirs, cp, up=up, want_col=False), want, "no seen_col", col=False)
    assert_located(launch_located(ids, depth, dirs, cp, up=up), want, "another up")
    assert (want[5][:, :, 2] != 0).any()


@pytest.mark.parametrize("count,width", [(1, 65), (2, 65), (300, 65), (2100, 3), (2100, 65)])
def test_many_eyes_in_one_launch(nb, count, width):
    """300 rows, and 2100: more than the 2048 workgroups a launch has at most, so some workgroups take a second eye"""
    rng = np.random.default_rng(count + width)
    ids = rng.integers(0, 40, (count, width)).astype(np.uint32)
    ids[rng.random((count, width)) < 0.4] = NONE
    depth = (rng.integers(1, 9, (count, width)) * F(0.0625)).astype(F)
    dirs = directions(count, count)
    cp = nb.eye_constant(width)
    assert_located(launch_located(ids, depth, dirs, cp), L.located_of_rows(ids, depth, dirs, UP, cp), f"count={count}")


@pytest.mark.parametrize("width", [3, 65, 1024])
def test_a_list_that_is_not_of_its_row(nb, width):
    """eye e is handed the list of eye e + 1: ascending and without duplicates as a list is, but of another row -- members that are not
    in the row, or not at that depth, get no column; and counts above the width, which read as the width"""
    ids, depth = crafted_rows(width, 2)
    dirs = directions(len(ids), 5)
    cp = nb.eye_constant(width)
    count, sids, sdepth, _ = S.seen_rows(ids, depth)
    count, sids, sdepth = np.roll(count, -1), np.roll(sids, -1, 0), np.roll(sdepth, -1, 0)
    count[2] = width + 7
    count[5] = 0xFFFFFFFF
    wcol, wrel = L.located_rows(ids, depth, count, sids, sdepth, dirs, UP, cp)
    got = launch_located(ids, depth, dirs, cp, lists=(count, sids, sdepth))
    assert (got[3] == wcol).all() and (got[4] == bits(wrel)).all()
    used = np.arange(width)[None, :] < np.minimum(count, width)[:, None]
    assert (wcol[used] == NONE).any()
    if width > 3:
        assert (wcol[used] != NONE).any()


# -- Scene.located against the restatement of Scene.eyes -------------------------------------------------------------------------------------
def assert_scene_located(sc, vel, what, width=1024, cp=None, **kw):
    import nenbody_amd as nb

    ids, depth = sc.eyes(width=width, cp=cp, **kw)
    first, count = kw.get("first", 0), len(ids)
    got = sc.located(width=width, cp=cp, **kw)
    want = L.located_of_rows(ids, depth, vel[first:first + count], UP, nb.eye_constant(width) if cp is None else cp)
    assert got[5].shape == (count, width, 4)
    assert_located((got[0], got[1], bits(got[2]), got[4], bits(got[5])), want, what)
    assert (got[3] == want[3]).all(), f"{what}: seen_cols differ"
    return want


@pytest.mark.parametrize("width", [64, 1024])
@pytest.mark.parametrize("n", [1, 2, 3, 100, 257])
def test_scene_located_is_the_located_set_of_scene_eyes(nb, oracle, n, width):
    pos, vel = oracle.init_state(n, 1000 + n)
    with nb.Scene(pos, vel) as sc:
        want = assert_scene_located(sc, vel, f"N={n} W={width}", width=width)
        assert_scene_located(sc, vel, f"N={n} W={width} see_self", width=width, see_self=True)
    if n >= 100:
        count, sids, col, rel = want[0], want[1], want[4], want[5]
        assert (count > 0).mean() > 0.5 and (col[np.arange(width)[None, :] < count[:, None]] != NONE).all()
        e = int(np.argmax(count))                     # against the truth: within the outline and the depth resolution (tests/test_located_cpu.py)
        true = pos[sids[e, :count[e]]].astype(np.float64) - pos[e]
        err = np.linalg.norm(rel[e, :count[e], :3] - true, axis=1)
        assert (err <= np.sqrt(2) + 4 * 1.33270 * 2.0 ** -24 * (true * true).sum(1)).all()


def test_scene_located_subsets_and_partial_outputs(nb, oracle):
    from nenbody_amd import _lib

    pos, vel = oracle.init_state(100, 12)
    with nb.Scene(pos, vel) as sc:
        for first, count in ((5, 10), (99, 1), (40, 0)):
            if count:
                assert_scene_located(sc, vel, f"first={first} count={count}", first=first, count=count)
            else:
                got = sc.located(first=first, count=0)
                assert got[0].shape == (0,) and got[5].shape == (0, 1024, 4)
        # one output is enough, none is refused; an orthographic caller camera gives rows but no located sets
        rel = np.empty((10, 1024, 4), F)
        upv, cpm = UP.copy(), np.ascontiguousarray(nb.eye_constant(1024), F).reshape(16)
        args = (sc._ctx, 5, 10, upv.ctypes.data, cpm.ctypes.data, 1024, 0)
        assert sc._lib.nb_eyes_located(*args, None, None, None, None, None, rel.ctypes.data) == _lib.NB_OK
        ids, depth = sc.eyes(first=5, count=10)
        assert (bits(rel) == bits(L.located_of_rows(ids, depth, vel[5:15], UP, cpm)[5])).all()
        assert sc._lib.nb_eyes_located(*args, None, None, None, None, None, None) == _lib.NB_ERR_INVALID
        lattice = R.lattice_camera()
        assert sc.eyes(cp=lattice)[0].shape == (100, 1024)
        with pytest.raises(nb.NbError, match=r"nb_eyes_located: cp16 cannot be inverted: cp16\[11\] must be -1"):
            sc.located(cp=lattice)
        with pytest.raises(nb.NbError, match=r"nb_step_nbody_located: cp16 cannot be inverted: cp16\[11\] must be -1"):
            sc.step_nbody_located(cp=lattice)
        assert sc.steps_done == 0


def three_dimensional(oracle, n=300, seed=9):
    pos, vel = oracle.init_state(n, seed)
    rng = np.random.default_rng(seed)
    pos[:, 2] = rng.uniform(-30, 30, n).astype(F)
    vel[:, 2] = rng.uniform(-0.05, 0.05, n).astype(F)
    return pos, vel, oracle.camera_constant(30.0, 1.0, 1.0, 10000.0)


def test_scene_located_three_dimensional_data(nb, oracle):
    pos, vel, cp = three_dimensional(oracle)
    with nb.Scene(pos, vel) as sc:
        want = assert_scene_located(sc, vel, "3-D", cp=cp)
    count, rel = want[0], want[5]
    assert count.sum() > 100 and (rel[:, :, 2] != 0).any()
    # the estimate lies in the plane through the eye spanned by f and s: no component along s x f
    f, s = L.axes(vel, UP)
    u = np.cross(s.astype(np.float64), f.astype(np.float64))
    off = np.abs((rel[:, :, :3].astype(np.float64) * u[:, None, :]).sum(2))
    assert (off <= 1e-5 * np.maximum(rel[:, :, 3], 1)).all()


# -- the fold alone: nb_nbody_located_step_launch ----------------------------------------------------------------------------------------------
def launch_fold(n_total, first, count, pos, vel, cnt, rel, params=None):
    """the launch on tensors with PAD records of NaNs behind n_total: (pos_out, vel_out) (n_total + PAD, 4) float32, every word -7
    before the launch; ``rel`` (count, stride, 4); ``params``: an NbParams, None for the defaults"""
    import torch

    from nenbody_amd import _lib

    dev = torch.device("cuda", 0)
    tp, tv = records(pos, dev, PAD), records(vel, dev, PAD)
    op = torch.full((n_total + PAD, 4), -7.0, dtype=torch.float32, device=dev)
    ov = torch.full((n_total + PAD, 4), -7.0, dtype=torch.float32, device=dev)
    tc = torch.from_numpy(np.ascontiguousarray(cnt, np.uint32).view(np.int32)).to(dev)
    tr = torch.from_numpy(np.ascontiguousarray(rel, F)).to(dev)
    assert tc.numel() == count and tr.shape[0] == count and tr.shape[2] == 4      # the kernel reads this many records, no more
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        _lib.check(_lib.load().nb_nbody_located_step_launch(ctypes.byref(params) if params is not None else None, n_total, first, count,
                                                            tp.data_ptr(), tv.data_ptr(), tc.data_ptr(), tr.data_ptr(), rel.shape[1],
                                                            op.data_ptr(), ov.data_ptr(), s.cuda_stream))
    s.synchronize()
    return op.cpu().numpy(), ov.cpu().numpy()


def exact_differences(pos):
    n = len(pos)
    rel = np.zeros((n, n, 4), F)
    rel[:, :, :3] = pos[None, :, :] - pos[:, None, :]
    rel[:, :, 3] = np.nan                                  # the fourth word of a record is not read
    return rel


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_exact_difference_lists_are_the_oracles_nbody_step(nb, oracle, n):
    pos, vel = oracle.init_state(n, 1000 + n)
    rel = exact_differences(pos)
    for consts in (None, (0.05, 0.02, 1e-3)):
        params, okw = None, {}
        if consts is not None:
            params = nb.default_params()
            params.dt, params.G, params.bias = consts
            okw = dict(dt=consts[0], g=consts[1], bias=consts[2])
        want_p, want_v = oracle.step_range(pos, vel, 0, n, **okw)
        gp, gv = launch_fold(n, 0, n, pos, vel, np.full(n, n, np.uint32), rel, params)
        assert (bits(gp[:n, :3]) == bits(want_p)).all() and (bits(gv[:n, :3]) == bits(want_v)).all(), consts
        assert (gp[:n, 3] == 0).all() and (gv[:n, 3] == 0).all() and (gp[n:] == -7).all() and (gv[n:] == -7).all()


def test_the_stride_clamps_the_count_and_slots_behind_the_count_are_not_read(nb, oracle):
    n, stride = 70, 16
    pos, vel = oracle.init_state(n, 70)
    rng = np.random.default_rng(70)
    rel = np.zeros((n, stride, 4), F)
    rel[:, :, :3] = rng.normal(scale=20, size=(n, stride, 3)).astype(F)
    cnt = rng.integers(0, stride + 1, n).astype(np.uint32)
    cnt[:4] = [0, stride, stride + 5, 0xFFFFFFFF]                     # nobody, a full row, counts above the stride: the clamp
    behind = np.arange(stride)[None, :] >= cnt.astype(np.int64)[:, None]
    rel[behind] = np.nan                                              # a missing guard shows as a NaN, not as a fault
    want_p, want_v = L.nbody_located_step(pos, vel, cnt, rel)
    assert np.isfinite(want_v).all()
    gp, gv = launch_fold(n, 0, n, pos, vel, cnt, rel)
    assert (bits(gp[:n, :3]) == bits(want_p)).all() and (bits(gv[:n, :3]) == bits(want_v)).all()
    assert (bits(gv[0, :3]) == bits(vel[0])).all() and (bits(gp[0, :3]) == bits(vel[0] + pos[0])).all()      # nobody seen: the body coasts


@pytest.mark.parametrize("first,count", [(0, 1), (5, 10), (69, 1), (13, 57)])
def test_subsets_write_only_their_range(nb, oracle, first, count):
    n = 70
    pos, vel = oracle.init_state(n, 70)
    rel = exact_differences(pos)
    want_p, want_v = oracle.step_range(pos, vel[first:first + count], first, count)
    rows = slice(first, first + count)
    gp, gv = launch_fold(n, first, count, pos, vel, np.full(count, n, np.uint32), rel[rows])      # row e of the lists is body first + e
    assert (bits(gp[rows, :3]) == bits(want_p)).all() and (bits(gv[rows, :3]) == bits(want_v)).all()
    rest = np.ones(n + PAD, bool)
    rest[rows] = False
    assert (gp[rest] == -7).all() and (gv[rest] == -7).all()


# -- the step --------------------------------------------------------------------------------------------------------------------------------
def assert_step(sc, what, **kw):
    """one located gravity step of the Scene's current state against the restatement, the rows from Scene.eyes of that state"""
    import nenbody_amd as nb

    p0, v0 = sc.state()
    view = {k: v for k, v in kw.items() if k in ("width", "cp")}
    ids, depth = sc.eyes(**view)
    cp = view.get("cp")
    count, _, _, _, _, rel = L.located_of_rows(ids, depth, v0, UP, nb.eye_constant(view.get("width", 1024)) if cp is None else cp)
    want_p, want_v = L.nbody_located_step(p0, v0, count, rel, dt=sc.params.dt, g=sc.params.G, bias=sc.params.bias)
    sc.step_nbody_located(**kw)
    p1, v1 = sc.state()
    bad = (bits(p1) != bits(want_p)).any(1) | (bits(v1) != bits(want_v)).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {sc.n} bodies differ, first {np.nonzero(bad)[0][:8]}"
    assert (bits(sc.positions()) == bits(p1)).all()                  # the mirrors were refreshed
    return count, v0, v1


@pytest.mark.parametrize("n", [1, 2, 100, 257, 2048])
def test_one_step_every_bit(nb, oracle, n):
    pos, vel = oracle.init_state(n, 1000 + n if n != 2048 else 5)
    with nb.Scene(pos, vel) as sc:
        count, v0, v1 = assert_step(sc, f"N={n}")
        assert sc.steps_done == 1
    blind = count == 0
    assert (bits(v1[blind]) == bits(v0[blind])).all()                # the blind coast
    if n >= 100:
        assert blind.any() and (~blind).mean() > 0.5 and (bits(v1[~blind]) != bits(v0[~blind])).any(1).all()


def test_three_consecutive_steps_and_other_constants(nb, oracle):
    pos, vel = oracle.init_state(257, 1257)
    with nb.Scene(pos, vel) as sc:
        for k in range(3):
            assert_step(sc, f"step {k}")
    prm = nb.default_params()
    prm.dt, prm.G, prm.bias = 0.05, 0.02, 1e-3
    with nb.Scene(pos, vel, prm) as sc:
        assert_step(sc, "other constants", width=64)


def test_three_dimensional_data(nb, oracle):
    pos, vel, cp = three_dimensional(oracle)
    with nb.Scene(pos, vel) as sc:
        count, v0, v1 = assert_step(sc, "3-D", cp=cp)
    assert count.sum() > 100 and (v1[:, 2] != v0[:, 2]).any()


def test_every_batch_size_gives_the_same_bits(nb, oracle):
    pos, vel = oracle.init_state(257, 1257)
    got = []
    for batch in (0, 64, 257, 1000):
        with nb.Scene(pos, vel) as sc:
            if batch == 0:
                assert_step(sc, "batch 0")
            else:
                sc.step_nbody_located(batch=batch)
            got.append(sc.state())
    for p, v in got[1:]:
        assert (bits(p) == bits(got[0][0])).all() and (bits(v) == bits(got[0][1])).all()


def test_interleaved_with_the_other_steps(nb, oracle):
    pos, vel = oracle.init_state(100, 1100)
    with nb.Scene(pos, vel) as sc:
        assert_step(sc, "first")
        sc.step()
        assert_step(sc, "behind step")
        sc.step_boids()
        assert_step(sc, "behind step_boids")
        sc.step_boids_seen()
        assert_step(sc, "behind step_boids_seen")
        sc.step_n(2)
        assert sc.steps_done == 9
        p, v = sc.state()
        assert np.isfinite(p).all() and np.isfinite(v).all()


def test_hand_case(nb):
    """tests/test_located_cpu.py derives it: eye 0 sees body 1 at column 440, rel = (9 - 2 ulp, 0.98712, 0), eye 1 sees nobody and coasts"""
    pos = np.array([[0, 0, 0], [10, 0, 0]], F)
    vel = np.array([[1, 0, 0], [1, 0, 0]], F)
    with nb.Scene(pos, vel) as sc:
        count, ids, depth, cols, col, rel = sc.located()
        assert (count == [1, 0]).all() and ids[0, 0] == 1 and cols[0, 0] == 144 and col[0, 0] == 440
        assert (col[0, 1:] == NONE).all() and (col[1] == NONE).all()
        assert (bits(rel[0, 0]) == [0x410FFFFE, 0x3F7CB3AE, 0, 0x410FFFFE]).all() and (bits(rel[0, 1:]) == 0).all() and (bits(rel[1]) == 0).all()
        sc.step_nbody_located()
        p, v = sc.state()
    want_p, want_v = L.nbody_located_step(pos, vel, count, rel)
    assert (bits(p) == bits(want_p)).all() and (bits(v) == bits(want_v)).all()
    assert (bits(v[1]) == bits(F([1, 0, 0]))).all() and (bits(p[1]) == bits(F([11, 0, 0]))).all() and v[0, 0] > 1 and v[0, 1] > 0


def test_two_calls_give_identical_bits(nb, oracle):
    pos, vel = oracle.init_state(2048, 21)
    got = []
    for _ in range(2):
        with nb.Scene(pos, vel) as sc:
            sets = sc.located(count=300)
            sc.step_nbody_located_n(2)
            got.append((sets, sc.state()))
    (la, (pa, va)), (lb, (pb, vb)) = got
    assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(la, lb))
    assert (bits(pa) == bits(pb)).all() and (bits(va) == bits(vb)).all()
    ids, depth = crafted_rows(1000)
    dirs = directions(len(ids), 3)
    a, b = launch_located(ids, depth, dirs, nb.eye_constant(1000)), launch_located(ids, depth, dirs, nb.eye_constant(1000))
    assert all((x == y).all() for x, y in zip(a, b))
    rel = exact_differences(pos[:257])
    fa, fb = (launch_fold(257, 0, 257, pos[:257], vel[:257], np.full(257, 257, np.uint32), rel) for _ in range(2))
    assert (bits(fa[0]) == bits(fb[0])).all() and (bits(fa[1]) == bits(fb[1])).all()


# -- the C++ host ----------------------------------------------------------------------------------------------------------------------------
def test_cpp_located_host_matches_the_restatement(nb, oracle, tmp_path):
    import test_located_cpu as C

    C.build_exe()
    n, width = 100, 1024
    out = tmp_path / "out.bin"
    r = subprocess.run([C.EXE, str(n), str(width), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint32)
    cells = n * width
    cuts = np.cumsum([n, cells, cells, cells, cells, 4 * cells, 3 * n])
    count, ids, depth, cols, col, rel, p, v = np.split(raw, cuts)
    pos, vel = oracle.init_state(n, 1234)
    cp = R.eye_constant(oracle, width)
    rows = R.eyes(oracle.cameras(pos, vel, UP, cp), oracle.instances(pos, vel), 0, width)
    want = L.located_of_rows(rows[0], rows[1], vel, UP, cp)
    assert_located((count, ids.reshape(n, width), depth.reshape(n, width), col.reshape(n, width), rel.reshape(n, width, 4)), want, "C++ located")
    assert (cols.reshape(n, width) == want[3]).all()
    want_p, want_v = L.nbody_located_step(pos, vel, want[0], want[5])
    assert (p.reshape(n, 3) == bits(want_p)).all() and (v.reshape(n, 3) == bits(want_v)).all()
