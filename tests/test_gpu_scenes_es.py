"""GPU tests of the scene batches' evolution-strategies generation: the three kernels of nb_scenes_es.inc
against the numpy restatement (tests/es_restatement.py), every word of the population, of the ranks, the fitnesses, the report and the
new mean (E1-E8).  A fitness that the restatement gives as a NaN is met by a NaN; every other comparison is of bit patterns, and two
runs of the device are compared byte for byte, NaNs included.

The cases are tests/es_cases.py's, and their expected values are computed once there; tests/test_scenes_es_cpu.py holds their
premises.  The context's loop is held to the chained restatements of the policy step, the score and the generation."""
import ctypes

import numpy as np
import pytest

import es_cases as K
import es_restatement as E
import policy_cases as PK
import policy_restatement as P
import score_restatement as Q
from nenbody_amd._lib import ES_PROTOTYPES   # noqa: F401  (the parent commit has no such table: the file fails here)

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0x07070707
PAD = 16                                                     # guard words on either side of every output


def ep_of(sigma, step, coef, seed):
    from nenbody_amd import _lib

    return _lib.NbEsParams(float(sigma), float(step), (ctypes.c_float * 6)(*[float(c) for c in coef]), int(seed))


class Guarded:
    """a device buffer of `words` 32-bit words between two runs of guard words"""

    def __init__(self, words, dev, init=None):
        import torch

        host = np.full(words + 2 * PAD, GUARD, np.uint32)
        if init is not None:
            host[PAD:PAD + words] = np.ascontiguousarray(init).view(np.uint32).reshape(-1)
        self.words, self.t = words, torch.from_numpy(host.view(np.int32)).to(dev)
        self.ptr = self.t.data_ptr() + 4 * PAD

    def read(self, dtype=np.uint32):
        out = self.t.cpu().numpy().view(np.uint32)
        assert (out[:PAD] == GUARD).all() and (out[PAD + self.words:] == GUARD).all(), "a guard word was written"
        return out[PAD:PAD + self.words].view(dtype).copy()


def perturb(case, ranges=None, mean=None):
    """nb_scenes_es_perturb_launch for a population case, by the scene ranges `ranges` ((first, count) relative to the case's own range,
    one launch each, in the order given; default: one launch): float32 (B, M)"""
    import torch

    from nenbody_amd import _lib

    lib, dev = _lib.load(), torch.device("cuda", 0)
    f, h, b, g, seed, sigma, first = case
    m = K.floats(f, h)
    mean = K.mean_of(m) if mean is None else mean
    t_mean, out = Guarded(m, dev, mean), Guarded(b * m, dev)
    stream = torch.cuda.Stream(dev)
    ep = ep_of(sigma, K.STEP, K.COEF_GOAL, seed)
    with torch.cuda.stream(stream):
        for lo, cnt in ranges or [(0, b)]:
            _lib.check(lib.nb_scenes_es_perturb_launch(ctypes.byref(ep), f, h, g, first + lo, cnt, t_mean.ptr, out.ptr + 4 * lo * m, stream.cuda_stream))
    stream.synchronize()
    assert t_mean.read(F).tobytes() == mean.tobytes()
    return out.read(F).reshape(b, m)


def update(case, in_place=False, step=K.STEP, optional=True):
    """nb_scenes_es_update_launch for an update case: (ranks, fitnesses or None, report or None, mean')"""
    import torch

    from nenbody_amd import _lib

    lib, dev = _lib.load(), torch.device("cuda", 0)
    f, h, b, kind = case
    m = K.floats(f, h)
    rec, coef = K.records(b, kind)
    mean = K.mean_of(m)
    t_rec, t_mean = Guarded(8 * b, dev, rec.view(np.uint32)), Guarded(m, dev, mean)
    t_new = t_mean if in_place else Guarded(m, dev)
    t_rank, t_fit, t_rep = Guarded(b, dev), Guarded(b, dev), Guarded(4, dev)
    stream = torch.cuda.Stream(dev)
    ep = ep_of(K.SIGMA, step, coef, K.SEED)
    score_ptr = t_rec.ptr
    assert score_ptr % 8 == 0                                                            # (an allocation is 256-byte aligned, the pad is 64 bytes)
    with torch.cuda.stream(stream):
        _lib.check(lib.nb_scenes_es_update_launch(ctypes.byref(ep), f, h, K.update_generation(case), b, score_ptr, t_mean.ptr, t_new.ptr, t_rank.ptr,
                                                  t_fit.ptr if optional else None, t_rep.ptr if optional else None, stream.cuda_stream))
    stream.synchronize()
    if not in_place:
        assert t_mean.read(F).tobytes() == mean.tobytes()
    t_rec.read()
    fit, rep = t_fit.read(F), t_rep.read()
    if not optional:
        assert (fit.view(np.uint32) == GUARD).all() and (rep == GUARD).all()
    return t_rank.read(), fit if optional else None, rep.view(E.REPORT_DTYPE)[0] if optional else None, t_new.read(F)


def assert_update(got, want, what):
    r, phi, rep, mean = got
    assert (r == want[0]).all(), (what, "ranks", np.argwhere(r != want[0])[:4].tolist())
    if phi is not None:
        assert E.same_floats(phi, want[1]), (what, "fitnesses")
        assert E.same_report(rep, want[2]), (what, "report", rep, want[2])
    assert mean.tobytes() == want[3].tobytes(), (what, "mean", np.argwhere(mean.view(np.uint32) != want[3].view(np.uint32))[:4].tolist())


# -- perturb ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted({c[:2] for c in K.population_cases()}))
def test_every_word_of_every_population(nb, shape):
    for case in K.population_cases():
        if case[:2] != shape:
            continue
        got, want = perturb(case), K.population(case)
        assert got.tobytes() == want.tobytes(), (case, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())


def test_a_scene_does_not_know_the_population_or_the_split(nb):
    """E8: scenes 0 .. 4 of 256 are the five of B = 5; a range that begins at an odd scene; the ranges of a split, in any order"""
    whole = perturb((8, 7, 256, 1, K.SEED, K.SIGMA, 0))
    assert whole[:5].tobytes() == perturb((8, 7, 5, 1, K.SEED, K.SIGMA, 0)).tobytes()
    assert whole[3:67].tobytes() == perturb((8, 7, 64, 1, K.SEED, K.SIGMA, 3)).tobytes()
    assert whole[255:].tobytes() == perturb((8, 7, 1, 1, K.SEED, K.SIGMA, 255)).tobytes()
    split = perturb((8, 7, 256, 1, K.SEED, K.SIGMA, 0), ranges=[(40, 25), (0, 7), (65, 191), (7, 33)])
    assert split.tobytes() == whole.tobytes()
    again = perturb((8, 7, 256, 1, K.SEED, K.SIGMA, 0))
    assert again.tobytes() == whole.tobytes()                                            # the same bytes from run to run
    zero = perturb((8, 7, 65, 1, K.SEED, F(0), 0))
    assert (zero == K.mean_of(79)[None]).all()
    tiny = perturb((8, 7, 64, 1, K.SEED, K.SUBNORMAL, 0), mean=np.zeros(79, F))
    assert tiny.tobytes() == E.population(np.zeros(79, F), K.SUBNORMAL, K.SEED, 1, 0, 64).tobytes() and (tiny != 0).any()   # subnormals are kept


# -- update ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", sorted({c[2] for c in K.update_cases()}))
def test_every_word_of_every_update_in_place_and_out_of_place(nb, b):
    for case in K.update_cases():
        if case[2] != b:
            continue
        want = K.update(case)
        assert_update(update(case), want, (case, "out of place"))
        assert_update(update(case, in_place=True), want, (case, "in place"))


def test_step_zero_the_optional_outputs_and_two_runs(nb):
    for case in ((8, 7, 65, "random"), (8, 7, 256, "ties"), (8, 7, 65, "special")):
        got = update(case, step=F(0))
        assert_update(got, K.update(case, step=F(0)), (case, "step 0"))
        assert got[3].tobytes() == K.mean_of(79).tobytes()
    for case in ((64, 32, 256, "random"), (8, 7, K.LIMIT_B, "special"), (8, 7, 65, "near")):
        a, b = update(case), update(case)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), case               # byte for byte, NaNs included
        bare = update(case, optional=False, in_place=True)
        assert bare[0].tobytes() == a[0].tobytes() and bare[3].tobytes() == a[3].tobytes()


def test_the_edges_of_near_and_the_specials(nb):
    """what the cases hold, read back from the device: near = 2^24 + 1, 2^60 + 2^36 + 1 and 2^64 - 1 converted once; a NaN and both
    infinities ranked; -0 and +0 tied"""
    r, phi, rep, _ = update((8, 7, 65, "near"))
    assert phi[64] == F(2.0 ** 24) and phi[63] == F(2.0 ** 60 + 2.0 ** 37) and phi[62] == F(2.0 ** 64) and rep["nan_count"] == 0
    assert r[62] == 64 and rep["best_scene"] == 62 and rep["best_fitness"] == F(2.0 ** 64)
    r, phi, rep, _ = update((8, 7, 65, "special"))
    assert np.isnan(phi[[1, 11]]).all() and rep["nan_count"] == 2 and r[1] == 0 and r[11] == 1
    assert phi[3] == -np.inf and r[3] == 2 and phi[5] == np.inf and r[5] == 64 and rep["best_scene"] == 5
    assert phi[7].view(np.uint32) == 0 and phi[9].view(np.uint32) == 0 and r[9] == r[7] + 1
    r, phi, rep, _ = update((8, 7, 256, "equal"))
    assert (r == np.arange(256)).all() and rep["best_scene"] == 255


# -- the context -----------------------------------------------------------------------------------------------------------------------------
def scene_rows(nb, pos, vel, width):
    out = []
    for s in range(len(pos)):
        with nb.Scene(pos[s], vel[s]) as sc:
            ids, depth = sc.eyes(width=width)
            out.append((ids.copy(), depth.copy()))
    return out


@pytest.mark.parametrize("b", [4, 5])
def test_three_generations_of_the_five_call_loop(nb, oracle, b):
    """rewind; score_reset; es_perturb; step_policy_scored(k); es_update, three times, against policy_restatement, score_restatement
    and es_restatement chained; a set_policy between two generations is overwritten; rewind restores the kept bytes and the step
    counter, also behind an upload"""
    n, width, features, hidden, k = 5, 64, 8, 7, 2
    pos, vel = PK.batch(oracle, (1100, n, width, 0.05, b))
    mean = PK.policies(features, hidden, 1)[0]
    sigma, step, seed, limit = F(0.05), F(1e-3), K.SEED_HIGH, PK.LIMIT
    coef = K.COEF_MIX
    radius_sq, goal = F(np.median(Q.pair_d2(pos[0])[np.triu_indices(n, 1)])), F([0.01, 0.02, 0.0])
    with nb.SceneBatch(pos, vel) as sb:
        sb.set_score(radius_sq, goal)
        sb.es_set(mean, features, hidden, sigma, step, coef, seed, limit)
        sb.step(1)
        sb.keep()
        kept_p, kept_v = sb.positions(), sb.velocities()
        assert sb.steps_done == 1 and sb.es_generation == 0 and sb.es_mean().tobytes() == mean.tobytes()
        for g in range(3):
            sb.rewind()
            sb.score_reset()
            sb.es_perturb()
            sb.step_policy_scored(k, width)
            sb.es_update()
            theta = E.population(mean, sigma, seed, g, 0, b)
            p, v, acc = kept_p, kept_v, None
            for _ in range(k):
                rows = scene_rows(nb, p, v, width)
                _, _, p, v = P.batch(lambda s, ps, vs: rows[s], p, v, theta, features, hidden, limit, PK.UP)
                acc = Q.batch(p, v, radius_sq, goal, acc=acc)
            assert Q.same(sb.scores(), acc), g
            want = E.rank_and_update(mean, sigma, step, coef, seed, g, acc)
            rep, phi, r = sb.es_result()
            assert_update((r, phi, rep, sb.es_mean()), want, (b, "generation", g))
            assert rep.dtype == nb.ES_REPORT_DTYPE and rep["generation"] == g and sb.es_generation == g + 1 and sb.steps_done == 1 + k
            assert (want[3] != mean).any()
            mean = want[3]
            assert P.same(sb.positions(), p) and P.same(sb.velocities(), v)
            if g == 0:
                sb.set_policy(PK.policies(features, hidden, 1, seed=9), features, hidden, 0.25)   # overwritten by the next es_perturb
        sb.rewind()
        assert sb.steps_done == 1 and sb.positions().tobytes() == kept_p.tobytes() and sb.velocities().tobytes() == kept_v.tobytes()
        from nenbody_amd import _lib
        _lib.check(sb._lib.nb_scenes_upload(sb._ctx, pos.ctypes.data, vel.ctypes.data))
        assert sb.steps_done == 0 and sb.positions().tobytes() == pos.tobytes()
        sb.rewind()                                                                      # an upload does not drop the kept state
        assert sb.steps_done == 1 and sb.positions().tobytes() == kept_p.tobytes() and sb.velocities().tobytes() == kept_v.tobytes()


def test_context_entries_refuse_with_their_texts(nb, oracle):
    from nenbody_amd import _lib

    lib = _lib.load()
    err = lambda ctx: lib.nb_scenes_last_error(ctx).decode()
    Es, Ep, Eu, Em, Er, Ke, Rw = ("nb_scenes_es_set: ", "nb_scenes_es_perturb: ", "nb_scenes_es_update: ", "nb_scenes_es_mean: ", "nb_scenes_es_result: ",
                                  "nb_scenes_keep: ", "nb_scenes_rewind: ")
    unset, no_score = "no search set (call nb_scenes_es_set first)", "no score set (call nb_scenes_set_score first)"
    mean = np.zeros(79, F)
    out = np.zeros(79, F)
    good = ep_of(0.1, 0.01, K.COEF_GOAL, 1)
    ctx = ctypes.c_void_p()
    _lib.check(lib.nb_scenes_create(3, 8, None, ctypes.byref(ctx)))
    try:
        assert lib.nb_scenes_keep(ctx) == _lib.NB_ERR_STATE and err(ctx) == Ke + "no state uploaded (call nb_scenes_upload first)"
        assert lib.nb_scenes_rewind(ctx) == _lib.NB_ERR_STATE and err(ctx) == Rw + "no state kept (call nb_scenes_keep first)"
        assert lib.nb_scenes_es_perturb(ctx) == _lib.NB_ERR_STATE and err(ctx) == Ep + unset
        assert lib.nb_scenes_es_update(ctx) == _lib.NB_ERR_STATE and err(ctx) == Eu + unset
        assert lib.nb_scenes_es_mean(ctx, out.ctypes.data) == _lib.NB_ERR_STATE and err(ctx) == Em + unset
        assert lib.nb_scenes_es_mean(ctx, None) == _lib.NB_ERR_INVALID and err(ctx) == Em + "null argument"
        assert lib.nb_scenes_es_result(ctx, None, None, None) == _lib.NB_ERR_STATE and err(ctx) == Er + unset
        assert lib.nb_scenes_es_generation(ctx) == 0
        assert lib.nb_scenes_es_set(ctx, 8, 7, None, 1.0, ctypes.byref(good)) == _lib.NB_ERR_INVALID and err(ctx) == Es + "null argument"
        assert lib.nb_scenes_es_set(ctx, 8, 7, mean.ctypes.data, 1.0, None) == _lib.NB_ERR_INVALID and err(ctx) == Es + "null argument"
        for f, h, limit, text in ((0, 7, 1.0, "features must be 1 .. NB_POLICY_MAX_FEATURES (256)"), (8, 65, 1.0, "hidden must be 1 .. NB_POLICY_MAX_HIDDEN (64)"),
                                  (8, 7, -1.0, "accel_limit must be at least 0 (+inf: no limit)"), (8, 7, float("nan"), "accel_limit must be at least 0 (+inf: no limit)")):
            assert lib.nb_scenes_es_set(ctx, f, h, mean.ctypes.data, limit, ctypes.byref(good)) == _lib.NB_ERR_INVALID and err(ctx) == Es + text
        for bad, text in ((ep_of(-1.0, 0.01, K.COEF_GOAL, 1), "sigma must be at least 0 and finite"), (ep_of(float("inf"), 0.01, K.COEF_GOAL, 1), "sigma must be at least 0 and finite"),
                          (ep_of(float("nan"), 0.01, K.COEF_GOAL, 1), "sigma must be at least 0 and finite"), (ep_of(0.1, float("inf"), K.COEF_GOAL, 1), "step must be finite"),
                          (ep_of(0.1, 0.01, (0, 0, float("nan"), 0, 0, 0), 1), "coef must be finite"), (ep_of(-1.0, float("nan"), K.COEF_GOAL, 1), "sigma must be at least 0 and finite")):
            assert lib.nb_scenes_es_set(ctx, 8, 7, mean.ctypes.data, 1.0, ctypes.byref(bad)) == _lib.NB_ERR_INVALID and err(ctx) == Es + text
        assert lib.nb_scenes_es_perturb(ctx) == _lib.NB_ERR_STATE and err(ctx) == Ep + unset                         # a refused search is none
        assert lib.nb_scenes_es_set(ctx, 8, 7, mean.ctypes.data, float("inf"), ctypes.byref(good)) == _lib.NB_OK       # a search before an upload
        assert lib.nb_scenes_es_perturb(ctx) == _lib.NB_OK
        assert lib.nb_scenes_es_update(ctx) == _lib.NB_ERR_STATE and err(ctx) == Eu + no_score
        assert lib.nb_scenes_es_result(ctx, None, None, None) == _lib.NB_ERR_STATE and err(ctx) == Er + "no generation updated (call nb_scenes_es_update first)"
        assert lib.nb_scenes_es_mean(ctx, out.ctypes.data) == _lib.NB_OK and out.tobytes() == mean.tobytes()
        assert lib.nb_scenes_es_generation(ctx) == 0
    finally:
        lib.nb_scenes_destroy(ctx)
    big = ctypes.c_void_p()
    _lib.check(lib.nb_scenes_create(4097, 1, None, ctypes.byref(big)))
    try:
        assert lib.nb_scenes_es_set(big, 8, 7, mean.ctypes.data, 1.0, ctypes.byref(good)) == _lib.NB_ERR_INVALID
        assert err(big) == Es + "a search takes a batch of at most NB_ES_MAX_POPULATION (4096) scenes"
    finally:
        lib.nb_scenes_destroy(big)
    pos, vel = PK.batch(oracle, (1100, 8, 64, 0.1, 3))
    with nb.SceneBatch(pos, vel) as sb:
        with pytest.raises(ValueError):
            sb.es_set(np.zeros(78, F), 8, 7, 0.1, 0.01, K.COEF_GOAL)
        with pytest.raises(ValueError):
            sb.es_set(mean, 8, 7, 0.1, 0.01, (0, 0, 0))
        with pytest.raises(nb.NbError, match="sigma must be at least 0 and finite"):
            sb.es_set(mean, 8, 7, -0.1, 0.01, K.COEF_GOAL)
        with pytest.raises(nb.NbError, match="no state kept"):
            sb.rewind()
        sb.set_policy(PK.policies(8, 7, 3), 8, 7, 0.5)
        sb.es_set(mean, 8, 7, 0.0, 0.01, K.COEF_GOAL)                                    # sigma 0: every scene gets the mean
        with pytest.raises(nb.NbError, match="no policy set"):                           # es_set leaves no policy set until es_perturb
            sb.step_policy(1, 64)
        sb.es_perturb()
        sb.set_score(1.0)
        sb.step_policy_scored(1, 64)
        sb.es_update()
        rep, phi, r = sb.es_result()
        assert sb.es_generation == 1 and rep["generation"] == 0 and sorted(r.tolist()) == [0, 1, 2]
