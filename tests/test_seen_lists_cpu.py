"""CPU tests of the list-order restatement of the seen boids step (seen_restatement.boids_seen_step_lists) and of the inputs the GPU
contract tests (tests/test_gpu_seen_contract.py) rest on: the restatement against the mask form on ascending lists and against the C
oracle on full lists under every constant set of the battery, and, on the very arrays the GPU tests use, that each rule's test holds
for some seen pairs and fails for others, that some body is blind, and that list order and a duplicate change the result.  A GPU test
that could tell nothing fails here."""
import numpy as np
import pytest

import eyes_restatement as R
import seen_cases as K
import seen_restatement as S

F = np.float32
UP = np.array([0, 0, 1], F)
OTHER = dict(dt=0.1, r1=1500.0, r2=12.0, r3=2.0, s2=0.2)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("positions", "velocities")):
        ok, rows = K.same_words(g, w)
        assert ok, f"{what}: {name} of {len(rows)} bodies differ, first {rows[:8]}"


def changed(a, b):
    """the bodies with some velocity word different"""
    return (bits(a[1]) != bits(b[1])).any(1)


# -- (a) ascending, duplicate-free lists: the mask form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, OTHER], ids=["defaults", "other constants"])
def test_ascending_lists_are_the_mask_form(oracle, kw):
    n, stride = 300, 48
    pos, vel = K.cut_cloud(oracle, n, 9)
    base_count, base = K.order_lists(n, stride - 2, 3)
    count, lists = np.zeros(n, np.uint32), np.full((n, stride), S.NONE, np.uint32)
    for e in range(n):                                               # with an entry outside the set, and every third body itself
        u = np.unique(np.concatenate([base[e, :base_count[e]], [n], [e] if e % 3 == 0 else []]).astype(np.uint32))
        count[e], lists[e, :len(u)] = len(u), u
    assert (lists == np.arange(n, dtype=np.uint32)[:, None]).any(1).sum() >= n // 3 and (lists == n).any(1).all()
    want = S.boids_seen_step(pos, vel, S.mask_of_lists(count, lists, n), **kw)
    got = S.boids_seen_step_lists(pos, vel, count, lists, **kw)
    assert (bits(got[0]) == bits(want[0])).all() and (bits(got[1]) == bits(want[1])).all()
    first, rows = 37, 100                                            # row e belongs to body first + e
    sub = S.boids_seen_step_lists(pos, vel, count[first:first + rows], lists[first:first + rows], first=first, **kw)
    assert (bits(sub[0]) == bits(want[0][first:first + rows])).all() and (bits(sub[1]) == bits(want[1][first:first + rows])).all()


# -- (b) full lists: the C oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.FULL_LIST_CASES)
def test_full_lists_are_the_oracle_step(oracle, name):
    pos, vel, kw = K.full_list_case(oracle, name)
    n = len(pos)
    got = S.boids_seen_step_lists(pos, vel, *K.full_lists(n, n), **kw)
    assert_same(got, oracle.boids_run(pos, vel, 1, K.oracle_params(oracle, **kw)), name)


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_full_lists_ragged_sizes_and_a_range(oracle, n):
    pos, vel = K.cloud(oracle, n, seed=n)
    assert_same(S.boids_seen_step_lists(pos, vel, *K.full_lists(n, n)), oracle.boids_run(pos, vel, 1), f"n={n}")
    first, rows = n // 3, n - n // 3
    got = S.boids_seen_step_lists(pos, vel, *K.full_lists(rows, n), first=first)
    assert_same(got, oracle.boids_step_range(pos, vel, first, rows), f"n={n} range")


# -- (c) the partial-mask data: every rule cuts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_every_rule_cuts_on_the_partial_mask_data(oracle, density):
    pos, vel = K.cut_cloud(oracle, 800, 5)
    s1, s2, s3, pairs = K.predicate_shares(pos, vel, K.bernoulli_mask(800, density, 5), **K.CUT)
    print(f"density {density}: rule 1 holds for {s1:.1%}, rule 2 for {s2:.1%}, rule 3 for {s3:.1%} of {pairs} seen pairs")
    assert all(0.01 < s < 0.99 for s in (s1, s2, s3)), (s1, s2, s3)


# -- (d) the chained-step data -----------------------------------------------------------------------------------------------------------
def test_every_rule_cuts_on_the_chained_step_data_and_some_body_is_blind(oracle):
    pos, vel = K.chain_state(oracle, 300, 41)
    ids, _ = R.eyes(oracle.cameras(pos, vel, UP, R.eye_constant(oracle, 1024)), oracle.instances(pos, vel), 0, 1024)
    mask = S.mask_of_rows(ids, 300)
    s1, s2, s3, pairs = K.predicate_shares(pos, vel, mask, **K.CHAIN)
    blind = int((mask.sum(1) == 0).sum())
    print(f"rule 1 holds for {s1:.1%}, rule 2 for {s2:.1%}, rule 3 for {s3:.1%} of {pairs} seen pairs; {blind} blind bodies")
    assert all(0.10 < s < 0.90 for s in (s1, s2, s3)), (s1, s2, s3)
    assert blind >= 1
    # a blind body stops, a stopped body has no heading, and an eye without a heading sees nobody: blind bodies stay blind
    pos, vel = S.boids_seen_step(pos, vel, mask, **K.CHAIN)
    ids, _ = R.eyes(oracle.cameras(pos, vel, UP, R.eye_constant(oracle, 1024)), oracle.instances(pos, vel), 0, 1024)
    after = S.mask_of_rows(ids, 300).sum(1) == 0
    assert after[mask.sum(1) == 0].all() and (~after).sum() > 150


# -- (e) the order data: list order and duplicates are observable ------------------------------------------------------------------------
def test_list_order_and_duplicates_change_the_result(oracle):
    n, stride = 300, 48
    pos, vel = K.cut_cloud(oracle, n, 9)
    v = K.contract_variants(n, stride, 9)
    step = lambda name: S.boids_seen_step_lists(pos, vel, *v[name], **K.CUT)
    base = step("ascending")
    by_order, by_dup = int(changed(step("permuted"), base).sum()), int(changed(step("duplicate appended"), base).sum())
    print(f"permuting each list changes {by_order} of {n} bodies, appending a duplicate of slot 0 changes {by_dup}")
    assert by_order >= n // 4 and by_dup >= n // 4
    # the other variants are what they are meant to be
    assert (v["count above stride"][0] > stride).all() and (v["count above stride"][1] < n).all()
    assert (v["count zero"][1] < n).all() and (v["valid ids behind the count"][1] < n).all()
    cnt, mid = v["own index and padding in the middle"]
    inside = np.arange(stride)[None, :] < cnt[:, None]
    assert ((mid == np.arange(n, dtype=np.uint32)[:, None]) & inside).any(1).all() and ((mid >= n) & (mid < n + K.PAD) & inside).any(1).all()
    assert ((mid < n + K.PAD) | ~inside).all()                       # nothing points behind the padding records
    stopped = step("count zero")
    assert (bits(stopped[1]) == 0).all() and (bits(stopped[0]) == bits(pos)).all()
    # the clamp and the slots behind the count: folding 48 entries is not folding 47 or none, and ids behind the count would show
    assert changed(step("count above stride"), stopped).all()
    folded = S.boids_seen_step_lists(pos, vel, np.full(n, stride, np.uint32), v["valid ids behind the count"][1], **K.CUT)
    assert changed(folded, step("valid ids behind the count")).mean() > 0.5
    assert (bits(step("valid ids behind the count")[1]) == bits(base[1])).all()
    c1, l1 = K.stride_one_lists(n, 4)
    assert set(c1) == {0, 1, 5} and (l1[:, 0] == np.arange(n)).any() and (l1 >= n).any() and (l1 < n + K.PAD).all()
