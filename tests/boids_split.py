"""Helpers for the tests of the boids split form (nb_launch_boids_step_split; test infrastructure): one step through it on the GPU,
and the tolerance criteria it is held to off the exact lattice (tests/boids_lattice.py holds it to every bit on the lattice)."""
import numpy as np


def split_step(nb, pos, vel, parts, bp=None, info=None):
    """one boids step of the set, every (first, count) of `parts` through the split form on the one GPU.  With a list `info`, one
    dict per part is appended: the scratch size the library asked for and the step's flag word, read from the end of the scratch
    (nb_api.hip:boids_split_pointers: [slice rows | per-1024-record velocity sums | flag word, 64 bytes])"""
    import torch

    from nenbody_amd.dist import HipBackend

    be, dev, n = HipBackend(), torch.device("cuda", 0), len(pos)
    bp = bp if bp is not None else nb.default_boids_params()

    def rec(a):
        t = torch.zeros((n, 4), dtype=torch.float32)
        t[:, :3] = torch.from_numpy(a)
        return t.to(dev)

    pin, vin = rec(pos), rec(vel)
    pout, vout = torch.full_like(pin, float("nan")), torch.full_like(vin, float("nan"))
    scratches = []
    for first, count in parts:
        nbytes = be.boids_split_scratch_bytes(bp, n, count)
        scratch = torch.empty((max(16, nbytes),), dtype=torch.uint8, device=dev)
        be.boids_step_split(bp, n, first, count, pin, vin, pout, vout, scratch)
        scratches.append((first, count, nbytes, scratch))
    torch.cuda.synchronize()
    if info is not None:
        for first, count, nbytes, scratch in scratches:
            word = int(scratch[nbytes - 64:nbytes - 60].cpu().numpy().view(np.uint32)[0])
            info.append(dict(first=first, count=count, scratch_bytes=nbytes, flags=word))
    return pout[:, :3].cpu().numpy(), vout[:, :3].cpu().numpy()


def boids_velocity_f64(pos, vel, i, bp):
    """the new velocity of body i (main.rs:471-518) with the reference's binary32 PREDICATES -- the same neighbour sets -- and every
    sum, mean and blend carried in binary64: the yardstick for the rounding error of a binary32 sum, the reference's included"""
    f = np.float32
    d = pos - pos[i]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    other = np.arange(len(pos)) != i
    with np.errstate(invalid="ignore"):
        p1 = (d2 < f(bp.rule_1_distance)) & other
        p2 = (np.sqrt(d2) < f(bp.rule_2_distance)) & other
        e = vel - vel[i]
        e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        p3 = (np.sqrt(e2) < f(bp.rule_3_distance)) & other
    c = pos[p1].astype(np.float64).sum(axis=0)
    r = -(d[p2].astype(np.float64)).sum(axis=0)
    m = vel[p3].astype(np.float64).sum(axis=0)
    if p1.sum():
        c = c / p1.sum()
    if p3.sum():
        m = m / p3.sum()
    v = c * float(f(bp.rule_1_scale)) + r * float(f(bp.rule_2_scale)) + m * float(f(bp.rule_3_scale))
    mag = np.sqrt((v * v).sum())
    return v / mag if mag > 1.0 else v


def close_to_the_reference(v, v_ref, p, p_ref, what="", state=None):
    """The split form against the bit-exact step.  Its neighbour sets and counts are the reference's; its sums are binary32 sums in
    another order, and a sequential binary32 sum of m terms carries ~sqrt(m) half-ulps of its own (6.9e-6 of a unit velocity on
    20 000 bodies in a 40 x 40 square), so "close" means: every body within 5e-5 of the largest velocity component, and -- with
    `state` = (pos, vel, bp) -- on the 48 bodies where the two differ most, plus 16 evenly spaced ones, the split form is NO FURTHER
    from the same sums carried in binary64 than the reference's own arithmetic is: worst body against worst body (plus four
    ulps of the result) and on average (body by body the two errors are independent: either may be the larger)."""
    sv = float(np.abs(v_ref).max())
    dv = np.abs(v - v_ref).max(axis=1)
    assert dv.max() <= 5e-5 * sv, f"{what}: max |dv| {dv.max():.3e} against {5e-5 * sv:.3e}"
    assert np.abs(p - p_ref).max() <= 5e-5 * sv + float(np.spacing(np.float32(np.abs(p_ref).max()))), what
    if state is None:
        return
    pos, vel, bp = state
    chosen = np.unique(np.concatenate([np.argsort(dv)[-48:], np.linspace(0, len(v) - 1, 16).astype(np.int64)]))
    ulp = float(np.spacing(np.float32(sv)))
    v64 = np.array([boids_velocity_f64(pos, vel, int(i), bp) for i in chosen])
    err_split, err_ref = np.abs(v[chosen] - v64).max(axis=1), np.abs(v_ref[chosen] - v64).max(axis=1)
    # the worst body against the reference's worst, and body by body with the slack of two independent roundings of a mean
    assert err_split.max() <= err_ref.max() + 4 * ulp, f"{what}: split {err_split.max():.3e} from the binary64 sums, the reference {err_ref.max():.3e}"
    assert err_split.mean() <= 1.5 * err_ref.mean() + ulp, f"{what}: mean error split {err_split.mean():.3e}, the reference {err_ref.mean():.3e}"


def headline_sample(parts):
    """the bodies test_boids_split_form_at_the_headline_size checks: the first, last, middle and one-third body of every share"""
    return np.unique(np.concatenate([[f, f + c - 1, f + c // 2, f + c // 3] for f, c in parts]))


def assert_sampled_close(p, v, pos, vel, idx, refs, bp):
    """the sampled criterion of the headline test: on bodies `idx`, with refs[k] = the oracle's (p, v) of body idx[k], within 5e-5 of
    the largest sampled velocity (positions 1e-5), and no further from the binary64 sums than the reference plus 2e-6 of it"""
    sv = max(float(np.abs(r[1]).max()) for r in refs)
    for i, (p_ref, v_ref) in zip(idx, refs):
        assert np.abs(v[i] - v_ref[0]).max() <= 5e-5 * sv and np.abs(p[i] - p_ref[0]).max() <= 1e-5, f"body {i}"
        v64 = boids_velocity_f64(pos, vel, int(i), bp)
        assert np.abs(v[i] - v64).max() <= np.abs(v_ref[0] - v64).max() + 2e-6 * sv, f"body {i}: further from the binary64 sums than the reference"
