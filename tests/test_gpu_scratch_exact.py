"""Every form that lays planes into the caller's scratch, given EXACTLY the bytes its nb_*scratch_bytes* entry names: the API's
documented contract.  The scratch is the middle of one tensor, `need` bytes between two guards of 4096 bytes, all of it filled
with 0xA5 -- a write past either end lands in memory the test owns and shows.  One step a run.  STRICT outputs are held to the
oracle bit for bit (a planar and a 3-D state each); FAST outputs to the same call given a scratch twice the size (these forms are
deterministic, which their own tests assert).  Shapes: the smallest at which the plan picks the form, or the knob may name it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xA5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def state(oracle, n, seed, three_d):
    pos, vel = oracle.init_state(n, seed)
    if three_d:
        rng = np.random.default_rng(seed)
        pos[:, 2] = rng.uniform(-100, 100, n).astype(np.float32)
        vel[:, 2] = rng.uniform(0, 0.1, n).astype(np.float32)
    return pos, vel


class Scratch:
    """`need` bytes between two guards (exact), or a plain tensor of twice the size (the comparison run)"""

    def __init__(self, torch, dev, need, exact):
        self.need, self.exact = need, exact
        if exact:
            self.whole = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device=dev)
            self.mid = self.whole[GUARD:GUARD + need]
            assert self.mid.data_ptr() == self.whole.data_ptr() + GUARD and self.mid.numel() == need
        else:
            self.whole = self.mid = torch.full((2 * need,), FILL, dtype=torch.uint8, device=dev)

    def assert_guards_untouched(self):
        if self.exact:
            lo, hi = self.whole[:GUARD].cpu().numpy(), self.whole[GUARD + self.need:].cpu().numpy()
            assert (lo == FILL).all(), f"{int((lo != FILL).sum())} bytes in front of the scratch were written"
            assert (hi == FILL).all(), f"{int((hi != FILL).sum())} bytes behind the scratch were written (first at +{int(np.argmax(hi != FILL))})"


def records(torch, dev, xyz):
    rec = torch.zeros((len(xyz), 4), dtype=torch.float32)
    rec[:, :3] = torch.from_numpy(np.ascontiguousarray(xyz))
    return rec.to(dev)


def one_step(nb, params, pos, vel, first, count, exact, phases=None):
    """one step of bodies [first, first + count) through nb_launch_step (phases = (j_lo, j_hi): nb_launch_step_phase, both phases) on
    a scratch of exactly the bytes asked for, or of twice as many; (positions, velocities) of the range"""
    import torch

    from nenbody_amd.dist import HipBackend

    be, dev, n = HipBackend(), torch.device("cuda", 0), len(pos)
    need = be.scratch_bytes_phased(params, n, count, *phases) if phases else be.scratch_bytes(params, n, count)
    assert need > 0
    sc = Scratch(torch, dev, need, exact)
    cur, nxt, v = records(torch, dev, pos), torch.zeros((n, 4), device=dev), records(torch, dev, vel[first:first + count])
    if phases:
        for phase in (nb._lib.NB_PHASE_RANGE, nb._lib.NB_PHASE_REST):
            be.step_phase(params, n, first, count, phases[0], phases[1], phase, cur, nxt, v, sc.mid)
    else:
        be.step(params, n, first, count, cur, nxt, v, sc.mid)
    nb._lib.check(be.lib.nb_launch_status(torch.cuda.current_stream(dev).cuda_stream))   # waits; a block chain that gave up would raise
    sc.assert_guards_untouched()
    return nxt[first:first + count, :3].cpu().numpy(), v[:, :3].cpu().numpy()


@pytest.mark.parametrize("three_d", [False, True], ids=["planar", "3d"])
@pytest.mark.parametrize("form", ["bc", "sl"])
def test_strict_forms_on_exactly_their_scratch(nb, oracle, monkeypatch, form, three_d):
    n = 1536   # the smallest set the plan gives the block chain; the scalar-load form by its knob
    if form == "sl":
        monkeypatch.setenv("NB_STRICT_BC", "0")
        monkeypatch.setenv("NB_STRICT_SL", "1")
    params = nb.default_params()
    assert nb._lib.planned_kernels(params, n, n)[0] == {"bc": "step_strict_bc_kernel", "sl": "step_strict_sl_kernel"}[form]
    pos, vel = state(oracle, n, 1536 + three_d, three_d)
    p, v = one_step(nb, params, pos, vel, 0, n, exact=True)
    p_ref, v_ref = oracle.run(pos, vel, 1)
    assert (bits(p) == bits(p_ref)).all() and (bits(v) == bits(v_ref)).all()


@pytest.mark.parametrize("form,n,first,count,phases,env,kernels", [
    ("fast-sl", 4096, 0, 4096, None, {}, ["step_fast_sl_kernel", "planes_kernel", "integrate_partials_kernel"]),
    ("fast-sl-slices", 4096, 1024, 1024, None, {}, ["step_fast_sl_kernel", "planes_kernel", "integrate_partials_kernel"]),
    ("fast-sl-phases", 4096, 1024, 1024, (1024, 2048), {}, None),
    ("pairs", 512, 0, 512, None, {"NB_FAST_PAIRS": "1"}, None),
], ids=["fast-sl", "fast-sl-slices", "fast-sl-phases", "pairs"])
def test_fast_forms_on_exactly_their_scratch(nb, oracle, monkeypatch, form, n, first, count, phases, env, kernels):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    params = nb.default_params(mode=nb.NB_MODE_FAST)
    planned = nb._lib.planned_kernels(params, n, count)
    if kernels:
        assert planned == kernels
    if form == "pairs":
        assert planned[0] == "step_fast_pairs_kernel"
    pos, vel = state(oracle, n, 4096 + n, True)
    p, v = one_step(nb, params, pos, vel, first, count, exact=True, phases=phases)
    p2, v2 = one_step(nb, params, pos, vel, first, count, exact=False, phases=phases)
    assert np.isfinite(p).all() and np.isfinite(v).all() and (v != vel[first:first + count]).any()
    assert (bits(p) == bits(p2)).all() and (bits(v) == bits(v2)).all()


def ring_rank(nb, params, pos, vel, world, rank, phases, exact):
    """rank `rank`'s launches of one step of the pairs form on shards, on a scratch of exactly nb_ring_scratch_bytes() (or twice that):
    the fold in one launch, or its three phases and the fused finish (what it received: zeros).  Every record the launches write."""
    import torch

    from nenbody_amd.dist import HipBackend

    be, dev, n, L = HipBackend(), torch.device("cuda", 0), len(pos), nb._lib
    S = n // world
    a = (params, n, rank * S, S)
    D = be.ring_partners(*a)
    assert D >= 1
    sc = Scratch(torch, dev, be.ring_scratch_bytes(*a), exact)
    cur, sums = records(torch, dev, pos), torch.full(((D + 1) * S, 4), float("nan"), device=dev)
    out = []
    if phases:
        assert be.ring_phased(*a)
        for phase in (L.NB_RING_OWN, L.NB_RING_REST, L.NB_RING_SUMS):
            be.ring_fold_phase(*a, phase, cur, sums, sc.mid)
        nxt, v, recv = torch.zeros((n, 4), device=dev), records(torch, dev, vel[rank * S:(rank + 1) * S]), torch.zeros((D * S, 4), device=dev)
        be.ring_finish_phase(*a, cur, nxt, v, sums, recv, sc.mid)
        out += [nxt, v]
    else:
        be.ring_fold(*a, cur, sums, sc.mid)
    torch.cuda.synchronize()
    sc.assert_guards_untouched()
    return [t.cpu().numpy() for t in [sums] + out]


@pytest.mark.parametrize("phases", [False, True], ids=["fold", "phases"])
def test_ring_forms_on_exactly_their_scratch(nb, oracle, monkeypatch, phases):
    n, world, rank = 2048, 2, 1   # the first rows of test_gpu_ring.py's tables
    monkeypatch.setenv("NB_RING", "1")
    monkeypatch.setenv("NB_RING_NP", "4")
    params = nb.default_params(mode=nb.NB_MODE_FAST)
    pos, vel = state(oracle, n, 2048, True)
    got = ring_rank(nb, params, pos, vel, world, rank, phases, exact=True)
    ref = ring_rank(nb, params, pos, vel, world, rank, phases, exact=False)
    assert np.isfinite(got[0]).all(), "a record of `sums` was not written"
    for g, r in zip(got, ref):
        assert (bits(g) == bits(r)).all()
