"""The exchanges between PROCESSES, bit for bit on the exact lattice (tests/exact_lattice.py), two steps, every rank.

The ranks are processes sharing the one GPU, as in the other multi-rank tests: ShardedScene over gloo through the host and over pulls
of IPC-mapped buffers (nb_peers_*), NativeShard with the host's gather and ring functions and with pulls only.  Every rank checks
every one of its own bodies and its whole replica of the positions against the closed form.  The lattices are mostly PERMUTED
(`permute`): the first step carries every site onto another, so the second step's pair terms are not the first's, and a stale
record of either exchange -- received halves, sums, a slot of the replica, the own-slot planes a fused finish leaves -- moves its
bodies.  The sites are random (runs=0), so every chunk that travels mixes sites.

A control arm (nb_diag_peers_lossy 2: rank 0's second pull of each kind copies nothing) shows the permuted lattice flagging exactly
rank 0's bodies where the translated one passes them.  The last test holds verify_exchanges / choose_exchange to the paths a pattern
was seen to arrive through, with rank 0's in-place all-gather broken.
"""
import os
import socket
import sys

import numpy as np
import pytest

from exact_lattice import assert_exact, lattice, wrong_bodies

pytestmark = pytest.mark.gpu

SWAPS = {"tetra": (1, 2, 3, 0), "tetra_mixed": (2, 3, 0, 1), "planar": (1, 0), "line": (1, 0)}
SCENE_N = {2: {"ordered": 4097, "ring": 8192}, 3: {"ordered": 1000, "ring": 12288}, 4: {"ordered": 5001, "ring": 16384}}
SHARD_N = {2: {"ordered": 3001, "ring": 32768}, 3: {"ordered": 1000, "ring": 49152}, 4: {"ordered": 4099, "ring": 32768}}


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spec(n, i, permute=True):
    """lattice parameters (rebuilt in every rank and in the parent): kinds and scales taken in turn, random sites"""
    kind = ("tetra", "tetra_mixed", "planar", "line")[i % 4]
    scale = (1.0, 2.0 ** 29, 2.0 ** -20, 2.0 ** 31)[i % 4]
    return dict(n=n, seed=1000 + i, kind=kind, scale=scale, steps=2, permute=SWAPS[kind] if permute else None)


def _params(nb, lat):
    p = nb.default_params(mode=nb.NB_MODE_FAST)
    p.dt, p.G, p.bias = (float(c) for c in lat.consts)
    return p


def _init(rank, world, port):
    from conftest import ROOT

    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["NB_RING"] = "1"   # (sets this small keep the ordered fold by themselves)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    import nenbody_amd

    nenbody_amd.reload_env()
    return dist, nenbody_amd


def nb_partition(n, world):
    from nenbody_amd.dist import partition

    return partition(n, world)


def _save(out_dir, case, rank, **arrays):
    np.savez(os.path.join(out_dir, f"{case}_rank{rank}.npz"), **arrays)


def _check(out_dir, case, world, spec, lenient=()):
    """every rank's own bodies and replica against the closed form; the ranks in `lenient` are not held to it (nor are the others'
    replicas of their slots): returns {rank: its wrong own bodies} for them"""
    lat = lattice(**spec)
    wrong, theirs = {}, np.zeros(len(lat.pos), bool)
    for r in lenient:
        first, count = nb_partition(len(lat.pos), world)[r]
        theirs[first:first + count] = True
    for r in range(world):
        got = np.load(os.path.join(out_dir, f"{case}_rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        if r in lenient:
            wrong[r] = wrong_bodies(lat, got["pos"][first:first + count], got["vel"], first, count)
            continue
        bad = np.flatnonzero((got["pos"].view(np.uint32) != lat.p_exp.view(np.uint32)).any(axis=1) & ~theirs)
        assert len(bad) == 0, f"{case}, rank {r} of {world}: {len(bad)} positions of the replica differ, first {bad[:1]}"
        assert_exact(lat, got["pos"][first:first + count], got["vel"], f"{case}, rank {r} of {world}: own bodies", first, count)
    return wrong


# -- ShardedScene: gloo through the host, or pulls over IPC ---------------------------------------------------------------------
FORMS = {   # ShardedScene arguments and what the scene must report having taken
    "ordered": dict(overlap=False, ring=False),
    "overlap": dict(overlap=True, ring=False),
    "ring": dict(ring=True, ring_overlap=False),
    "ring_overlap": dict(ring=True, ring_overlap=True),
}


def _scene_worker(rank, world, port, out_dir, cases, exchange, lossy):
    dist, nenbody_amd = _init(rank, world, port)
    try:
        import torch

        torch.cuda.set_device(0)
        for case, spec, form in cases:
            lat = lattice(**spec)
            sc = nenbody_amd.ShardedScene(lat.pos, lat.vel, _params(nenbody_amd, lat), exchange=exchange, **FORMS[form])
            assert (sc.partners > 0) == form.startswith("ring") and sc.ring_overlap == (form == "ring_overlap")
            assert sc.overlap == (form == "overlap") and (sc.first, sc.count) == nenbody_amd.partition(lat.pos.shape[0], world)[rank]
            try:
                if exchange == "peers":
                    rep = sc.verify_exchanges()
                    assert rep["all_gather"] == "peers" and rep["ring_exchange"] == ("peers" if sc.partners else None), rep
                    assert sc.exchange == "peers"
                if lossy:   # from here on rank 0's second pull of each kind copies nothing: step 2's received halves are step 1's
                    nenbody_amd.load().nb_diag_peers_lossy(2)
                sc.step_n(lat.steps)
                sc.sync()
            finally:
                if lossy:
                    nenbody_amd.load().nb_diag_peers_lossy(0)
            _save(out_dir, case, rank, pos=sc.positions(), vel=sc.local_velocities(), first=sc.first, count=sc.count)
            dist.barrier()   # every rank's pulls from this scene's buffers are done before any rank frees them
            sc.close()
    finally:
        dist.destroy_process_group()


def _scene_cases(world, forms):
    out = []
    for i, form in enumerate(forms):
        n = SCENE_N[world]["ring" if form.startswith("ring") else "ordered"]
        out.append((form, _spec(n, world + i), form))
    return out


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_scene_over_gloo_every_form_bit_exact(tmp_path, world):
    """ordered fold, ordered fold with the exchange overlapped, the pairs form, the pairs form in phases (fused finish); the
    ordered forms on ragged ranks"""
    import torch.multiprocessing as mp

    cases = _scene_cases(world, list(FORMS))
    mp.spawn(_scene_worker, args=(world, _port(), str(tmp_path), cases, "collective", False), nprocs=world, join=True)
    for case, spec, _ in cases:
        _check(str(tmp_path), case, world, spec)


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_scene_over_pulls_every_form_bit_exact(tmp_path, world):
    """exchange="peers" after verify_exchanges(): the all-gather and the second exchange as pulls over IPC-mapped buffers"""
    import torch.multiprocessing as mp

    cases = _scene_cases(world, ["overlap", "ring", "ring_overlap"])
    mp.spawn(_scene_worker, args=(world, _port(), str(tmp_path), cases, "peers", False), nprocs=world, join=True)
    for case, spec, _ in cases:
        _check(str(tmp_path), case, world, spec)


def _control_arm(out_dir, world, cases):
    """rank 0's second pull of each kind lost (step 2's received halves are step 1's; its replica after step 2 is stale): on the
    permuted lattice exactly its own bodies fail, on the translated one they pass (the blind spot this file closes); every other
    rank's own bodies and replica are exact either way, but for rank 0's slot, which holds what rank 0 computed"""
    for case, spec, *_ in cases:
        wrong = _check(out_dir, case, world, spec, lenient=(0,))
        lat = lattice(**spec)
        mine = np.load(os.path.join(out_dir, f"{case}_rank0.npz"))
        first, count = 0, int(mine["count"])
        for r in range(1, world):
            slot0 = np.load(os.path.join(out_dir, f"{case}_rank{r}.npz"))["pos"][:count]
            assert (slot0.view(np.uint32) == mine["pos"][:count].view(np.uint32)).all(), f"{case}: rank {r}'s replica of rank 0's slot"
        if lat.permute is None:
            assert len(wrong[0]) == 0, f"{case}: the translated lattice was expected to pass a stale second exchange"
        else:
            assert wrong[0].tolist() == list(range(first, first + count)), f"{case}: {len(wrong[0])} of rank 0's {count} bodies flagged"


def test_control_arm_sharded_scene_lossy_pulls(tmp_path):
    import torch.multiprocessing as mp

    world, n = 4, SCENE_N[4]["ring"]
    cases = [("translated", _spec(n, 0, permute=False), "ring"), ("permuted", _spec(n, 0), "ring")]
    mp.spawn(_scene_worker, args=(world, _port(), str(tmp_path), cases, "peers", True), nprocs=world, join=True)
    _control_arm(str(tmp_path), world, cases)


# -- NativeShard: the host's gather and ring functions (gloo through the host), or pulls only --------------------------------------
def _shard_worker(rank, world, port, out_dir, cases):
    """case: (name, spec, second spec uploaded after the first two steps or None, options): options overlap, ring (the host's
    second exchange), peers ("only": pulls, no host exchange), verify ("pulls" / "choose"), lossy"""
    dist, nenbody_amd = _init(rank, world, port)
    try:
        import torch

        from test_gpu_native_shard import _hip_runtime

        nenbody_amd.load()   # brings the HIP runtime into the global symbol scope
        hip = _hip_runtime()

        def gather(buf, slot_bytes, rank_, world_, stream):
            assert (rank_, world_) == (rank, world) and hip.hipStreamSynchronize(stream) == 0
            mine = torch.empty(slot_bytes, dtype=torch.uint8)
            assert hip.hipMemcpy(mine.data_ptr(), buf + rank * slot_bytes, slot_bytes, 2) == 0
            full = torch.empty(world * slot_bytes, dtype=torch.uint8)
            dist.all_gather_into_tensor(full, mine)
            assert hip.hipMemcpy(buf, full.data_ptr(), world * slot_bytes, 1) == 0

        def ring(send, recv, chunk_bytes, partners, rank_, world_, stream):
            assert (rank_, world_) == (rank, world) and hip.hipStreamSynchronize(stream) == 0
            out = torch.empty(partners * chunk_bytes, dtype=torch.uint8)
            assert hip.hipMemcpy(out.data_ptr(), send, partners * chunk_bytes, 2) == 0
            got = torch.empty(partners * chunk_bytes, dtype=torch.uint8)
            ops = []
            for d in range(1, partners + 1):
                ops.append(dist.P2POp(dist.isend, out[(d - 1) * chunk_bytes:d * chunk_bytes], (rank + d) % world, tag=d))
                ops.append(dist.P2POp(dist.irecv, got[(d - 1) * chunk_bytes:d * chunk_bytes], (rank - d) % world, tag=d))
            for req in dist.batch_isend_irecv(ops):
                req.wait()
            assert hip.hipMemcpy(recv, got.data_ptr(), partners * chunk_bytes, 1) == 0

        def swap_blobs(blob):
            every = [None] * world
            dist.all_gather_object(every, blob)
            return b"".join(every)

        for case, spec, spec2, opt in cases:
            lat = lattice(**spec)
            pulls_only = opt.get("peers") == "only"
            with nenbody_amd.NativeShard(lat.pos, lat.vel, _params(nenbody_amd, lat), rank=rank, world=world,
                                         gather=None if pulls_only else gather, ring=ring if opt.get("ring") and not pulls_only else None,
                                         overlap=opt.get("overlap", False), peers=swap_blobs if opt.get("peers") else None) as sh:
                want_partners = 0 if not opt.get("ring") else sh.partners
                assert (sh.partners > 0) == bool(opt.get("ring")) and sh.pairs_overlapped == bool(opt.get("ring") and opt.get("overlap"))
                extra = {}
                try:
                    if opt.get("verify") == "pulls":
                        assert sh.verify_exchanges() == (2, 3 if sh.partners else -1)
                    elif opt.get("verify") == "choose":   # the timing steps leave recv, sums and the planes dirty; the state comes back
                        assert sh.verify_exchanges() == (0, 0)
                        chosen, ms = sh.choose_form(2)
                        assert chosen in (0, 1, 2) and ms[chosen] == min(x for x in ms if x > 0), (chosen, ms)
                        assert sh.partners == (0 if chosen == 0 else want_partners) and sh.pairs_overlapped == (chosen == 2)
                        extra["chosen"] = chosen
                    if opt.get("lossy"):
                        nenbody_amd.load().nb_diag_peers_lossy(2)
                    sh.step(lat.steps)
                    sh.sync()
                finally:
                    if opt.get("lossy"):
                        nenbody_amd.load().nb_diag_peers_lossy(0)
                _save(out_dir, case, rank, pos=sh.positions(), vel=sh.local_velocities(), first=sh.first, count=sh.count, **extra)
                if spec2 is not None:   # another lattice (other site counts) into the same shard: nothing of the first may survive
                    lat2 = lattice(**spec2)
                    assert all(a == b for a, b in zip(lat.consts, lat2.consts))
                    sh.upload(lat2.pos, lat2.vel)
                    sh.step(lat2.steps)
                    sh.sync()
                    _save(out_dir, case + "_upload", rank, pos=sh.positions(), vel=sh.local_velocities(), first=sh.first, count=sh.count)
                dist.barrier()   # every rank's pulls from this shard's buffers are done before any rank frees them
    finally:
        dist.destroy_process_group()


def _shard_cases(world, forms, i0=0, **common):
    out = []
    for i, (name, opt) in enumerate(forms):
        n = SHARD_N[world]["ring" if opt.get("ring") else "ordered"]
        spec = _spec(n, world + i0 + i)
        # the upload: other site counts (and another kind where one shares the constants -- the shard keeps its G, dt and bias)
        kind = {"tetra": "tetra_mixed", "tetra_mixed": "planar", "planar": "tetra", "line": "line"}[spec["kind"]]
        spec2 = dict(spec, seed=spec["seed"] + 1000, kind=kind, skew=(1, 6, 2, 1) if len(SWAPS[kind]) == 4 else (5, 1), permute=SWAPS[kind])
        assert all(a == b for a, b in zip(lattice(**spec).consts, lattice(**spec2).consts))
        out.append((name, spec, spec2, dict(opt, **common)))
    return out


SHARD_FORMS = [("ordered_overlap", dict(overlap=True)), ("pairs", dict(ring=True)), ("pairs_overlapped", dict(ring=True, overlap=True))]


@pytest.mark.parametrize("world", [2, 3, 4])
def test_native_shards_with_host_exchanges_bit_exact(tmp_path, world):
    """the ordered fold with the exchange overlapped (ragged ranks), the pairs form, the pairs form overlapped -- each on a lattice,
    then on another uploaded into the same shard; and verify_exchanges -> choose_form(2) -> two steps, whichever form is chosen"""
    import torch.multiprocessing as mp

    cases = _shard_cases(world, SHARD_FORMS)
    cases.append(("choose", _spec(SHARD_N[world]["ring"], 40 + world), None, dict(ring=True, verify="choose")))
    mp.spawn(_shard_worker, args=(world, _port(), str(tmp_path), cases), nprocs=world, join=True)
    for case, spec, spec2, _ in cases:
        _check(str(tmp_path), case, world, spec)
        if spec2 is not None:
            _check(str(tmp_path), case + "_upload", world, spec2)
    chosen = {int(np.load(os.path.join(str(tmp_path), f"choose_rank{r}.npz"))["chosen"]) for r in range(world)}
    assert len(chosen) == 1, "every rank takes the same form"


@pytest.mark.parametrize("world", [2, 4])
def test_native_shards_with_pulls_only_bit_exact(tmp_path, world):
    import torch.multiprocessing as mp

    cases = _shard_cases(world, SHARD_FORMS[1:], i0=10, peers="only", verify="pulls")
    mp.spawn(_shard_worker, args=(world, _port(), str(tmp_path), cases), nprocs=world, join=True)
    for case, spec, spec2, _ in cases:
        _check(str(tmp_path), case, world, spec)
        _check(str(tmp_path), case + "_upload", world, spec2)


def test_control_arm_native_shard_lossy_pulls(tmp_path):
    import torch.multiprocessing as mp

    world, n = 4, SHARD_N[4]["ring"]
    opt = dict(ring=True, peers="only", verify="pulls", lossy=True)
    cases = [("translated", _spec(n, 0, permute=False), None, opt), ("permuted", _spec(n, 0), None, opt)]
    mp.spawn(_shard_worker, args=(world, _port(), str(tmp_path), cases), nprocs=world, join=True)
    _control_arm(str(tmp_path), world, cases)


# -- verify_exchanges / choose_exchange with a broken in-place all-gather on rank 0 ------------------------------------------------
def _broken_gather_worker(rank, world, port, out_dir, spec, outcome):
    dist, nenbody_amd = _init(rank, world, port)
    try:
        import torch

        from nenbody_amd import dist as ndist

        torch.cuda.set_device(0)
        real = ndist.ShardedScene._all_gather_slots
        fired = []

        def broken(self, buf, async_op=False, slot=None):   # a broken RCCL in-place gather, stood in for on rank 0: one record spoiled
            out = real(self, buf, async_op=async_op, slot=slot)
            if self.exchange == "collective" and self.gather_in_place and slot is None:
                other = (self.rank + 1) % self.world
                buf[other * self.slot, 0] += 1.0
                fired.append(1)
            return out

        if rank == 0:
            ndist.ShardedScene._all_gather_slots = broken
        lat = lattice(**spec)
        sc = nenbody_amd.ShardedScene(lat.pos, lat.vel, _params(nenbody_amd, lat), ring=True)
        verified = sc.verify_exchanges()
        assert verified["all_gather"] == "out_of_place" and verified["ring_exchange"] == "grouped" and not sc.gather_in_place, verified
        assert len(fired) == (1 if rank == 0 else 0)

        class Clock:   # choose_exchange's timing, made to prefer `outcome`: the other kind's timed steps take a second each
            t = 0.0

            @staticmethod
            def perf_counter():
                Clock.t += 1.0 if sc.exchange != outcome else 1e-3
                return Clock.t

        real_time, ndist.time = ndist.time, Clock
        try:
            chosen = sc.choose_exchange(steps=1, warm=1)
        finally:
            ndist.time = real_time
        assert chosen == outcome == sc.exchange and set(sc.exchange_times) == {"peers", "collective"}, (chosen, sc.exchange_times)
        assert not sc.gather_in_place and sc.ring_grouped and len(fired) == (1 if rank == 0 else 0), "the collective ran on an unverified path"
        rep = sc.exchange_report
        assert verified["collective"] == {"all_gather": "out_of_place", "ring_exchange": "grouped"}, verified
        assert rep["verified"] and rep["collective"] == {"all_gather": "out_of_place", "ring_exchange": "grouped"}, rep
        assert (rep["all_gather"], rep["ring_exchange"]) == (("peers", "peers") if outcome == "peers" else ("out_of_place", "grouped")), rep
        sc.step_n(lat.steps)   # the corruption is still armed
        sc.sync()
        assert len(fired) == (1 if rank == 0 else 0)
        _save(out_dir, outcome, rank, pos=sc.positions(), vel=sc.local_velocities(), first=sc.first, count=sc.count)
        dist.barrier()
        sc.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("outcome", ["collective", "peers"])
def test_choose_exchange_keeps_the_verified_collective_paths(tmp_path, outcome):
    """verify_exchanges finds rank 0's in-place all-gather broken and takes the gather from a copy; choose_exchange must then verify
    the pulls WITHOUT moving the collective back in place, time the collective on its verified paths, and report the paths of the
    exchange it keeps.  Each outcome forced once through the clock.  Two permuted-lattice steps follow, the corruption still armed."""
    import torch.multiprocessing as mp

    world, spec = 2, _spec(SCENE_N[2]["ring"], 50)
    mp.spawn(_broken_gather_worker, args=(world, _port(), str(tmp_path), spec, outcome), nprocs=world, join=True)
    _check(str(tmp_path), outcome, world, spec)
