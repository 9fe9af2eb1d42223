"""GPU tests of the sharded host inside the library (nb_shard_*, include/nenbody.h): index ranges,
one exchange per step, STRICT bits independent of the world size.  RCCL itself needs one GPU per rank, so on this
one-GPU box it runs with a world of one; worlds of 2 and 3 run as processes sharing the GPU with a host-supplied
exchange (gloo through the host), which drives every line of the stepping logic that RCCL would."""
import ctypes
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def matrices_equal(got, ref):
    """model matrices (main.rs:437-439) word for word: since round 4 the device computes the angle, its sine and cosine as the host's
    libm does (nenbody_amd/csrc/nb_libm.h); NaN entries (non-finite velocities) compare equal whatever their payload"""
    g, r = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    return g.shape == r.shape and bool(((g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r))).all())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what=""):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, f"{what}: shape {g.shape} vs {r.shape}"
    assert (g == r).all(), f"{what}: {(g != r).sum()} of {g.size} words differ, first at {np.argwhere(g != r)[0]}"


def state3d(oracle, n, seed):
    pos, vel = oracle.init_state(n, seed)
    rng = np.random.default_rng(seed)
    pos[:, 2] = rng.uniform(-100, 100, n).astype(np.float32)
    vel[:, 2] = rng.uniform(0, 0.1, n).astype(np.float32)
    return (pos * np.float32(0.3)).astype(np.float32), vel


def reference(oracle, pos, vel, schedule):
    for what, k in schedule:
        pos, vel = oracle.run(pos, vel, k) if what == "nbody" else oracle.boids_run(pos, vel, k)
    return pos, vel


SCHEDULE = (("nbody", 2), ("boids", 2), ("nbody", 1), ("boids", 1))


def drive(sh, schedule, after_each=None):
    """schedule: (what, k) or (what, k, boids constants as a dict); after_each(sh) is called after every entry"""
    import nenbody_amd

    for what, k, *consts in schedule:
        if what == "nbody":
            sh.step(k)
        else:
            bp = None
            if consts:
                bp = nenbody_amd.default_boids_params()
                for name, value in consts[0].items():
                    setattr(bp, name, value)
            sh.step_boids(k, bp)
        if after_each is not None:
            sh.sync()
            after_each(sh)
    sh.sync()


@pytest.mark.parametrize("n", [1, 700, 2049])
def test_world_of_one_needs_no_exchange(nb, oracle, n):
    pos, vel = state3d(oracle, n, seed=n)
    with nb.NativeShard(pos, vel) as sh:
        assert (sh.first, sh.count) == (0, n)
        drive(sh, SCHEDULE)
        p, v, inst = sh.positions(), sh.local_velocities(), sh.local_instances()
    p_ref, v_ref = reference(oracle, pos, vel, SCHEDULE)
    assert_bits_equal(p, p_ref, "positions")
    assert_bits_equal(v, v_ref, "velocities")
    assert matrices_equal(inst, oracle.instances(p_ref, v_ref))


def test_rccl_world_of_one(nb, oracle):
    """ncclGetUniqueId -> ncclCommInitRank -> ncclAllGather in place between the kernels, on the library's stream."""
    n = 1500
    pos, vel = state3d(oracle, n, seed=3)
    cid = nb.comm_id()
    assert len(cid) == 128 and any(cid)
    with nb.NativeShard(pos, vel, rank=0, world=1, comm_id=cid) as sh:
        drive(sh, SCHEDULE)
        p, v = sh.positions(), sh.local_velocities()
    p_ref, v_ref = reference(oracle, pos, vel, SCHEDULE)
    assert_bits_equal(p, p_ref, "positions")
    assert_bits_equal(v, v_ref, "velocities")


def test_a_world_above_one_refuses_to_step_without_an_exchange(nb, oracle):
    from nenbody_amd import _lib

    pos, vel = state3d(oracle, 100, seed=4)
    with nb.NativeShard(pos, vel, rank=1, world=2) as sh:
        assert (sh.first, sh.count) == (50, 50)
        with pytest.raises(nb.NbError) as ei:
            sh.step()
        assert ei.value.status == _lib.NB_ERR_STATE and "nb_shard_use_rccl" in str(ei.value)


def test_failing_host_exchange_fails_the_step(nb, oracle):
    from nenbody_amd import _lib

    def broken(buf, slot_bytes, rank, world, stream):
        raise RuntimeError("link down")

    pos, vel = state3d(oracle, 64, seed=5)
    with nb.NativeShard(pos, vel, rank=0, world=2, gather=broken) as sh:
        with pytest.raises(nb.NbError) as ei:
            sh.step()
        assert ei.value.status == _lib.NB_ERR_STATE


def test_upload_after_overlapped_steps_waits_for_the_exchange_in_flight(nb, oracle):
    """with nb_shard_set_overlap on, nb_shard_step returns while the all-gather of the new positions is
    still running on the second stream; after an even number of steps it writes into pos[0], the buffer nb_shard_upload packs
    the new state into.  Here the host-supplied exchange is asynchronous and SLOW (a long fill ahead of the copy that lands
    the other rank's slot, all on the stream the library hands over) and lands poison: an upload that does not join the
    exchange is overwritten by it."""
    import torch

    n, world = 4096, 2
    pos, vel = state3d(oracle, n, seed=11)
    pos2, vel2 = state3d(oracle, n, seed=12)
    ballast = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    hip = _hip_runtime()
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemsetAsync.restype = ctypes.c_int
    landed = []

    def slow_async_gather(buf, slot_bytes, rank, world_, stream):
        for _ in range(8):      # a few milliseconds of work ahead of the landing copy, on the exchange's stream
            assert hip.hipMemsetAsync(ballast.data_ptr(), 0, ballast.numel(), stream) == 0
        other = buf + (1 - rank) * slot_bytes
        assert hip.hipMemsetAsync(other, 0xFF, slot_bytes, stream) == 0   # all-ones words: NaN records
        landed.append(slot_bytes)

    with nb.NativeShard(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST), rank=0, world=world, gather=slow_async_gather,
                        overlap=True) as sh:
        sh.step(2)              # even: the exchange in flight targets pos[0]
        sh.upload(pos2, vel2)
        got = sh.positions()
        got_v = sh.local_velocities()
    assert len(landed) == 2
    assert_bits_equal(got, pos2, "the re-uploaded replica (the old exchange must not land on it)")
    assert_bits_equal(got_v, vel2[:sh.count], "the re-uploaded velocities")


# -- worlds of 2 and 3 as processes on the one GPU, exchange = gloo through the host ------------------------------------
def _hip_runtime():
    """The HIP runtime already in the process (nenbody_amd preloads it globally), for raw memcpy on device pointers."""
    hip = ctypes.CDLL(None)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamSynchronize.restype = ctypes.c_int
    return hip


def _rank_worker(rank, world, port, n, mode, out_dir, overlap=False, schedule=None, with_ring=False, seed=None, force_pairs=False,
                 verify=None, peers=False, boids_split=False, state=None, nbody=None):
    """one rank of a world on the one GPU; state = (pos, vel) replaces the generated one, nbody = {dt, G, bias} the n-body
    constants, boids_split=True the boids step's split form; with `state`, the positions and local velocities after every schedule
    entry are saved as pos_<k>, vel_<k>"""
    import sys

    from conftest import ROOT

    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import nenbody_amd
        import oracle

        nenbody_amd.load()   # brings the HIP runtime into the global symbol scope
        if force_pairs:   # below the library's own line (2^30 ordered pairs per rank and step) the pairs form is a test knob
            os.environ["NB_RING"] = "1"
            nenbody_amd.reload_env()
        hip = _hip_runtime()
        calls = []

        def gather(buf, slot_bytes, rank_, world_, stream):
            assert (rank_, world_) == (rank, world)
            assert hip.hipStreamSynchronize(stream) == 0          # this rank's slot is ready
            mine = torch.empty(slot_bytes, dtype=torch.uint8)
            assert hip.hipMemcpy(mine.data_ptr(), buf + rank * slot_bytes, slot_bytes, 2) == 0   # device -> host
            full = torch.empty(world * slot_bytes, dtype=torch.uint8)
            dist.all_gather_into_tensor(full, mine)
            assert hip.hipMemcpy(buf, full.data_ptr(), world * slot_bytes, 1) == 0               # host -> device
            calls.append(slot_bytes)

        ring_calls = []

        def ring(send, recv, chunk_bytes, partners, rank_, world_, stream):
            """the pairs form's second exchange through the host: chunk d - 1 of `send` to rank + d, of `recv` from rank - d"""
            assert (rank_, world_) == (rank, world)
            assert hip.hipStreamSynchronize(stream) == 0
            out = torch.empty(partners * chunk_bytes, dtype=torch.uint8)
            assert hip.hipMemcpy(out.data_ptr(), send, partners * chunk_bytes, 2) == 0
            got = torch.empty(partners * chunk_bytes, dtype=torch.uint8)
            ops = []
            for d in range(1, partners + 1):
                ops.append(dist.P2POp(dist.isend, out[(d - 1) * chunk_bytes:d * chunk_bytes], (rank + d) % world, tag=d))
                ops.append(dist.P2POp(dist.irecv, got[(d - 1) * chunk_bytes:d * chunk_bytes], (rank - d) % world, tag=d))
            for req in dist.batch_isend_irecv(ops):
                req.wait()
            if verify == "lossy_ring" and rank == 0:   # a second exchange that loses data on one rank: every rank must drop the pairs form
                got[:16] = 0
            assert hip.hipMemcpy(recv, got.data_ptr(), partners * chunk_bytes, 1) == 0
            ring_calls.append(partners)

        def swap_blobs(blob):   # the handles of every rank's buffers, through the host's own channel (here: gloo)
            every = [None] * world
            dist.all_gather_object(every, blob)
            return b"".join(every)

        pos, vel = state if state is not None else state3d(oracle, n, seed=n) if seed is None else oracle.init_state(n, seed)
        params = nenbody_amd.default_params(mode=mode)
        for name, value in (nbody or {}).items():
            setattr(params, name, value)
        with nenbody_amd.NativeShard(pos, vel, params, rank=rank, world=world,
                                     gather=None if peers == "only" else gather, overlap=overlap, ring=ring if (with_ring and peers != "only") else None,
                                     peers=swap_blobs if peers else None, boids_split=boids_split) as sh:
            extra = {}
            if verify in ("lossy_pulls", "stale_pulls"):   # pulls that lose a record on rank 0 / that deliver the first time only (the second
                # pattern round catches those): every rank goes back to the host's exchanges, in both
                nenbody_amd.load().nb_diag_peers_lossy(1 if verify == "lossy_pulls" else 2)
                try:
                    assert sh.verify_exchanges() == (0, 0 if sh.partners else -1)
                finally:
                    nenbody_amd.load().nb_diag_peers_lossy(0)
            elif verify == "verify_only":   # the pattern through whatever exchange the shard uses; the form stays the one asked for
                assert sh.verify_exchanges() == ((2, 3 if sh.partners else -1) if peers else (0, 0 if sh.partners else -1))
                assert sh.pairs_overlapped == bool(overlap and sh.partners)
            elif verify:   # both exchanges on a known pattern first, then the machine is asked which form to take
                before = sh.partners
                paths = sh.verify_exchanges()
                assert paths == ((0, 2) if verify == "lossy_ring" else (0, 0 if before else -1)), paths
                assert sh.partners == (0 if verify == "lossy_ring" else before)
                sh.step(1)   # (a state that is not the upload's: choose_form must put THIS one back)
                p0, v0 = sh.positions(), sh.local_velocities()
                chosen, ms = sh.choose_form(2)
                assert (sh.positions().view(np.uint32) == p0.view(np.uint32)).all() and (sh.local_velocities().view(np.uint32) == v0.view(np.uint32)).all()
                if before and verify != "lossy_ring":
                    assert chosen in (0, 1, 2) and ms[0] > 0 and ms[1] > 0 and ms[2] > 0 and ms[chosen] == min(ms), (chosen, ms)
                    assert sh.partners == (0 if chosen == 0 else before) and sh.pairs_overlapped == (chosen == 2)
                else:
                    assert chosen == 0 and sh.partners == 0
                extra = dict(chosen=chosen, ms=np.array(ms))
                calls.clear(), ring_calls.clear()
            partners, overlapped = sh.partners, sh.pairs_overlapped
            every = []
            drive(sh, schedule or SCHEDULE, (lambda sh_: every.append((sh_.positions(), sh_.local_velocities()))) if state is not None else None)
            for k, (p_k, v_k) in enumerate(every):
                extra[f"pos_{k}"], extra[f"vel_{k}"] = p_k, v_k
            np.savez(os.path.join(out_dir, f"rank{rank}.npz"), pos=sh.positions(), vel=sh.local_velocities(),
                     inst=sh.local_instances(), first=sh.first, count=sh.count, calls=len(calls), ring_calls=len(ring_calls),
                     partners=partners, overlapped=overlapped, **extra)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 3000), (3, 1000), (3, 2)])
def test_worlds_of_two_and_three_equal_the_oracle(tmp_path, nb, oracle, world, n):
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_worker, args=(world, port, n, nb.NB_MODE_STRICT, str(tmp_path)), nprocs=world, join=True)
    pos, vel = state3d(oracle, n, seed=n)
    p_ref, v_ref = reference(oracle, pos, vel, SCHEDULE)
    inst_ref = oracle.instances(p_ref, v_ref)
    covered = 0
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        assert (first, count) == nb.partition(n, world)[r]
        assert_bits_equal(got["pos"], p_ref, f"rank {r} positions (replica)")
        assert_bits_equal(got["vel"], v_ref[first:first + count], f"rank {r} velocities")
        assert matrices_equal(got["inst"], inst_ref[first:first + count])
        # n-body: one exchange per step; boids: ONE per step too (positions and velocities travel in one staging buffer),
        # + one rebuild of the velocity replica each time boids follows n-body steps
        assert int(got["calls"]) == 3 + (1 + 2) + (1 + 1)
        covered += count
    assert covered == n


@pytest.mark.parametrize("world,n", [(2, 3000), (3, 1000), (3, 2), (2, 40000)])
def test_fast_shards_with_overlapped_exchange(tmp_path, nb, oracle, world, n):
    """nb_shard_set_overlap (FAST): each step folds the rank's own slot while the exchange of the others is in flight on a
    second stream, then the rest.  n-body steps only (the boids predicates are discontinuous: a FAST rounding difference may
    flip one); within FAST's tolerance of the oracle on every rank, the exchange called once per step as before."""
    schedule = (("nbody", 3), ("nbody", 2))
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_worker, args=(world, port, n, nb.NB_MODE_FAST, str(tmp_path), True, schedule), nprocs=world, join=True)
    pos, vel = state3d(oracle, n, seed=n)
    p_ref, v_ref = reference(oracle, pos, vel, schedule)
    covered = 0
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        assert (first, count) == nb.partition(n, world)[r]
        assert np.abs(got["pos"] - p_ref).max() <= 1e-4, f"rank {r} positions (replica)"
        assert count == 0 or np.abs(got["vel"] - v_ref[first:first + count]).max() <= 1e-5, f"rank {r} velocities"
        assert int(got["calls"]) == 5
        covered += count
    assert covered == n


@pytest.mark.parametrize("world,n,partners", [(2, 32768, 1), (3, 49152, 2), (4, 32768, 2)])
def test_fast_shards_in_the_pairs_form_with_a_second_exchange(tmp_path, nb, oracle, world, n, partners):
    """FAST with equal ranks of whole blocks: every unordered pair once (nb_nbody_ring.inc), the other ranks' halves leaving in
    a second exchange -- here both exchanges are the host's (gloo), the ranks are processes sharing the GPU.  Two exchanges per
    step, results within FAST's tolerance of the oracle on every rank; without a second exchange function the same shard keeps
    the ordered fold and its one exchange."""
    schedule = (("nbody", 2), ("nbody", 1))
    import torch.multiprocessing as mp

    # (the last arm: the pairs form with nb_shard_set_overlap -- round 5: the step in phases, both exchanges handed the second
    # stream, pairs inside the rank's own slot while the all-gather lands; and the scratch the ordered fold's phases would need must
    # not replace the larger one the ring needs)
    for with_ring, overlap in ((True, False), (False, False), (True, True)):
        out = tmp_path / (("ring" if with_ring else "ordered") + ("-overlap" if overlap else ""))
        out.mkdir()
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        mp.spawn(_rank_worker, args=(world, port, n, nb.NB_MODE_FAST, str(out), overlap, schedule, with_ring, 77, True), nprocs=world, join=True)
        pos, vel = oracle.init_state(n, 77)
        p_ref, v_ref = reference(oracle, pos, vel, schedule)
        for r in range(world):
            got = np.load(os.path.join(str(out), f"rank{r}.npz"))
            first, count = int(got["first"]), int(got["count"])
            assert (first, count) == nb.partition(n, world)[r]
            assert int(got["partners"]) == (partners if with_ring else 0)
            assert bool(got["overlapped"]) == (with_ring and overlap)
            assert int(got["calls"]) == 3 and int(got["ring_calls"]) == (3 if with_ring else 0)
            # three steps of tens of thousands of bodies: a few pairs come within the softening length, where any rounding
            # difference is amplified -- the bulk at FAST's per-step tolerance, the worst body bounded
            scale = float(np.abs(v_ref - vel).max())
            dv = np.abs(got["vel"] - v_ref[first:first + count]).max(axis=1)
            assert np.quantile(dv, 0.999) <= 1e-4 * scale and dv.max() <= 1e-2 * scale, f"rank {r} velocities: {np.quantile(dv, 0.999) / scale:.2e} {dv.max() / scale:.2e}"
            dp = np.abs(got["pos"] - p_ref).max(axis=1)
            assert np.quantile(dp, 0.999) <= 2e-4 * scale and dp.max() <= 2e-2 * scale, f"rank {r} positions (replica)"


@pytest.mark.parametrize("world,n,verify", [(2, 32768, "ok"), (4, 32768, "ok"), (3, 49152, "lossy_ring")])
def test_native_shard_verifies_its_exchanges_and_asks_the_machine_for_the_form(tmp_path, nb, oracle, world, n, verify):
    """nb_shard_verify_exchanges + nb_shard_choose_form (the native shard had no way to find out whether the pairs form
    pays -- or works -- between real GPUs): both exchanges move a known pattern and every rank checks what arrived, the ranks agreeing
    on the verdict through the host's gather; then every form the shard can take is timed on the state in hand (slowest rank), the
    fastest kept, the state put back bit for bit.  With a second exchange that loses data on one rank, every rank drops the pairs form
    for the ordered fold.  The steps that follow are the oracle's to FAST's tolerance either way."""
    import torch.multiprocessing as mp

    schedule = (("nbody", 2),)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_worker, args=(world, port, n, nb.NB_MODE_FAST, str(tmp_path), False, schedule, True, 77, True, verify), nprocs=world, join=True)
    pos, vel = oracle.init_state(n, 77)
    p_ref, v_ref = reference(oracle, pos, vel, (("nbody", 3),))     # (one step before the choice, two after)
    chosen = set()
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        chosen.add(int(got["chosen"]))
        scale = float(np.abs(v_ref - vel).max())
        dv = np.abs(got["vel"] - v_ref[first:first + count]).max(axis=1)
        assert np.quantile(dv, 0.999) <= 1e-4 * scale and dv.max() <= 1e-2 * scale, f"rank {r} velocities"
        assert int(got["ring_calls"]) == (2 if int(got["partners"]) else 0)
    assert len(chosen) == 1     # every rank took the same form


@pytest.mark.parametrize("world,n,mode_name,overlap", [(2, 3000, "strict", False), (3, 1001, "strict", False), (4, 32768, "fast", False),
                                                       (4, 32768, "fast", True), (2, 32768, "fast", True), (3, 49152, "fast", True)])
def test_shards_that_pull_their_exchanges_over_ipc(tmp_path, nb, oracle, world, n, mode_name, overlap):
    """nb_shard_peer_export / _import (round 5): NO collective library and no host exchange function -- every rank maps the others'
    position replicas and `sums` through IPC memory handles (swapped here over gloo), and an exchange is a signal in the rank's own
    memory, stream waits on the peers' flag words and one copy kernel on the shard's own stream.  The ranks are PROCESSES sharing the
    one GPU: the protocol (who waits for whom, which buffer is pulled when, that nothing is overwritten under a peer's pull) is what
    is tested; that a peer's stores are visible when its flag says so is a property of two GPUs, which verify_exchanges checks where
    it first meets them.  STRICT: ragged worlds, bit-identical to the oracle; FAST: the pairs form, its second exchange pulled too --
    in sequence and in phases (the signal behind the finish, the pull behind the next step's own-slot pairs) -- at FAST's tolerance."""
    import torch.multiprocessing as mp

    strict = mode_name == "strict"
    schedule = (("nbody", 3), ("nbody", 2))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_worker, args=(world, port, n, nb.NB_MODE_STRICT if strict else nb.NB_MODE_FAST, str(tmp_path), overlap, schedule, not strict, 77,
                                 not strict, "verify_only", "only"), nprocs=world, join=True)
    pos, vel = oracle.init_state(n, 77)
    p_ref, v_ref = reference(oracle, pos, vel, schedule)
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        assert (first, count) == nb.partition(n, world)[r]
        assert int(got["calls"]) == 0 and int(got["ring_calls"]) == 0          # no host exchange ran
        if strict:
            assert_bits_equal(got["pos"], p_ref, f"rank {r} positions (replica)")
            assert_bits_equal(got["vel"], v_ref[first:first + count], f"rank {r} velocities")
        else:
            scale = float(np.abs(v_ref - vel).max())
            dv = np.abs(got["vel"] - v_ref[first:first + count]).max(axis=1)
            assert np.quantile(dv, 0.999) <= 2e-4 * scale and dv.max() <= 2e-2 * scale, f"rank {r}: {np.quantile(dv, 0.999) / scale:.2e} {dv.max() / scale:.2e}"
            dp = np.abs(got["pos"] - p_ref).max(axis=1)
            assert np.quantile(dp, 0.999) <= 4e-4 * scale and dp.max() <= 4e-2 * scale, f"rank {r} positions (replica)"


@pytest.mark.parametrize("fault", ["lossy_pulls", "stale_pulls"])
def test_pulls_that_lose_data_send_both_exchanges_back_to_the_hosts(tmp_path, nb, oracle, fault):
    """nb_shard_verify_exchanges on a shard that pulls its exchanges over IPC, with rank 0's pulls made lossy (nb_diag_peers_lossy 1: the
    first record of what it pulls is overwritten -- what stores that are not visible when their flag says so would look like; 2: only
    the first pull of each kind copies anything -- a reader served from a cache; the second pattern round is there for it): every
    rank must see the verdict and go back to the exchanges chosen before (here the host's gather and ring functions), and the steps
    that follow run through those and are right."""
    import torch.multiprocessing as mp

    world, n, schedule = 4, 32768, (("nbody", 3),)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_worker, args=(world, port, n, nb.NB_MODE_FAST, str(tmp_path), False, schedule, True, 77, True, fault, True), nprocs=world, join=True)
    pos, vel = oracle.init_state(n, 77)
    p_ref, v_ref = reference(oracle, pos, vel, schedule)
    scale = float(np.abs(v_ref - vel).max())
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        first, count = int(got["first"]), int(got["count"])
        assert int(got["partners"]) == 2 and int(got["ring_calls"]) >= 3 and int(got["calls"]) >= 3      # the host's exchanges carried the steps
        dv = np.abs(got["vel"] - v_ref[first:first + count]).max(axis=1)
        assert np.quantile(dv, 0.999) <= 1e-4 * scale and dv.max() <= 1e-2 * scale, f"rank {r}"


def test_native_shard_boids_split_form(nb, oracle):
    """nb_shard_set_boids_split: the boids step of the native shard with its j range in slices (the reference's neighbour sets and
    counts, reassociated sums; rule 3 from the total of the velocities where it holds for every pair) -- close to the bit-exact
    step, identical from run to run, and mixing with n-body steps keeps working (the velocity replica is rebuilt)"""
    n = 6000
    pos, vel = oracle.init_state(n, 5)
    pos *= np.float32(0.3)
    outs = []
    for _ in range(2):
        with nb.NativeShard(pos, vel, boids_split=True) as sh:
            sh.step_boids(2)
            sh.step(1)
            sh.step_boids(1)
            sh.sync()
            outs.append((sh.positions(), sh.local_velocities()))
    assert_bits_equal(outs[0][0], outs[1][0], "run to run")
    assert_bits_equal(outs[0][1], outs[1][1], "run to run")
    p_ref, v_ref = reference(oracle, pos, vel, (("boids", 2), ("nbody", 1), ("boids", 1)))
    assert np.abs(outs[0][1] - v_ref).max() <= 1e-4 * np.abs(v_ref).max() and np.abs(outs[0][0] - p_ref).max() <= 1e-4


def test_rccl_leg_of_the_pairs_form_on_a_one_rank_communicator(nb, oracle):
    """The RCCL calls of a pairs-form step -- ncclGroupStart, D x (ncclSend, ncclRecv), ncclGroupEnd, then ncclAllGather -- on the
    library's stream, with rank 0 of EIGHT on a communicator of ONE (nb_diag_rccl_solo: the sends go to the rank itself, the
    gather moves nothing): the whole call path of the second exchange on a one-GPU box.  The physics of such a step means nothing
    (the rank receives its own halves back); what is held is that every call succeeds, the step completes and stays finite, and
    the shard reports the form it took."""
    n = 131072
    pos, vel = nb.init_state(n, 1234)
    lib = nb.load()
    lib.nb_diag_rccl_solo(1)
    try:
        with nb.NativeShard(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST), rank=0, world=8, comm_id=nb.comm_id()) as sh:
            assert sh.partners == 4 and (sh.first, sh.count) == (0, 16384)
            sh.step(2)           # (an even count: the replica in hand is the buffer the upload filled)
            sh.sync()
            p, v = sh.positions(), sh.local_velocities()
        with nb.NativeShard(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST), rank=0, world=8, comm_id=nb.comm_id(), pairs=False) as sh:
            assert sh.partners == 0
            sh.step(1)
            sh.sync()
    finally:
        lib.nb_diag_rccl_solo(0)
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert (p[16384:] == pos[16384:]).all()          # the other ranks' slots: nothing arrived, nothing was touched
    assert np.abs(p[:16384] - pos[:16384]).max() > 0


@pytest.mark.parametrize("mode_name", ["strict", "fast", "fast_overlapped"])
def test_eight_ranks_as_threads_of_one_process(nb, oracle, monkeypatch, mode_name):
    """EIGHT ranks -- the world of BASELINE.json's configs 4 and 5 -- as eight threads of this process, each with its own native
    shard and stream on the one GPU ("one process (or thread) per GPU"), both exchanges supplied by the
    host through a barrier: nb_shard_step's indexing at the world size the 8-GPU node will run (D = 4 partners of the pairs form,
    the antipodal rank among them), and the library's per-thread plan caches under eight concurrent callers.  STRICT: every
    rank's bits equal the oracle's; FAST: the pairs form, two exchanges per step, within FAST's tolerance; fast_overlapped: the same
    step in phases (nb_shard_set_overlap), both exchanges on the shards' second streams."""
    import threading

    world, n, steps = 8, 32768, 2
    monkeypatch.setenv("NB_RING", "1")   # (a set this small keeps the ordered fold by itself)
    mode = nb.NB_MODE_STRICT if mode_name == "strict" else nb.NB_MODE_FAST
    pos, vel = oracle.init_state(n, 77)
    nb.load()
    hip = _hip_runtime()
    barrier = threading.Barrier(world, timeout=120)
    slots, halves, calls, results, errors = {}, {}, {"gather": 0, "ring": 0}, {}, []
    mu = threading.Lock()

    def rank_thread(rank):
        def gather(buf, slot_bytes, rank_, world_, stream):
            assert (rank_, world_) == (rank, world)
            assert hip.hipStreamSynchronize(stream) == 0
            mine = np.empty(slot_bytes, np.uint8)
            assert hip.hipMemcpy(mine.ctypes.data, buf + rank * slot_bytes, slot_bytes, 2) == 0
            slots[rank] = mine
            barrier.wait()
            full = np.concatenate([slots[r] for r in range(world)])
            assert hip.hipMemcpy(buf, full.ctypes.data, world * slot_bytes, 1) == 0
            barrier.wait()   # nobody replaces its slot before everyone has read it
            with mu:
                calls["gather"] += 1

        def ring(send, recv, chunk_bytes, partners, rank_, world_, stream):
            assert (rank_, world_, partners) == (rank, world, 4)
            assert hip.hipStreamSynchronize(stream) == 0
            out = np.empty(partners * chunk_bytes, np.uint8)
            assert hip.hipMemcpy(out.ctypes.data, send, partners * chunk_bytes, 2) == 0
            halves[rank] = out
            barrier.wait()
            got = np.concatenate([halves[(rank - d) % world][(d - 1) * chunk_bytes:d * chunk_bytes] for d in range(1, partners + 1)])
            assert hip.hipMemcpy(recv, got.ctypes.data, partners * chunk_bytes, 1) == 0
            barrier.wait()
            with mu:
                calls["ring"] += 1

        try:
            with nb.NativeShard(pos, vel, nb.default_params(mode=mode), rank=rank, world=world, gather=gather,
                                ring=ring if mode == nb.NB_MODE_FAST else None, overlap=mode_name == "fast_overlapped") as sh:
                partners = sh.partners
                assert sh.pairs_overlapped == (mode_name == "fast_overlapped")
                sh.step(steps)
                sh.sync()
                results[rank] = (sh.first, sh.count, partners, sh.positions(), sh.local_velocities(), sh.local_instances())
        except Exception as e:  # a rank that fails must not leave the others at the barrier
            errors.append((rank, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=rank_thread, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    assert sorted(results) == list(range(world))
    p_ref, v_ref = oracle.run(pos, vel, steps)
    inst_ref = oracle.instances(p_ref, v_ref)
    assert calls["gather"] == world * steps and calls["ring"] == (world * steps if mode == nb.NB_MODE_FAST else 0)
    scale = float(np.abs(v_ref - vel).max())
    for r in range(world):
        first, count, partners, p, v, inst = results[r]
        assert (first, count) == nb.partition(n, world)[r] and partners == (4 if mode == nb.NB_MODE_FAST else 0)
        if mode == nb.NB_MODE_STRICT:
            assert_bits_equal(p, p_ref, f"rank {r} positions (replica)")
            assert_bits_equal(v, v_ref[first:first + count], f"rank {r} velocities")
            assert matrices_equal(inst, inst_ref[first:first + count])
        else:
            dv = np.abs(v - v_ref[first:first + count]).max(axis=1)
            assert np.quantile(dv, 0.999) <= 1e-4 * scale and dv.max() <= 1e-2 * scale, f"rank {r}: {np.quantile(dv, 0.999) / scale:.2e} {dv.max() / scale:.2e}"
            dp = np.abs(p - p_ref).max(axis=1)
            assert np.quantile(dp, 0.999) <= 2e-4 * scale and dp.max() <= 2e-2 * scale, f"rank {r} positions (replica)"
