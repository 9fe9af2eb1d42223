"""Every FAST form against the exact lattice (tests/exact_lattice.py): every body, every component, every bit.

On the lattice every term and every partial sum is an exact binary32 number, so the order in which a form adds its pairs cannot
change a bit and the closed form is the only right answer.  A pair a form drops or counts twice moves its bodies by a whole unit;
FAST's global tolerance (2e-5 of the largest |dv|) cannot see that at production sizes, this can.  The FAST forms' reciprocals
are all of powers of two here, so the design also assumes v_rcp_f32(2^k) == 2^-k: the first test decides that on two bodies.
"""
import ctypes

import numpy as np
import pytest

from exact_lattice import assert_exact, lattice, wrong_bodies

pytestmark = pytest.mark.gpu

KINDS = ["tetra", "tetra_mixed", "planar", "line"]
SCALES = [1.0, 2.0 ** -20, 2.0 ** 29, 2.0 ** 31]


def params_of(nb, lat, mode=None, tile=0):
    p = nb.default_params(mode=nb.NB_MODE_FAST if mode is None else mode, tile=tile)
    p.dt, p.G, p.bias = (float(c) for c in lat.consts)
    return p


def scene(nb, lat, params):
    with nb.Scene(lat.pos, lat.vel, params) as sc:
        sc.step_n(lat.steps)
        return sc.state()


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# -- 1. two bodies through each form: if v_rcp_f32 of a power of two is not exact, this points at that, not at a form -------------
TWO_BODY_FORMS = {   # name: (environment, tile, the kernel the plan must name first, bodies)
    "strict": (None, 0, None, 2),
    "wave": ({}, 0, "step_fast_wave_kernel", 2),
    "wave_no_share": ({"NB_FAST_NO_SHARE": "1"}, 0, "step_fast_wave_kernel", 2),
    "lds": ({"NB_FAST_WAVES": "0"}, 256, "step_fast_kernel", 2),
    "scalar_load": ({"NB_FAST_SL": "1"}, 0, "step_fast_sl_kernel", 2),
    "pairs": ({"NB_FAST_PAIRS": "1"}, 0, "step_fast_pairs_kernel", 256),   # whole blocks of 256 only: two sites of 128 bodies
}


@pytest.mark.parametrize("form", list(TWO_BODY_FORMS))
def test_two_bodies_through_each_form(nb, monkeypatch, form):
    from nenbody_amd import _lib

    env, tile, kernel, n = TWO_BODY_FORMS[form]
    lat = lattice(n, seed=1, kind="tetra", sites=np.repeat([0, 1], n // 2), steps=2)
    if env is None:
        params = params_of(nb, lat, nb.NB_MODE_STRICT)
    else:
        set_env(monkeypatch, env)
        params = params_of(nb, lat, tile=tile)
        assert _lib.planned_kernels(params, n, n)[0] == kernel
    p, v = scene(nb, lat, params)
    d = np.abs(v.astype(np.float64) - lat.v_exp).max()
    assert_exact(lat, p, v, f"{form}: (every reciprocal here is of 2^2: |v - exact| = {d!r}; if STRICT passes and every FAST form "
                            f"is off, v_rcp_f32(1.0) is not 1.0)")


# -- 2. whole sets through Scene, the library's own plan, on both sides of every line make_plan draws -----------------------------
WAVE, LDS_SLICES = ["step_fast_wave_kernel"], ["step_fast_wave_kernel", "integrate_partials_kernel"]
SL = ["step_fast_sl_kernel", "planes_kernel", "integrate_partials_kernel"]
PAIRS = ["step_fast_pairs_kernel", "planes_kernel", "pairs_diag_kernel", "pairs_integrate_kernel"]
PAIRS_CHUNKED = ["step_fast_pairs_kernel", "planes_kernel", "pairs_diag_kernel", "pairs_accumulate_kernel", "pairs_finish_kernel"]
PLAN = [   # n, the kernels one step launches (what the line is)
    (1, WAVE), (2, WAVE), (255, WAVE), (256, WAVE),
    (4095, LDS_SLICES), (4096, SL),                                   # scalar loads from 4 096
    (32512, SL), (32767, SL), (32768, PAIRS),                         # pairs from 32 768 at multiples of 256
    (98304, PAIRS), (131072, PAIRS),                                  # eight bodies per lane from 98 304 (same kernels)
    (262144, PAIRS), (262400, PAIRS_CHUNKED), (1 << 20, PAIRS_CHUNKED), (4194304, PAIRS_CHUNKED),   # chunked walk above 262 144
    (4194304 + 256, ["step_fast_sl_kernel", "planes_kernel"]),        # pairs refused above 4 194 304
]


@pytest.mark.parametrize("n,kernels", PLAN, ids=lambda x: str(x) if isinstance(x, int) else None)
def test_whole_sets_on_the_plans_own_form_bit_exact(nb, n, kernels):
    from nenbody_amd import _lib

    steps = 1 if n >= 1 << 20 else 2
    for variant in (dict(), dict(runs=512, skew=(3, 1, 1, 2))):
        if n >= 1 << 20 and variant:
            continue
        lat = lattice(n, seed=n % 9973, kind="tetra", G0=2.0 ** -3, dt=2.0 ** -1, steps=steps, **variant)
        params = params_of(nb, lat)
        assert _lib.planned_kernels(params, n, n) == kernels, "the plan moved: update the sizes around its lines"
        p, v = scene(nb, lat, params)
        assert_exact(lat, p, v, f"n={n} {variant}")


# -- 3. every pinned FAST shape of test_gpu_parity.py, on every kind and scale, sharing on and off --------------------------------
def _every_kind_and_scale(nb, monkeypatch, n, what, tile=0, kernel=None, steps=2):
    from nenbody_amd import _lib

    for i, kind in enumerate(KINDS):
        for j, scale in enumerate(SCALES):
            no_share = "1" if (i + j) % 2 else "0"
            monkeypatch.setenv("NB_FAST_NO_SHARE", no_share)
            lat = lattice(n, seed=n + 7 * i + j, kind=kind, scale=scale, steps=steps, runs=0 if j < 2 else 256)
            params = params_of(nb, lat, tile=tile)
            if kernel:
                assert _lib.planned_kernels(params, n, n)[0] == kernel
            p, v = scene(nb, lat, params)
            assert_exact(lat, p, v, f"{what} no_share={no_share}")


@pytest.mark.parametrize("ib,groups,slices,tile", [(1, 1, 1, 256), (2, 1, 1, 512), (4, 1, 1, 1024), (1, 1, 4, 256), (2, 1, 7, 512),
                                                   (4, 1, 64, 256), (1, 2, 1, 256), (2, 2, 3, 512), (4, 2, 1, 256), (1, 4, 1, 512),
                                                   (2, 4, 2, 256), (4, 4, 1, 512), (4, 4, 5, 256), (4, 4, 16, 512)])
def test_lds_form_every_launch_shape(nb, monkeypatch, ib, groups, slices, tile):
    """the workgroup-tile form (NB_FAST_WAVES=0: step_fast_kernel) at every shape the parity tests name"""
    set_env(monkeypatch, {"NB_FAST_WAVES": "0", "NB_FAST_IB": str(ib), "NB_FAST_GROUPS": str(groups), "NB_FAST_SLICES": str(slices)})
    _every_kind_and_scale(nb, monkeypatch, 5000, f"lds ib={ib} groups={groups} slices={slices} tile={tile}", tile, "step_fast_kernel")


@pytest.mark.parametrize("ib,waves,slices,tile", [(1, 1, 1, 256), (1, 4, 3, 256), (1, 16, 1, 256), (2, 8, 1, 256), (2, 16, 2, 512), (4, 4, 5, 256),
                                                  (4, 8, 1, 256), (4, 16, 1, 256), (4, 16, 2, 512), (2, 4, 64, 256)])
def test_wave_form_every_launch_shape(nb, monkeypatch, ib, waves, slices, tile):
    set_env(monkeypatch, {"NB_FAST_IB": str(ib), "NB_FAST_WAVES": str(waves), "NB_FAST_SLICES": str(slices)})
    for n in (5000, 64 * ib, 777):
        _every_kind_and_scale(nb, monkeypatch, n, f"wave ib={ib} waves={waves} slices={slices} tile={tile} n={n}", tile,
                              "step_fast_wave_kernel")


@pytest.mark.parametrize("ib,slices", [(1, 1), (2, 1), (4, 1), (1, 3), (2, 5), (4, 2), (4, 64)])
def test_scalar_load_form_every_launch_shape(nb, monkeypatch, ib, slices):
    set_env(monkeypatch, {"NB_FAST_SL": "1", "NB_FAST_IB": str(ib), "NB_FAST_SLICES": str(slices)})
    for n in (5000, 64 * ib, 777, 1, 15, 4099):
        _every_kind_and_scale(nb, monkeypatch, n, f"scalar-load ib={ib} slices={slices} n={n}", 0, "step_fast_sl_kernel")


@pytest.mark.parametrize("n,w,chunk", [(256, 8, 0), (512, 1, 0), (512, 8, 0), (2048, 2, 0), (2304, 8, 0), (2304, 4, 0), (4096, 1, 0), (4096, 8, 0),
                                       (6400, 8, 0), (6400, 2, 0), (8192, 4, 0), (32768, 0, 0),
                                       (4096, 1, 1024), (6400, 2, 2048), (6400, 1, 256), (8192, 4, 2048), (7168, 8, 4096), (32768, 4, 8192),
                                       (512, -1, 0), (1024, -4, 0), (4096, -2, 0), (6656, -4, 0), (8192, -4, 4096), (7168, -2, 2048), (7168, -1, 512)])
def test_pairs_form_every_launch_shape(nb, monkeypatch, n, w, chunk):
    """the pairs form at every shape of test_fast_pairs_form: widths, eight or four bodies per lane, one superblock, a last superblock of
    one block (2 304, 6 400), the two-level walk with ragged last chunks"""
    from nenbody_amd import _lib

    set_env(monkeypatch, {"NB_FAST_PAIRS": "1", "NB_FAST_PAIRS_NP": "4" if w < 0 else "2"})
    if w:
        monkeypatch.setenv("NB_FAST_PAIRS_W", str(abs(w)))
    if chunk:
        monkeypatch.setenv("NB_FAST_PAIRS_CHUNK", str(chunk))
        assert "pairs_accumulate_kernel" in _lib.planned_kernels(nb.default_params(mode=nb.NB_MODE_FAST), n, n)
    _every_kind_and_scale(nb, monkeypatch, n, f"pairs n={n} w={w} chunk={chunk}", 0, "step_fast_pairs_kernel")


# -- 4. the launch API: shards of one set, and the step in two phases ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("parts", [[(0, 1), (1, 2047), (2048, 3000), (5048, 952)], [(0, 6000)], [(0, 3000), (3000, 3000)]], ids=len)
def test_sharded_launches_bit_exact(nb, mode, parts):
    from test_gpu_parity import _sharded_step_on_one_gpu

    for kind, scale in (("tetra", 1.0), ("tetra_mixed", 2.0 ** 29)):
        lat = lattice(6000, seed=len(parts), kind=kind, scale=scale, steps=2, runs=0 if scale == 1.0 else 1000)
        params = params_of(nb, lat, nb.NB_MODE_FAST if mode == "fast" else nb.NB_MODE_STRICT)
        p, v = _sharded_step_on_one_gpu(nb, lat.pos, lat.vel, parts, params, 2)
        assert_exact(lat, p, v, f"{mode} shards {parts}")


@pytest.mark.parametrize("waves", [0, 8])
@pytest.mark.parametrize("n,first,count,j_lo,j_hi", [(6000, 0, 6000, 0, 750), (6000, 1500, 750, 1500, 2250), (6000, 5250, 750, 5250, 6000),
                                                     (5001, 1000, 333, 0, 0), (5001, 0, 5001, 0, 5001), (131072, 16384, 16384, 16384, 32768)])
def test_step_in_two_phases_bit_exact(nb, monkeypatch, waves, n, first, count, j_lo, j_hi):
    import torch

    from nenbody_amd import _lib

    if waves:
        monkeypatch.setenv("NB_FAST_WAVES", str(waves))
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for kind, scale in (("tetra", 1.0), ("tetra_mixed", 2.0 ** -20), ("planar", 2.0 ** 29)):
        lat = lattice(n, seed=first + j_lo, kind=kind, scale=scale)
        fast = params_of(nb, lat)
        cur = torch.zeros((n, 4), dtype=torch.float32)
        cur[:, :3] = torch.from_numpy(lat.pos)
        cur = cur.to(dev)
        nxt = torch.zeros_like(cur)
        v = torch.zeros((count, 4), dtype=torch.float32)
        v[:, :3] = torch.from_numpy(lat.vel[first:first + count])
        v = v.to(dev)
        sb = lib.nb_scratch_bytes_phased(ctypes.byref(fast), n, count, j_lo, j_hi)
        scratch = torch.empty((sb,), dtype=torch.uint8, device=dev)
        for phase in (_lib.NB_PHASE_RANGE, _lib.NB_PHASE_REST):
            _lib.check(lib.nb_launch_step_phase(ctypes.byref(fast), n, first, count, j_lo, j_hi, phase, cur.data_ptr(), nxt.data_ptr(),
                                               v.data_ptr(), scratch.data_ptr(), sb, stream))
        torch.cuda.synchronize()
        assert_exact(lat, nxt[first:first + count, :3].cpu().numpy(), v[:, :3].cpu().numpy(), f"phases {kind}", first, count)


# -- 5. the pairs form across ranks (nb_launch_ring_*), two steps: the fused finish's second step included (a stale hand-off between
#    the steps shows on the permuted lattices only) ------------------------------------------------------------------------------
RING_SHAPES = [(2048, 2, 4, 0, 0), (1536, 3, 4, 0, 0), (4096, 4, 4, 1, 4), (4096, 8, 4, 0, 8), (3072, 3, 2, 2, 0), (2560, 2, 2, 3, 12),
               (8192, 2, 4, 0, 0), (12288, 3, 4, 5, 0)]
RING_PHASE_SHAPES = [(2048, 2, 4, 0, 0, 0), (1536, 3, 4, 0, 0, 0), (4096, 8, 4, 0, 0, 0), (4096, 4, 4, 4, 8, 4), (3072, 3, 2, 4, 4, 8),
                     (8192, 2, 4, 8, 12, 24), (12288, 3, 4, 5, 7, 12), (16384, 4, 4, 0, 0, 1000), (16384, 4, 4, 0, 0, 0)]


def _ring_lattices(n, world):
    S = n // world
    yield lattice(n, seed=n + world, kind="tetra", steps=2)
    yield lattice(n, seed=n + world + 1, kind="tetra_mixed", scale=2.0 ** 29, steps=2, runs=S)        # whole ranks of one site
    yield lattice(n, seed=n + world + 2, kind="planar", scale=2.0 ** -20, steps=2, runs=256)
    yield lattice(n, seed=n + world + 3, kind="line", scale=2.0 ** 31, steps=2, skew=(9, 1))
    # permuted: the first step carries every site onto another, so the second step's terms differ from the first's and a record
    # (received halves, sums, the fused finish's own-slot planes) left over from the first step shows
    yield lattice(n, seed=n + world + 4, kind="tetra", scale=2.0 ** -20, steps=2, permute=(1, 2, 3, 0))
    yield lattice(n, seed=n + world + 5, kind="tetra_mixed", scale=2.0 ** 29, steps=2, runs=S, permute=(2, 3, 0, 1))


@pytest.mark.parametrize("n,world,np_,ga,wpb", RING_SHAPES)
def test_ring_shapes_bit_exact(nb, monkeypatch, n, world, np_, ga, wpb):
    from test_gpu_ring import ring_steps_on_one_gpu

    set_env(monkeypatch, {"NB_RING": "1", "NB_RING_NP": str(np_)})
    if ga:
        monkeypatch.setenv("NB_RING_GA", str(ga))
    if wpb:
        monkeypatch.setenv("NB_RING_WPB", str(wpb))
    for lat in _ring_lattices(n, world):
        p, v = ring_steps_on_one_gpu(nb, lat.pos, lat.vel, world, params_of(nb, lat), 2)
        assert_exact(lat, p, v, f"ring n={n} ranks={world}")


@pytest.mark.parametrize("n,world,np_,c4_own,c4_rest,cap", RING_PHASE_SHAPES)
def test_ring_phases_bit_exact(nb, monkeypatch, n, world, np_, c4_own, c4_rest, cap):
    from test_gpu_ring import ring_steps_on_one_gpu

    set_env(monkeypatch, {"NB_RING": "1", "NB_RING_NP": str(np_)})
    for name, val in (("NB_RING_C4_OWN", c4_own), ("NB_RING_C4_REST", c4_rest), ("NB_RING_CAP", cap)):
        if val:
            monkeypatch.setenv(name, str(val))
    for lat in _ring_lattices(n, world):
        for phases in (True, "fused"):
            p, v = ring_steps_on_one_gpu(nb, lat.pos, lat.vel, world, params_of(nb, lat), 2, phases=phases)
            assert_exact(lat, p, v, f"ring phases={phases} n={n} ranks={world}")


@pytest.mark.parametrize("n,world,phases", [(131072, w, ph) for w in (2, 4, 8) for ph in (False, True, "fused")] +
                         [(1 << 20, w, False) for w in (2, 4, 8)], ids=str)
def test_every_rank_of_configs_4_and_5_bit_exact(nb, n, world, phases):
    from test_gpu_ring import ring_steps_on_one_gpu

    lat = lattice(n, seed=world, kind="tetra", G0=2.0 ** -3, dt=2.0 ** -1, steps=2)
    p, v = ring_steps_on_one_gpu(nb, lat.pos, lat.vel, world, params_of(nb, lat), 2, phases=phases)
    assert_exact(lat, p, v, f"n={n} ranks={world} phases={phases}")
    if phases:   # the second step of the phases starts from the planes the first one's finish left: on the permuted lattice too
        lat = lattice(n, seed=world + 1, kind="tetra", G0=2.0 ** -3, dt=2.0 ** -1, steps=2, permute=(1, 2, 3, 0))
        p, v = ring_steps_on_one_gpu(nb, lat.pos, lat.vel, world, params_of(nb, lat), 2, phases=phases)
        assert_exact(lat, p, v, f"permuted n={n} ranks={world} phases={phases}")


@pytest.mark.parametrize("phases", [False, "fused"])
def test_ring_control_arm_one_corrupted_record(nb, monkeypatch, phases):
    """One record of one rank's received halves spoiled in the last step: exactly that body must fail the lattice check (received
    record l of rank r's buffer belongs to body r * S + l)."""
    from test_gpu_ring import ring_steps_on_one_gpu

    n, world, rank, chunk, rec = 131072, 8, 5, 2, 777
    S = n // world
    lat = lattice(n, seed=3, kind="tetra", G0=2.0 ** -3, dt=2.0 ** -1, steps=2)
    hits = []

    def corrupt(step, recv):
        if step == lat.steps - 1:
            r = recv[rank][chunk * S + rec]
            hits.append(r[:3].cpu().numpy().copy())
            recv[rank][chunk * S + rec, 0] = r[0] * 2 + 1
    p, v = ring_steps_on_one_gpu(nb, lat.pos, lat.vel, world, params_of(nb, lat), 2, phases=phases, corrupt=corrupt)
    assert len(hits) == 1
    assert wrong_bodies(lat, p, v).tolist() == [rank * S + rec], f"record {hits[0]} spoiled"
    p, v = ring_steps_on_one_gpu(nb, lat.pos, lat.vel, world, params_of(nb, lat), 2, phases=phases)
    assert_exact(lat, p, v, "the same run without the corruption")


# -- 6. native shards: eight ranks as threads of one process, FAST in the pairs form and overlapped, two steps ------------------------
@pytest.mark.parametrize("overlap", [False, True], ids=["pairs", "pairs_overlapped"])
def test_eight_native_shards_as_threads_bit_exact(nb, monkeypatch, overlap):
    world, n = 8, 32768
    monkeypatch.setenv("NB_RING", "1")
    nb.load()
    for lat in (lattice(n, seed=8, kind="tetra_mixed", steps=2, runs=1024),
                lattice(n, seed=9, kind="tetra_mixed", steps=2, permute=(2, 3, 0, 1))):   # (permuted: bodies change layer between steps)
        _eight_native_shards_two_steps(nb, lat, overlap)


def _eight_native_shards_two_steps(nb, lat, overlap):
    import threading

    from test_gpu_native_shard import _hip_runtime

    world = 8
    params = params_of(nb, lat)
    hip = _hip_runtime()
    barrier = threading.Barrier(world, timeout=120)
    slots, halves, results, errors = {}, {}, {}, []

    def rank_thread(rank):
        def gather(buf, slot_bytes, rank_, world_, stream):
            assert hip.hipStreamSynchronize(stream) == 0
            mine = np.empty(slot_bytes, np.uint8)
            assert hip.hipMemcpy(mine.ctypes.data, buf + rank * slot_bytes, slot_bytes, 2) == 0
            slots[rank] = mine
            barrier.wait()
            full = np.concatenate([slots[r] for r in range(world)])
            assert hip.hipMemcpy(buf, full.ctypes.data, world * slot_bytes, 1) == 0
            barrier.wait()

        def ring(send, recv, chunk_bytes, partners, rank_, world_, stream):
            assert hip.hipStreamSynchronize(stream) == 0
            out = np.empty(partners * chunk_bytes, np.uint8)
            assert hip.hipMemcpy(out.ctypes.data, send, partners * chunk_bytes, 2) == 0
            halves[rank] = out
            barrier.wait()
            got = np.concatenate([halves[(rank - d) % world][(d - 1) * chunk_bytes:d * chunk_bytes] for d in range(1, partners + 1)])
            assert hip.hipMemcpy(recv, got.ctypes.data, partners * chunk_bytes, 1) == 0
            barrier.wait()

        try:
            with nb.NativeShard(lat.pos, lat.vel, params, rank=rank, world=world, gather=gather, ring=ring, overlap=overlap) as sh:
                assert sh.partners == 4 and sh.pairs_overlapped == overlap
                sh.step(lat.steps)
                sh.sync()
                results[rank] = (sh.first, sh.count, sh.positions(), sh.local_velocities())
        except Exception as e:  # a rank that fails must not leave the others at the barrier
            errors.append((rank, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=rank_thread, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    for r in range(world):
        first, count, p, v = results[r]
        assert (p.view(np.uint32) == lat.p_exp.view(np.uint32)).all(), f"rank {r}: replica of positions"
        assert_exact(lat, p[first:first + count], v, f"rank {r} of {world}", first, count)


# -- 7. STRICT at the sizes its other tests only sample: every body ------------------------------------------------------------------
@pytest.mark.parametrize("n,scale", [(1 << 20, 1.0), (1 << 20, 2.0 ** 29), (4194304, 1.0)], ids=str)
def test_strict_every_body_at_large_sizes(nb, n, scale):
    lat = lattice(n, seed=17, kind="tetra", scale=scale, G0=2.0 ** -3, dt=2.0 ** -1)
    p, v = scene(nb, lat, params_of(nb, lat, nb.NB_MODE_STRICT))
    assert_exact(lat, p, v, f"STRICT n={n}")
