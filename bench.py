#!/usr/bin/env python3
"""bench.py -- body-updates/s of nenbody's all-pairs gravity + Euler step on MI355X.

    python bench.py --gpus N --steps K --warmup W            (N > 1: starts its own N ranks as child processes)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W                 (ranks started by the caller: RANK / WORLD_SIZE in the env)

Workload (BASELINE.json): N = 131 072 bodies, reference initial distributions (src/main.rs:738-747, seeded),
reference constants (src/main.rs:411-413); a "step" is one update_instance_nbody over the whole set.  With N
GPUs the set is sharded by index range (strong scaling: total work fixed) and positions are all-gathered
once per step (RCCL); FAST on equal ranks evaluates every unordered pair once across the ranks, the other bodies' halves
leaving in a second, point-to-point exchange per step (--no-ring: the ordered fold and its one exchange).  Inputs are
resident in HBM before the timed region.

Prints ONE JSON line on rank 0.  `value` = body-updates/s = N * steps / s of the whole job, STRICT arithmetic (the
reference's own, bit for bit) unless --mode fast; `ms_per_step` = milliseconds of one timed step.  `roofline` prices the
pair-fold kernel against the fp32 vector peak (the binding roofline: SURVEY.md section 8d) at the reference's 18 flop
per interaction, from the kernel times of the timed steps themselves.  `targets` says which mode meets which line of
BASELINE.json's north_star: no single mode meets both.

A plain run does what the headline needs and nothing else: set up, preheat, warm up, time exactly --steps steps, print the line.
Every leg starts its warm-up from the initial state (the preheat's steps are undone), so with the same arguments the state the last
timed step leaves is the same from run to run; --dump-outputs DIR writes it as DIR/positions.npy and DIR/velocities.npy (float32,
(n, 3); above 64 MB in all, a fixed seeded sample of the rows).

--full adds everything else, after the headline: the line's own `parity_check`, the other mode, the 3-D data, the boids controller,
the unpreheated legs, the per-call drop-in latency, the rate this device's vector ALU was measured to issue in the same process
(`roofline.measured_issue_ceiling`), and `cpu_baseline`: the CPU oracle (a C restatement of the reference's Rust; kind "port") timed
on the host cores this process may really use (--no-secondary / --no-cpu-baseline leave parts of it out).

Exit code: 0; with --full, 3 when an informational leg (other mode, 3-D data, boids, CPU baseline) hung -- the headline line is still
printed, with `aux_error` naming the leg -- and 4 when the line's own `parity_check` failed (STRICT: some bit of the final state
differs from the golden checksums of that step; FAST: one step further from STRICT than its tolerance) -- the line is printed all the
same.
"""
import argparse
import json
import os
import sys
import time

# Memory handles between the ranks' processes (RCCL's own, and the pulls of nb_peers_*) need the dmabuf IPC mode on this platform: the
# image exports it; a launcher that builds its own environment may not.  Before anything touches the GPU.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_VECTOR_TFLOPS = 157.3   # MI355X chip-level parameters (vendor specification)
PEAK_HBM_GBPS = 8000.0            # same specification: HBM3E ~8 TB/s
SPEC_LANE_OPS_PER_S = PEAK_FP32_VECTOR_TFLOPS * 1e12 / 2.0   # one vector operation per lane per cycle (the flop peak counts an FMA twice)
BYTES_PER_BODY_STEP = 64          # algorithmic HBM bytes: 16-B position + 16-B velocity record, read and written once
FLOP_PER_INTERACTION = 18         # src/main.rs:428-430 as written: 3 sub, 3 mul + 2 add, 1 add, 3 mul, 3 div, 3 add
# What the kernels execute per interaction on the vector ALU, in full-rate lane-ops + quarter-rate
# v_rcp_f32: the 18-flop figure above is the reference's NOMINAL count and is what `frac` is quoted against.
EXECUTED_OPS = {
    ("strict", "planar"): {"full_rate_ops": 18, "v_rcp_f32": 1.0, "note": "exact divide = 4 ops after a shared refined reciprocal"},
    ("strict", "3d"): {"full_rate_ops": 26, "v_rcp_f32": 1.0},
    ("fast", "planar"): {"full_rate_ops": 7.5, "v_rcp_f32": 0.5, "note": "two pairs share one reciprocal: 3 extra multiplies per two pairs"},
    ("fast", "3d"): {"full_rate_ops": 10.5, "v_rcp_f32": 0.5},
    # the pairs form (step_fast_pairs_kernel): every UNORDERED pair evaluated once and credited to both bodies; per ordered pair:
    ("fast", "planar", "step_fast_pairs_kernel"): {"full_rate_ops": 5.0, "v_rcp_f32": 0.25,
                                                   "note": "per ORDERED pair; one evaluation serves both bodies of a pair (36 v_pk_* + 4 v_mul + 4 v_sub "
                                                           "+ 4 v_rcp per eight unordered pairs of a lane's eight bodies), two evaluations share one reciprocal"},
    ("fast", "3d", "step_fast_pairs_kernel"): {"full_rate_ops": 7.125, "v_rcp_f32": 0.25},
}


def executed_ops(mode, data, kernel):
    return EXECUTED_OPS.get((mode, data, kernel), EXECUTED_OPS[(mode, data)])


def roofline_fractions(mode, data, form, n, count, kernel_ms):
    """What one launch of kernel form `form` over `count` of `n` bodies achieves against the fp32 vector roofline, every figure saying
    what it divides.  Pure arithmetic (tests/test_bench_math.py).

    Pair EVALUATIONS a launch executes: the ordered folds evaluate every ordered pair the reference does (count x n, self pairs
    included).  The pairs forms evaluate an unordered pair ONCE for both bodies: a whole set n^2 / 2 + superblock / 2 x n (the pairs
    between superblocks once, the pairs inside them as an ordered fold; superblocks of 2 048 bodies from 131 072 bodies on, nb_api.hip:
    make_plan); a rank of the multi-GPU form count x n / 2 + 256 count (its blocks against the half of the ring behind them + each
    block of 512 against itself).
      achieved / frac          18 flop x the evaluations EXECUTED / time (/ the spec peak): can never pass 1
      achieved_nominal / frac_nominal   18 flop x the reference's count x n ordered pairs / time: what the work is worth in the
                               reference's own count; passes 1 where one evaluation serves two bodies
      frac_executed            vector lane operations per second (full-rate ops + reciprocals per ordered pair of the reference)
                               over the spec issue rate of one per lane per cycle"""
    kernel_s = kernel_ms * 1e-3
    nominal = FLOP_PER_INTERACTION * count * n / kernel_s / 1e12 if kernel_s > 0 else 0.0
    ex = dict(executed_ops(mode, data, "step_fast_pairs_kernel" if form == "step_fast_ring_kernel" else form))
    if form == "step_fast_pairs_kernel":
        superblock = 2048.0 if n >= 131072 and n % 512 == 0 else 1024.0
        evaluations = float(n) * n / 2.0 + superblock / 2.0 * n
    elif form == "step_fast_ring_kernel":
        evaluations = float(count) * n / 2.0 + 256.0 * count
    else:
        evaluations = float(count) * n
    achieved = FLOP_PER_INTERACTION * evaluations / kernel_s / 1e12 if kernel_s > 0 else 0.0
    lane_ops = (ex["full_rate_ops"] + ex["v_rcp_f32"]) * float(count) * n / kernel_s if kernel_s > 0 else 0.0
    return {"achieved": achieved, "frac": achieved / PEAK_FP32_VECTOR_TFLOPS, "achieved_nominal": nominal,
            "frac_nominal": nominal / PEAK_FP32_VECTOR_TFLOPS, "lane_ops_per_s": lane_ops, "frac_executed": lane_ops / SPEC_LANE_OPS_PER_S,
            "pair_evaluations_per_launch": evaluations, "executed_per_interaction": ex}


def state_checksums(positions, velocities):
    """XOR and wrapping 32-bit sum of every bit pattern of the (n, 3) float32 positions and of the velocities: what
    tests/golden/nbody_golden_c3.npz holds for the headline set after each of 1 000 steps of the CPU oracle (make_golden.py --c3).
    Returns ([xor_p, xor_v], [sum_p, sum_v]) as Python ints.  Pure numpy (tests/test_bench_math.py)."""
    import numpy as np

    out_x, out_s = [], []
    for a in (positions, velocities):
        u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).ravel()
        out_x.append(int(np.bitwise_xor.reduce(u)) if u.size else 0)
        out_s.append(int(u.sum(dtype=np.uint64) & 0xFFFFFFFF))
    return out_x, out_s


DUMP_LIMIT_BYTES = 60 * 10 ** 6   # --dump-outputs: what all arrays may hold together (under 64 MB with the .npy headers)


def write_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: every (n, k) array as out_dir/<name>.npy in float32.  Where all of them together pass `limit` bytes, the same
    fixed, seeded sample of rows (sorted) is written of each.  Returns the rows written (None: all).  Pure numpy
    (tests/test_bench_math.py)."""
    import numpy as np

    arrays = {name: np.ascontiguousarray(a, dtype=np.float32) for name, a in arrays.items()}
    n = len(next(iter(arrays.values())))
    row_bytes = sum(a[:1].nbytes for a in arrays.values())
    rows = None
    if n * row_bytes > limit:
        rows = np.sort(np.random.default_rng(1234).choice(n, size=limit // row_bytes, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a if rows is None else a[rows])
    return rows


def parity_against_golden(n, seed, steps_done, positions, velocities, path=None):
    """The bench line's own proof of parity: after `steps_done` STRICT steps of the headline set (n = 131 072,
    seed 1234, the reference's constants) every bit of every body must be the CPU oracle's -- compared through the XOR and the wrapping
    sum of all position and velocity bit patterns against the committed golden checksums of exactly that step.  Returns the
    `parity_check` object of the JSON line; `bits_equal` is None (with `why`) where no golden step exists for this run."""
    import numpy as np

    path = path or os.path.join(ROOT, "tests", "golden", "nbody_golden_c3.npz")
    out = {"k": int(steps_done), "bits_equal": None, "against": "tests/golden/nbody_golden_c3.npz: XOR + wrapping sum of every position and velocity bit "
                                                                "pattern after step k of the CPU oracle (C restatement of src/main.rs:404-441)"}
    try:
        g = np.load(path)
    except Exception as e:
        out["why"] = f"no golden file ({e.__class__.__name__})"
        return out
    if n != 131072 or int(g["seed"][0]) != seed or f"n{n}_xor" not in g.files:
        out["why"] = f"the golden checksums are of n = 131072, seed {int(g['seed'][0])}: nothing to compare n = {n}, seed {seed} with"
        return out
    steps = g[f"n{n}_steps"]
    if steps_done < int(steps[0]) or steps_done > int(steps[-1]):
        out["why"] = f"the golden file holds steps {int(steps[0])}..{int(steps[-1])}; this run made {steps_done}"
        return out
    i = int(steps_done - int(steps[0]))
    x, s = state_checksums(positions, velocities)
    gx, gs = [int(v) for v in g[f"n{n}_xor"][i]], [int(v) for v in g[f"n{n}_sum"][i]]
    out["bits_equal"] = bool(x == gx and s == gs)
    out["checksums"] = {"xor": x, "sum": s, "golden_xor": gx, "golden_sum": gs}
    return out


def committed_traffic(nb, kernels, n, count):
    """HBM bytes per step from the committed rocprofv3 --pmc passes (tools/pmc_summary.py --json), or (None, why).

    bench.py cannot collect PMC counters itself; the file is refused when it was taken from other kernel sources, another
    shape, or does not hold every kernel this step launches."""
    path = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    try:
        t = json.load(open(path))
    except Exception as e:
        return None, f"no usable profiles/hbm_traffic.json ({e.__class__.__name__})"
    try:
        running = nb._lib.kernel_code_sha()
    except Exception as e:   # (a library built another way -- compressed offload bundles, say: no stamp to compare, no traffic reported)
        return None, f"the built library's device code could not be hashed ({e.__class__.__name__}: {e}): traffic not reported"
    if t.get("code_sha") != running:
        return None, "profiles/hbm_traffic.json was measured on other device code (code_sha differs from the built library's): stale, not reported"
    if t.get("n") == n and t.get("count") != count and str(count) in t.get("shards", {}):   # one rank's share of a multi-GPU job
        t = dict(t["shards"][str(count)], code_sha=running)
    if t.get("n") != n or t.get("count") != count:
        return None, "profiles/hbm_traffic.json is for another shape"
    missing = [k for k in kernels if k not in t.get("kernels", {})]
    if missing:
        return None, f"profiles/hbm_traffic.json lacks {missing}"
    return sum(t["kernels"][k]["bytes_per_launch"] for k in kernels), f"rocprofv3 --pmc passes committed under {t.get('source', 'profiles/')} (not measured in this run)"


def step_kernels(nb, mode, n, count):
    """the kernels one step launches, dominant one first -- asked of the library (nb_diag_plan), not restated here"""
    return nb._lib.planned_kernels(nb.default_params(mode=mode), n, count)


def preheat(step, torch, dist, world, dev, ms):
    """Untimed steps until the device holds its clock: after the idle gap in front of a leg (context creation, uploads) the part
    ramps its clock over tens of milliseconds -- rocprofv3's trace of this bench shows the first launches of every leg 15-25 %
    slow (profiles/r03/kernel_stats_all.csv: 6.7 -> 5.4 ms over the first six STRICT launches) -- which a warm-up counted in
    steps (3 x 2.3 ms for FAST) does not cover.  The same number of steps on every rank (rank 0 decides).  Returns the count."""
    if ms <= 0:
        return 0

    def sync():
        if getattr(dev, "type", "cuda") == "cuda":   # (a CPU device: the gloo test of this function)
            torch.cuda.synchronize(dev)

    sync()
    t = time.perf_counter()
    step()
    step()
    sync()
    per = max((time.perf_counter() - t) / 2.0, 1e-5)
    k = torch.tensor([min(2000, max(0, int(ms / 1e3 / per) - 1))], dtype=torch.int64, device=dev)
    if world > 1:
        dist.broadcast(k, 0)   # every step holds a collective: ranks that disagreed on the count would hang in it
    for _ in range(int(k.item())):
        step()
    sync()
    return int(k.item()) + 2


def time_mode(nb, torch, dist, args, mode, rank, world, pos, vel, steps=None, warmup=None, overlap=False, ring=None, preheat_ms=None,
              ring_overlap=None, choose=False, parity=False, exchange_kind=None, dump=None):
    """ring: None = the library's plan (FAST on equal ranks of a multi-GPU job: every unordered pair once, two exchanges per
    step), False = the ordered fold with its one exchange.  ring_overlap: the pairs form in phases, its exchanges behind compute.
    choose: FAST at world > 1 -- let ShardedScene.choose_form time every form this shape can take and keep the fastest (the
    timed region then runs that form; `form` in the result says which and what each cost).  parity: check the final state (STRICT:
    every bit against the golden checksums of that step; FAST: one step against STRICT).  dump: a directory -- rank 0 writes the
    positions and velocities the last timed step left there (write_outputs)."""
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    params = nb.default_params(mode=mode)
    sc = nb.ShardedScene(pos, vel, params, overlap=overlap, ring=ring, ring_overlap=ring_overlap)
    dev = sc.device
    initial = (sc.pos[0].clone(), sc.pos[1].clone(), sc.vel.clone())

    def fence():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    # untimed: bring the communicator and its channels up even when --warmup 0, and VERIFY both exchanges on a known pattern before
    # any step relies on them (a mismatch moves the exchange to its fallback; `exchange_paths` in the line says which path ran)
    exchange_paths = sc.verify_exchanges() if world > 1 else None
    exchange = None
    if world > 1 and exchange_kind is not None:   # an informational leg: the headline's choice, not another round of timing
        if exchange_kind == "peers" and sc.setup_peers():
            sc.exchange = "peers"
        exchange = {"chosen": sc.exchange, "requested": exchange_kind}
    elif world > 1 and args.exchange != "collective":
        # the same exchanges as pulls over xGMI (IPC-mapped buffers, stream value waits, one copy kernel): mapped, verified on the
        # pattern and TIMED against the collectives on this machine; the faster runs (--exchange peers: required, not timed)
        if args.exchange == "peers":
            ok = sc.setup_peers()
            if ok:
                sc.exchange = "peers"
                exchange_paths = sc.verify_exchanges()
            exchange = {"chosen": sc.exchange, "requested": "peers", "mapped": ok, "why": sc.peers_error}
        else:
            chosen = sc.choose_exchange(steps=6, warm=2)
            exchange = {"chosen": chosen, "requested": "auto", "mapped": sc._peers is not None, "why": sc.peers_error,
                        "ms_per_step": None if sc.exchange_times is None else {k_: (None if v_ is None else 1e3 * v_) for k_, v_ in sc.exchange_times.items()},
                        "what": "ShardedScene.choose_exchange: RCCL's collectives against pulls over xGMI ordered by stream value waits "
                                "(nb_peers_*), each verified on a pattern, 6 steps of this form each, slowest rank"}
            if sc.exchange_report is not None:
                exchange_paths = sc.exchange_report
    form = None
    if choose and world > 1 and sc.partners:
        pre0 = preheat(sc.step, torch, dist, world, dev, args.preheat_ms if preheat_ms is None else preheat_ms)
        chosen = sc.choose_form(steps=10, warm=3)
        form = {"chosen": chosen, "ms_per_step": {k_: 1e3 * v_ for k_, v_ in sc.form_times.items()}, "preheat_steps": pre0,
                "what": "ShardedScene.choose_form(steps=10) on this machine, slowest rank's wall time: the pairs form with its two exchanges in "
                        "sequence / behind compute (nb_launch_ring_fold_phase), the ordered fold with its one exchange; the timed region runs "
                        "the fastest"}
    pre = preheat(sc.step, torch, dist, world, dev, args.preheat_ms if preheat_ms is None else preheat_ms)
    if pre:
        # the preheat's step count follows the wall clock: undo its steps, so that the warm-up starts from the initial state and the
        # state the timed steps leave depends on the arguments alone (every rank: no pull of a peer's buffer is in flight around it)
        sc._wait_pending()
        fence()
        for buf, saved in zip((sc.pos[0], sc.pos[1], sc.vel), initial):
            buf.copy_(saved)
        sc.cur, sc.steps_done, sc.velfull_valid, sc._own_ready = 0, 0, False, None
        fence()
    del initial
    for _ in range(warmup):
        sc.step()
    # kernel-only timing: events on the stream the kernels are launched on (torch's current stream), around every launch call of
    # a step (one: nb_launch_step; the pairs form on shards: nb_launch_ring_fold and nb_launch_ring_finish -- or the three phases --
    # the exchanges between them outside the events)
    # (in phases: OWN / REST / SUMS / the fused finish; pulls run in-stream, nothing runs beside them: the finish adds the own records itself)
    calls = (("ring_fold_phase", "ring_finish_phase") if sc.ring_overlap else ("ring_fold", "ring_finish")) if sc.partners else ("step",)
    sums_in_finish = sc.exchange == "peers" and bool(getattr(sc, "_peers_sums", None))
    per_step = ((3 if sums_in_finish else 4) if sc.ring_overlap else 2) if sc.partners else 1
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps * per_step)]
    real = {name: getattr(sc.backend, name) for name in calls}
    used = [0]

    def timed(fn):
        def call(*a, **kw):
            e0, e1 = ev[used[0]]
            used[0] += 1
            e0.record()
            fn(*a, **kw)
            e1.record()
        return call

    for name in calls:
        setattr(sc.backend, name, timed(real[name]))
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        sc.step()
    sc._wait_pending()   # (an overlapped form: the last step's all-gather belongs to the timed region)
    fence()
    t1 = time.perf_counter()
    for name in calls:
        setattr(sc.backend, name, real[name])
    sc.sync()  # nb_launch_status: a kernel-reported failure fails the bench instead of timing garbage
    if dump is not None:
        outputs = {"positions": sc.positions(), "velocities": sc.velocities()}   # (world > 1: the velocities are gathered: every rank)
        if rank == 0:
            write_outputs(dump, outputs)
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    # (the overlapped ORDERED form launches its two phases through step_phase: no per-kernel events there, wall time only)
    kern_ms = sum(a.elapsed_time(b) for a, b in ev) / steps if sc.count and used[0] == len(ev) else 0.0
    kernels = ((["step_fast_ring_kernel", "ring_planes_kernel", "ring_reduce_kernel", "ring_finish_phase_kernel"] if sc.ring_overlap
                else ["step_fast_ring_kernel", "planes_kernel", "ring_reduce_kernel", "ring_finish_kernel"]) if sc.partners
               else step_kernels(nb, mode, sc.n, sc.count))
    each = [sum(a.elapsed_time(b) for a, b in ev[i * per_step:(i + 1) * per_step]) for i in range(steps)] if sc.count and used[0] == len(ev) else []
    out = {"elapsed_s": float(elapsed.item()), "kernel_ms": kern_ms, "kernel_ms_each": each, "count": sc.count, "n": sc.n, "steps": steps, "preheat_steps": pre,
           "kernels": kernels, "mode": "fast" if mode == nb.NB_MODE_FAST else "strict", "partners": sc.partners, "world": world,
           "ring_overlap": bool(sc.ring_overlap), "exchange_paths": exchange_paths, "form": form, "exchange": exchange}
    if parity:
        import numpy as np

        if mode == nb.NB_MODE_STRICT:
            # every step since the upload counts: preheat + warm-up + timed (+ the form choice restores its state)
            out["parity_check"] = parity_against_golden(sc.n, 1234, sc.steps_done, sc.positions(), sc.velocities())
        else:
            # FAST reassociates: one step of this very form against one STRICT step of the same state, on all bodies
            a = nb.ShardedScene(pos, vel, nb.default_params(mode=nb.NB_MODE_STRICT))
            b = nb.ShardedScene(pos, vel, params, ring=bool(sc.partners), ring_overlap=bool(sc.ring_overlap)) if sc.partners else nb.ShardedScene(pos, vel, params, ring=False)
            b.gather_in_place, b.ring_grouped = sc.gather_in_place, sc.ring_grouped
            a.step()
            b.step()
            pa, pb, va, vb = a.positions(), b.positions(), a.velocities(), b.velocities()
            scale = float(np.abs(va - vel).max())
            out["parity_check"] = {"k": 1, "bits_equal": None, "max_abs_dr": float(np.abs(pa - pb).max()), "max_abs_dv": float(np.abs(va - vb).max()),
                                   "max_abs_dv_over_max_dv": float(np.abs(va - vb).max() / scale) if scale > 0 else None,
                                   "within_tolerance": bool(np.abs(va - vb).max() <= 1e-3 * scale and np.abs(pa - pb).max() <= 1e-3 * scale + 1e-5),
                                   "against": "one STRICT step (= the reference's arithmetic, bit for bit) of the same initial state, all bodies; "
                                              "FAST is the same law reassociated: the worst body (a neighbour at r ~ 1e-4) is held to 1e-3 of the "
                                              "largest velocity change, as tests/test_gpu_ring.py holds it"}
            a.sync(); b.sync()
    sc.close()   # (the mappings of the other ranks' buffers, where the exchange is pulls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=131072, help="bodies (BASELINE: 131072)")
    ap.add_argument("--mode", choices=["strict", "fast"], default="strict",
                    help="arithmetic of the headline number: strict = bit-identical to the reference (default)")
    ap.add_argument("--preheat-ms", type=float, default=250.0,
                    help="untimed steps for this long in front of every leg's warm-up steps, until the clock ramp after the idle gap is over")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the informational legs (other mode, 3-D data, boids)")
    ap.add_argument("--no-ring", action="store_true",
                    help="multi-GPU FAST: keep the ordered fold with its one exchange per step instead of the pairs form on shards "
                         "(every unordered pair once, two exchanges per step)")
    ap.add_argument("--fast-form", choices=["auto", "pairs", "pairs_overlapped", "ordered"], default="auto",
                    help="multi-GPU --mode fast: the form a step takes -- auto (default): ShardedScene.choose_form times every form this "
                         "shape can take on this machine and the timed region runs the fastest; or name one (ordered == --no-ring)")
    ap.add_argument("--exchange", choices=["auto", "collective", "peers"], default="auto",
                    help="multi-GPU: how the ranks exchange -- collective: RCCL's all-gather (and grouped send / receive) through "
                         "torch.distributed; peers: pulls over xGMI ordered by stream value waits (nb_peers_*: IPC-mapped buffers, no "
                         "collective kernel); auto (default): both are verified on a pattern and timed on this machine, the faster runs")
    ap.add_argument("--overlap-leg", action="store_true",
                    help="multi-GPU only: also time FAST with the exchange overlapped (ShardedScene(overlap=True)); off by default "
                         "so that nothing untried on hardware can cost the scaling run its exit code")
    ap.add_argument("--aux-timeout", type=float, default=180.0,
                    help="seconds the informational legs (other mode, 3-D data, boids, CPU baseline) may take before the headline "
                         "is printed without them and the run exits 3")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also everything else: the line's parity check, the other mode, 3-D data, boids, the "
                         "unpreheated legs, the drop-in calls, the issue-ceiling streams, the CPU baseline (off: the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the positions and velocities the last timed step left as DIR/positions.npy and DIR/velocities.npy "
                         "(float32; above 64 MB in all, a fixed seeded sample of the rows)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # Started bare with --gpus N: run the N ranks as CHILD processes of a parent that never touches the GPU (no torch
        # import, no HIP call here; nothing is exec'd over an initialised process), relay their output -- rank 0 prints the
        # JSON line -- and leave with their exit code.
        import socket
        import subprocess

        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.run(cmd).returncode)

    import torch
    import torch.distributed as dist

    import nenbody_amd as nb

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: nenbody_amd has no CPU path")
    # NB_BENCH_BACKEND=gloo is a REHEARSAL mode for a one-GPU box (ranks share devices, positions are gathered
    # through the host): it exercises the multi-rank control flow, its numbers mean nothing.
    backend = os.environ.get("NB_BENCH_BACKEND", "nccl")
    device_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(device_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    # what the communicator saw: the backend, the world, how many DISTINCT devices the ranks sit on (their
    # UUIDs all-gathered: a rehearsal that shares one GPU says so), the collective library's version
    def device_uuid():
        try:
            return str(torch.cuda.get_device_properties(device_index).uuid)
        except Exception:   # (a torch without the attribute: the device's index and name still tell ranks on one GPU apart from ranks on eight)
            return f"{os.uname().nodename}:{device_index}:{torch.cuda.get_device_name(device_index)}"

    uuids = [device_uuid()]
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, uuids[0])
        uuids = gathered
    try:
        ccl = ".".join(str(x) for x in torch.cuda.nccl.version())
    except Exception as e:
        ccl = f"unknown ({e.__class__.__name__})"
    comm = {"backend": (backend if world > 1 else None), "backend_is": "torch.distributed 'nccl' = RCCL on ROCm" if backend == "nccl" else
            "REHEARSAL backend (ranks may share devices; exchanges staged through the host)", "world": world,
            "distinct_devices": len(set(uuids)), "device_uuids": uuids, "rccl_version": ccl,
            "device": torch.cuda.get_device_name(device_index)}

    n = args.n
    pos, vel = nb.init_state(n, 1234)
    primary = nb.NB_MODE_STRICT if args.mode == "strict" else nb.NB_MODE_FAST
    # FAST on several GPUs: which form a step takes is decided by TIMING on this machine (the pairs form with its exchanges in sequence
    # or behind compute, or the ordered fold), after both exchanges were verified on a known pattern -- no multi-GPU box saw this code
    # before the driver's; --no-ring keeps the ordered fold outright
    if args.fast_form == "ordered":
        args.no_ring = True
    named = {"pairs": False, "pairs_overlapped": True}.get(args.fast_form)   # None: auto / ordered
    res = time_mode(nb, torch, dist, args, primary, rank, world, pos, vel, ring=False if args.no_ring else None, ring_overlap=named,
                    choose=primary == nb.NB_MODE_FAST and not args.no_ring and args.fast_form == "auto", parity=args.full,
                    dump=args.dump_outputs)

    headline_exchange = (res["exchange"] or {}).get("chosen", "collective") if world > 1 else None

    def summarise(r, data="planar"):
        steps_per_s = r["steps"] / r["elapsed_s"]
        kernel_s = r["kernel_ms"] * 1e-3
        fr = roofline_fractions(r["mode"], data, r["kernels"][0], r["n"], r["count"], r["kernel_ms"])
        nominal, evaluations, achieved, lane_ops, ex = fr["achieved_nominal"], fr["pair_evaluations_per_launch"], fr["achieved"], fr["lane_ops_per_s"], fr["executed_per_interaction"]
        traffic, source = committed_traffic(nb, r["kernels"], r["n"], r["count"])
        roof = {"bound": "fp32_valu", "achieved": achieved, "peak": PEAK_FP32_VECTOR_TFLOPS, "unit": "TFLOP/s",
                "frac": achieved / PEAK_FP32_VECTOR_TFLOPS,
                "frac_is": "18 flop (the reference's count per pair, src/main.rs:428-430) x the pair evaluations the launch EXECUTES "
                           "(pair_evaluations_per_launch) / kernel time, over the spec fp32 vector peak"
                           + (": this form evaluates an unordered pair once for both bodies, so it executes about half of the reference's "
                              "ordered evaluations; frac_nominal prices the reference's n^2 ordered pairs instead and may pass 1"
                              if evaluations != float(r["count"]) * r["n"] else ""),
                "frac_nominal": nominal / PEAK_FP32_VECTOR_TFLOPS, "achieved_nominal": nominal,
                "frac_executed": lane_ops / SPEC_LANE_OPS_PER_S,
                "frac_executed_is": "vector lane operations the kernel executes per second (executed_per_interaction: full-rate ops + "
                                    "reciprocals, per ordered pair of the reference) over the spec issue rate of one operation per lane per "
                                    "cycle (256 CUs x 128 lanes x 2.4 GHz = 7.86e13/s; an FMA counts once here, twice in the flop peak)",
                "pair_evaluations_per_launch": evaluations,
                "bound_note": "fp32 vector ALU (SURVEY.md 8d): an all-pairs fp32 fold is neither HBM- nor MFMA-bound; see 'hbm'",
                "traffic": traffic, "traffic_unit": "bytes/step (HBM, PMC)", "traffic_source": source,
                "algorithmic_bytes_per_launch": BYTES_PER_BODY_STEP * r["count"],
                "kernel": r["kernels"][0], "kernels_per_step": r["kernels"],
                "kernel_ms": r["kernel_ms"],
                "flop_per_interaction": FLOP_PER_INTERACTION, "interactions_per_launch": float(r["count"]) * r["n"],
                "executed_per_interaction": ex}
        if traffic is not None and kernel_s > 0:  # how far from the HBM roofline the same launch is
            gbps = traffic / kernel_s / 1e9
            roof["hbm"] = {"achieved": gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": gbps / PEAK_HBM_GBPS}
        return {
            "body_updates_per_s": n * steps_per_s,
            "interactions_per_s": float(n) * n * steps_per_s,
            "ms_per_step": 1e3 / steps_per_s,
            "kernel_ms": r["kernel_ms"],
            "roofline": roof,
        }

    s = summarise(res)
    line = {
        "metric": f"body-updates/sec (N x steps/s) at N={n}, all-pairs gravity + Euler step",
        "value": s["body_updates_per_s"],
        "unit": "body-updates/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "preheat": {"ms": args.preheat_ms, "steps": res["preheat_steps"],
                    "what": "untimed steps in front of the warm-up steps of every leg, until the clock ramp that follows an idle gap is over "
                            "(--preheat-ms 0: none), then undone: the warm-up starts from the initial state; the timed region is exactly "
                            "`steps` steps"},
        "ms_per_step": s["ms_per_step"],
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic" if backend == "nccl" or world == 1 else "synthetic (REHEARSAL backend, not a measurement)",
        "config": {"workload": f"N={n} bodies, fp32, reference init distributions (seed 1234; planar: z = 0 as main.rs:740,745), "
                               "dt=0.1 G=0.001 bias=1e-7",
                   "mode": args.mode,
                   "sharding": f"index range x{world}, all-gather of positions per step" +
                               (f"; every unordered pair evaluated once, the halves of the {res['partners']} ranks in front leaving in a second, "
                                "point-to-point exchange per step" + ("; both exchanges behind compute (the step in phases)" if res["ring_overlap"] else "")
                                if res["partners"] else ""),
                   "tile": "library default"},
        "interactions_per_s": s["interactions_per_s"],
        "roofline": s["roofline"],
        "parity_check": res.get("parity_check"),
        "comm": dict(comm, exchange_paths=res["exchange_paths"], fast_form=res["form"], exchange=res["exchange"]),
        # BASELINE.json's north_star asks for >= 40 % of the fp32 roofline AND |dr| < 1e-4 against the reference after 1 000
        # steps.  The system is chaotic: only arithmetic identical to the reference's holds the second
        # line, and an exact binary32 divide costs 4 vector ops where the flop count says 1, which caps STRICT near 1/3.
        "targets": {"roofline_40pct_met_by": "fast", "parity_1000_steps_met_by": "strict", "both_met_by": None,
                    "note": "STRICT = the reference's arithmetic bit for bit (|dr| = 0 on every body after every one of 1 000 steps at this "
                            "size) at ~0.36 of the fp32 peak; FAST = same law reassociated, above 0.40 -- the system is chaotic, and at "
                            "N = 131 072 FAST's WORST body leaves |dr| < 1e-4 at step 2, the 99.9 % quantile at step 8, the median body at "
                            "about step 30 (at N = 1 024: all bodies within 1e-4 for 100-200 steps); a one-ulp change of one coordinate in "
                            "STRICT's own input diverges as fast (tests/test_gpu_parity.py)"},
    }

    # Everything after this point is informational, and runs with --full only.  If it wedges (a collective that never completes,
    # say), the headline measured above must still be reported -- and the run must NOT look clean: the watchdog prints the line
    # with the leg that was running and ends this rank with exit code 3.
    import threading

    leg = {"name": "start"}

    def give_up():  # pragma: no cover
        if rank == 0:
            line["aux_error"] = f"informational leg '{leg['name']}' did not finish within {args.aux_timeout} s"
            print(json.dumps(line), flush=True)
        os._exit(3)

    watchdog = threading.Timer(args.aux_timeout, give_up)
    watchdog.daemon = True
    if args.full:
        watchdog.start()

    if args.full and not args.no_secondary:
        other_mode = nb.NB_MODE_FAST if primary == nb.NB_MODE_STRICT else nb.NB_MODE_STRICT
        leg["name"] = "other_mode"
        try:
            # (multi-GPU: FAST as the ordered fold with its one exchange here; the pairs form on shards is a leg of its own below)
            o = summarise(time_mode(nb, torch, dist, args, other_mode, rank, world, pos, vel, ring=False, exchange_kind=headline_exchange))
            line["other_mode"] = {"mode": "fast" if primary == nb.NB_MODE_STRICT else "strict",
                                  "value": o["body_updates_per_s"], "ms_per_step": o["ms_per_step"], "roofline": o["roofline"]}
        except Exception as e:  # pragma: no cover
            line["other_mode"] = {"error": repr(e)}

        if world > 1 and not (primary == nb.NB_MODE_FAST and res["partners"] and not res["ring_overlap"]):
            leg["name"] = "fast_pairs_on_shards"
            try:
                r2 = time_mode(nb, torch, dist, args, nb.NB_MODE_FAST, rank, world, pos, vel, ring_overlap=False, exchange_kind=headline_exchange)
                if r2["partners"]:
                    o = summarise(r2)
                    line["fast_pairs_on_shards"] = {"what": "FAST, every unordered pair evaluated once across the ranks: a rank folds its bodies "
                                                            "against the half of the ring behind them, the other bodies' halves leave in a second "
                                                            "(point-to-point) exchange per step (nb_launch_ring_fold / nb_launch_ring_finish)",
                                                    "partners": r2["partners"], "value": o["body_updates_per_s"], "ms_per_step": o["ms_per_step"],
                                                    "roofline": o["roofline"]}
            except Exception as e:  # pragma: no cover
                line["fast_pairs_on_shards"] = {"error": repr(e)}

        if world > 1 and not (primary == nb.NB_MODE_FAST and res["ring_overlap"]):
            # the same with both exchanges behind compute (the step in phases: nb_launch_ring_fold_phase)
            leg["name"] = "fast_pairs_on_shards_overlapped"
            try:
                probe = nb.ShardedScene(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST))
                can = bool(probe.partners) and probe.backend.ring_phased(probe.params, probe.n, probe.first, probe.count)
                del probe
                if can:
                    r3 = time_mode(nb, torch, dist, args, nb.NB_MODE_FAST, rank, world, pos, vel, ring_overlap=True, exchange_kind=headline_exchange)
                    o = summarise(r3)
                    line["fast_pairs_on_shards_overlapped"] = {"what": "the pairs form on shards in phases: pairs inside the rank's own slot while the last "
                                                                       "step's all-gather lands, every other pair, the second exchange beside the reduce of the "
                                                                       "rank's own sums", "partners": r3["partners"], "value": o["body_updates_per_s"],
                                                               "ms_per_step": o["ms_per_step"], "kernel_ms": o["kernel_ms"]}
            except Exception as e:  # pragma: no cover
                line["fast_pairs_on_shards_overlapped"] = {"error": repr(e)}

        if world > 1 and not args.no_ring and primary != nb.NB_MODE_FAST:
            # which of the two FAST forms the MACHINE prefers: ShardedScene.choose_form times both on the state in hand (the slowest
            # rank's time counts) -- the answer a host gets when it asks instead of trusting the library's one-GPU line
            leg["name"] = "fast_form_chosen_by_timing"
            try:
                sc = nb.ShardedScene(pos, vel, nb.default_params(mode=nb.NB_MODE_FAST))
                if sc.partners:
                    preheat(sc.step, torch, dist, world, sc.device, args.preheat_ms)
                    chosen = sc.choose_form(steps=10, warm=3)
                    line["fast_form_chosen_by_timing"] = {"chosen": chosen, "partners": sc.partners,
                                                          "ms_per_step": {k_: 1e3 * v_ for k_, v_ in sc.form_times.items()},
                                                          "what": "ShardedScene.choose_form(steps=10): the pairs form (two exchanges per step) "
                                                                  "against the ordered fold (one), wall time of the slowest rank"}
                sc.sync()
                del sc
            except Exception as e:  # pragma: no cover
                line["fast_form_chosen_by_timing"] = {"error": repr(e)}

        # what a leg costs WITHOUT the preheat: timed steps right behind the idle gap of a fresh scene, the clock ramp included -- and
        # shown: the kernel time of every one of the first launches, which falls to the preheated figure as the part brings its clock up
        leg["name"] = "unpreheated"
        try:
            cold = {}
            for name, mode in (("strict", nb.NB_MODE_STRICT), ("fast", nb.NB_MODE_FAST)):
                time.sleep(0.2)
                r0 = time_mode(nb, torch, dist, args, mode, rank, world, pos, vel, steps=5, preheat_ms=0.0,
                               ring=False if args.no_ring else None, exchange_kind=headline_exchange)
                cold[name] = {"ms_per_step": 1e3 * r0["elapsed_s"] / r0["steps"], "kernel_ms": r0["kernel_ms"]}
                time.sleep(0.2)
                ramp = time_mode(nb, torch, dist, args, mode, rank, world, pos, vel, steps=24 if mode == nb.NB_MODE_FAST else 12, warmup=0,
                                 preheat_ms=0.0, ring=False if args.no_ring else None, exchange_kind=headline_exchange)
                cold[name]["kernel_ms_by_launch_from_idle"] = [round(x, 4) for x in ramp["kernel_ms_each"]]
            line["unpreheated"] = {"what": f"the same legs with --preheat-ms 0: {args.warmup} warm-up + 5 timed steps behind the idle gap a fresh "
                                           "scene leaves (the part ramps its clock for 30-40 ms after such a gap); kernel_ms_by_launch_from_idle: the "
                                           "kernel time of each launch from the very first one after the gap (no warm-up) -- the same kernel, the "
                                           "same work, a rising clock: the difference to the headline is the part's, not the code's", "steps": 5, **cold}
        except Exception as e:  # pragma: no cover
            line["unpreheated"] = {"error": repr(e)}

        if args.overlap_leg and world > 1:
            leg["name"] = "fast_overlap"
            try:
                o = summarise(time_mode(nb, torch, dist, args, nb.NB_MODE_FAST, rank, world, pos, vel, overlap=True, exchange_kind=headline_exchange))
                line["fast_overlap"] = {"what": "FAST, each step folds the rank's own slot while the all-gather of the others is in "
                                                "flight (nb_launch_step_phase), then the rest",
                                        "value": o["body_updates_per_s"], "ms_per_step": o["ms_per_step"]}
            except Exception as e:  # pragma: no cover
                line["fast_overlap"] = {"error": repr(e)}

        # the same set with the planar shortcut switched off (NB_FORCE_3D=1): what 3-D data costs.  The reference's own
        # initial state is planar and stays planar (z = 0, vz = 0 is a fixed point of its arithmetic), which the headline rides.
        leg["name"] = "force_3d"
        try:
            os.environ["NB_FORCE_3D"] = "1"
            nb.reload_env()
            f3 = {}
            for name, mode in (("strict", nb.NB_MODE_STRICT), ("fast", nb.NB_MODE_FAST)):
                o = summarise(time_mode(nb, torch, dist, args, mode, rank, world, pos, vel, steps=max(3, min(args.steps, 10)), warmup=1,
                                        exchange_kind=headline_exchange), data="3d")
                f3[name] = {"ms_per_step": o["ms_per_step"], "value": o["body_updates_per_s"], "roofline_frac": o["roofline"]["frac"],
                            "executed_per_interaction": o["roofline"]["executed_per_interaction"]}
            line["force_3d"] = f3
        except Exception as e:  # pragma: no cover
            line["force_3d"] = {"error": repr(e)}
        finally:
            os.environ.pop("NB_FORCE_3D", None)
            nb.reload_env()

        # the boids controller (update_instance_boids, main.rs:443-526), same set and sharding
        leg["name"] = "boids_controller"
        try:
            sc = nb.ShardedScene(pos, vel)
            preheat(sc.step_boids, torch, dist, world, sc.device, args.preheat_ms)
            for _ in range(2):
                sc.step_boids()
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            bsteps = max(2, min(args.steps, 10))
            t0 = time.perf_counter()
            for _ in range(bsteps):
                sc.step_boids()
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            bt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=sc.device)
            if world > 1:
                dist.all_reduce(bt, op=dist.ReduceOp.MAX)
            line["boids_controller"] = {"metric": "body-updates/s, update_instance_boids (bit-exact)",
                                        "value": n * bsteps / float(bt.item()),
                                        "ms_per_step": 1e3 * float(bt.item()) / bsteps, "steps": bsteps,
                                        "pair_evaluations_per_s": float(n) * n * bsteps / float(bt.item()),
                                        "executed_per_pair": {"full_rate_ops": 14,
                                                              "note": "planar tiles whose velocities cannot fail the rule-3 test "
                                                                      "(the reference's constants: every tile); 21 when it is tested; each "
                                                                      "radius test is one fma with a clamp"}}
            if world > 1:
                # the opt-in split form (the reference's neighbour sets and counts, reassociated sums): what lets a small shard fill the chip
                for _ in range(3):
                    sc.step_boids(split=True)
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                for _ in range(bsteps):
                    sc.step_boids(split=True)
                torch.cuda.synchronize()
                dist.barrier()
                bt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=sc.device)
                dist.all_reduce(bt, op=dist.ReduceOp.MAX)
                line["boids_controller"]["split_form"] = {"what": "nb_launch_boids_step_split: the j range in slices, the reference's predicates and "
                                                                  "counts, sums added slice by slice (not bit-identical)",
                                                          "value": n * bsteps / float(bt.item()), "ms_per_step": 1e3 * float(bt.item()) / bsteps}
        except Exception as e:  # pragma: no cover
            line["boids_controller"] = {"error": repr(e)}

        if world == 1:
            # the per-frame drop-in calls at the reference's own sizes (entity_count = 100, main.rs:654; its stated ceiling
            # 2 048, main.rs:653): upload + one step + download of positions, velocities and model matrices, per call
            leg["name"] = "dropin_call_at_reference_sizes"
            try:
                import numpy as np

                lat = {}
                for m in (100, 2048):
                    p0, v0 = nb.init_state(m, 1234)
                    inst = np.zeros((m, 4, 4), np.float32)
                    row = {}
                    for name, fn in (("update_instance_nbody", nb.update_instance_nbody), ("update_instance_boids", nb.update_instance_boids)):
                        p, v = p0.copy(), v0.copy()
                        op, ov = np.zeros_like(p), np.zeros_like(v)
                        for _ in range(20):
                            fn(inst, p, op, v, ov)
                        t0 = time.perf_counter()
                        for _ in range(200):
                            fn(inst, p, op, v, ov)
                        row[name] = round((time.perf_counter() - t0) / 200 * 1e6, 1)
                    lat[str(m)] = row
                nb.update_release()
                line["dropin_call_us"] = {"unit": "microseconds per call (PCIe-inclusive; never `value`)", "entities": lat}
            except Exception as e:  # pragma: no cover
                line["dropin_call_us"] = {"error": repr(e)}

    if args.full and world == 1:
        # Last of the GPU legs: these streams load the vector ALU harder than any kernel here, and the part answers a
        # sustained load by lowering its clock for tens of milliseconds -- timed before the other legs they slow them down.
        leg["name"] = "measured_issue_ceiling"
        try:
            import ctypes

            rates, clocks = {}, {}
            for name, mix in (("fma", 0), ("mix", 1), ("pk_mix", 2), ("fma_distinct_sources", 3), ("fmac_distinct_sources", 4)):
                r, mhz = ctypes.c_double(), ctypes.c_double()
                nb._lib.check(nb.load().nb_selftest_valu_rate(mix, 0.05, ctypes.byref(r), ctypes.byref(mhz)))
                rates[name], clocks[name] = r.value, mhz.value
            # the clock the part holds under the two folds themselves (stamps inside the kernels: nb_diag_step_clock)
            held = {}
            for name, mode in (("strict", nb.NB_MODE_STRICT), ("fast", nb.NB_MODE_FAST)):
                mhz, cyc, kms = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
                pm = nb.default_params(mode=mode)
                try:   # (shapes whose kernel is not stamped -- block chain, LDS forms at small --n -- answer NB_ERR_UNSUPPORTED: keep the streams)
                    nb._lib.check(nb.load().nb_diag_step_clock(ctypes.byref(pm), n, 0.3, ctypes.byref(mhz), ctypes.byref(cyc), ctypes.byref(kms)))
                    held[name] = {"held_clock_mhz": mhz.value, "wave_cycles": cyc.value, "kernel_ms": kms.value}
                except nb.NbError as e:
                    held[name] = {"held_clock_mhz": None, "wave_cycles": None, "kernel_ms": None, "why": str(e)}
            ex = line["roofline"]["executed_per_interaction"]
            slots = ex["full_rate_ops"] + 4.0 * ex["v_rcp_f32"]   # a quarter-rate v_rcp_f32 takes the slots of four
            kernel_rate = slots * line["roofline"]["interactions_per_launch"] / (line["roofline"]["kernel_ms"] * 1e-3)
            simds = 256 * 4

            def cpi(rate, mhz, lane_ops_per_inst=1.0):  # shader cycles per wave-instruction per SIMD at the stamped clock
                return mhz * 1e6 / (rate / lane_ops_per_inst / 64.0 / simds) if rate > 0 and mhz > 0 else None

            hk = held[args.mode]
            if hk["held_clock_mhz"] is None:
                hk = {"held_clock_mhz": 0.0}
            line["roofline"]["measured_issue_ceiling"] = {
                "fma_stream_tflops": 2.0 * rates["fma"] / 1e12, "fma_stream_frac_of_spec_peak": 2.0 * rates["fma"] / 1e12 / PEAK_FP32_VECTOR_TFLOPS,
                "mix_stream_lane_ops_per_s": rates["mix"], "fma_stream_lane_ops_per_s": rates["fma"],
                "pk_mix_stream_lane_ops_per_s": rates["pk_mix"],
                "fma_distinct_sources_lane_ops_per_s": rates["fma_distinct_sources"],
                "fmac_distinct_sources_lane_ops_per_s": rates["fmac_distinct_sources"],
                "stream_held_clock_mhz": clocks,
                "stream_cycles_per_instruction_per_simd": {"fma": cpi(rates["fma"], clocks["fma"]), "mix": cpi(rates["mix"], clocks["mix"]),
                                                           "pk_mix": cpi(rates["pk_mix"], clocks["pk_mix"], 2.0),
                                                           "fma_distinct_sources": cpi(rates["fma_distinct_sources"], clocks["fma_distinct_sources"]),
                                                           "fmac_distinct_sources": cpi(rates["fmac_distinct_sources"], clocks["fmac_distinct_sources"])},
                "kernels_held_clock": held,
                "kernel_issue_slots_per_s": kernel_rate, "kernel_over_mix_stream": kernel_rate / rates["mix"],
                "kernel_over_pk_mix_stream": kernel_rate / rates["pk_mix"],
                # the same two ratios with the clock taken out: issue slots per shader cycle of the kernel over lane operations per
                # shader cycle of the stream, each at the clock stamped inside it
                "kernel_over_mix_stream_per_cycle": (kernel_rate / hk["held_clock_mhz"]) / (rates["mix"] / clocks["mix"]) if hk["held_clock_mhz"] and clocks["mix"] else None,
                "kernel_over_pk_mix_stream_per_cycle": (kernel_rate / hk["held_clock_mhz"]) / (rates["pk_mix"] / clocks["pk_mix"]) if hk["held_clock_mhz"] and clocks["pk_mix"] else None,
                "frac_at_held_clock": line["roofline"]["achieved"] / (PEAK_FP32_VECTOR_TFLOPS * hk["held_clock_mhz"] / 2400.0) if hk["held_clock_mhz"] else None,
                "what": "register-only streams of independent vector instructions on every SIMD (8 waves each), 50 ms each, in this "
                        "process after the timed legs: v_fma_f32 only (what the spec peak assumes), the folds' own mix of fma/add/mul/sub as "
                        "plain and as packed (v_pk_*, two lane operations each) instructions, and v_fma_f32 / v_fmac_f32 with source registers "
                        "of their own per chain (the plain fma stream shares two sources among its chains).  Every stream and both folds are "
                        "stamped with s_memtime and s_memrealtime inside the kernel: held_clock_mhz is the shader clock the part held under "
                        "that code (spec: 2400).  kernel_issue_slots_per_s = interactions/s x the issue slots the kernel executes per "
                        "interaction (full-rate ops + 4 per v_rcp_f32); kernel_over_*_stream says how close the kernel runs to what this "
                        "device issues for that kind of instruction, *_per_cycle the same per shader cycle; frac_at_held_clock prices the "
                        "headline against the spec peak scaled to the clock the kernel was actually given"}
        except Exception as e:  # pragma: no cover
            line["roofline"]["measured_issue_ceiling"] = {"error": repr(e)}

    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        leg["name"] = "cpu_baseline"
        import oracle  # cpu_baseline leg: the oracle is timed here, never used by the product path

        lim = oracle.cpu_limits()
        threads = lim["threads"]
        # how many cores' worth of work the threads really deliver: one thread against all of them on a small set
        ps, vs = pos[:32768], vel[:32768]
        oracle.run(ps[:2048], vs[:2048], 1, threads=threads)  # page the library in
        t0 = time.perf_counter()
        oracle.run(ps, vs, 1, threads=1)
        t_one = time.perf_counter() - t0
        thr0 = oracle.throttled_usec()
        t0 = time.perf_counter()
        oracle.run(ps, vs, 1, threads=threads)
        t_all = time.perf_counter() - t0
        t0 = time.perf_counter()
        oracle.run(pos, vel, 1, threads=threads)
        dt = time.perf_counter() - t0
        throttled = oracle.throttled_usec() - thr0
        batched = None
        try:  # the same arithmetic, eight bodies per AVX2 vector (bit-identical; not how the reference's loop is written)
            if oracle.load().nbo_batched_available():
                t0 = time.perf_counter()
                oracle.run(pos, vel, 1, threads=threads, batched=True)
                tb = time.perf_counter() - t0
                batched = {"value": n / tb, "seconds": tb,
                           "what": "the same step with eight bodies per AVX2 vector (bit-identical sums); informational: the reference's "
                                   "loop is one body per thread at a time, which is what `value` times"}
        except Exception as e:  # pragma: no cover
            batched = {"error": repr(e)}
        line["cpu_baseline"] = {"value": n / dt, "unit": "body-updates/s", "cores": threads, "kind": "port",
                                "sample": f"1 full step of the same N={n} workload ({n * n:.3e} interactions) on {threads} threads, "
                                          "C restatement of src/main.rs:404-441 (-O2 -ffp-contract=off)",
                                "seconds": dt, "threads": threads, "affinity_cpus": lim["affinity"],
                                "cgroup_quota_cores": lim["cgroup_quota_cores"],
                                "effective_cores": t_one / t_all if t_all > 0 else None,
                                "one_core_interactions_per_s": 32768.0 * 32768.0 / t_one,
                                "interactions_per_s_per_thread": float(n) * n / dt / threads,
                                "throttled_usec_during_run": throttled,
                                "calibration": f"N=32768, one step: 1 thread {t_one:.3f} s, {threads} threads {t_all:.3f} s",
                                "avx2_batched": batched}
    watchdog.cancel()
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    # a line whose own parity check failed is still printed -- and the run does not look clean
    pc = line.get("parity_check") or {}
    code = 4 if (pc.get("bits_equal") is False or pc.get("within_tolerance") is False) else 0
    why = str(((line.get("comm") or {}).get("exchange") or {}).get("why") or "")
    if "abandoned" in why:
        # the first contact of the pulls over xGMI hit its deadline on this rank: a stream of its own is still blocked behind a word that
        # never became visible, and the runtime's teardown would wait for it -- leave without it (everything is printed and flushed)
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(code)
    if code:
        raise SystemExit(code)


if __name__ == "__main__":
    main()
