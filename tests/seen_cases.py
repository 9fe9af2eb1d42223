"""Inputs of the seen boids step's contract tests (tests/test_seen_lists_cpu.py, tests/test_gpu_seen_contract.py): the data on which
the three rules cut, the whole-set kernels' hostile battery (tests/test_gpu_boids.py) as (pos, vel, constants) cases, and the lists
that tell list order from index order.

TEST INFRASTRUCTURE.  The CPU file checks on these very arrays that the GPU tests can tell something; the GPU file feeds them to the
kernel.  Constants travel as the restatement's keywords (dt, r1, r2, r3, s1, s2, s3); `oracle_params` / `device_params` turn them
into the two C structs."""
import numpy as np

import seen_restatement as S
from test_gpu_boids import cloud

F = np.float32
NONE = S.NONE
PAD = 4                                                   # NaN records behind n_total: where every out-of-set entry points
FIELDS = {"dt": "dt", "r1": "rule_1_distance", "r2": "rule_2_distance", "r3": "rule_3_distance", "s1": "rule_1_scale",
          "s2": "rule_2_scale", "s3": "rule_3_scale"}
CUT = dict(r1=1500.0, r2=12.0, r3=2.0)                    # on cut_cloud data each rule holds for some seen pairs and fails for others
CHAIN = dict(r1=200.0, r2=10.0, r3=2.0)                   # the same for chain_state data


def oracle_params(oracle, **kw):
    p = oracle.boids_params()
    for k, val in kw.items():
        setattr(p, FIELDS[k], val)
    return p


def device_params(nb, tile=0, **kw):
    p = nb.default_boids_params(tile=tile)
    for k, val in kw.items():
        setattr(p, FIELDS[k], val)
    return p


def same_words(got, want):
    """every word equal, a NaN of the reference met by a NaN (payload and sign belong to the machine): (ok, rows that differ)"""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert g.shape == w.shape, (g.shape, w.shape)
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    return bool(ok.all()), np.nonzero(~ok.reshape(len(ok), -1).all(1))[0]


def cut_cloud(oracle, n, seed):
    """3-D positions over about +-75, velocity differences up to about 4"""
    pos, vel = cloud(oracle, n, seed)
    return pos, (vel * F(30)).astype(F)


def chain_state(oracle, n, seed):
    """the reference's planar initial state, drawn together and sped up: what Scene.eyes sees of it leaves every rule undecided"""
    pos, vel = oracle.init_state(n, seed)
    return (pos * F(0.3)).astype(F), (vel * F(30)).astype(F)


def bernoulli_mask(n, density, seed):
    return np.random.default_rng(seed).random((n, n)) < density


def predicate_shares(pos, vel, mask, r1, r2, r3):
    """over the seen pairs (e sees i, i != e): the shares for which rule 1, 2 and 3's test holds, and the number of pairs"""
    e, i = np.nonzero(mask & ~np.eye(len(pos), dtype=bool))
    d = pos[i] - pos[e]
    d2 = ((d * d)[:, 0] + (d * d)[:, 1]) + (d * d)[:, 2]
    w = vel[i] - vel[e]
    e2 = ((w * w)[:, 0] + (w * w)[:, 1]) + (w * w)[:, 2]
    return float((d2 < F(r1)).mean()), float((np.sqrt(d2) < F(r2)).mean()), float((np.sqrt(e2) < F(r3)).mean()), len(e)


# -- the whole-set battery, for full lists against the C oracle ---------------------------------------------------------------------------
def boundary_rows():
    """pairs exactly at, just inside and just outside rule 2's 5.0 and rule 1's sqrt(1000): test_boids_radius_boundaries_are_exact"""
    xs = [F(0)]
    x = F(5.0)
    for _ in range(6):
        x = np.nextafter(x, F(0))
    for _ in range(13):
        xs.append(x)
        x = np.nextafter(x, F(10))
    x = F(np.sqrt(1000.0))
    for _ in range(4):
        x = np.nextafter(x, F(0))
    for _ in range(9):
        xs.append(x)
        x = np.nextafter(x, F(100))
    pos = np.zeros((len(xs), 3), F)
    pos[:, 0] = xs
    pos[1::2, 1] = F(1e-4)
    vel = np.zeros_like(pos)
    vel[:, 0] = np.linspace(0, 0.05, len(xs), dtype=F)
    return pos, vel


CONSTANT_SETS = [(1.0, 3.0, 400.0), (2.5, 0.0, 1e9), (np.inf, 7.5, 0.5), (0.5, -1.0, np.nan)]            # (r3, r2, r1)
LIMIT_SETS = [(1e-20, 3e-40, 2e-20, 1e-19), (1e-12, 2e-24, 1.5e-12, 1e-11), (1e15, 2e30, 3e15, 5e15),     # (scale, r1, r2, r3)
              (3e18, 3.0e38, 1.5e19, 1.8e19), (1.0, 1000.0, 5.0, float("inf"))]
FULL_LIST_CASES = (["boundaries", "nonfinite"] + [f"constants{k}" for k in range(len(CONSTANT_SETS))]
                   + [f"limits{k}" for k in range(len(LIMIT_SETS))])


def full_list_case(oracle, name):
    """(pos, vel, constants) of one case of tests/test_gpu_boids.py's battery"""
    if name == "boundaries":
        return boundary_rows() + ({},)
    if name == "nonfinite":
        pos, vel = cloud(oracle, 300, seed=8)
        pos[10, 0] = np.inf
        pos[20, 1] = np.nan
        return pos, vel, {}
    k = int(name[-1])
    if name.startswith("constants"):          # a rule-3 radius that cuts, radii 0, -1, NaN and +inf
        r3, r2, r1 = CONSTANT_SETS[k]
        return cut_cloud(oracle, 800, 5) + (dict(r1=r1, r2=r2, r3=r3, dt=0.1, s2=0.2),)
    scale, r1, r2, r3 = LIMIT_SETS[k]         # subnormal and huge thresholds, d2 overflowing to +inf, an infinite radius
    rng = np.random.default_rng(7 + k)
    pos = (rng.uniform(-1, 1, (700, 3)) * scale).astype(F)
    vel = (rng.uniform(-1, 1, (700, 3)) * scale).astype(F)
    return pos, vel, dict(r1=r1, r2=r2, r3=r3)


def full_lists(rows, n):
    """0 .. n-1 for every one of `rows` bodies, stride n"""
    return np.full(rows, n, np.uint32), np.tile(np.arange(n, dtype=np.uint32), (rows, 1))


# -- lists that tell list order from index order -----------------------------------------------------------------------------------------
def order_lists(n, stride, seed):
    """ascending lists without duplicates of 8 .. stride - 1 bodies of the set each, NONE behind them"""
    rng = np.random.default_rng(seed)
    count = rng.integers(8, stride, n).astype(np.uint32)
    lists = np.full((n, stride), NONE, np.uint32)
    for e in range(n):
        lists[e, :count[e]] = np.sort(rng.choice(n, count[e], replace=False))
    return count, lists


def contract_variants(n, stride, seed):
    """name -> (count, lists): the base lists and what the header's contract says about order, duplicates, the clamp and the slots
    behind the count.  Out-of-set entries are n .. n + PAD - 1."""
    count, lists = order_lists(n, stride, seed)
    rng = np.random.default_rng(seed + 1)
    full = np.stack([rng.choice(n, stride, replace=False) for _ in range(n)]).astype(np.uint32)    # every slot a body of the set
    out = {"ascending": (count, lists)}
    perm = lists.copy()
    for e in range(n):
        perm[e, :count[e]] = rng.permutation(lists[e, :count[e]])
    out["permuted"] = (count, perm)
    dup = lists.copy()
    dup[np.arange(n), count] = lists[:, 0]                                   # count <= stride - 1: there is room
    out["duplicate appended"] = (count + np.uint32(1), dup)
    out["one entry repeated"] = (np.full(n, stride, np.uint32), np.repeat(((np.arange(n) + 7) % n).astype(np.uint32)[:, None], stride, 1))
    out["count above stride"] = (np.where(np.arange(n) % 2 == 0, stride + 1, 0xFFFFFFFF).astype(np.uint32), full)
    out["count zero"] = (np.zeros(n, np.uint32), full)
    behind = np.where(np.arange(stride)[None, :] < count[:, None], lists, full)
    out["valid ids behind the count"] = (count, behind.astype(np.uint32))
    mid = perm.copy()
    mid[np.arange(n), count // 2] = np.arange(n, dtype=np.uint32)            # the body itself
    mid[np.arange(n), count // 2 - 2] = (n + np.arange(n) % PAD).astype(np.uint32)   # a padding record
    mid[np.arange(n), count // 2 + 2] = np.uint32(n + PAD - 1)
    out["own index and padding in the middle"] = (count, mid)
    return out


def stride_one_lists(n, seed):
    """stride 1: counts 0, 1 and 5, entries of the set, the body itself, or a padding record"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n, n).astype(np.uint32)
    ids[::7] = np.arange(n, dtype=np.uint32)[::7]
    ids[3::11] = np.uint32(n + 1)
    return np.array([0, 1, 5], np.uint32)[rng.integers(0, 3, n)], ids[:, None]
