"""The per-thread plan caches of the stateless launch API (nb_api.hip: PlanCache; 4 whole-step plans, 2 two-phase plans, 2 ring
plans): a walk over more shapes than any of them holds gives the answers of the uncached planner -- on the first visit, on a
repeat (entries hit, evicted and made again) and after the overrides were read again (every entry's generation is stale).
Host arithmetic only; the cached entries are reached through calls that stop before the device."""
import ctypes

from nenbody_amd import _lib

A, B, C, D = 0x100000, 0x200000, 0x300000, 0x400000   # fake device addresses: never dereferenced, validation fails first

# (n_total, first, count): equal ranks, so that the ring plan has something to say; eight shapes, twice the largest cache
SHAPES = [(65536, 0, 16384), (65536, 16384, 16384), (131072, 0, 16384), (131072, 65536, 32768), (4096, 0, 1024), (8192, 4096, 4096),
          (65536, 32768, 32768), (262144, 0, 32768)]


def walk(lib, fast):
    """every answer the walk gives, in order"""
    out = []
    for n, first, count in SHAPES:
        plan = ctypes.create_string_buffer(256)
        assert lib.nb_diag_plan(ctypes.byref(fast), n, count, plan, len(plan)) == _lib.NB_OK
        need = lib.nb_scratch_bytes(ctypes.byref(fast), n, count)                      # uncached: make_plan itself
        partners = lib.nb_ring_partners(ctypes.byref(fast), n, first, count)           # the ring cache
        phased = lib.nb_ring_phased(ctypes.byref(fast), n, first, count)
        ring_need = lib.nb_ring_scratch_bytes(ctypes.byref(fast), n, first, count)     # uncached: make_ring_plan itself
        assert partners >= 0 and phased in (0, 1)
        assert (partners > 0) == (ring_need > 0) and (not phased or partners > 0)
        # the whole-step cache: the plan nb_launch_step finds asks for the scratch the uncached planner names -- one byte less is refused
        # (the call with enough would go on to the device, so the walk keeps to shapes that need some)
        assert need > 0
        assert lib.nb_launch_step(ctypes.byref(fast), n, first, count, A, B, C, D, need - 1, None) == _lib.NB_ERR_INVALID
        assert _lib.last_error() == "nb_launch_step: scratch smaller than nb_scratch_bytes()"
        # the two-phase cache likewise
        need2 = lib.nb_scratch_bytes_phased(ctypes.byref(fast), n, count, first, first + count)
        assert need2 > 0
        assert lib.nb_launch_step_phase(ctypes.byref(fast), n, first, count, first, first + count, _lib.NB_PHASE_RANGE, A, B, C, D, need2 - 1,
                                        None) == _lib.NB_ERR_INVALID
        assert _lib.last_error() == "nb_launch_step_phase: scratch smaller than nb_scratch_bytes_phased()"
        # the ring cache behind a launch entry: its size check is the uncached size
        if partners:
            assert lib.nb_launch_ring_fold(ctypes.byref(fast), n, first, count, A, B, C, ring_need - 1, None) == _lib.NB_ERR_INVALID
            assert _lib.last_error() == "nb_launch_ring_fold: scratch smaller than nb_ring_scratch_bytes()"
        out.append((plan.value, need, need2, partners, phased, ring_need))
    return out


def test_cached_plans_are_the_uncached_ones_before_and_after_a_reload(nb):
    lib = _lib.load()
    fast = nb.default_params(mode=nb.NB_MODE_FAST)
    first = walk(lib, fast)
    assert any(p for _, _, _, p, _, _ in first) and any(not p for _, _, _, p, _, _ in first)   # both kinds of ring answer
    assert walk(lib, fast) == first               # entries hit, evicted, made again
    assert lib.nb_debug_reload_env() == _lib.NB_OK
    assert walk(lib, fast) == first               # every entry stale: all made again, the same
    strict = nb.default_params()                  # another parameter block for the same shape words is another key
    assert all(lib.nb_ring_partners(ctypes.byref(strict), n, f, c) == 0 for n, f, c in SHAPES)
    assert walk(lib, fast) == first


def test_a_reload_that_changes_a_knob_changes_the_cached_answer(nb, monkeypatch):
    lib = _lib.load()
    fast = nb.default_params(mode=nb.NB_MODE_FAST)
    n, first, count = SHAPES[0]
    assert lib.nb_ring_partners(ctypes.byref(fast), n, first, count) > 0
    monkeypatch.setenv("NB_RING", "0")            # (the fixture has the library read its overrides again)
    assert lib.nb_ring_partners(ctypes.byref(fast), n, first, count) == 0
    assert lib.nb_ring_scratch_bytes(ctypes.byref(fast), n, first, count) == 0
    monkeypatch.delenv("NB_RING")
    assert lib.nb_ring_partners(ctypes.byref(fast), n, first, count) > 0
