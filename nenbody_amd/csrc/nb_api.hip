// nb_api.hip -- the extern "C" boundary declared in include/nenbody.h.
//
// Host-side only: argument checking, launch-shape selection, device buffers of a context.  There is no
// CPU implementation of the step in this library: without a HIP device every compute call fails.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nenbody.h"
#include "../../include/nenbody_diag.h"
#include "nb_kernels.h"
#include "nb_plan.h"
#include "nb_eyes.h"
#include "nb_frame.h"
#include "nb_seen.h"
#include "nb_located.h"
#include "nb_scenes.h"
#define NB_SRGB_TABLE static const
#define NB_SRGB_WANT_DECODE
#include "nb_srgb_tables.h"
#undef NB_SRGB_WANT_DECODE
#undef NB_SRGB_TABLE

#define NB_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local std::string g_tls_error = "";

using nbp::DebugOverrides;
using nbp::floor_log2f;
using nbp::Form;
using nbp::Knob;
using nbp::PhasePlan;
using nbp::Plan;
using nbp::valid_tile;

// ---- diagnostic overrides -----------------------------------------------------------------------------------
// The parity tests pin every kernel form and the sweeps in tools/ time them; both do it through NB_* environment
// variables.  They are read ONLY after a diagnostic call has asked for it -- nb_debug_reload_env() or nb_diag_enable_env(1)
// (include/nenbody_diag.h; the test suite's fixtures and every script under tools/ make it): a host that merely loads the
// library is steered by nothing its environment happens to export (round 4; VERDICT r03 item 11: until then an inherited
// NB_TILE or NB_FAST_SL changed which kernels ran).  The one exception is NB_ROCTX, which is a feature for the host (tracing),
// not a kernel form.  No launch path calls getenv.
Knob read_knob(const char *name)
{
    Knob k;
    const char *s = std::getenv(name);
    if (s && *s) {
        k.set = true;
        k.v = (uint32_t)std::strtoul(s, nullptr, 10);
    }
    return k;
}

std::atomic<const DebugOverrides *> g_overrides{nullptr};
std::atomic<bool> g_env_enabled{false};  // nb_diag_enable_env / nb_debug_reload_env
// nb_diag_rccl_solo (include/nenbody_diag.h): the test suite's way to run the RCCL leg of a shard on a one-GPU box.  Not an
// environment variable: nothing a deployment inherits can turn a world of 8 into eight communicators of one.
std::atomic<bool> g_rccl_solo{false};
std::mutex g_overrides_mu;

const DebugOverrides *parse_overrides(uint32_t generation)
{
    DebugOverrides *d = new DebugOverrides();  // never freed: a handful per process at most (one, outside the test suite)
    d->generation = generation;
    d->roctx = read_knob("NB_ROCTX");
    if (!g_env_enabled.load(std::memory_order_relaxed)) return d;  // a bare load of the library: no kernel-form override is read
    for (const nbp::KnobName &k : nbp::kKnobNames) d->*k.knob = read_knob(k.name);
    return d;
}

const DebugOverrides &overrides()
{
    const DebugOverrides *d = g_overrides.load(std::memory_order_acquire);
    if (d) return *d;
    std::lock_guard<std::mutex> lock(g_overrides_mu);
    d = g_overrides.load(std::memory_order_acquire);
    if (!d) {
        d = parse_overrides(1);
        g_overrides.store(d, std::memory_order_release);
    }
    return *d;
}

// The planner itself is nb_plan.h (pure host arithmetic); here it meets the process's overrides and the kernels' own sizes.
int make_plan(const nb_params &p, uint32_t n_total, uint32_t count, Plan *out, std::string *err)
{
    return nbp::make_plan(p, n_total, count, overrides(), out, err);
}

struct KernelSizes {
    size_t planes_bytes(uint32_t n) const { return nbk::strict_bc_scratch_bytes(n); }
    uint32_t pairs_chunk(uint32_t n, uint32_t chunk) const { return nbk::fast_pairs_chunk(n, chunk); }
    uint32_t pairs_rows(uint32_t n, uint32_t w, uint32_t np) const { return nbk::fast_pairs_rows(n, w, np); }
    size_t pairs_scratch_floats(uint32_t n, uint32_t w, uint32_t np, uint32_t chunk) const { return nbk::fast_pairs_scratch_floats(n, w, np, chunk); }
};
size_t plan_scratch_bytes(const Plan &pl, uint32_t count) { return nbp::plan_scratch_bytes(pl, count, KernelSizes{}); }

// The launch API is stateless; a rank calls it with the same shape every step.  A few planned shapes per thread are kept (no lock:
// one thread drives one GPU), keyed by everything the planners read: the parameters, the shape words and the overrides'
// generation.  The key is compared with memcmp, so plan_key() zeroes it whole -- padding included -- before it fills it.
struct PlanKey {
    nb_params p;
    uint32_t shape[4];
    uint32_t generation;
};
PlanKey plan_key(const nb_params &p, uint32_t s0, uint32_t s1, uint32_t s2 = 0, uint32_t s3 = 0)
{
    PlanKey k;
    std::memset(&k, 0, sizeof(k));
    k.p = p;
    k.shape[0] = s0;
    k.shape[1] = s1;
    k.shape[2] = s2;
    k.shape[3] = s3;
    k.generation = overrides().generation;
    return k;
}
// N entries, replaced in turn.  get(): the cached value for `key`, else make(&value) -- kept only when it succeeds.
template <typename Key, typename Value, int N>
class PlanCache {
    struct Entry {
        bool valid = false;
        Key key;
        Value value;
    };
    Entry entries_[N];
    int next_ = 0;

public:
    template <typename Make>
    int get(const Key &key, const Value **out, Make make)
    {
        for (const Entry &e : entries_)
            if (e.valid && std::memcmp(&e.key, &key, sizeof(Key)) == 0) {
                *out = &e.value;
                return NB_OK;
            }
        Value v;
        int rc = make(&v);
        if (rc != NB_OK) return rc;
        Entry &e = entries_[next_];
        next_ = (next_ + 1) % N;
        e.valid = true;
        e.key = key;
        e.value = v;
        *out = &e.value;
        return NB_OK;
    }
};

int cached_plan(const nb_params &p, uint32_t n_total, uint32_t count, const Plan **out, std::string *err)
{
    thread_local PlanCache<PlanKey, Plan, 4> cache;
    return cache.get(plan_key(p, n_total, count), out, [&](Plan *pl) { return make_plan(p, n_total, count, pl, err); });
}

// ---- roctx ranges (tracing) -----------------------------------------------------------------
// NB_ROCTX=1: the step loops of the context and shard APIs are bracketed with roctx ranges ("nb_step", "nb_shard_step",
// "nb_shard_exchange", ...), which rocprofv3 --marker-trace puts on the timeline.  The library is loaded with dlopen at first
// use (librocprofiler-sdk-roctx.so, else libroctx64.so); without NB_ROCTX nothing is loaded and a range costs one branch.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
};
const Roctx *roctx_api()
{
    if (!overrides().roctx.on()) return nullptr;
    static const Roctx *api = [] {
        Roctx *r = new Roctx();
        void *h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_LOCAL);
        if (h) {
            r->push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
            r->pop = (int (*)())dlsym(h, "roctxRangePop");
        }
        return (const Roctx *)r;
    }();
    return (api->push && api->pop) ? api : nullptr;
}
struct RoctxRange {
    const Roctx *api;
    explicit RoctxRange(const char *name) : api(roctx_api())
    {
        if (api) (void)api->push(name);
    }
    ~RoctxRange()
    {
        if (api) (void)api->pop();
    }
    RoctxRange(const RoctxRange &) = delete;
    RoctxRange &operator=(const RoctxRange &) = delete;
};

// ---- sticky device status ------------------------------------------------------------------------------------
// One word per device, owned by the library, zero at allocation.  The block-chain kernel ORs 1 into it when a wave gave
// up waiting for its turn (its workgroup's outputs are NaN then).  check_device_status() -- called by every entry point
// that waits for the device -- turns a set word into NB_ERR_STATE and clears it.
constexpr int kMaxDevices = 64;
uint32_t *g_status_word[kMaxDevices] = {};
std::mutex g_status_mu;

int device_status_word(uint32_t **out, std::string *err)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        *err = std::string("nb: hipGetDevice failed: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    std::lock_guard<std::mutex> lock(g_status_mu);
    if (!g_status_word[dev]) {
        uint32_t *w = nullptr;
        e = hipMalloc((void **)&w, 64);
        if (e == hipSuccess) e = hipMemset(w, 0, 64);
        if (e != hipSuccess) {
            *err = std::string("nb: allocating the device status word failed: ") + hipGetErrorString(e);
            return e == hipErrorOutOfMemory ? NB_ERR_ALLOC : NB_ERR_HIP;
        }
        g_status_word[dev] = w;
    }
    *out = g_status_word[dev];
    return NB_OK;
}

// The caller has already waited for the work in question.  NB_OK, or NB_ERR_STATE (and the word cleared) if a kernel
// reported a failure through `w` since the last check.
int check_status_word(uint32_t *w, std::string *err)
{
    if (!w) return NB_OK;  // no block-chain launch yet
    uint32_t v = 0;
    hipError_t e = hipMemcpy(&v, w, sizeof(v), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        *err = std::string("nb: reading the device status word failed: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    if (v == 0u) return NB_OK;
    (void)hipMemset(w, 0, sizeof(v));
    *err = "nb: a STRICT block-chain workgroup gave up waiting for its turn (its outputs are NaN): the state is invalid; "
           "upload it again";
    return NB_ERR_STATE;
}

// the launch API's word: the current device's
int check_device_status(std::string *err)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return NB_OK;
    uint32_t *w;
    {
        std::lock_guard<std::mutex> lock(g_status_mu);
        w = g_status_word[dev];
    }
    return check_status_word(w, err);
}

// a context's / shard's own word (allocated at the first block-chain launch), so that one object's failure is not
// reported to another; `dirty` = a block-chain launch since the last check (keeps the check off paths that never use it)
struct StatusWord {
    uint32_t *w = nullptr;
    bool dirty = false;
};

int status_word_for_launch(StatusWord *sw, std::string *err)
{
    if (!sw->w) {
        hipError_t e = hipMalloc((void **)&sw->w, 64);
        if (e == hipSuccess) e = hipMemset(sw->w, 0, 64);
        if (e != hipSuccess) {
            *err = std::string("nb: allocating the status word failed: ") + hipGetErrorString(e);
            return e == hipErrorOutOfMemory ? NB_ERR_ALLOC : NB_ERR_HIP;
        }
    }
    sw->dirty = true;
    return NB_OK;
}

int check_status(StatusWord *sw, std::string *err)
{
    if (!sw->dirty) return NB_OK;
    sw->dirty = false;
    return check_status_word(sw->w, err);
}

// What every step launch fills alike: the buffers, the shape, the constants, every plan-derived word (nb_plan.h: plan_step_args), and a
// whole-set fold -- partial rows in `partial`, the whole set as the j range, no hole.  The phases name their own rows, range and hole;
// the ring launches read none of the three.
nbk::StepArgs step_args(const nb_params &p, const Plan &pl, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                        void *pos_out, void *vel, void *partial = nullptr)
{
    nbk::StepArgs a{};
    a.pos_in = (const float4 *)pos_in;
    a.pos_out = (float4 *)pos_out;
    a.vel = (float4 *)vel;
    a.partial = (float4 *)partial;
    a.n_total = n_total;
    a.first = first;
    a.count = count;
    a.dt = p.dt;
    a.G = p.G;
    a.bias = p.bias;
    a.j_count = n_total;
    a.hole_lo = 0xffffffffu;
    nbp::plan_step_args(pl, &a);
    return a;
}

// The one dispatch: nb_plan.h's visit_launch() names the launcher and its scalar arguments, this calls it.
struct Launchers {
    const nbk::StepArgs &a;
    void *scratch;
    uint32_t *status;
    hipStream_t s;
    hipError_t strict(uint32_t tile, uint32_t unroll, uint32_t lanes) const { return nbk::launch_strict(a, tile, unroll, lanes, s); }
    hipError_t strict_pc(uint32_t producers) const { return nbk::launch_strict_pc(a, producers, s); }
    hipError_t strict_bc() const { return nbk::launch_strict_bc(a, scratch, status, s); }
    hipError_t strict_sl(uint32_t shape) const { return nbk::launch_strict_sl(a, shape, scratch, s); }
    hipError_t fast(uint32_t tile, uint32_t ib, uint32_t groups, uint32_t slices) const { return nbk::launch_fast(a, tile, ib, groups, slices, s); }
    hipError_t fast_wave(uint32_t tile, uint32_t ib, uint32_t waves, uint32_t slices) const { return nbk::launch_fast_wave(a, tile, ib, waves, slices, s); }
    hipError_t fast_sl(uint32_t ib, uint32_t slices) const { return nbk::launch_fast_sl(a, ib, slices, scratch, s); }
    hipError_t fast_pairs(uint32_t w, uint32_t np, uint32_t chunk) const { return nbk::launch_fast_pairs(a, w, np, chunk, scratch, s); }
};
hipError_t launch_planned(const Plan &pl, const nbk::StepArgs &a, void *scratch, uint32_t *status, hipStream_t stream)
{
    return nbp::visit_launch(pl, Launchers{a, scratch, status, stream});
}

// A launcher's answer as a status: NB_ERR_HIP with `what` (the caller's own text, up to and including ": ") and the runtime's words.
// The string is built only for a failure.
int launch_status(hipError_t e, const char *what, std::string *err)
{
    if (e == hipSuccess) return NB_OK;
    *err = std::string(what) + hipGetErrorString(e);
    return NB_ERR_HIP;
}

int launch_step_planned(const nb_params &p, const Plan &pl, uint32_t n_total, uint32_t first, uint32_t count,
                        const void *pos_in, void *pos_out, void *vel, void *scratch, hipStream_t stream, std::string *err,
                        StatusWord *sw = nullptr)
{
    const nbk::StepArgs a = step_args(p, pl, n_total, first, count, pos_in, pos_out, vel, scratch);
    uint32_t *status = nullptr;
    if (nbp::form_info(pl.form).status_word) {
        int rc = sw ? status_word_for_launch(sw, err) : device_status_word(&status, err);
        if (rc != NB_OK) return rc;
        if (sw) status = sw->w;
    }
    hipError_t e = launch_planned(pl, a, scratch, status, stream);
    if (e == hipErrorNotSupported) {  // a launch shape only the diagnostic knobs can name, in a build without -DNB_LEGACY_FORMS
        *err = "nb: this launch shape is one of the legacy forms (NB_STRICT_PC / NB_STRICT_LANES / NB_STRICT_UNROLL / NB_STRICT_SL=2,3 / "
               "NB_FAST_WAVES / NB_FAST_GROUPS / NB_FAST_PAIRS_W): this library was built without them (make -C nenbody_amd/csrc legacy "
               "builds libnenbody_hip_legacy.so, which holds every form)";
        return NB_ERR_UNSUPPORTED;
    }
    return launch_status(e, "nb: kernel launch failed: ", err);
}

int check_device(std::string *err)
{
    static std::atomic<bool> seen{false};  // a device does not disappear; cache only the positive answer (any thread may ask)
    if (seen.load(std::memory_order_relaxed)) return NB_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        *err = std::string("nb: no HIP device available (") + (e == hipSuccess ? "0 devices" : hipGetErrorString(e)) +
               "); this library has no CPU path";
        return NB_ERR_NO_DEVICE;
    }
    seen.store(true, std::memory_order_relaxed);
    return NB_OK;
}

// Largest binary32 x >= 0 with sqrtf(x) < r (correctly rounded sqrt, as the reference's f32::sqrt), or -1 if there is
// none: then `sqrtf(d2) < r` <=> `d2 <= T` for every d2 (NaN fails both; sqrt and rounding are monotonic).
float sqrt_threshold(float r)
{
    if (!(r > 0.0f)) return -1.0f;  // r <= 0 or NaN: sqrt(d2) >= 0 is never below it
    uint32_t lo = 0u, hi = 0x7f7fffffu;  // bit patterns of +0 .. FLT_MAX: monotonic in value
    auto below = [&](uint32_t b) {
        float x;
        std::memcpy(&x, &b, 4);
        return std::sqrt(x) < r;
    };
    if (!below(lo)) return -1.0f;
    if (below(hi)) {
        float x;
        std::memcpy(&x, &hi, 4);
        return x;
    }
    while (hi - lo > 1u) {  // invariant: below(lo) && !below(hi)
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (below(mid))
            lo = mid;
        else
            hi = mid;
    }
    float x;
    std::memcpy(&x, &lo, 4);
    return x;
}

// Largest binary32 V >= 0 such that rule 3 (main.rs:497-498) holds for EVERY pair of velocities whose components all lie in
// [-V, V], or -1 if there is none.  |v_i - v_n| <= 2V per component (2V is representable, rounding is monotonic), so the
// squared distance as the reference rounds it, ((ex*ex) + (ey*ey)) + (ez*ez), is at most the same expression at
// ex = ey = ez = 2V; the bound is monotonic in V, so bisection over the bit patterns finds the largest V that keeps it <= t3.
float rule3_always_bound(float t3)
{
    if (!(t3 >= 0.0f)) return -1.0f;
    auto holds = [&](uint32_t b) {
        float v;
        std::memcpy(&v, &b, 4);
        const volatile float w = v + v;
        const volatile float q = w * w;
        const volatile float two = q + q;
        const volatile float bound = two + q;
        return bound <= t3;  // false when anything overflowed to +inf
    };
    uint32_t lo = 0u, hi = 0x7f7fffffu;
    if (!holds(lo)) return -1.0f;
    if (!holds(hi)) {
        while (hi - lo > 1u) {  // invariant: holds(lo) && !holds(hi)
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (holds(mid))
                lo = mid;
            else
                hi = mid;
        }
    } else {
        lo = hi;
    }
    float x;
    std::memcpy(&x, &lo, 4);
    return x;
}

// boids launch form (nb_kernels.h:launch_boids), by bodies per rank.  Measured at N = 131 072 (tools/sweep.py boidsshard,
// profiles/r02/boids_forms.log), ms per step for shards of 16 384 / 32 768 / 49 152 / 65 536 / 131 072 bodies:
//   1  producer/consumer                      1.43 / 2.28 / 3.44 / 4.14 / 8.0   (rounds of 512 workgroups of 64 bodies: steps, not a line)
//   3  chain split, two waves per 64 bodies   3.54 / 3.53 / 3.54 / 3.56 / 7.17  (one round of 256 workgroups up to 65 536 bodies; 7.3 beyond)
//   2  one lane per body, (x, y) packed       3.84 / 3.87 / 3.86 / 3.86 / 5.79  (a lone wave per SIMD is bound by its instruction count)
//   0  one lane per body                      4.81 / 4.82 / 4.83 / 4.84 / 4.96-5.3 (two waves per SIMD are bound by lane operations)
//   4  chain split packed                     3.88 / 3.90 / 3.90 / 3.91 / 7.85
// so: producer/consumer up to 48 K bodies, chain split up to 64 K, one lane per body above.
// NB_BOIDS_PC: 1 = producer/consumer, 2 / 3 = one lane per body packed / plain, 4 / 5 = chain split plain / packed,
// 0 = one lane per body, packed while the launch has at most one wave per SIMD.
uint32_t boids_form(uint32_t count)
{
    const Knob &k = overrides().boids_pc;
    if (k.set) return k.v == 1u ? 1u : k.v == 2u ? 2u : k.v == 3u ? 0u : k.v == 4u ? 3u : k.v == 5u ? 4u : (count <= 65536u ? 2u : 0u);
    return count <= 49152u ? 1u : count <= 65536u ? 3u : 0u;
}

int make_boids_args(const nb_boids_params &p, uint32_t n_total, uint32_t first, uint32_t count, nbk::BoidsArgs *out,
                    uint32_t *tile, std::string *err)
{
    if (n_total == 0 || count == 0 || (uint64_t)first + count > n_total) {
        *err = "nb: boids: need count > 0 and [first, first+count) inside n_total";
        return NB_ERR_INVALID;
    }
    const uint32_t t = p.tile ? p.tile : overrides().boids_tile.or_else(1024u);
    if (!valid_tile(t)) {
        *err = "nb: boids params.tile must be 0, 256, 512 or 1024";
        return NB_ERR_INVALID;
    }
    nbk::BoidsArgs a{};
    a.n_total = n_total;
    a.first = first;
    a.count = count;
    a.dt = p.dt;
    a.r1 = p.rule_1_distance;
    a.t2 = sqrt_threshold(p.rule_2_distance);
    a.t3 = sqrt_threshold(p.rule_3_distance);
    a.s1 = p.rule_1_scale;
    a.s2 = p.rule_2_scale;
    a.s3 = p.rule_3_scale;
    if (n_total >= (1u << 24)) {
        *err = "nb: boids: neighbour counts are kept in binary32 and need n_total < 2^24";
        return NB_ERR_UNSUPPORTED;
    }
    a.force_flags = overrides().boids_force.or_else(0u) & 7u;
    // the radius tests as single instructions (nb_boids.inc:boids_below): `x < T` needs T finite, positive and not tiny, so that
    // k = 2^(30 - e_T) and T * k are ordinary binary32 numbers; "nothing passes" (T <= 0) is the constant mask 0.  A radius
    // without such constants switches the masked form off for the step (flag 1: the select form, same bits).
    auto mask_consts = [](float T, float *k, float *tk) {
        if (!(T > 0.0f)) {  // T <= 0, -inf or NaN: x < T never holds for x >= 0
            *k = 0.0f;
            *tk = -1.0f;
            return true;
        }
        if (!std::isfinite(T) || T < 0x1p-90f) return false;
        const int e = floor_log2f(T);
        *k = std::ldexp(1.0f, 30 - e);  // e in [-90, 127]: 2^-97 .. 2^120
        *tk = T * *k;                   // exact: a power-of-two scaling into [2^30, 2^31)
        return true;
    };
    auto above = [](float t) { return t < 0.0f ? -1.0f : std::nextafter(t, INFINITY); };  // x <= t  <=>  x < above(t)
    if (!mask_consts(a.r1, &a.mk.k1, &a.mk.tk1) || !mask_consts(above(a.t2), &a.mk.k2, &a.mk.tk2) ||
        !mask_consts(above(a.t3), &a.mk.k3, &a.mk.tk3)) {
        a.force_flags |= 1u;
        a.mk = nbk::BoidsMaskK{0.f, -1.f, 0.f, -1.f, 0.f, -1.f};
        a.mk_valid = 0u;
    } else {
        a.mk_valid = 1u;
    }
    const float v_lim = rule3_always_bound(a.t3);
    if (v_lim < 0.0f)
        a.force_flags |= 4u;  // no such bound (rule_3_distance <= 0 or NaN): always test
    else
        std::memcpy(&a.vlim_bits, &v_lim, 4);
    *out = a;
    *tile = t;
    return NB_OK;
}

// The split form of the boids step (nb_launch_boids_step_split): slices of the j range so that one lane per body per slice gives
// the chip two waves per SIMD (512 workgroups of four waves), whole tiles per slice.  NB_BOIDS_SLICES names the count (tests, tools/).
void boids_split_shape(uint32_t n_total, uint32_t count, uint32_t tile, uint32_t *slices, uint32_t *j_chunk)
{
    // (an empty rank -- count == 0 -- launches nothing; it still gets a shape, so that a host can size scratch for every rank alike)
    const uint32_t ntiles = (n_total + tile - 1u) / tile, groups = std::max(1u, (count + 255u) / 256u);
    uint32_t sl = overrides().boids_slices.or_else((512u + groups - 1u) / groups);
    if (sl < 1u) sl = 1u;
    if (sl > ntiles) sl = ntiles;
    if (sl > 64u) sl = 64u;
    const uint32_t per = (ntiles + sl - 1u) / sl;
    *slices = (ntiles + per - 1u) / per;  // no empty slice
    *j_chunk = per * tile;
}
// the slices' rows, then the per-1024-record velocity sums of the whole set, then the step's flag word
size_t boids_split_rows_bytes(uint32_t count, uint32_t slices) { return (size_t)slices * count * 3u * sizeof(float4); }
size_t boids_split_bytes(uint32_t n_total, uint32_t count, uint32_t slices)
{
    return boids_split_rows_bytes(count, slices) + (size_t)((n_total + 1023u) / 1024u) * sizeof(float4) + 64u;
}
void boids_split_pointers(nbk::BoidsArgs *a, void *scratch, uint32_t slices, uint32_t chunk)
{
    a->partial = (float4 *)scratch;
    a->j_chunk = chunk;
    a->vtot = (float4 *)((char *)scratch + boids_split_rows_bytes(a->count, slices));
    a->gflags = (uint32_t *)(a->vtot + (a->n_total + 1023u) / 1024u);
}

// Launch-API calls run on the device that owns the caller's buffers, not on whatever device happens to be current in
// this thread (one process per GPU normally makes them equal; a host that forgot hipSetDevice would otherwise launch on
// device 0 against another device's memory).
int select_device_of(const void *dev_ptr, std::string *err)
{
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, dev_ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return NB_OK;  // not a pointer the runtime knows (e.g. a test's fake address): leave the current device alone
    }
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != attr.device) {
        e = hipSetDevice(attr.device);
        if (e != hipSuccess) {
            *err = std::string("nb: hipSetDevice failed: ") + hipGetErrorString(e);
            return NB_ERR_HIP;
        }
    }
    return NB_OK;
}

// ---- the preamble of the stateless launch API ------------------------------------------------------------------------
nb_params params_or_default(const nb_params *params)
{
    nb_params p;
    if (params)
        p = *params;
    else
        nb_default_params(&p);
    return p;
}
nb_boids_params boids_params_or_default(const nb_boids_params *params)
{
    nb_boids_params p;
    if (params)
        p = *params;
    else
        nb_boids_default_params(&p);
    return p;
}

// A device is present, and the device that owns the caller's buffers (`anchor`: one of them) is current.  Two rules say when the
// library makes it so, and every entry keeps the rule it was written with:
//   kForNullStream  nb_launch_step, nb_launch_step_phase and the nb_launch_ring_* entries: a caller that brings a stream has made that
//                   stream's device current; the NULL stream says nothing about the device, so only then do the buffers decide.
//   kAlways         the boids, eyes, frame and seen entries: the buffers decide whatever the stream.
// (nb_launch_instances / _cameras / _random_step / _pack / _unpack select nothing: NB_LAUNCH_TLS asks for a device only.)
enum class SelectDevice { kForNullStream, kAlways };
int device_for_launch(const void *anchor, const void *stream, SelectDevice rule)
{
    int rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    if (rule == SelectDevice::kAlways || !stream) return select_device_of(anchor, &g_tls_error);
    return NB_OK;
}

uint64_t splitmix64(uint64_t &s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

float uniform_f32(uint64_t &s, float lo, float hi)
{
    const uint32_t bits24 = (uint32_t)(splitmix64(s) >> 40);
    const float u = (float)bits24 * 0x1.0p-24f;
    const float scale = hi - lo;
    const float v = scale * u;
    return lo + v;
}

}  // namespace

// A device buffer of a context (nb_ctx, nb_scenes): its pointer `p`, which the launches take, and its capacity in cells of T.  It is
// freed with the context and cannot be copied.  reserve(cells) does nothing while the buffer is large enough; otherwise it frees the
// buffer and allocates a larger one -- the contents are not carried over, and it never shrinks.  After a failure it is empty.  A
// buffer of a fixed size (vel_alt, cams, inst, frame_cam: allocated at first use) is reserved with that size at every use.
template <typename T>
struct DeviceBuffer {
    T *p = nullptr;
    size_t cells = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cells = 0;
    }
    hipError_t reserve(size_t want)
    {
        if (want <= cells) return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e == hipSuccess)
            cells = want;
        else
            p = nullptr;
        return e;
    }
    void swap(DeviceBuffer &other)
    {
        std::swap(p, other.p);
        std::swap(cells, other.cells);
    }
};

struct nb_ctx {
    uint32_t n = 0;
    nb_params p{};
    Plan plan{};
    hipStream_t stream = nullptr;
    DeviceBuffer<float4> pos[2];
    DeviceBuffer<float4> vel;
    DeviceBuffer<float4> vel_alt;  // second velocity buffer: boids reads every old velocity, so velocities ping-pong too
    DeviceBuffer<float> stage;     // 3n floats: stride-3 staging for upload/download
    DeviceBuffer<float4> inst;     // 4n float4, allocated on first use
    DeviceBuffer<float4> cams;     // 4n float4, allocated on first use (nb_cameras, nb_eyes)
    DeviceBuffer<uint32_t> eye_ids;  // nb_eyes' rows, allocated on first use and grown on demand: one word a column (a sample under 8 samples)
    DeviceBuffer<float> eye_depth;
    DeviceBuffer<float4> eye_rgba;   // nb_eyes_colour's rows, likewise: one record / one word a column
    DeviceBuffer<uint32_t> eye_bgra;
    DeviceBuffer<uint32_t> seen_count;  // nb_eyes_seen's and nb_step_boids_seen's lists, likewise: one count an eye, one slot a column
    DeviceBuffer<uint32_t> seen_ids;
    DeviceBuffer<float> seen_depth;
    DeviceBuffer<uint32_t> seen_cols;
    DeviceBuffer<uint32_t> loc_col;     // nb_eyes_located's and nb_step_nbody_located's located rows, likewise: one word / one record a slot
    DeviceBuffer<float4> loc_rel;
    DeviceBuffer<float> skin;        // nb_eyes_skin's texels (skin_w x skin_h x 4 floats); empty: the 1 x 1 white skin
    uint32_t skin_w = 0, skin_h = 0;
    DeviceBuffer<uint64_t> frame_keys;  // nb_frame's and nb_frame_msaa's key plane, grown on demand (their rows are the eye rows above)
    DeviceBuffer<float4> frame_cam;     // 6 float4: nb_frame's camera, then nb_camera_at's eye and direction records
    DeviceBuffer<float> xfer;    // 22n floats [matrices 16n | positions 3n | velocities 3n] and a tail: one-copy round trip of the drop-in calls
    float *hxfer = nullptr;   // its pinned host twin (hipHostMalloc: freed by the destructor below)
    float *hxfer_dev = nullptr;  // the device's address of hxfer (mapped host memory: kernels of the small-set drop-in read and write it directly)
    DeviceBuffer<uint32_t> done_counter;  // export_kernel's workgroup counter (ExportDone)
    uint32_t done_seq = 0, polled_calls = 0;
    uint32_t poll_holdoff = 0, poll_backoff = 0;  // calls that take the stream wait after a poll that timed out (wait_export)
    DeviceBuffer<char> scratch;
    StatusWord status;        // sticky failure word of this context's block-chain launches
    int cur = 0;
    bool uploaded = false;
    uint64_t steps = 0;
    std::string err;
    // what no DeviceBuffer holds: the pinned buffer and the status word (StatusWord is nb_shard's too)
    ~nb_ctx()
    {
        if (hxfer) (void)hipHostFree(hxfer);
        if (status.w) (void)hipFree(status.w);
    }
};

#define NB_HIP(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->err = std::string("nb: " #call " failed: ") + hipGetErrorString(e_);            \
            return (e_ == hipErrorOutOfMemory) ? NB_ERR_ALLOC : NB_ERR_HIP;                        \
        }                                                                                          \
    } while (0)

// A context entry's first checks, for nb_ctx and nb_scenes alike: the context is there (the text goes to the thread) and, where
// `state_hint` is given, it holds a state (the text goes to the context).  state_hint: what the entry's text has behind "no state
// uploaded" -- "", kCallUpload or kCallScenesUpload --; NULL: the entry needs no state, or checks its arguments first and calls again.
static const char kCallUpload[] = " (call nb_upload first)";
static const char kCallScenesUpload[] = " (call nb_scenes_upload first)";
template <typename Ctx>
static int ctx_check(Ctx *ctx, const char *fn, const char *state_hint = nullptr)
{
    if (!ctx) {
        g_tls_error = std::string(fn) + ": ctx is null";
        return NB_ERR_INVALID;
    }
    if (state_hint && !ctx->uploaded) {
        ctx->err = std::string(fn) + ": no state uploaded" + state_hint;
        return NB_ERR_STATE;
    }
    return NB_OK;
}

// the model matrices of the n records pos / vel on `stream`, into the context's `inst` (4n float4, allocated on first use)
static hipError_t launch_matrices(uint32_t n, const float4 *pos, const float4 *vel, DeviceBuffer<float4> *inst, hipStream_t stream)
{
    const hipError_t e = inst->reserve((size_t)n * 4);
    if (e != hipSuccess) return e;
    return nbk::launch_instances(n, pos, vel, inst->p, stream, overrides().inst_device_libm.on() ? 1u : 0u);
}

// a step of the context is enqueued: the position buffers flip, the velocity buffers swap where the step wrote vel_alt, and it counts
static void step_done(nb_ctx *c, bool wrote_vel_alt)
{
    c->cur ^= 1;
    if (wrote_vel_alt) c->vel.swap(c->vel_alt);
    c->steps++;
}

NB_EXPORT int nb_abi_version(void) { return NB_ABI_VERSION; }

NB_EXPORT void nb_default_params(nb_params *p)
{
    if (!p) return;
    p->dt = 0.1f;          // main.rs:411
    p->G = 0.001f;         // main.rs:412
    p->bias = 0.0000001f;  // main.rs:413
    p->tile = 0;
    p->mode = NB_MODE_STRICT;
}

NB_EXPORT int nb_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g_tls_error = std::string("nb: hipGetDeviceCount failed: ") + hipGetErrorString(e);
        return NB_ERR_NO_DEVICE;
    }
    return n;
}

NB_EXPORT const char *nb_last_error(const nb_ctx *ctx) { return ctx ? ctx->err.c_str() : g_tls_error.c_str(); }

NB_EXPORT int nb_init_state(uint64_t seed, uint32_t n, float *pos_xyz, float *vel_xyz)
{
    if (!pos_xyz || !vel_xyz) {
        g_tls_error = "nb_init_state: null array";
        return NB_ERR_INVALID;
    }
    uint64_t s = seed;
    for (uint32_t i = 0; i < n; ++i) {  // main.rs:738-742
        vel_xyz[3 * (size_t)i + 0] = uniform_f32(s, -0.0f, 0.1f);
        vel_xyz[3 * (size_t)i + 1] = uniform_f32(s, -0.0f, 0.1f);
        vel_xyz[3 * (size_t)i + 2] = 0.0f;
    }
    for (uint32_t i = 0; i < n; ++i) {  // main.rs:743-747
        pos_xyz[3 * (size_t)i + 0] = uniform_f32(s, -100.0f, 100.0f);
        pos_xyz[3 * (size_t)i + 1] = uniform_f32(s, -100.0f, 100.0f);
        pos_xyz[3 * (size_t)i + 2] = 0.0f;
    }
    return NB_OK;
}

NB_EXPORT void nb_destroy(nb_ctx *ctx)
{
    if (!ctx) return;
    const hipStream_t stream = ctx->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete ctx;  // frees its buffers: behind the wait, in front of the stream's end
    if (stream) (void)hipStreamDestroy(stream);
}

// Sets up to this size cross the bus as ONE pinned copy each way (they are all latency: every separate copy and wait
// shows); larger sets are all bandwidth and copy straight from / to the caller's arrays.  Measured: tools/crossover.py.
constexpr uint32_t kRoundtripMax = 16384;
// Small sets: the pack / unpack kernels read and write the pinned host buffer through the bus themselves instead of a DMA copy
// each way -- 7-14 us less per call at every size up to kRoundtripMax (tools/dropin_small.py, profiles/r02/dropin_small.log:
// N = 100 32.6 -> 25.6 us, N = 2 048 66.7 -> 52.8, N = 16 384 240 -> 226).  NB_DROPIN_ZERO_COPY=0 stages through DMA copies.
constexpr uint32_t kZeroCopyMax = kRoundtripMax;
static bool small_set_zero_copy(uint32_t n) { return overrides().dropin_zero_copy.or_else(n <= kZeroCopyMax ? 1u : 0u) != 0u; }

// after a small-set export whose kernel copied the status word behind the 22n floats of hxfer (and the wait)
static int status_from_tail(nb_ctx *c, bool with_status)
{
    if (!with_status) return NB_OK;
    uint32_t v;
    std::memcpy(&v, c->hxfer + 22 * (size_t)c->n, sizeof(v));
    if (v == 0u) {
        c->status.dirty = false;
        return NB_OK;
    }
    return check_status(&c->status, &c->err);  // reads it again, clears it, reports NB_ERR_STATE
}

// The smallest sets are ALL latency, the wait included: hipStreamSynchronize returns ~4 us after a kernel's last store has reached
// the host (tools/ubench_sync.hip, profiles/r04/ubench_sync.log: 12.5 against 8.3 us for launch + wait of an empty kernel).  So
// where the export kernel writes mapped host memory anyway, its last workgroup also writes a sequence number behind the
// results and the host polls that word: per call 28.4 -> 24.4 us at N = 100, 52.8 -> 49.6 at 2 048 (profiles/r04/dropin_small.log).
// Up to kPollMax bodies -- the reference's own ceiling (main.rs:653); from 4 096 bodies on the system-scope fences of the many
// workgroups cost more than the wait saves (72.6 -> 77.3 us).  A word that does not arrive within kPollBudget falls back to the
// stream wait, which also reports what went wrong.  NB_DROPIN_POLL=0: always the stream wait; =1: polled up to kZeroCopyMax.
constexpr uint32_t kPollMax = 2048;
constexpr size_t kDoneWordAt = 8;  // floats behind the 22n results (the status word is at 0)
static bool small_set_poll(uint32_t n) { return small_set_zero_copy(n) && overrides().dropin_poll.or_else(n <= kPollMax ? 1u : 0u) != 0u; }

static int ensure_xfer(nb_ctx *c)
{
    const size_t floats = (size_t)c->n * 22 + 16;  // + a tail: the status word and the completion word ride along
    NB_HIP(c, c->xfer.reserve(floats));
    if (!c->hxfer) {
        NB_HIP(c, hipHostMalloc((void **)&c->hxfer, floats * sizeof(float), hipHostMallocMapped));
        NB_HIP(c, hipHostGetDevicePointer((void **)&c->hxfer_dev, c->hxfer, 0));
        std::memset(c->hxfer + 22 * (size_t)c->n, 0, 16 * sizeof(float));
    }
    if (!c->done_counter.p) {
        NB_HIP(c, c->done_counter.reserve(1));
        NB_HIP(c, hipMemset(c->done_counter.p, 0, sizeof(uint32_t)));
    }
    return NB_OK;
}

// what export_kernel is to signal for this call (nothing unless the set is polled)
static nbk::ExportDone export_done(nb_ctx *c, bool polled)
{
    nbk::ExportDone d;
    if (polled && c->poll_holdoff) {  // the word kept the host spinning not long ago (wait_export): the stream wait for a while
        --c->poll_holdoff;
        polled = false;
    }
    if (polled) {
        d.counter = c->done_counter.p;
        d.word = (uint32_t *)(c->hxfer_dev + 22 * (size_t)c->n + kDoneWordAt);
        d.seq = ++c->done_seq ? c->done_seq : ++c->done_seq;  // never 0 (the word's initial value)
    }
    return d;
}

static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#else
    std::this_thread::yield();
#endif
}

// waits for the export launched last: the polled word, or the stream.  The poll is ADAPTIVE: a word that does not arrive within
// kPollBudget (the GPU is busy with something else -- the reference renders through the same device every frame, so the export
// kernel may routinely queue behind graphics work) costs that call the spin AND the stream wait, so the next 64 calls of the
// context go straight to the stream wait, twice as many after every further timeout (up to 4 096); a poll that succeeds
// resets the back-off.  The fallback also re-zeroes the workgroup counter: only the LAST workgroup of an export launch resets it,
// so a launch that died half way would leave every later polled call waiting for a count that never comes.
static int wait_export(nb_ctx *c, const nbk::ExportDone &d)
{
    if (d.word) {
        const volatile uint32_t *const w = (const volatile uint32_t *)(c->hxfer + 22 * (size_t)c->n + kDoneWordAt);
        const auto kPollBudget = std::chrono::microseconds(overrides().dropin_poll_budget_us.or_else(2000u));  // (the knob: tests)
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spins = 1;; ++spins) {
            if (*w == d.seq) {
                std::atomic_thread_fence(std::memory_order_acquire);
                c->poll_backoff = 0;
                // (now and then the runtime gets to see the stream idle: it retires its own bookkeeping at a wait)
                if ((++c->polled_calls & 1023u) == 0u) NB_HIP(c, hipStreamSynchronize(c->stream));
                return NB_OK;
            }
            if ((spins & 255u) == 0u && std::chrono::steady_clock::now() - t0 > kPollBudget) break;
            cpu_relax();
        }
        c->poll_backoff = c->poll_backoff ? std::min(c->poll_backoff * 2u, 4096u) : 64u;
        c->poll_holdoff = c->poll_backoff;
        NB_HIP(c, hipStreamSynchronize(c->stream));
        if (*w != d.seq) NB_HIP(c, hipMemsetAsync(c->done_counter.p, 0, sizeof(uint32_t), c->stream));  // (stream-ordered in front of the next export)
        return NB_OK;
    }
    NB_HIP(c, hipStreamSynchronize(c->stream));
    return NB_OK;
}

static int create_impl(nb_ctx *c)
{
    NB_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    NB_HIP(c, c->pos[0].reserve(c->n));
    NB_HIP(c, c->pos[1].reserve(c->n));
    NB_HIP(c, c->vel.reserve(c->n));
    NB_HIP(c, c->stage.reserve((size_t)c->n * 3));
    NB_HIP(c, c->scratch.reserve(plan_scratch_bytes(c->plan, c->n)));  // (none for most plans)
    return NB_OK;
}

NB_EXPORT int nb_create(uint32_t n, uint32_t n_devices, const nb_params *params, nb_ctx **out)
{
    if (!out) {
        g_tls_error = "nb_create: out is null";
        return NB_ERR_INVALID;
    }
    *out = nullptr;
    if (n_devices != 1) {
        g_tls_error =
            "nb_create: n_devices must be 1 (one process drives one GPU; shard with nb_launch_step and an all-gather)";
        return NB_ERR_UNSUPPORTED;
    }
    const nb_params p = params_or_default(params);
    Plan plan;
    int rc = make_plan(p, n, n, &plan, &g_tls_error);
    if (rc != NB_OK) return rc;
    rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    nb_ctx *c = new (std::nothrow) nb_ctx();
    if (!c) {
        g_tls_error = "nb_create: out of host memory";
        return NB_ERR_ALLOC;
    }
    c->n = n;
    c->p = p;
    c->plan = plan;
    rc = create_impl(c);
    if (rc != NB_OK) {
        g_tls_error = c->err;
        nb_destroy(c);
        return rc;
    }
    *out = c;
    return NB_OK;
}

// The two halves of a small set's round trip (n <= kRoundtripMax; ensure_xfer() has been called), shared by nb_upload / nb_download
// and the drop-ins (nb_dropin.inc: update_roundtrip).  hxfer and xfer hold [matrices 16n | positions 3n | velocities 3n | tail] on
// the way out and [positions 3n | velocities 3n] on the way in.

// The way in, enqueued and not waited for: the caller's arrays into hxfer, from there into pos[0] and vel.
static int small_import(nb_ctx *c, const float *pos_xyz, const float *vel_xyz)
{
    const size_t n = c->n, bytes = n * 3 * sizeof(float);
    std::memcpy(c->hxfer, pos_xyz, bytes);
    std::memcpy(c->hxfer + 3 * n, vel_xyz, bytes);
    float *src = c->hxfer_dev;  // the kernel reads the pinned buffer through the bus ...
    if (!small_set_zero_copy(c->n)) {  // ... or a DMA copy stages it in device memory first
        NB_HIP(c, hipMemcpyAsync(c->xfer.p, c->hxfer, 2 * bytes, hipMemcpyHostToDevice, c->stream));
        src = c->xfer.p;
    }
    NB_HIP(c, nbk::launch_import(c->n, src, src + 3 * n, c->pos[0].p, c->vel.p, c->stream));
    return NB_OK;
}

// The way out, up to "the parts wanted and the status are in hxfer" (one launch, one wait): the caller copies them out and reports
// status_from_tail(c, *with_status), in the order it owes its own caller.
static int small_export(nb_ctx *c, bool inst, bool pos, bool vel, bool *with_status)
{
    const size_t n = c->n;
    const bool zero_copy = small_set_zero_copy(c->n);
    float *const dst = zero_copy ? c->hxfer_dev : c->xfer.p;
    // the sticky status word of this context's block-chain launches comes home in the same buffer: no second wait
    const bool ws = *with_status = c->status.dirty && c->status.w;
    const nbk::ExportDone done = export_done(c, small_set_poll(c->n));
    NB_HIP(c, nbk::launch_export(c->n, c->pos[c->cur].p, c->vel.p, inst ? (float4 *)dst : nullptr, pos ? dst + 16 * n : nullptr,
                                 vel ? dst + 19 * n : nullptr, ws ? c->status.w : nullptr, ws ? (uint32_t *)(dst + 22 * n) : nullptr,
                                 c->stream, overrides().inst_device_libm.on() ? 1u : 0u, done));
    if (!zero_copy) {  // the floats from the first part wanted to the last one, in one DMA copy
        const size_t lo = inst ? 0 : (pos ? 16 * n : 19 * n), hi = ws ? 22 * n + 1 : vel ? 22 * n : (pos ? 19 * n : 16 * n);
        NB_HIP(c, hipMemcpyAsync(c->hxfer + lo, c->xfer.p + lo, (hi - lo) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    return wait_export(c, done);
}

NB_EXPORT int nb_upload(nb_ctx *ctx, const float *pos_xyz, const float *vel_xyz)
{
    int rc = ctx_check(ctx, "nb_upload");
    if (rc != NB_OK) return rc;
    if (!pos_xyz || !vel_xyz) {
        ctx->err = "nb_upload: null array";
        return NB_ERR_INVALID;
    }
    const size_t bytes = (size_t)ctx->n * 3 * sizeof(float);
    ctx->cur = 0;
    if (ctx->n <= kRoundtripMax) {  // one pinned copy, no wait: the stream orders it before the first step
        rc = ensure_xfer(ctx);
        if (rc != NB_OK) return rc;
        NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a download still reading hxfer must be done (it always is: downloads wait)
        rc = small_import(ctx, pos_xyz, vel_xyz);
        if (rc != NB_OK) return rc;
        NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // hxfer / xfer are reused by the next call
        ctx->uploaded = true;
        ctx->steps = 0;
        return NB_OK;
    }
    NB_HIP(ctx, hipMemcpyAsync(ctx->stage.p, pos_xyz, bytes, hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, nbk::launch_pack(ctx->n, ctx->stage.p, ctx->pos[0].p, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // stage is reused; the host array is not retained
    NB_HIP(ctx, hipMemcpyAsync(ctx->stage.p, vel_xyz, bytes, hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, nbk::launch_pack(ctx->n, ctx->stage.p, ctx->vel.p, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->uploaded = true;
    ctx->steps = 0;
    return NB_OK;
}

NB_EXPORT int nb_step(nb_ctx *ctx, uint32_t k)
{
    int rc = ctx_check(ctx, "nb_step", kCallUpload);
    if (rc != NB_OK) return rc;
    RoctxRange range("nb_step");
    for (uint32_t s = 0; s < k; ++s) {
        rc = launch_step_planned(ctx->p, ctx->plan, ctx->n, 0, ctx->n, ctx->pos[ctx->cur].p, ctx->pos[ctx->cur ^ 1].p, ctx->vel.p,
                                 ctx->scratch.p, ctx->stream, &ctx->err, &ctx->status);
        if (rc != NB_OK) return rc;
        step_done(ctx, false);
    }
    return NB_OK;
}

NB_EXPORT void nb_boids_default_params(nb_boids_params *p)
{
    if (!p) return;
    p->dt = 0.04f;                // main.rs:450
    p->rule_1_distance = 1000.0f; // main.rs:451
    p->rule_2_distance = 5.0f;    // main.rs:452
    p->rule_3_distance = 500.0f;  // main.rs:453
    p->rule_1_scale = 0.02f;      // main.rs:454
    p->rule_2_scale = 0.05f;      // main.rs:455
    p->rule_3_scale = 0.5f;       // main.rs:456
    p->tile = 0;
}

NB_EXPORT int nb_step_boids(nb_ctx *ctx, uint32_t k, const nb_boids_params *params)
{
    int rc = ctx_check(ctx, "nb_step_boids", kCallUpload);
    if (rc != NB_OK) return rc;
    const nb_boids_params p = boids_params_or_default(params);
    nbk::BoidsArgs a;
    uint32_t tile = 0;
    rc = make_boids_args(p, ctx->n, 0, ctx->n, &a, &tile, &ctx->err);
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, ctx->vel_alt.reserve(ctx->n));
    RoctxRange range("nb_step_boids");
    for (uint32_t s = 0; s < k; ++s) {
        a.pos_in = ctx->pos[ctx->cur].p;
        a.pos_out = ctx->pos[ctx->cur ^ 1].p;
        a.vel_in = ctx->vel.p;
        a.vel_out = ctx->vel_alt.p;
        NB_HIP(ctx, nbk::launch_boids(a, tile, boids_form(a.count), ctx->stream));
        step_done(ctx, true);
    }
    return NB_OK;
}

NB_EXPORT int nb_step_random(nb_ctx *ctx, uint32_t k, uint64_t seed)
{
    const int rc = ctx_check(ctx, "nb_step_random", kCallUpload);
    if (rc != NB_OK) return rc;
    for (uint32_t s = 0; s < k; ++s) {
        NB_HIP(ctx, nbk::launch_random(0, ctx->n, ctx->pos[ctx->cur].p, ctx->vel.p, seed, ctx->steps, ctx->stream));
        ctx->steps++;
    }
    return NB_OK;
}

NB_EXPORT int nb_device_state(nb_ctx *ctx, const void **pos_rec, const void **vel_rec, const void **inst_16n)
{
    const int rc = ctx_check(ctx, "nb_device_state", "");
    if (rc != NB_OK) return rc;
    if (inst_16n) {
        NB_HIP(ctx, launch_matrices(ctx->n, ctx->pos[ctx->cur].p, ctx->vel.p, &ctx->inst, ctx->stream));
        *inst_16n = ctx->inst.p;
    }
    if (pos_rec) *pos_rec = ctx->pos[ctx->cur].p;
    if (vel_rec) *vel_rec = ctx->vel.p;
    return NB_OK;
}

// The constant of a camera array: OPENGL_TO_WGPU_MATRIX * perspective(vertical_fov, aspect, near, far) (src/gfx.rs:12-17, 365,
// 367).  Host arithmetic only (one tanf per ARRAY, not per entity): cgmath 0.17's Deg -> Rad (deg * PI/180, the constant
// formed in binary64), PerspectiveFov -> Matrix4 (f = 1 / tan(fovy / 2); f / aspect, f, (far + near) / (near - far), -1,
// (2 far near) / (near - far)) and Matrix4 * Matrix4 (((a r0 + b r1) + c r2) + d r3 per entry), its assertions as an error.
NB_EXPORT int nb_camera_constant(float vertical_fov_deg, float aspect_ratio, float near_plane, float far_plane, float *cp16)
{
    if (!cp16) {
        g_tls_error = "nb_camera_constant: cp16 is null";
        return NB_ERR_INVALID;
    }
    const float pi = (float)3.14159265358979323846;
    const float fovy = vertical_fov_deg * (float)(3.14159265358979323846 / 180.0);
    if (!(fovy > 0.0f) || !(fovy < pi) || !(aspect_ratio != 0.0f) || !(near_plane > 0.0f) || !(far_plane > 0.0f) || !(far_plane != near_plane)) {
        g_tls_error = "nb_camera_constant: cgmath::perspective asserts 0 < fovy < 180 degrees, aspect != 0, near > 0, far > 0, far != near";
        return NB_ERR_INVALID;
    }
    const float f = 1.0f / std::tan(fovy / 2.0f);
    float proj[16] = {0.0f};  // column-major
    proj[0] = f / aspect_ratio;
    proj[5] = f;
    proj[10] = (far_plane + near_plane) / (near_plane - far_plane);
    proj[11] = -1.0f;
    proj[14] = ((2.0f * far_plane) * near_plane) / (near_plane - far_plane);
    const float corr[16] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.5f, 0.0f, 0.0f, 0.0f, 0.5f, 1.0f};  // src/gfx.rs:12-17
    for (int col = 0; col < 4; ++col)
        for (int row = 0; row < 4; ++row) {
            const float t0 = corr[row] * proj[4 * col], t1 = corr[4 + row] * proj[4 * col + 1];
            const float t2 = corr[8 + row] * proj[4 * col + 2], t3 = corr[12 + row] * proj[4 * col + 3];
            cp16[4 * col + row] = ((t0 + t1) + t2) + t3;
        }
    return NB_OK;
}

NB_EXPORT int nb_cameras(nb_ctx *ctx, const float *up_xyz, const float *cp16, float *out_16n)
{
    int rc = ctx_check(ctx, "nb_cameras");
    if (rc != NB_OK) return rc;
    if (!up_xyz || !cp16 || !out_16n) {
        ctx->err = "nb_cameras: null argument";
        return NB_ERR_INVALID;
    }
    rc = ctx_check(ctx, "nb_cameras", "");
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, ctx->cams.reserve((size_t)ctx->n * 4));
    NB_HIP(ctx, nbk::launch_cameras(ctx->n, ctx->pos[ctx->cur].p, ctx->vel.p, up_xyz, cp16, ctx->cams.p, ctx->stream));
    NB_HIP(ctx, hipMemcpyAsync(out_16n, ctx->cams.p, (size_t)ctx->n * 16 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

// [a, a + an) and [b, b + bn) share a byte (a NULL or empty range shares none)
static bool ranges_overlap(const void *a, size_t an, const void *b, size_t bn)
{
    if (!a || !b || !an || !bn) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

// What the eye and frame entries check before anything touches the device, the nb_launch_* variants included: first their own
// extent, range and flags (eyes_range_check / frame_extent_check), then their outputs (outputs_check).
struct ByteRange {
    const void *p;
    size_t bytes;
};

static const char kNoIdsDepth[] = ": ids and depth are both NULL";
static const char kNoColour[] = ": rgba and bgra8 are both NULL (ids and depth alone: nb_eyes / nb_launch_eyes)";
static const char kNoOutputs[] = ": ids, depth, rgba and bgra8 are all NULL";
static const char kNoOutputs8[] = ": ids8, depth8, rgba and bgra8 are all NULL";
static const char kEyesAlias[] = ": the outputs must not alias each other or an input";
static const char kFrameAlias[] = ": the outputs must not alias each other, an input or the scratch";

// the width (msaa: the 8-sample rows' limit), the range of eyes, the flags
static int eyes_range_check(const char *fn, uint32_t n, uint32_t first, uint32_t count, uint32_t width, bool msaa, uint32_t flags,
                            std::string *err)
{
    if (width == 0 || width > (msaa ? NB_EYES_MSAA_MAX_WIDTH : NB_EYES_MAX_WIDTH)) {
        *err = std::string(fn) + (msaa ? ": width must be 1 .. NB_EYES_MSAA_MAX_WIDTH (2048)" : ": width must be 1 .. NB_EYES_MAX_WIDTH (4096)");
        return NB_ERR_INVALID;
    }
    if ((uint64_t)first + count > n) {
        *err = std::string(fn) + ": eyes [first, first + count) exceed the set";
        return NB_ERR_INVALID;
    }
    if (flags & ~NB_EYES_SEE_SELF) {
        *err = std::string(fn) + ": unknown flag bits";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// the extent (msaa: the 8-sample frame's limit), the flags
static int frame_extent_check(const char *fn, uint32_t width, uint32_t height, bool msaa, uint32_t flags, std::string *err)
{
    const uint32_t max_dim = msaa ? NB_FRAME_MSAA_MAX_DIM : NB_FRAME_MAX_DIM;
    if (width == 0 || width > max_dim || height == 0 || height > max_dim) {
        *err = std::string(fn) + (msaa ? ": width and height must be 1 .. NB_FRAME_MSAA_MAX_DIM (2048)"
                                       : ": width and height must be 1 .. NB_FRAME_MAX_DIM (4096)");
        return NB_ERR_INVALID;
    }
    if (flags) {
        *err = std::string(fn) + ": flags must be 0";
        return NB_ERR_INVALID;
    }
    return NB_OK;
}

// The outputs of an entry (ids, depth, rgba, bgra8; the lists of a seen or located set; NULL: not wanted): one of those in `need`
// (bit a: out[a]) at least, or none_msg; 4-byte aligned where aligned4 asks for it; no two may overlap, and none may overlap one of
// the inputs `in` (a frame's scratch among them).
template <int N>
static int outputs_check(const char *fn, const ByteRange (&out)[N], uint32_t need, const char *none_msg, bool aligned4, const ByteRange *in,
                         int n_in, const char *alias_msg, std::string *err)
{
    uintptr_t bits = 0;
    bool any = false;
    for (int a = 0; a < N; ++a) {
        bits |= (uintptr_t)out[a].p;
        any = any || ((need >> a & 1u) && out[a].p);
    }
    if (!any) {
        *err = std::string(fn) + none_msg;
        return NB_ERR_INVALID;
    }
    if (aligned4 && (bits & 3u)) {
        *err = std::string(fn) + ": the outputs must be 4-byte aligned";
        return NB_ERR_INVALID;
    }
    for (int a = 0; a < N; ++a) {
        bool alias = false;
        for (int b = a + 1; b < N; ++b)
            alias = alias || (out[a].p && out[a].p == out[b].p) || ranges_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes);
        for (int b = 0; b < n_in; ++b) alias = alias || ranges_overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes);
        if (alias) {
            *err = std::string(fn) + alias_msg;
            return NB_ERR_INVALID;
        }
    }
    return NB_OK;
}

// The context's entries then read: check, stage, launch, download.  The three helpers below are their staging and their download,
// every operation on the context's stream in the order given.

// the context's output rows for the outputs wanted (a NULL host pointer: not wanted): `words` entries of ids and depth, `cells` of
// rgba and bgra8
static int grow_rows(nb_ctx *ctx, const void *ids, const void *depth, const void *rgba, const void *bgra8, size_t words, size_t cells)
{
    if (ids) NB_HIP(ctx, ctx->eye_ids.reserve(words));
    if (depth) NB_HIP(ctx, ctx->eye_depth.reserve(words));
    if (rgba) NB_HIP(ctx, ctx->eye_rgba.reserve(cells));
    if (bgra8) NB_HIP(ctx, ctx->eye_bgra.reserve(cells));
    return NB_OK;
}

// up_xyz given: the eye cameras of [first, first + count) as nb_cameras forms them; then the model matrices of the whole set as
// nb_download does (both allocated on first use, both formed afresh from the state in place)
static int stage_matrices(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16)
{
    if (up_xyz) {
        NB_HIP(ctx, ctx->cams.reserve((size_t)ctx->n * 4));
        NB_HIP(ctx, nbk::launch_cameras(count, ctx->pos[ctx->cur].p + first, ctx->vel.p + first, up_xyz, cp16, ctx->cams.p, ctx->stream));
    }
    NB_HIP(ctx, launch_matrices(ctx->n, ctx->pos[ctx->cur].p, ctx->vel.p, &ctx->inst, ctx->stream));
    return NB_OK;
}

// the rows to the host, for the outputs wanted, and the wait for them
static int download_rows(nb_ctx *ctx, uint32_t *ids, float *depth, float *rgba, uint32_t *bgra8, size_t words, size_t cells)
{
    if (ids) NB_HIP(ctx, hipMemcpyAsync(ids, ctx->eye_ids.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (depth) NB_HIP(ctx, hipMemcpyAsync(depth, ctx->eye_depth.p, words * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (rgba) NB_HIP(ctx, hipMemcpyAsync(rgba, ctx->eye_rgba.p, cells * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (bgra8) NB_HIP(ctx, hipMemcpyAsync(bgra8, ctx->eye_bgra.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

// What differs between the entries of one view body (the eyes' or the frame's; the context's or the stateless one's).
struct ViewForm {
    const char *fn;           // the entry's name, for its messages
    bool msaa;                // 8 samples a cell: the narrower limit, eight words a cell of ids and depth
    uint32_t need;            // the outputs of which one at least must be wanted (bit a: out[a]) ...
    const char *none_msg;     // ... and what to say otherwise
    bool aligned4;            // the outputs must be 4-byte aligned
    const char *align16_msg;  // stateless entries: what must be 16-byte aligned
};

// The context's eye entries: check, stage, launch, download.  `launch` is the entry's own launch on the context's rows and
// stream (its failure text names the call: NB_HIP).
template <typename Launch>
static int ctx_eyes(nb_ctx *ctx, const ViewForm &f, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width,
                    uint32_t flags, uint32_t *ids, float *depth, float *rgba, uint32_t *bgra8, Launch launch)
{
    int rc = ctx_check(ctx, f.fn);
    if (rc != NB_OK) return rc;
    if (!up_xyz || !cp16) {
        ctx->err = std::string(f.fn) + ": null argument";
        return NB_ERR_INVALID;
    }
    const size_t cells = (size_t)count * width, words = f.msaa ? cells * NB_EYES_SAMPLES : cells;
    const ByteRange in[2] = {{up_xyz, 3 * sizeof(float)}, {cp16, 16 * sizeof(float)}};
    const ByteRange out[4] = {{ids, words * 4u}, {depth, words * 4u}, {rgba, cells * 16u}, {bgra8, cells * 4u}};
    rc = eyes_range_check(f.fn, ctx->n, first, count, width, f.msaa, flags, &ctx->err);
    if (rc == NB_OK) rc = outputs_check(f.fn, out, f.need, f.none_msg, f.aligned4, in, 2, kEyesAlias, &ctx->err);
    if (rc == NB_OK) rc = ctx_check(ctx, f.fn, "");
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    rc = grow_rows(ctx, ids, depth, rgba, bgra8, words, cells);
    if (rc == NB_OK) rc = stage_matrices(ctx, first, count, up_xyz, cp16);
    if (rc == NB_OK) rc = launch();
    if (rc != NB_OK) return rc;
    return download_rows(ctx, ids, depth, rgba, bgra8, words, cells);
}

NB_EXPORT int nb_eyes(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width,
                      uint32_t flags, uint32_t *ids, float *depth)
{
    static const ViewForm f = {"nb_eyes", false, 0x3u, kNoIdsDepth, false, nullptr};
    return ctx_eyes(ctx, f, first, count, up_xyz, cp16, width, flags, ids, depth, nullptr, nullptr, [&]() -> int {
        NB_HIP(ctx, nbk::launch_eyes(ctx->n, first, count, (const float *)ctx->cams.p, (const float *)ctx->inst.p, width, flags,
                                     ids ? ctx->eye_ids.p : nullptr, depth ? ctx->eye_depth.p : nullptr, ctx->stream));
        return NB_OK;
    });
}

NB_EXPORT int nb_srgb_decode_table(float *out256)
{
    if (!out256) {
        g_tls_error = "nb_srgb_decode_table: null argument";
        return NB_ERR_INVALID;
    }
    memcpy(out256, kSrgbDecode, sizeof(kSrgbDecode));
    return NB_OK;
}

NB_EXPORT int nb_srgb_encode(const float *linear, size_t n, uint8_t *out)
{
    if (n && (!linear || !out)) {
        g_tls_error = "nb_srgb_encode: null argument";
        return NB_ERR_INVALID;
    }
    for (size_t i = 0; i < n; ++i) {   // the number of T[1..255] that are <= c: a NaN gives 0
        const float c = linear[i];
        uint32_t b = 0;
        for (uint32_t step = 128; step; step >>= 1)
            if (kSrgbEncodeT[b + step] <= c) b += step;
        out[i] = (uint8_t)b;
    }
    return NB_OK;
}

NB_EXPORT int nb_eyes_skin(nb_ctx *ctx, const float *rgba_linear, uint32_t tw, uint32_t th)
{
    const int rc = ctx_check(ctx, "nb_eyes_skin");
    if (rc != NB_OK) return rc;
    if (rgba_linear && (tw == 0 || th == 0 || tw > NB_EYES_MAX_SKIN || th > NB_EYES_MAX_SKIN)) {
        ctx->err = "nb_eyes_skin: tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)";
        return NB_ERR_INVALID;
    }
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (every eye call waits for its kernel: nothing reads the old skin any more)
    ctx->skin.release();                              // (a skin is as large as it says: none is kept for a smaller one)
    ctx->skin_w = ctx->skin_h = 0;
    if (!rgba_linear) return NB_OK;                   // back to the 1 x 1 white skin
    const size_t floats = (size_t)tw * th * 4;
    NB_HIP(ctx, ctx->skin.reserve(floats));
    NB_HIP(ctx, hipMemcpyAsync(ctx->skin.p, rgba_linear, floats * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->skin_w = tw, ctx->skin_h = th;
    return NB_OK;
}

// The colour row: a colour output at least.
NB_EXPORT int nb_eyes_colour(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width,
                             uint32_t flags, uint32_t *ids, float *depth, float *rgba, uint32_t *bgra8)
{
    static const ViewForm f = {"nb_eyes_colour", false, 0xCu, kNoColour, true, nullptr};
    return ctx_eyes(ctx, f, first, count, up_xyz, cp16, width, flags, ids, depth, rgba, bgra8, [&]() -> int {
        NB_HIP(ctx, nbk::launch_eyes_colour(ctx->n, first, count, (const float *)ctx->cams.p, (const float *)ctx->inst.p, width, flags, ctx->skin.p,
                                            ctx->skin_w, ctx->skin_h, ids ? ctx->eye_ids.p : nullptr, depth ? ctx->eye_depth.p : nullptr,
                                            rgba ? (float *)ctx->eye_rgba.p : nullptr, bgra8 ? ctx->eye_bgra.p : nullptr, ctx->stream));
        return NB_OK;
    });
}

NB_EXPORT int nb_eyes_sample_offsets(float *out8)
{
    if (!out8) {
        g_tls_error = "nb_eyes_sample_offsets: null argument";
        return NB_ERR_INVALID;
    }
    static_assert(NB_EYES_SAMPLES == 8, "nb_eyes.h lists eight");
    for (uint32_t k = 0; k < NB_EYES_SAMPLES; ++k) out8[k] = (float)nbk::kEyeSampleX16[k] / 16.0f;   // exact
    return NB_OK;
}

// The eye rows through 8 samples per column: the rows are the eye rows (one set of output rows
// per context), eight words a column for the samples.
NB_EXPORT int nb_eyes_msaa(nb_ctx *ctx, uint32_t first, uint32_t count, const float *up_xyz, const float *cp16, uint32_t width,
                           uint32_t flags, uint32_t *ids8, float *depth8, float *rgba, uint32_t *bgra8)
{
    static const ViewForm f = {"nb_eyes_msaa", true, 0xFu, kNoOutputs8, true, nullptr};
    return ctx_eyes(ctx, f, first, count, up_xyz, cp16, width, flags, ids8, depth8, rgba, bgra8, [&]() -> int {
        NB_HIP(ctx, nbk::launch_eyes_msaa(ctx->n, first, count, (const float *)ctx->cams.p, (const float *)ctx->inst.p, width, flags, ctx->skin.p,
                                          ctx->skin_w, ctx->skin_h, ids8 ? ctx->eye_ids.p : nullptr, depth8 ? ctx->eye_depth.p : nullptr,
                                          rgba ? (float *)ctx->eye_rgba.p : nullptr, bgra8 ? ctx->eye_bgra.p : nullptr, ctx->stream));
        return NB_OK;
    });
}

NB_EXPORT size_t nb_frame_scratch_bytes(uint32_t width, uint32_t height)
{
    if (width == 0 || width > NB_FRAME_MAX_DIM || height == 0 || height > NB_FRAME_MAX_DIM) return 0;
    return (size_t)width * height * sizeof(uint64_t);
}

NB_EXPORT int nb_camera_at(nb_ctx *ctx, const float *eye_xyz, const float *dir_xyz, const float *up_xyz, const float *cp16, float *out16)
{
    const int rc = ctx_check(ctx, "nb_camera_at");
    if (rc != NB_OK) return rc;
    if (!eye_xyz || !dir_xyz || !up_xyz || !cp16 || !out16) {
        ctx->err = "nb_camera_at: null argument";
        return NB_ERR_INVALID;
    }
    NB_HIP(ctx, ctx->frame_cam.reserve(6));
    // the eye and the direction as the 16-byte records the camera kernel reads, behind the camera's own four
    const float rec[8] = {eye_xyz[0], eye_xyz[1], eye_xyz[2], 0.0f, dir_xyz[0], dir_xyz[1], dir_xyz[2], 0.0f};
    NB_HIP(ctx, hipMemcpyAsync(ctx->frame_cam.p + 4, rec, sizeof(rec), hipMemcpyHostToDevice, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (rec is on the stack)
    NB_HIP(ctx, nbk::launch_cameras(1, ctx->frame_cam.p + 4, ctx->frame_cam.p + 5, up_xyz, cp16, ctx->frame_cam.p, ctx->stream));
    NB_HIP(ctx, hipMemcpyAsync(out16, ctx->frame_cam.p, 16 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NB_OK;
}

// the frame's own staging: the key plane (one per context, grown on demand) and the camera
static int stage_frame(nb_ctx *ctx, const float *cam16, size_t keys)
{
    NB_HIP(ctx, ctx->frame_keys.reserve(keys));
    NB_HIP(ctx, ctx->frame_cam.reserve(6));
    NB_HIP(ctx, hipMemcpyAsync(ctx->frame_cam.p, cam16, 16 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return NB_OK;
}

// The context's frame entries: check, stage, launch, download (as ctx_eyes; `keys`: the key plane's entries, one a sample).
template <typename Launch>
static int ctx_frame(nb_ctx *ctx, const ViewForm &f, const float *cam16, uint32_t width, uint32_t height, uint32_t flags, uint32_t *ids,
                     float *depth, float *rgba, uint32_t *bgra8, Launch launch)
{
    int rc = ctx_check(ctx, f.fn);
    if (rc != NB_OK) return rc;
    if (!cam16) {
        ctx->err = std::string(f.fn) + ": null argument";
        return NB_ERR_INVALID;
    }
    const size_t cells = (size_t)width * height, words = f.msaa ? cells * NB_EYES_SAMPLES : cells;
    const ByteRange in[1] = {{cam16, 16 * sizeof(float)}};
    const ByteRange out[4] = {{ids, words * 4u}, {depth, words * 4u}, {rgba, cells * 16u}, {bgra8, cells * 4u}};
    rc = frame_extent_check(f.fn, width, height, f.msaa, flags, &ctx->err);
    if (rc == NB_OK) rc = outputs_check(f.fn, out, f.need, f.none_msg, f.aligned4, in, 1, kFrameAlias, &ctx->err);
    if (rc == NB_OK) rc = ctx_check(ctx, f.fn, "");
    if (rc != NB_OK) return rc;
    rc = grow_rows(ctx, ids, depth, rgba, bgra8, words, cells);
    if (rc == NB_OK) rc = stage_frame(ctx, cam16, words);
    if (rc == NB_OK) rc = stage_matrices(ctx, 0, 0, nullptr, nullptr);
    if (rc == NB_OK) rc = launch();
    if (rc != NB_OK) return rc;
    return download_rows(ctx, ids, depth, rgba, bgra8, words, cells);
}

// The scene camera's frame: the rows are the eye rows, the key plane is the frame's own.
NB_EXPORT int nb_frame(nb_ctx *ctx, const float *cam16, uint32_t width, uint32_t height, uint32_t flags, uint32_t *ids, float *depth,
                       float *rgba, uint32_t *bgra8)
{
    static const ViewForm f = {"nb_frame", false, 0xFu, kNoOutputs, true, nullptr};
    return ctx_frame(ctx, f, cam16, width, height, flags, ids, depth, rgba, bgra8, [&]() -> int {
        NB_HIP(ctx, nbk::launch_frame(ctx->n, (const float *)ctx->frame_cam.p, (const float *)ctx->inst.p, width, height, ctx->skin.p, ctx->skin_w,
                                      ctx->skin_h, ctx->frame_keys.p, ids ? ctx->eye_ids.p : nullptr, depth ? ctx->eye_depth.p : nullptr,
                                      rgba ? (float *)ctx->eye_rgba.p : nullptr, bgra8 ? ctx->eye_bgra.p : nullptr, ctx->stream));
        return NB_OK;
    });
}

NB_EXPORT size_t nb_frame_msaa_scratch_bytes(uint32_t width, uint32_t height)
{
    if (width == 0 || width > NB_FRAME_MSAA_MAX_DIM || height == 0 || height > NB_FRAME_MSAA_MAX_DIM) return 0;
    return (size_t)width * height * NB_EYES_SAMPLES * sizeof(uint64_t);
}

NB_EXPORT int nb_frame_sample_offsets(float *out16)
{
    if (!out16) {
        g_tls_error = "nb_frame_sample_offsets: null argument";
        return NB_ERR_INVALID;
    }
    for (uint32_t k = 0; k < NB_EYES_SAMPLES; ++k) {   // exact
        out16[k] = (float)nbk::kEyeSampleX16[k] / 16.0f;
        out16[NB_EYES_SAMPLES + k] = (float)nbk::kFrameSampleY16[k] / 16.0f;
    }
    return NB_OK;
}

// The frame through 8 samples per pixel: the rows and the key plane are nb_frame's, eight words a pixel for
// the samples.
NB_EXPORT int nb_frame_msaa(nb_ctx *ctx, const float *cam16, uint32_t width, uint32_t height, uint32_t flags, uint32_t *ids8, float *depth8,
                            float *rgba, uint32_t *bgra8)
{
    static const ViewForm f = {"nb_frame_msaa", true, 0xFu, kNoOutputs8, true, nullptr};
    return ctx_frame(ctx, f, cam16, width, height, flags, ids8, depth8, rgba, bgra8, [&]() -> int {
        NB_HIP(ctx, nbk::launch_frame_msaa(ctx->n, (const float *)ctx->frame_cam.p, (const float *)ctx->inst.p, width, height, ctx->skin.p, ctx->skin_w,
                                           ctx->skin_h, ctx->frame_keys.p, ids8 ? ctx->eye_ids.p : nullptr, depth8 ? ctx->eye_depth.p : nullptr,
                                           rgba ? (float *)ctx->eye_rgba.p : nullptr, bgra8 ? ctx->eye_bgra.p : nullptr, ctx->stream));
        return NB_OK;
    });
}

NB_EXPORT int nb_sync(nb_ctx *ctx)
{
    const int rc = ctx_check(ctx, "nb_sync");
    if (rc != NB_OK) return rc;
    NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return check_status(&ctx->status, &ctx->err);
}

NB_EXPORT uint64_t nb_steps_done(const nb_ctx *ctx) { return ctx ? ctx->steps : 0; }

NB_EXPORT int nb_download(nb_ctx *ctx, float *pos_xyz, float *vel_xyz, float *inst_16n)
{
    int rc = ctx_check(ctx, "nb_download", "");
    if (rc != NB_OK) return rc;
    const size_t bytes = (size_t)ctx->n * 3 * sizeof(float);
    if (ctx->n <= kRoundtripMax && (pos_xyz || vel_xyz || inst_16n)) {  // [matrices 16n | positions 3n | velocities 3n], one copy, one wait
        rc = ensure_xfer(ctx);
        if (rc != NB_OK) return rc;
        const size_t n = ctx->n;
        bool with_status = false;
        rc = small_export(ctx, inst_16n != nullptr, pos_xyz != nullptr, vel_xyz != nullptr, &with_status);
        if (rc != NB_OK) return rc;
        if (inst_16n) std::memcpy(inst_16n, ctx->hxfer, n * 16 * sizeof(float));
        if (pos_xyz) std::memcpy(pos_xyz, ctx->hxfer + 16 * n, bytes);
        if (vel_xyz) std::memcpy(vel_xyz, ctx->hxfer + 19 * n, bytes);
        return status_from_tail(ctx, with_status);
    }
    if (pos_xyz) {
        NB_HIP(ctx, nbk::launch_unpack(ctx->n, ctx->pos[ctx->cur].p, ctx->stage.p, ctx->stream));
        NB_HIP(ctx, hipMemcpyAsync(pos_xyz, ctx->stage.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (vel_xyz) {
        NB_HIP(ctx, nbk::launch_unpack(ctx->n, ctx->vel.p, ctx->stage.p, ctx->stream));
        NB_HIP(ctx, hipMemcpyAsync(vel_xyz, ctx->stage.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (inst_16n) {
        NB_HIP(ctx, launch_matrices(ctx->n, ctx->pos[ctx->cur].p, ctx->vel.p, &ctx->inst, ctx->stream));
        NB_HIP(ctx, hipMemcpyAsync(inst_16n, ctx->inst.p, (size_t)ctx->n * 16 * sizeof(float), hipMemcpyDeviceToHost,
                                   ctx->stream));
        NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (!pos_xyz && !vel_xyz && !inst_16n) NB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return check_status(&ctx->status, &ctx->err);
}

#include "nb_dropin.inc"

#include "nb_selftest.inc"

// ---- launch API -----------------------------------------------------------------------------------------

NB_EXPORT size_t nb_scratch_bytes(const nb_params *params, uint32_t n_total, uint32_t count)
{
    const nb_params p = params_or_default(params);
    Plan pl;
    std::string err;
    if (make_plan(p, n_total, count, &pl, &err) != NB_OK) return 0;
    return plan_scratch_bytes(pl, count);
}

NB_EXPORT int nb_launch_step(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, const void *pos_in,
                             void *pos_out, void *vel, void *scratch, size_t scratch_bytes, void *stream)
{
    const nb_params p = params_or_default(params);
    if (!pos_in || !pos_out || !vel || pos_in == pos_out) {
        g_tls_error = "nb_launch_step: pos_in, pos_out, vel must be non-null and pos_out must not alias pos_in";
        return NB_ERR_INVALID;
    }
    if ((uint64_t)first + (uint64_t)count > (uint64_t)n_total) {
        g_tls_error = "nb_launch_step: [first, first+count) exceeds n_total";
        return NB_ERR_INVALID;
    }
    const Plan *pl = nullptr;
    int rc = cached_plan(p, n_total, count, &pl, &g_tls_error);
    if (rc != NB_OK) return rc;
    const size_t need = plan_scratch_bytes(*pl, count);
    if (need && (!scratch || scratch_bytes < need)) {
        g_tls_error = "nb_launch_step: scratch smaller than nb_scratch_bytes()";
        return NB_ERR_INVALID;
    }
    rc = device_for_launch(pos_in, stream, SelectDevice::kForNullStream);
    if (rc != NB_OK) return rc;
    return launch_step_planned(p, *pl, n_total, first, count, pos_in, pos_out, vel, scratch, (hipStream_t)stream, &g_tls_error);
}

NB_EXPORT int nb_launch_status(void *stream)
{
    int rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    // the status word is per device: ask about the device the stream belongs to, not whichever is current -- and leave the
    // caller's current device as it was (a host that drives several GPUs from one thread goes on allocating where it was)
    int cur = -1, restore = -1;
    if (stream) {
        hipDevice_t sdev = -1;
        if (hipStreamGetDevice((hipStream_t)stream, &sdev) == hipSuccess && hipGetDevice(&cur) == hipSuccess && sdev >= 0 && sdev != cur) {
            if (hipSetDevice(sdev) == hipSuccess) restore = cur;
        } else {
            (void)hipGetLastError();
        }
    }
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) {
        g_tls_error = std::string("nb_launch_status: hipStreamSynchronize failed: ") + hipGetErrorString(e);
        rc = NB_ERR_HIP;
    } else {
        rc = check_device_status(&g_tls_error);
    }
    if (restore >= 0) (void)hipSetDevice(restore);
    return rc;
}

// ---- a FAST step in two phases ("Overlap") -------------------------------------------------
namespace {
// the two-phase planner is nb_plan.h's too
int make_phase_plan(const nb_params &p, uint32_t n_total, uint32_t count, uint32_t j_lo, uint32_t j_hi, PhasePlan *out, std::string *err)
{
    return nbp::make_phase_plan(p, n_total, count, j_lo, j_hi, overrides(), out, err);
}
size_t phase_scratch_bytes(const PhasePlan &pp, uint32_t count) { return nbp::phase_scratch_bytes(pp, count, KernelSizes{}); }

// as cached_plan: a rank asks for the same two phases every step
int cached_phase_plan(const nb_params &p, uint32_t n_total, uint32_t count, uint32_t j_lo, uint32_t j_hi, const PhasePlan **out,
                      std::string *err)
{
    thread_local PlanCache<PlanKey, PhasePlan, 2> cache;
    return cache.get(plan_key(p, n_total, count, j_lo, j_hi), out,
                     [&](PhasePlan *pp) { return make_phase_plan(p, n_total, count, j_lo, j_hi, pp, err); });
}
}  // namespace

NB_EXPORT size_t nb_scratch_bytes_phased(const nb_params *params, uint32_t n_total, uint32_t count, uint32_t j_lo, uint32_t j_hi)
{
    const nb_params p = params_or_default(params);
    PhasePlan pp;
    std::string err;
    if (make_phase_plan(p, n_total, count, j_lo, j_hi, &pp, &err) != NB_OK) return 0;
    return phase_scratch_bytes(pp, count);
}

namespace {
// one phase of a FAST step on planned shapes (nb_launch_step_phase, nb_shard_step with the overlapped exchange)
int launch_phase_planned(const nb_params &p, const PhasePlan &pp, uint32_t n_total, uint32_t first, uint32_t count, uint32_t j_lo,
                         int phase, const void *pos_in, void *pos_out, void *vel, void *scratch, hipStream_t stream, std::string *err)
{
    nbk::StepArgs a = step_args(p, pp.base, n_total, first, count, pos_in, pos_out, vel);
    char *const rows = nbp::phase_sl(pp) ? nbk::plane_scratch(scratch, n_total).behind : (char *)scratch;  // the partial rows: behind the planes area
    a.partial = (float4 *)rows;
    a.always_partial = 1;
    // an ordered FAST fold of this plan with phase ph's slices / groups / chunk into its rows, or those rows zeroed where it folds nothing
    auto fold = [&](int ph, bool range, uint32_t r0, uint32_t r1) {
        a.j_count = pp.len[ph];
        a.j_chunk = pp.chunk[ph];
        a.partial_row0 = ph ? pp.slices[0] : 0u;
        if (!pp.len[ph]) return hipMemsetAsync(rows + (size_t)a.partial_row0 * count * sizeof(float4), 0, (size_t)pp.slices[ph] * count * sizeof(float4), stream);
        if (nbp::phase_sl(pp)) return nbk::launch_fast_sl_phase(a, pp.base.ib, pp.slices[ph], range, r0, r1, scratch, stream);
        Plan lds = pp.base;  // the tile or wave form, split as this phase is
        lds.groups = pp.groups[ph];
        lds.slices = pp.slices[ph];
        return launch_planned(lds, a, scratch, nullptr, stream);
    };
    hipError_t e = hipSuccess;
    if (phase == NB_PHASE_RANGE) {  // records [j_lo, j_lo + len[0]) -> partial rows [0, slices[0])
        a.j_base = j_lo;
        e = fold(0, true, j_lo, j_lo + pp.len[0]);
    } else {  // the set without that range -> rows [slices[0], slices[0] + slices[1]), then every row in order + integrate
        a.hole_lo = j_lo;
        a.hole_len = pp.len[0];
        e = fold(1, false, 0, 0);
        if (e == hipSuccess) e = nbk::launch_integrate_partials(a, pp.slices[0] + pp.slices[1], stream);
    }
    return launch_status(e, "nb: kernel launch failed (step phase): ", err);
}
}  // namespace

NB_EXPORT int nb_launch_step_phase(const nb_params *params, uint32_t n_total, uint32_t first, uint32_t count, uint32_t j_lo,
                                   uint32_t j_hi, int phase, const void *pos_in, void *pos_out, void *vel, void *scratch,
                                   size_t scratch_bytes, void *stream)
{
    const nb_params p = params_or_default(params);
    if (!pos_in || !pos_out || !vel || pos_in == pos_out || !scratch || (phase != NB_PHASE_RANGE && phase != NB_PHASE_REST)) {
        g_tls_error = "nb_launch_step_phase: pos_in, pos_out, vel, scratch must be non-null, pos_out must not alias pos_in, phase is "
                      "NB_PHASE_RANGE or NB_PHASE_REST";
        return NB_ERR_INVALID;
    }
    if ((uint64_t)first + (uint64_t)count > (uint64_t)n_total) {
        g_tls_error = "nb_launch_step_phase: [first, first+count) exceeds n_total";
        return NB_ERR_INVALID;
    }
    const PhasePlan *ppp = nullptr;
    int rc = cached_phase_plan(p, n_total, count, j_lo, j_hi, &ppp, &g_tls_error);
    if (rc != NB_OK) return rc;
    const PhasePlan &pp = *ppp;
    if (scratch_bytes < phase_scratch_bytes(pp, count)) {
        g_tls_error = "nb_launch_step_phase: scratch smaller than nb_scratch_bytes_phased()";
        return NB_ERR_INVALID;
    }
    rc = device_for_launch(pos_in, stream, SelectDevice::kForNullStream);
    if (rc != NB_OK) return rc;
    return launch_phase_planned(p, pp, n_total, first, count, j_lo, phase, pos_in, pos_out, vel, scratch, (hipStream_t)stream, &g_tls_error);
}

#include "nb_ring_api.inc"


// 1: this library holds every launch shape the diagnostic knobs can name (built with -DNB_LEGACY_FORMS: make legacy); 0: the product
// build, which holds the shapes make_plan reaches by itself
NB_EXPORT int nb_diag_legacy_forms(void)
{
#ifdef NB_LEGACY_FORMS
    return 1;
#else
    return 0;
#endif
}

NB_EXPORT int nb_diag_rccl_solo(int on)
{
    g_rccl_solo.store(on != 0, std::memory_order_relaxed);
    return NB_OK;
}

// The kernels one step of this shape launches, dominant one first, as the library itself plans it (bench.py labels its
// roofline with this instead of restating make_plan).
NB_EXPORT int nb_diag_plan(const nb_params *params, uint32_t n_total, uint32_t count, char *out, size_t out_bytes)
{
    if (!out || out_bytes == 0) {
        g_tls_error = "nb_diag_plan: out is null";
        return NB_ERR_INVALID;
    }
    const nb_params p = params_or_default(params);
    Plan pl;
    int rc = make_plan(p, n_total, count, &pl, &g_tls_error);
    if (rc != NB_OK) return rc;
    const std::string k = nbp::plan_kernels(pl, KernelSizes{});
    if (k.size() + 1 > out_bytes) {
        g_tls_error = "nb_diag_plan: out too small";
        return NB_ERR_INVALID;
    }
    std::memcpy(out, k.c_str(), k.size() + 1);
    return NB_OK;
}

namespace {
int reread_overrides(bool enable)
{
    std::lock_guard<std::mutex> lock(g_overrides_mu);
    g_env_enabled.store(enable, std::memory_order_relaxed);
    const DebugOverrides *old = g_overrides.load(std::memory_order_acquire);
    g_overrides.store(parse_overrides(old ? old->generation + 1u : 1u), std::memory_order_release);
    return NB_OK;
}
}  // namespace
NB_EXPORT int nb_diag_enable_env(int on) { return reread_overrides(on != 0); }
NB_EXPORT int nb_debug_reload_env(void) { return reread_overrides(true); }  // asking for a re-read is asking for the knobs

NB_EXPORT int nb_launch_boids_step(const nb_boids_params *params, uint32_t n_total, uint32_t first, uint32_t count,
                                   const void *pos_in, const void *vel_in, void *pos_out, void *vel_out, void *stream)
{
    const nb_boids_params p = boids_params_or_default(params);
    if (!pos_in || !vel_in || !pos_out || !vel_out || pos_in == pos_out || vel_in == vel_out) {
        g_tls_error = "nb_launch_boids_step: buffers must be non-null and the outputs must not alias the inputs";
        return NB_ERR_INVALID;
    }
    nbk::BoidsArgs a;
    uint32_t tile = 0;
    int rc = make_boids_args(p, n_total, first, count, &a, &tile, &g_tls_error);
    if (rc != NB_OK) return rc;
    rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    a.pos_in = (const float4 *)pos_in;
    a.vel_in = (const float4 *)vel_in;
    a.pos_out = (float4 *)pos_out;
    a.vel_out = (float4 *)vel_out;
    return launch_status(nbk::launch_boids(a, tile, boids_form(a.count), (hipStream_t)stream), "nb: boids kernel launch failed: ", &g_tls_error);
}

NB_EXPORT size_t nb_boids_split_scratch_bytes(const nb_boids_params *params, uint32_t n_total, uint32_t count)
{
    const nb_boids_params p = boids_params_or_default(params);
    nbk::BoidsArgs a;
    uint32_t tile = 0, slices = 0, chunk = 0;
    std::string err;
    if (count == 0u) return 0;  // a rank without bodies launches nothing
    if (make_boids_args(p, n_total, 0, count, &a, &tile, &err) != NB_OK) return 0;
    boids_split_shape(n_total, count, tile, &slices, &chunk);
    return boids_split_bytes(n_total, count, slices);
}

NB_EXPORT int nb_launch_boids_step_split(const nb_boids_params *params, uint32_t n_total, uint32_t first, uint32_t count,
                                         const void *pos_in, const void *vel_in, void *pos_out, void *vel_out, void *scratch,
                                         size_t scratch_bytes, void *stream)
{
    const nb_boids_params p = boids_params_or_default(params);
    if (!pos_in || !vel_in || !pos_out || !vel_out || !scratch || pos_in == pos_out || vel_in == vel_out) {
        g_tls_error = "nb_launch_boids_step_split: buffers must be non-null and the outputs must not alias the inputs";
        return NB_ERR_INVALID;
    }
    nbk::BoidsArgs a;
    uint32_t tile = 0, slices = 0, chunk = 0;
    int rc = make_boids_args(p, n_total, first, count, &a, &tile, &g_tls_error);
    if (rc != NB_OK) return rc;
    boids_split_shape(n_total, count, tile, &slices, &chunk);
    if (scratch_bytes < boids_split_bytes(n_total, count, slices)) {
        g_tls_error = "nb_launch_boids_step_split: scratch smaller than nb_boids_split_scratch_bytes()";
        return NB_ERR_INVALID;
    }
    rc = device_for_launch(pos_in, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    a.pos_in = (const float4 *)pos_in;
    a.vel_in = (const float4 *)vel_in;
    a.pos_out = (float4 *)pos_out;
    a.vel_out = (float4 *)vel_out;
    boids_split_pointers(&a, scratch, slices, chunk);
    return launch_status(nbk::launch_boids_split(a, tile, slices, (hipStream_t)stream), "nb: boids kernel launch failed (split form): ",
                         &g_tls_error);
}

// the small launches: a device is asked for, none is selected; the failure's text names the call
#define NB_LAUNCH_TLS(call)                                                   \
    do {                                                                      \
        int rc_ = check_device(&g_tls_error);                                 \
        if (rc_ != NB_OK) return rc_;                                         \
        return launch_status((call), "nb: " #call " failed: ", &g_tls_error); \
    } while (0)

NB_EXPORT int nb_launch_instances(uint32_t count, const void *pos, const void *vel, void *inst_16n, void *stream)
{
    if (!count || !pos || !vel || !inst_16n) {
        g_tls_error = "nb_launch_instances: bad argument";
        return NB_ERR_INVALID;
    }
    NB_LAUNCH_TLS(nbk::launch_instances(count, (const float4 *)pos, (const float4 *)vel, (float4 *)inst_16n, (hipStream_t)stream, overrides().inst_device_libm.on() ? 1u : 0u));
}

NB_EXPORT int nb_launch_cameras(uint32_t count, const void *eyes, const void *dirs, const float *up_xyz, const float *cp16,
                                void *out_16n, void *stream)
{
    if (!count || !eyes || !dirs || !up_xyz || !cp16 || !out_16n) {
        g_tls_error = "nb_launch_cameras: bad argument";
        return NB_ERR_INVALID;
    }
    NB_LAUNCH_TLS(nbk::launch_cameras(count, (const float4 *)eyes, (const float4 *)dirs, up_xyz, cp16, (float4 *)out_16n,
                                      (hipStream_t)stream));
}

// The stateless eye entries: every check, then the device of inst_16n, then `launch` (the entry's own nbk::launch_*).
// nb_launch_eyes passes no skin and no colour rows: NULL takes part in no check.
static const char kAlign16Eyes[] = ": cams_16 and inst_16n must be 16-byte aligned";
static const char kAlign16Colour[] = ": cams_16, inst_16n, skin and rgba must be 16-byte aligned";
static const char kAlign16Frame[] = ": cam_16, inst_16n, skin and rgba must be 16-byte aligned";
static const char kSkinExtent[] = ": tw and th must be 1 .. NB_EYES_MAX_SKIN (2048)";

template <typename Launch>
static int launch_eyes_form(const ViewForm &f, uint32_t n_total, uint32_t first, uint32_t count, const void *cams_16, const void *inst_16n,
                            uint32_t width, uint32_t flags, const void *skin, uint32_t tw, uint32_t th, void *ids, void *depth, void *rgba,
                            void *bgra8, void *stream, Launch launch)
{
    if (!cams_16 || !inst_16n) {
        g_tls_error = std::string(f.fn) + ": null argument";
        return NB_ERR_INVALID;
    }
    if (((uintptr_t)cams_16 | (uintptr_t)inst_16n | (uintptr_t)skin | (uintptr_t)rgba) & 15u) {
        g_tls_error = std::string(f.fn) + f.align16_msg;
        return NB_ERR_INVALID;
    }
    if (skin && (tw == 0 || th == 0 || tw > NB_EYES_MAX_SKIN || th > NB_EYES_MAX_SKIN)) {
        g_tls_error = std::string(f.fn) + kSkinExtent;
        return NB_ERR_INVALID;
    }
    const ByteRange in[3] = {{cams_16, (size_t)count * 16 * sizeof(float)}, {inst_16n, (size_t)n_total * 16 * sizeof(float)},
                             {skin, skin ? (size_t)tw * th * 4 * sizeof(float) : 0}};
    const size_t cells = (size_t)count * width, words = f.msaa ? cells * NB_EYES_SAMPLES : cells;
    const ByteRange out[4] = {{ids, words * 4u}, {depth, words * 4u}, {rgba, cells * 16u}, {bgra8, cells * 4u}};
    int rc = eyes_range_check(f.fn, n_total, first, count, width, f.msaa, flags, &g_tls_error);
    if (rc == NB_OK) rc = outputs_check(f.fn, out, f.need, f.none_msg, f.aligned4, in, 3, kEyesAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (count == 0) return NB_OK;
    rc = device_for_launch(inst_16n, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    return launch_status(launch(), "nb: eyes kernel launch failed: ", &g_tls_error);
}

// The stateless frame entries likewise; the device is the scratch's.
template <typename Launch>
static int launch_frame_form(const ViewForm &f, uint32_t n_total, const void *cam_16, const void *inst_16n, uint32_t width, uint32_t height,
                             uint32_t flags, const void *skin, uint32_t tw, uint32_t th, void *scratch, void *ids, void *depth, void *rgba,
                             void *bgra8, void *stream, Launch launch)
{
    if (!cam_16 || !scratch || (n_total && !inst_16n)) {
        g_tls_error = std::string(f.fn) + ": null argument";
        return NB_ERR_INVALID;
    }
    if (((uintptr_t)cam_16 | (uintptr_t)inst_16n | (uintptr_t)skin | (uintptr_t)rgba) & 15u) {
        g_tls_error = std::string(f.fn) + f.align16_msg;
        return NB_ERR_INVALID;
    }
    if ((uintptr_t)scratch & 7u) {
        g_tls_error = std::string(f.fn) + ": scratch must be 8-byte aligned";
        return NB_ERR_INVALID;
    }
    if (skin && (tw == 0 || th == 0 || tw > NB_EYES_MAX_SKIN || th > NB_EYES_MAX_SKIN)) {
        g_tls_error = std::string(f.fn) + kSkinExtent;
        return NB_ERR_INVALID;
    }
    const ByteRange in[4] = {{cam_16, 16 * sizeof(float)}, {inst_16n, (size_t)n_total * 16 * sizeof(float)},
                             {skin, skin ? (size_t)tw * th * 4 * sizeof(float) : 0},
                             {scratch, f.msaa ? nb_frame_msaa_scratch_bytes(width, height) : nb_frame_scratch_bytes(width, height)}};
    const size_t cells = (size_t)width * height, words = f.msaa ? cells * NB_EYES_SAMPLES : cells;
    const ByteRange out[4] = {{ids, words * 4u}, {depth, words * 4u}, {rgba, cells * 16u}, {bgra8, cells * 4u}};
    int rc = frame_extent_check(f.fn, width, height, f.msaa, flags, &g_tls_error);
    if (rc == NB_OK) rc = outputs_check(f.fn, out, f.need, f.none_msg, f.aligned4, in, 4, kFrameAlias, &g_tls_error);
    if (rc != NB_OK) return rc;
    rc = device_for_launch(scratch, stream, SelectDevice::kAlways);
    if (rc != NB_OK) return rc;
    return launch_status(launch(), "nb: frame kernel launch failed: ", &g_tls_error);
}

NB_EXPORT int nb_launch_eyes(uint32_t n_total, uint32_t first, uint32_t count, const void *cams_16, const void *inst_16n, uint32_t width,
                             uint32_t flags, void *ids, void *depth, void *stream)
{
    static const ViewForm f = {"nb_launch_eyes", false, 0x3u, kNoIdsDepth, false, kAlign16Eyes};
    return launch_eyes_form(f, n_total, first, count, cams_16, inst_16n, width, flags, nullptr, 0, 0, ids, depth, nullptr, nullptr, stream, [&] {
        return nbk::launch_eyes(n_total, first, count, (const float *)cams_16, (const float *)inst_16n, width, flags, (uint32_t *)ids,
                                (float *)depth, (hipStream_t)stream);
    });
}

NB_EXPORT int nb_launch_eyes_colour(uint32_t n_total, uint32_t first, uint32_t count, const void *cams_16, const void *inst_16n,
                                    uint32_t width, uint32_t flags, const void *skin, uint32_t tw, uint32_t th, void *ids, void *depth,
                                    void *rgba, void *bgra8, void *stream)
{
    static const ViewForm f = {"nb_launch_eyes_colour", false, 0xCu, kNoColour, true, kAlign16Colour};
    return launch_eyes_form(f, n_total, first, count, cams_16, inst_16n, width, flags, skin, tw, th, ids, depth, rgba, bgra8, stream, [&] {
        return nbk::launch_eyes_colour(n_total, first, count, (const float *)cams_16, (const float *)inst_16n, width, flags, (const float *)skin,
                                       tw, th, (uint32_t *)ids, (float *)depth, (float *)rgba, (uint32_t *)bgra8, (hipStream_t)stream);
    });
}

NB_EXPORT int nb_launch_eyes_msaa(uint32_t n_total, uint32_t first, uint32_t count, const void *cams_16, const void *inst_16n,
                                  uint32_t width, uint32_t flags, const void *skin, uint32_t tw, uint32_t th, void *ids8, void *depth8,
                                  void *rgba, void *bgra8, void *stream)
{
    static const ViewForm f = {"nb_launch_eyes_msaa", true, 0xFu, kNoOutputs8, true, kAlign16Colour};
    return launch_eyes_form(f, n_total, first, count, cams_16, inst_16n, width, flags, skin, tw, th, ids8, depth8, rgba, bgra8, stream, [&] {
        return nbk::launch_eyes_msaa(n_total, first, count, (const float *)cams_16, (const float *)inst_16n, width, flags, (const float *)skin,
                                     tw, th, (uint32_t *)ids8, (float *)depth8, (float *)rgba, (uint32_t *)bgra8, (hipStream_t)stream);
    });
}

NB_EXPORT int nb_launch_frame(uint32_t n_total, const void *cam_16, const void *inst_16n, uint32_t width, uint32_t height, uint32_t flags,
                              const void *skin, uint32_t tw, uint32_t th, void *scratch, void *ids, void *depth, void *rgba, void *bgra8,
                              void *stream)
{
    static const ViewForm f = {"nb_launch_frame", false, 0xFu, kNoOutputs, true, kAlign16Frame};
    return launch_frame_form(f, n_total, cam_16, inst_16n, width, height, flags, skin, tw, th, scratch, ids, depth, rgba, bgra8, stream, [&] {
        return nbk::launch_frame(n_total, (const float *)cam_16, (const float *)inst_16n, width, height, (const float *)skin, tw, th,
                                 (uint64_t *)scratch, (uint32_t *)ids, (float *)depth, (float *)rgba, (uint32_t *)bgra8, (hipStream_t)stream);
    });
}

NB_EXPORT int nb_launch_frame_msaa(uint32_t n_total, const void *cam_16, const void *inst_16n, uint32_t width, uint32_t height, uint32_t flags,
                                   const void *skin, uint32_t tw, uint32_t th, void *scratch, void *ids8, void *depth8, void *rgba,
                                   void *bgra8, void *stream)
{
    static const ViewForm f = {"nb_launch_frame_msaa", true, 0xFu, kNoOutputs8, true, kAlign16Frame};
    return launch_frame_form(f, n_total, cam_16, inst_16n, width, height, flags, skin, tw, th, scratch, ids8, depth8, rgba, bgra8, stream, [&] {
        return nbk::launch_frame_msaa(n_total, (const float *)cam_16, (const float *)inst_16n, width, height, (const float *)skin, tw, th,
                                      (uint64_t *)scratch, (uint32_t *)ids8, (float *)depth8, (float *)rgba, (uint32_t *)bgra8,
                                      (hipStream_t)stream);
    });
}

NB_EXPORT int nb_launch_random_step(uint32_t first, uint32_t count, void *pos, void *vel, uint64_t seed, uint64_t step, void *stream)
{
    if (!count || !pos || !vel) {
        g_tls_error = "nb_launch_random_step: bad argument";
        return NB_ERR_INVALID;
    }
    NB_LAUNCH_TLS(nbk::launch_random(first, count, (float4 *)pos, (float4 *)vel, seed, step, (hipStream_t)stream));
}

NB_EXPORT int nb_launch_pack(uint32_t count, const void *xyz, void *rec4, void *stream)
{
    if (!count || !xyz || !rec4) {
        g_tls_error = "nb_launch_pack: bad argument";
        return NB_ERR_INVALID;
    }
    NB_LAUNCH_TLS(nbk::launch_pack(count, (const float *)xyz, (float4 *)rec4, (hipStream_t)stream));
}

NB_EXPORT int nb_launch_unpack(uint32_t count, const void *rec4, void *xyz, void *stream)
{
    if (!count || !rec4 || !xyz) {
        g_tls_error = "nb_launch_unpack: bad argument";
        return NB_ERR_INVALID;
    }
    NB_LAUNCH_TLS(nbk::launch_unpack(count, (const float4 *)rec4, (float *)xyz, (hipStream_t)stream));
}

#include "nb_vision_api.inc"   // the seen and located sets and the steps over them (DESIGN.md sections 12 and 13)
#include "nb_scenes_api.inc"   // scene batches: B small scenes, k steps, one launch
#include "nb_peers.inc"
#include "nb_shard.inc"
