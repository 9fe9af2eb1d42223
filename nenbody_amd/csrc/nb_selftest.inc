// nb_selftest.inc -- the self-tests and measurements of include/nenbody_diag.h: the division ladder against the IEEE divide, the restated libm against the host's, v_rcp_f32's scaling, the issue rate of the vector ALU, the clock a kernel holds.
// Included by nb_api.hip (it uses that file's planning, context and launch helpers); not a translation unit of its own.


NB_EXPORT int nb_selftest_divide(const nb_params *params, uint64_t pairs, uint64_t seed, uint64_t *mismatches, float *bad_pair)
{
    if (!mismatches) {
        g_tls_error = "nb_selftest_divide: mismatches is null";
        return NB_ERR_INVALID;
    }
    nb_params p = params_or_default(params);
    p.mode = NB_MODE_STRICT;
    Plan pl;
    int rc = make_plan(p, 1024, 1024, &pl, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (pl.guard.force_ieee && !overrides().strict_force_ieee.on()) {
        g_tls_error = "nb_selftest_divide: these parameters have no guarded range (STRICT always divides with '/')";
        return NB_ERR_UNSUPPORTED;
    }
    if (pl.guard.force_ieee) {  // forced by the environment only: recompute the range without the override is not possible here
        g_tls_error = "nb_selftest_divide: unset NB_STRICT_FORCE_IEEE";
        return NB_ERR_UNSUPPORTED;
    }
    rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    // what the kernels can meet inside the guard (see make_plan):
    //   d = |dp|^2 + bias  in [2^c, 2^max(2b+4, c+2)),   n = dx*G, nonzero dx in [2^(a-23), 2^(b+1)]  ->  |n| in [2^(a-23+g), 2^(b+g+2))
    const int d_lo = pl.guard.c, d_hi = std::max(2 * pl.guard.b + 4, pl.guard.c + 2) - 1;
    const int n_lo = pl.guard.a - 23 + pl.guard.g, n_hi = pl.guard.b + pl.guard.g + 1;
    unsigned long long *d_bad = nullptr;
    float *d_pair = nullptr;
    hipError_t e = hipMalloc((void **)&d_bad, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&d_pair, 2 * sizeof(float));
    if (e == hipSuccess) e = hipMemset(d_bad, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_pair, 0, 2 * sizeof(float));
    const uint32_t blocks = 4096;
    const uint64_t threads = (uint64_t)blocks * 256u;
    uint64_t per_thread = (pairs + threads - 1) / threads;
    if (per_thread > 0xffffffffull) per_thread = 0xffffffffull;
    const bool control = overrides().selftest_control.on();  // NB_SELFTEST_CONTROL=1: compare the UNCORRECTED product n*r instead (control arm: must report mismatches)
    if (e == hipSuccess)
        e = nbk::launch_divide_selftest(blocks, seed, (uint32_t)per_thread, d_lo, d_hi, n_lo, n_hi, d_bad, d_pair, control, nullptr);
    unsigned long long bad = 0;
    float pair[2] = {0.f, 0.f};
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(pair, d_pair, sizeof(pair), hipMemcpyDeviceToHost);
    if (d_bad) (void)hipFree(d_bad);
    if (d_pair) (void)hipFree(d_pair);
    if (e != hipSuccess) {
        g_tls_error = std::string("nb_selftest_divide: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    *mismatches = bad;
    if (bad_pair) {
        bad_pair[0] = pair[0];
        bad_pair[1] = pair[1];
    }
    return NB_OK;
}

NB_EXPORT int nb_selftest_ladder(uint32_t first_significand, uint32_t count, uint64_t *mismatches, float *bad_pair)
{
    if (!mismatches || count == 0 || first_significand >= (1u << 23) || count > (1u << 23) - first_significand) {
        g_tls_error = "nb_selftest_ladder: need mismatches != NULL and a non-empty range of denominator significands inside [0, 2^23)";
        return NB_ERR_INVALID;
    }
    int rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    const bool control = overrides().selftest_control.on();  // NB_SELFTEST_CONTROL=1: the same steps on the UNREFINED reciprocal (control arm: must report mismatches)
    unsigned long long *d_bad = nullptr;
    float *d_pair = nullptr;
    hipError_t e = hipMalloc((void **)&d_bad, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&d_pair, 2 * sizeof(float));
    if (e == hipSuccess) e = hipMemset(d_bad, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_pair, 0, 2 * sizeof(float));
    const uint32_t slab = 1u << 13;  // 2^36 pairs per launch: a fraction of a second each, so no launch runs long
    for (uint32_t done = 0; e == hipSuccess && done < count; done += slab) {
        e = nbk::launch_ladder_exhaustive(first_significand + done, std::min(slab, count - done), control, d_bad, d_pair, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    unsigned long long bad = 0;
    float pair[2] = {0.f, 0.f};
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(pair, d_pair, sizeof(pair), hipMemcpyDeviceToHost);
    if (d_bad) (void)hipFree(d_bad);
    if (d_pair) (void)hipFree(d_pair);
    if (e != hipSuccess) {
        g_tls_error = std::string("nb_selftest_ladder: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    *mismatches = bad;
    if (bad_pair) {
        bad_pair[0] = pair[0];
        bad_pair[1] = pair[1];
    }
    return NB_OK;
}

// Do the model matrices of THIS device equal what THIS host's C library computes?  nb_libm.h restates one libm (glibc 2.35, the
// build of sinf / cosf it selects on CPUs with FMA); a host with another one -- musl, a glibc with CORE-MATH's correctly rounded
// sinf -- rounds a few arguments in a billion differently.  `count` velocities (the step's own range, every binade 2^-40..2^40,
// near-axis directions) go through nb_launch_instances and through the host's atan2f / sinf / cosf; *mismatches = matrices whose
// rotation entries differ in some bit (0 on the hosts this was built for); bad_velocity, if non-NULL, receives one offender (x, y).
NB_EXPORT int nb_selftest_matrices(uint32_t count, uint64_t seed, uint64_t *mismatches, float *bad_velocity)
{
    if (!mismatches || count == 0 || count > (1u << 26)) {
        g_tls_error = "nb_selftest_matrices: need mismatches != NULL and 0 < count <= 2^26";
        return NB_ERR_INVALID;
    }
    int rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    std::vector<float4> pos(count), vel(count);
    uint64_t st = seed;
    for (uint32_t i = 0; i < count; ++i) {
        float x, y;
        switch (i & 3u) {
        case 0: x = uniform_f32(st, -0.2f, 0.2f), y = uniform_f32(st, -0.2f, 0.2f); break;   // what a step produces
        case 1: {                                                                              // every binade, either sign
            const int ex = (int)(splitmix64(st) % 81u) - 40, ey = (int)(splitmix64(st) % 81u) - 40;
            x = std::ldexp(uniform_f32(st, 1.0f, 2.0f), ex) * ((splitmix64(st) & 1u) ? -1.f : 1.f);
            y = std::ldexp(uniform_f32(st, 1.0f, 2.0f), ey) * ((splitmix64(st) & 1u) ? -1.f : 1.f);
            break;
        }
        case 2: {                                                                              // any direction, any length
            const float ang = uniform_f32(st, -3.14159f, 3.14159f), r = std::ldexp(1.0f, (int)(splitmix64(st) % 41u) - 20);
            x = r * std::cos(ang), y = r * std::sin(ang);
            break;
        }
        default: {                                                                             // near the axes and the diagonals
            static const float bx[8] = {1, 0, -1, 0, 1, -1, 1, -1}, by[8] = {0, 1, 0, -1, 1, 1, -1, -1};
            const uint32_t k = (uint32_t)(splitmix64(st) & 7u);
            const float eps = std::ldexp(1.0f, -(int)(splitmix64(st) % 30u) - 1);
            x = bx[k] + uniform_f32(st, -1.f, 1.f) * eps, y = by[k] + uniform_f32(st, -1.f, 1.f) * eps;
        }
        }
        vel[i] = make_float4(x, y, 0.f, 0.f);
        pos[i] = make_float4(uniform_f32(st, -100.f, 100.f), uniform_f32(st, -100.f, 100.f), 0.f, 0.f);
    }
    float4 *d_pos = nullptr, *d_vel = nullptr, *d_inst = nullptr;
    std::vector<float4> inst((size_t)count * 4);
    hipError_t e = hipMalloc((void **)&d_pos, (size_t)count * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void **)&d_vel, (size_t)count * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void **)&d_inst, (size_t)count * 4 * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpy(d_pos, pos.data(), (size_t)count * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_vel, vel.data(), (size_t)count * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = nbk::launch_instances(count, d_pos, d_vel, d_inst, nullptr, 0u);
    if (e == hipSuccess) e = hipMemcpy(inst.data(), d_inst, (size_t)count * 4 * sizeof(float4), hipMemcpyDeviceToHost);
    for (void *p : {(void *)d_pos, (void *)d_vel, (void *)d_inst})
        if (p) (void)hipFree(p);
    if (e != hipSuccess) {
        g_tls_error = std::string("nb_selftest_matrices: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    uint64_t bad = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const float theta = std::atan2(vel[i].y, vel[i].x);   // the float overloads: the host's atan2f / sinf / cosf
        const float sn = std::sin(theta), cs = std::cos(theta);
        const float4 c0 = inst[(size_t)i * 4], c1 = inst[(size_t)i * 4 + 1];
        const float want[4] = {cs, sn, -sn, cs}, got[4] = {c0.x, c0.y, c1.x, c1.y};
        if (std::memcmp(want, got, sizeof(want)) != 0) {
            if (bad == 0 && bad_velocity) bad_velocity[0] = vel[i].x, bad_velocity[1] = vel[i].y;
            ++bad;
        }
    }
    *mismatches = bad;
    return NB_OK;
}

// The device's atan2f / sinf / cosf / atanf (nb_libm.h) against THIS host's C library, argument by argument: `count` consecutive
// binary32 bit patterns from `first` (count = 0 with first = 0: all 2^32) through function fn -- 0 sinf, 1 cosf, 2 atanf, 3
// atan2f(y = the argument, x = the float with bit pattern x_bits) -- on the device in chunks of 2^24 and through std::sin / cos /
// atan / atan2 on `threads` host threads; NaN results compare equal whatever their payload.  All of sinf takes about a minute.
NB_EXPORT int nb_selftest_libm(int fn, uint32_t first, uint64_t count, uint32_t x_bits, uint64_t *mismatches, uint32_t *first_bad)
{
    if (!mismatches || fn < 0 || fn > 3 || count > (1ull << 32) || (uint64_t)first + count > (1ull << 32)) {
        g_tls_error = "nb_selftest_libm: need mismatches != NULL, fn in 0..3 and first + count <= 2^32";
        return NB_ERR_INVALID;
    }
    if (count == 0 && first == 0) count = 1ull << 32;
    int rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    constexpr uint32_t kChunk = 1u << 24;
    uint32_t *d_out = nullptr;
    hipError_t e = hipMalloc((void **)&d_out, (size_t)kChunk * sizeof(uint32_t));
    std::vector<uint32_t> got(kChunk);
    const unsigned threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::atomic<uint64_t> bad{0};
    std::atomic<uint64_t> where{~0ull};
    float xo;
    std::memcpy(&xo, &x_bits, 4);
    for (uint64_t done = 0; done < count && e == hipSuccess; done += kChunk) {
        const uint32_t base = (uint32_t)(first + done), m = (uint32_t)std::min<uint64_t>(kChunk, count - done);
        e = nbk::launch_libm_selftest(fn, base, m, x_bits, d_out, nullptr);
        if (e == hipSuccess) e = hipMemcpy(got.data(), d_out, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) break;
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                uint64_t mine = 0;
                for (uint32_t i = t; i < m; i += threads) {
                    const uint32_t u = base + i;
                    float x, r;
                    std::memcpy(&x, &u, 4);
                    r = fn == 0 ? std::sin(x) : fn == 1 ? std::cos(x) : fn == 2 ? std::atan(x) : std::atan2(x, xo);
                    uint32_t rb;
                    std::memcpy(&rb, &r, 4);
                    float g;
                    std::memcpy(&g, &got[i], 4);
                    if (rb != got[i] && !(r != r && g != g)) {
                        ++mine;
                        uint64_t cur = where.load();
                        while ((uint64_t)u < cur && !where.compare_exchange_weak(cur, (uint64_t)u)) {
                        }
                    }
                }
                bad += mine;
            });
        for (auto &th : pool) th.join();
    }
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) {
        g_tls_error = std::string("nb_selftest_libm: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    *mismatches = bad.load();
    if (first_bad) *first_bad = where.load() == ~0ull ? 0u : (uint32_t)where.load();
    return NB_OK;
}

NB_EXPORT int nb_selftest_rcp_scaling(int k_lo, int k_hi, uint64_t *violations)
{
    if (!violations || k_lo > k_hi || k_lo < -125 || k_hi > 125) {
        g_tls_error = "nb_selftest_rcp_scaling: need violations != NULL and -125 <= k_lo <= k_hi <= 125";
        return NB_ERR_INVALID;
    }
    int rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    unsigned long long *d_bad = nullptr;
    hipError_t e = hipMalloc((void **)&d_bad, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_bad, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = nbk::launch_rcp_scaling(k_lo, k_hi, d_bad, nullptr);
    unsigned long long bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
    if (d_bad) (void)hipFree(d_bad);
    if (e != hipSuccess) {
        g_tls_error = std::string("nb_selftest_rcp_scaling: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    *violations = bad;
    return NB_OK;
}

namespace {
// The clock a kernel ran at, from the (s_memtime, s_memrealtime) stamps its workgroups' first waves left at entry and exit
// (4 words per workgroup): median over workgroups of d(s_memtime) / d(s_memrealtime) x 100 MHz -- s_memrealtime ticks at a
// constant 100 MHz, s_memtime at the shader clock (MI355X_MICROARCH.md, "DVFS give-back" (6)).  Also the median lifetime of
// those waves in shader cycles.  Workgroups too short to time well (< 20 us: 2 000 ticks) are left out where any ran longer; a step
// so small that none did (a few thousand bodies) is timed from every workgroup the counter saw run, at that coarser resolution.
bool clock_from_stamps(const std::vector<unsigned long long> &st, double *mhz, double *cycles)
{
    std::vector<double> f, c;
    for (unsigned long long min_ticks : {2000ull, 0ull}) {
        for (size_t i = 0; i + 3 < st.size(); i += 4) {
            const unsigned long long t0 = st[i], r0 = st[i + 1], t1 = st[i + 2], r1 = st[i + 3];
            if (r1 <= r0 + min_ticks || t1 <= t0) continue;
            f.push_back((double)(t1 - t0) / (double)(r1 - r0) * 100.0);
            c.push_back((double)(t1 - t0));
        }
        if (!f.empty()) break;
    }
    if (f.empty()) return false;
    std::sort(f.begin(), f.end());
    std::sort(c.begin(), c.end());
    *mhz = f[f.size() / 2];
    *cycles = c[c.size() / 2];
    return true;
}
}  // namespace

NB_EXPORT int nb_selftest_valu_rate(int mix, double seconds, double *lane_ops_per_s, double *clock_mhz)
{
    if (!lane_ops_per_s || !(seconds > 0.0) || seconds > 2.0 || (mix < 0 || mix > 4)) {
        g_tls_error = "nb_selftest_valu_rate: need lane_ops_per_s != NULL, mix 0 .. 4 and 0 < seconds <= 2";
        return NB_ERR_INVALID;
    }
    int rc = check_device(&g_tls_error);
    if (rc != NB_OK) return rc;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    float *sink = nullptr;
    unsigned long long *stamps = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const uint32_t blocks = (uint32_t)cus * 8u;  // 256 lanes = one wave per SIMD each: 8 waves per SIMD
    if (e == hipSuccess) e = hipMalloc((void **)&sink, 64);
    if (e == hipSuccess && clock_mhz) e = hipMalloc((void **)&stamps, (size_t)blocks * 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    auto timed = [&](uint32_t trips, float *ms) {
        hipError_t x = hipEventRecord(e0, nullptr);
        if (x == hipSuccess) x = nbk::launch_valu_stream(mix, blocks, trips, sink, stamps, nullptr);
        if (x == hipSuccess) x = hipEventRecord(e1, nullptr);
        if (x == hipSuccess) x = hipEventSynchronize(e1);
        if (x == hipSuccess) x = hipEventElapsedTime(ms, e0, e1);
        return x;
    };
    float ms = 0.f;
    uint32_t trips = 2000;
    if (e == hipSuccess) e = timed(trips, &ms);  // warm-up + calibration (~ 1 ms)
    if (e == hipSuccess && ms > 0.f) {
        const double want = seconds * 1e3 / (double)ms * (double)trips;
        trips = (uint32_t)std::min(std::max(want, 1000.0), 4.0e8);
        e = timed(trips, &ms);
    }
    if (e == hipSuccess && clock_mhz) {
        std::vector<unsigned long long> st((size_t)blocks * 4);
        e = hipMemcpy(st.data(), stamps, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        double cycles = 0.0;
        if (e == hipSuccess && !clock_from_stamps(st, clock_mhz, &cycles)) *clock_mhz = 0.0;
    }
    if (sink) (void)hipFree(sink);
    if (stamps) (void)hipFree(stamps);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess || !(ms > 0.f)) {
        g_tls_error = std::string("nb_selftest_valu_rate: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    // 64 instructions per trip and lane; a packed instruction (mix 2) is two lane operations
    *lane_ops_per_s = (mix == 2 ? 128.0 : 64.0) * (double)trips * 256.0 * (double)blocks / ((double)ms * 1e-3);
    return NB_OK;
}

// The clock the part holds under the whole-set step kernel of `params` (step_strict_kernel / step_fast_wave_kernel) on n
// bodies of the reference's initial distribution: back-to-back steps for about `seconds`, the last one stamped.
NB_EXPORT int nb_diag_step_clock(const nb_params *params, uint32_t n, double seconds, double *clock_mhz, double *wave_cycles,
                                 double *kernel_ms)
{
    if (!clock_mhz || !(seconds > 0.0) || seconds > 5.0 || n == 0) {
        g_tls_error = "nb_diag_step_clock: need clock_mhz != NULL, n > 0 and 0 < seconds <= 5";
        return NB_ERR_INVALID;
    }
    nb_params p = params_or_default(params);
    Plan pl;
    int rc = make_plan(p, n, n, &pl, &g_tls_error);
    if (rc != NB_OK) return rc;
    if (!pl.stamped) {
        g_tls_error = "nb_diag_step_clock: only the whole-set kernels carry stamps (STRICT one lane per body, FAST wave and pairs forms)";
        return NB_ERR_UNSUPPORTED;
    }
    nb_ctx *c = nullptr;
    rc = nb_create(n, 1, &p, &c);
    if (rc != NB_OK) return rc;
    std::vector<float> pos((size_t)n * 3), vel((size_t)n * 3);
    nb_init_state(1234, n, pos.data(), vel.data());
    rc = nb_upload(c, pos.data(), vel.data());
    const size_t groups = nbp::stamp_groups(pl, n, KernelSizes{});
    unsigned long long *stamps = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipSuccess;
    float ms = 0.f;
    if (rc == NB_OK) {
        e = hipMalloc((void **)&stamps, groups * 4 * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemsetAsync(stamps, 0, groups * 4 * sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        // calibrate on two steps, then fill `seconds`
        if (e == hipSuccess) rc = nb_step(c, 1);
        if (e == hipSuccess && rc == NB_OK) e = hipEventRecord(e0, c->stream);
        if (e == hipSuccess && rc == NB_OK) rc = nb_step(c, 1);
        if (e == hipSuccess && rc == NB_OK) e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess && rc == NB_OK) e = hipEventSynchronize(e1);
        if (e == hipSuccess && rc == NB_OK) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && rc == NB_OK && ms > 0.f) {
            const uint32_t k = (uint32_t)std::min(std::max(seconds * 1e3 / (double)ms, 2.0), 100000.0);
            rc = nb_step(c, k - 1u);
            // the stamped step: the same launch with StepArgs::stamps set
            if (rc == NB_OK) e = hipEventRecord(e0, c->stream);
            if (rc == NB_OK && e == hipSuccess) {
                nbk::StepArgs a = step_args(p, pl, n, 0, n, c->pos[c->cur].p, c->pos[c->cur ^ 1].p, c->vel.p, c->scratch.p);
                a.stamps = stamps;
                e = launch_planned(pl, a, c->scratch.p, nullptr, c->stream);  // (no stamped form reports through the status word)
            }
            if (rc == NB_OK && e == hipSuccess) e = hipEventRecord(e1, c->stream);
            if (rc == NB_OK && e == hipSuccess) e = hipEventSynchronize(e1);
            if (rc == NB_OK && e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        }
    }
    double mhz = 0.0, cycles = 0.0;
    if (rc == NB_OK && e == hipSuccess) {
        std::vector<unsigned long long> st(groups * 4);
        e = hipMemcpy(st.data(), stamps, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (e == hipSuccess && !clock_from_stamps(st, &mhz, &cycles)) {
            g_tls_error = "nb_diag_step_clock: no workgroup ran long enough to time";
            rc = NB_ERR_STATE;
        }
    }
    if (rc != NB_OK && c) g_tls_error = c->err.empty() ? g_tls_error : c->err;
    if (stamps) (void)hipFree(stamps);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    nb_destroy(c);
    if (rc != NB_OK) return rc;
    if (e != hipSuccess) {
        g_tls_error = std::string("nb_diag_step_clock: ") + hipGetErrorString(e);
        return NB_ERR_HIP;
    }
    *clock_mhz = mhz;
    if (wave_cycles) *wave_cycles = cycles;
    if (kernel_ms) *kernel_ms = (double)ms;
    return NB_OK;
}

