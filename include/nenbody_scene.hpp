// nenbody_scene.hpp -- header-only C++ host mirror of the reference's update interface, over the C ABI (nenbody.h).
//
// The reference is compiled code (Rust) whose toolchain is absent from the build image, so besides the Rust shim
// (integration/rust/scene.rs, uncompiled) the same host side is given in C++: `nenbody::Scene` is the type the
// reference's empty src/scene.rs (src/scene.rs:1) was meant to hold; `nenbody::update_instance_nbody` keeps the
// five-argument signature of src/main.rs:404-410.  Plumbing only: all arithmetic runs in libnenbody_hip.so.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "nenbody.h"

namespace nenbody {

using Vec3 = std::array<float, 3>;                 // memory of cgmath::Point3<f32> / Vector3<f32>
using Mat4 = std::array<std::array<float, 4>, 4>;  // memory of [[f32; 4]; 4], column-major

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &m) : std::runtime_error(m), status(s) {}
};

inline void check(int rc, const nb_ctx *ctx)
{
    if (rc != NB_OK) throw Error(rc, nb_last_error(ctx));
}

// The library that got loaded must speak the ABI this header was written against: a symbol may keep its name and change its
// arguments between versions (nb_update_instance_random: eight in ABI 1, six since ABI 2), and the linker cannot tell.  Checked
// once per process, by every entry point of this header, before anything else crosses the boundary.
inline void check_abi()
{
    static const int got = nb_abi_version();
    if (got != NB_ABI_VERSION)
        throw Error(NB_ERR_UNSUPPORTED, "libnenbody_hip.so speaks ABI " + std::to_string(got) + ", this host was built against ABI " +
                                            std::to_string(NB_ABI_VERSION));
}

inline nb_params default_params(uint32_t mode = NB_MODE_STRICT)
{
    check_abi();
    nb_params p;
    nb_default_params(&p);  // src/main.rs:411-413
    p.mode = mode;
    return p;
}

class Scene {
public:
    std::vector<Vec3> positions;   // src/main.rs:743
    std::vector<Vec3> velocities;  // src/main.rs:738
    std::vector<Mat4> instances;   // instance_data, uploaded at src/main.rs:932-936

    // the reference's initial distributions (src/main.rs:738-747), seeded
    Scene(uint32_t n, const nb_params &params, uint64_t seed) : positions(n), velocities(n), instances(n)
    {
        check(nb_init_state(seed, n, positions[0].data(), velocities[0].data()), nullptr);
        create(params);
    }
    Scene(std::vector<Vec3> pos, std::vector<Vec3> vel, const nb_params &params)
        : positions(std::move(pos)), velocities(std::move(vel)), instances(positions.size())
    {
        // copy_from_slice panics on unequal lengths (src/main.rs:415-416)
        if (positions.size() != velocities.size()) throw std::invalid_argument("positions and velocities differ in length");
        create(params);
    }
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;
    ~Scene() { nb_destroy(ctx_); }

    // one update_instance_nbody (src/main.rs:404-441); host mirrors refreshed for the consumers at src/main.rs:932-945
    void step()
    {
        check(nb_step(ctx_, 1), ctx_);
        check(nb_download(ctx_, positions[0].data(), velocities[0].data(), instances[0][0].data()), ctx_);
    }
    // k steps, device-resident, no download
    void step_n(uint32_t k) { check(nb_step(ctx_, k), ctx_); }
    // one update_instance_boids (src/main.rs:443-526), reference constants unless given; host mirrors refreshed
    void step_boids(const nb_boids_params *params = nullptr)
    {
        check(nb_step_boids(ctx_, 1, params), ctx_);
        check(nb_download(ctx_, positions[0].data(), velocities[0].data(), instances[0][0].data()), ctx_);
    }
    void step_boids_n(uint32_t k, const nb_boids_params *params = nullptr) { check(nb_step_boids(ctx_, k, params), ctx_); }
    void sync() { check(nb_sync(ctx_), ctx_); }
    void refresh() { check(nb_download(ctx_, positions[0].data(), velocities[0].data(), instances[0][0].data()), ctx_); }
    uint64_t steps_done() const { return nb_steps_done(ctx_); }

    // Every entity's eye view (nb_eyes: the reference's eye pass, src/main.rs:585-647, 962-998) for bodies [first, first + count) of
    // the current state, rows of `width` pixels: per column the nearest body's index (NB_EYES_NONE where none) and the depth
    // attachment's value.  cp16: the eyes' camera constant, column-major (nb_camera_constant(90.0f / width, width, 1, 10000) is
    // the reference's); up: its `normal`.
    struct Eyes {
        uint32_t width = 0;
        std::vector<uint32_t> ids;
        std::vector<float> depth;
    };
    Eyes eyes(const Mat4 &cp, uint32_t width = 1024, uint32_t first = 0, uint32_t count = UINT32_MAX, bool see_self = false,
              const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (count == UINT32_MAX) count = first <= positions.size() ? (uint32_t)positions.size() - first : 0;
        Eyes e;
        e.width = width;
        const size_t cells = (size_t)count * width;
        sized(cells, [&] {
            return nb_eyes(ctx_, first, count, up.data(), cp[0].data(), width, see_self ? NB_EYES_SEE_SELF : 0u, e.ids.data(), e.depth.data());
        }, e.ids, e.depth);
        return e;
    }
    // The seen set of every eye (nb_eyes_seen): which entities occur in the eye's row of eyes() (same arguments), ascending, with
    // the nearest depth and the number of columns of each.  Row e of ids / depth / cols has `width` slots, count[e] of them used;
    // the others read NB_EYES_NONE, 1.0f and 0.
    struct Seen {
        uint32_t width = 0;
        std::vector<uint32_t> count, ids;
        std::vector<float> depth;
        std::vector<uint32_t> cols;
    };
    Seen seen(const Mat4 &cp, uint32_t width = 1024, uint32_t first = 0, uint32_t count = UINT32_MAX, bool see_self = false,
              const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (count == UINT32_MAX) count = first <= positions.size() ? (uint32_t)positions.size() - first : 0;
        Seen s;
        s.width = width;
        const size_t cells = (size_t)count * width;
        s.count.resize(count ? count : 1);
        sized(cells, [&] {
            return nb_eyes_seen(ctx_, first, count, up.data(), cp[0].data(), width, see_self ? NB_EYES_SEE_SELF : 0u, s.count.data(),
                                s.ids.data(), s.depth.data(), s.cols.data());
        }, s.ids, s.depth, s.cols);
        s.count.resize(count);
        return s;
    }
    // one update_instance_boids restricted to what each entity sees (nb_step_boids_seen: body n folds over the entities of its own
    // row of eyes() instead of over every entity; one that sees nobody stops); host mirrors refreshed.  batch: eyes processed at a
    // time, 0 = the library's choice.
    void step_boids_seen(const Mat4 &cp, uint32_t width = 1024, const nb_boids_params *params = nullptr, uint32_t batch = 0,
                         const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        step_boids_seen_n(1, cp, width, params, batch, up);
        check(nb_download(ctx_, positions[0].data(), velocities[0].data(), instances[0][0].data()), ctx_);
    }
    void step_boids_seen_n(uint32_t k, const Mat4 &cp, uint32_t width = 1024, const nb_boids_params *params = nullptr, uint32_t batch = 0,
                           const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        check(nb_step_boids_seen(ctx_, k, params, up.data(), cp[0].data(), width, batch), ctx_);
    }
    // Where every eye sees the members of its seen set (nb_eyes_located): seen()'s lists (same arguments) plus, per member, the
    // column at which it is nearest (col) and the seen point relative to the eye in world axes with its range (rel: x, y, z, r),
    // formed from the eye's row, its heading, `up` and `cp` alone.  cp must be a perspective constant as nb_camera_constant forms
    // it.  Behind the count[e] used slots col reads NB_EYES_NONE and rel four +0.
    struct Located {
        uint32_t width = 0;
        std::vector<uint32_t> count, ids;
        std::vector<float> depth;
        std::vector<uint32_t> cols, col;
        std::vector<std::array<float, 4>> rel;
    };
    Located located(const Mat4 &cp, uint32_t width = 1024, uint32_t first = 0, uint32_t count = UINT32_MAX, bool see_self = false,
                    const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (count == UINT32_MAX) count = first <= positions.size() ? (uint32_t)positions.size() - first : 0;
        Located s;
        s.width = width;
        const size_t cells = (size_t)count * width;
        s.count.resize(count ? count : 1);
        sized(cells, [&] {
            return nb_eyes_located(ctx_, first, count, up.data(), cp[0].data(), width, see_self ? NB_EYES_SEE_SELF : 0u, s.count.data(),
                                   s.ids.data(), s.depth.data(), s.cols.data(), s.col.data(), s.rel[0].data());
        }, s.ids, s.depth, s.cols, s.col, s.rel);
        s.count.resize(count);
        return s;
    }
    // one update_instance_nbody from vision alone (nb_step_nbody_located: body n folds the reference's law over the relative positions
    // of located() instead of over p_i - p_n; one that sees nobody coasts); host mirrors refreshed.  batch: eyes processed at a time,
    // 0 = the library's choice.
    void step_nbody_located(const Mat4 &cp, uint32_t width = 1024, uint32_t batch = 0, const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        step_nbody_located_n(1, cp, width, batch, up);
        check(nb_download(ctx_, positions[0].data(), velocities[0].data(), instances[0][0].data()), ctx_);
    }
    void step_nbody_located_n(uint32_t k, const Mat4 &cp, uint32_t width = 1024, uint32_t batch = 0, const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        check(nb_step_nbody_located(ctx_, k, up.data(), cp[0].data(), width, batch), ctx_);
    }
    // The skin the colour rows sample: tw x th linear RGBA texels, row 0 first; an empty vector: the 1 x 1 white skin.
    void set_skin(const std::vector<std::array<float, 4>> &rgba_linear, uint32_t tw, uint32_t th)
    {
        if (!rgba_linear.empty() && rgba_linear.size() != (size_t)tw * th) throw std::invalid_argument("a skin needs tw * th texels");
        check(nb_eyes_skin(ctx_, rgba_linear.empty() ? nullptr : rgba_linear[0].data(), tw, th), ctx_);
    }
    // The same pass with its colour row (nb_eyes_colour): rgba = what the fragment shader writes (texel under the vignette, or the
    // clear colour), bgra8 = the texel of the reference's Bgra8UnormSrgb target, bytes B, G, R, A -- what a host uploads to its
    // imgui texture instead of running the eye and viewport passes.
    struct EyesColour {
        uint32_t width = 0;
        std::vector<uint32_t> ids;
        std::vector<float> depth;
        std::vector<std::array<float, 4>> rgba;
        std::vector<uint32_t> bgra8;
    };
    EyesColour eyes_colour(const Mat4 &cp, uint32_t width = 1024, uint32_t first = 0, uint32_t count = UINT32_MAX, bool see_self = false,
                           const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (count == UINT32_MAX) count = first <= positions.size() ? (uint32_t)positions.size() - first : 0;
        EyesColour e;
        e.width = width;
        const size_t cells = (size_t)count * width;
        sized(cells, [&] {
            return nb_eyes_colour(ctx_, first, count, up.data(), cp[0].data(), width, see_self ? NB_EYES_SEE_SELF : 0u, e.ids.data(),
                                  e.depth.data(), e.rgba[0].data(), e.bgra8.data());
        }, e.ids, e.depth, e.rgba, e.bgra8);
        return e;
    }

    // The eye rows through 8 samples per column, resolved as the reference's targets are (nb_eyes_msaa; msaa_samples = 8 and
    // resolve_target, src/main.rs:652, 547, 611): ids8 / depth8 hold the eight samples of every column, sample k of column c of row
    // e at (e * width + c) * 8 + k; rgba / bgra8 are the resolved rows, shaped as eyes_colour's.  width <= NB_EYES_MSAA_MAX_WIDTH.
    struct EyesMsaa {
        uint32_t width = 0;
        std::vector<std::array<uint32_t, NB_EYES_SAMPLES>> ids8;
        std::vector<std::array<float, NB_EYES_SAMPLES>> depth8;
        std::vector<std::array<float, 4>> rgba;
        std::vector<uint32_t> bgra8;
    };
    EyesMsaa eyes_msaa(const Mat4 &cp, uint32_t width = 1024, uint32_t first = 0, uint32_t count = UINT32_MAX, bool see_self = false,
                       const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (count == UINT32_MAX) count = first <= positions.size() ? (uint32_t)positions.size() - first : 0;
        EyesMsaa e;
        e.width = width;
        const size_t cells = (size_t)count * width;
        sized(cells, [&] {
            return nb_eyes_msaa(ctx_, first, count, up.data(), cp[0].data(), width, see_self ? NB_EYES_SEE_SELF : 0u, e.ids8[0].data(),
                                e.depth8[0].data(), e.rgba[0].data(), e.bgra8.data());
        }, e.ids8, e.depth8, e.rgba, e.bgra8);
        return e;
    }

    // One camera from a host-supplied eye and direction (nb_camera_at): cp * look_at_dir(eye, dir, up).  The reference's scene
    // camera (src/main.rs:753-762, 940-942) is camera_at({p.x, p.y, 990}, {0, 0, -1}, {1, 0, 0}, cp) above the body p it follows,
    // with cp = nb_camera_constant(90.0f / a, a, 1, 10000), a = (float)width / (float)height.
    Mat4 camera_at(const Vec3 &eye, const Vec3 &dir, const Vec3 &up, const Mat4 &cp)
    {
        Mat4 out{};
        check(nb_camera_at(ctx_, eye.data(), dir.data(), up.data(), cp[0].data(), out[0].data()), ctx_);
        return out;
    }
    // The scene camera's frame (nb_frame: the reference's display pass, src/main.rs:948-960) of the current state through `camera`,
    // height rows of width pixels, row 0 the top: per pixel the instance drawn there (NB_EYES_NONE where none), the depth
    // attachment's value, the linear colour and the Bgra8UnormSrgb texel -- what a headless host presents instead of running
    // render(&display, ...).  The skin is set_skin's.
    struct Frame {
        uint32_t width = 0, height = 0;
        std::vector<uint32_t> ids;
        std::vector<float> depth;
        std::vector<std::array<float, 4>> rgba;
        std::vector<uint32_t> bgra8;
    };
    Frame frame(const Mat4 &camera, uint32_t width = 1920, uint32_t height = 1080)
    {
        Frame f;
        f.width = width, f.height = height;
        const size_t cells = (size_t)width * height;
        f.ids.resize(cells ? cells : 1);      // (a pointer the library can check even where the extent is invalid)
        f.depth.resize(cells ? cells : 1);
        f.rgba.resize(cells ? cells : 1);
        f.bgra8.resize(cells ? cells : 1);
        check(nb_frame(ctx_, camera[0].data(), width, height, 0u, f.ids.data(), f.depth.data(), f.rgba[0].data(), f.bgra8.data()), ctx_);
        return f;
    }

    // The same frame through 8 samples per pixel, resolved as the reference's display target is (nb_frame_msaa; msaa_samples = 8,
    // src/main.rs:652, 685-690, 545-548): ids8 / depth8 hold the eight samples of every pixel, sample k of pixel (c, r) at
    // (r * width + c) * 8 + k; rgba / bgra8 are the resolved frame, shaped as frame's.  width, height <= NB_FRAME_MSAA_MAX_DIM.
    struct FrameMsaa {
        uint32_t width = 0, height = 0;
        std::vector<std::array<uint32_t, NB_EYES_SAMPLES>> ids8;
        std::vector<std::array<float, NB_EYES_SAMPLES>> depth8;
        std::vector<std::array<float, 4>> rgba;
        std::vector<uint32_t> bgra8;
    };
    FrameMsaa frame_msaa(const Mat4 &camera, uint32_t width = 1920, uint32_t height = 1080)
    {
        FrameMsaa f;
        f.width = width, f.height = height;
        const bool valid = width >= 1 && width <= NB_FRAME_MSAA_MAX_DIM && height >= 1 && height <= NB_FRAME_MSAA_MAX_DIM;
        const size_t cells = valid ? (size_t)width * height : 0;   // (an extent the library refuses: nothing to allocate)
        f.ids8.resize(cells ? cells : 1);     // (a pointer the library can check even where the extent is invalid)
        f.depth8.resize(cells ? cells : 1);
        f.rgba.resize(cells ? cells : 1);
        f.bgra8.resize(cells ? cells : 1);
        check(nb_frame_msaa(ctx_, camera[0].data(), width, height, 0u, f.ids8[0].data(), f.depth8[0].data(), f.rgba[0].data(), f.bgra8.data()),
              ctx_);
        return f;
    }

private:
    // `rows` at least one element long for `call` (pointers the library can check even where count = 0), `cells` behind it
    template <typename Call, typename... Rows>
    void sized(size_t cells, Call call, Rows &...rows)
    {
        (rows.resize(cells ? cells : 1), ...);
        check(call(), ctx_);
        (rows.resize(cells), ...);
    }
    void create(const nb_params &params)
    {
        check_abi();
        if (positions.empty()) throw std::invalid_argument("a Scene needs at least one body");
        check(nb_create((uint32_t)positions.size(), 1, &params, &ctx_), nullptr);
        int rc = nb_upload(ctx_, positions[0].data(), velocities[0].data());
        if (rc != NB_OK) {
            std::string msg = nb_last_error(ctx_);
            nb_destroy(ctx_);
            ctx_ = nullptr;
            throw Error(rc, msg);
        }
    }
    nb_ctx *ctx_ = nullptr;
};

// B independent scenes of n <= NB_SCENES_MAX_BODIES bodies, device-resident (nb_scenes_* of nenbody.h): one launch steps every scene
// k times, one workgroup per scene, and every scene gets the bits a Scene of its n bodies gets.  Body i of scene s is element
// s * n + i of every array.  Steps are asynchronous on the batch's stream; download() waits.
class SceneBatch {
public:
    // scene s starts from the reference's initial distributions drawn with seed + s
    SceneBatch(uint32_t scenes, uint32_t n, uint64_t seed, const nb_params &params) : scenes_(scenes), n_(n)
    {
        check_abi();
        std::vector<Vec3> pos((size_t)scenes * n + 1), vel((size_t)scenes * n + 1);
        for (uint32_t s = 0; s < scenes; ++s)
            check(nb_init_state(seed + s, n, pos[(size_t)s * n].data(), vel[(size_t)s * n].data()), nullptr);
        create(pos, vel, params);
    }
    SceneBatch(uint32_t scenes, uint32_t n, const std::vector<Vec3> &pos, const std::vector<Vec3> &vel, const nb_params &params)
        : scenes_(scenes), n_(n)
    {
        check_abi();
        if (pos.size() != (size_t)scenes * n || vel.size() != pos.size() || pos.empty())
            throw std::invalid_argument("positions and velocities must hold scenes * n bodies");
        create(pos, vel, params);
    }
    SceneBatch(const SceneBatch &) = delete;
    SceneBatch &operator=(const SceneBatch &) = delete;
    ~SceneBatch() { nb_scenes_destroy(ctx_); }

    uint32_t scenes() const { return scenes_; }
    uint32_t n() const { return n_; }
    void step(uint32_t k = 1) { check_sc(nb_scenes_step(ctx_, k)); }
    void step_boids(uint32_t k = 1, const nb_boids_params *params = nullptr) { check_sc(nb_scenes_step_boids(ctx_, k, params)); }
    // k update_instance_boids of every scene restricted to what each entity sees of its own scene (nb_scenes_step_boids_seen,
    // DESIGN.md section 14.1): the bits Scene::step_boids_seen_n gives each scene; one fused launch per step for the whole batch
    void step_boids_seen(uint32_t k, const Mat4 &cp, uint32_t width = 1024, const nb_boids_params *params = nullptr,
                         const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        check_sc(nb_scenes_step_boids_seen(ctx_, k, params, up.data(), cp[0].data(), width));
    }
    // The seen sets that step folds over (nb_scenes_eyes_seen) for scenes [first_scene, first_scene + scene_count): count[s * n + i]
    // members of eye i of scene s, its `width` slots at ids[(s * n + i) * width], scene-local ids ascending, NB_EYES_NONE behind them.
    // Depths and column counts are not kept by the batch's step and are not offered.
    struct Seen {
        uint32_t width = 0;
        std::vector<uint32_t> count, ids;
    };
    Seen seen(const Mat4 &cp, uint32_t width = 1024, uint32_t first_scene = 0, uint32_t scene_count = UINT32_MAX,
              const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (scene_count == UINT32_MAX) scene_count = first_scene <= scenes_ ? scenes_ - first_scene : 0;
        Seen s;
        s.width = width;
        const size_t eyes = (size_t)scene_count * n_;
        s.count.resize(eyes ? eyes : 1);
        s.ids.resize(eyes && width ? eyes * width : 1);
        check_sc(nb_scenes_eyes_seen(ctx_, first_scene, scene_count, up.data(), cp[0].data(), width, s.count.data(), s.ids.data()));
        s.count.resize(eyes);
        s.ids.resize(eyes * width);
        return s;
    }
    // k update_instance_nbody of every scene from vision alone (nb_scenes_step_nbody_located): the bits
    // Scene::step_nbody_located_n gives each scene; one fused launch per step for the whole batch.  cp: a perspective constant
    void step_nbody_located(uint32_t k, const Mat4 &cp, uint32_t width = 1024, const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        check_sc(nb_scenes_step_nbody_located(ctx_, k, up.data(), cp[0].data(), width));
    }
    // The located sets that step folds over (nb_scenes_eyes_located) for scenes [first_scene, first_scene + scene_count): per eye
    // s * n + i its count and `width` slots each of ids, depth, col and rel (4 floats a slot: x, y, z, range), the words of
    // Scene's located sets per scene, padding included.  Column counts are not kept by the batch's step and are not offered.
    struct Located {
        uint32_t width = 0;
        std::vector<uint32_t> count, ids, col;
        std::vector<float> depth, rel;
    };
    Located located(const Mat4 &cp, uint32_t width = 1024, uint32_t first_scene = 0, uint32_t scene_count = UINT32_MAX,
                    const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (scene_count == UINT32_MAX) scene_count = first_scene <= scenes_ ? scenes_ - first_scene : 0;
        Located l;
        l.width = width;
        const size_t eyes = (size_t)scene_count * n_, cells = eyes * width;
        l.count.resize(eyes ? eyes : 1);
        l.ids.resize(cells ? cells : 1), l.depth.resize(cells ? cells : 1), l.col.resize(cells ? cells : 1);
        l.rel.resize(cells ? cells * 4 : 4);
        check_sc(nb_scenes_eyes_located(ctx_, first_scene, scene_count, up.data(), cp[0].data(), width, l.count.data(), l.ids.data(),
                                        l.depth.data(), l.col.data(), l.rel.data()));
        l.count.resize(eyes);
        l.ids.resize(cells), l.depth.resize(cells), l.col.resize(cells), l.rel.resize(cells * 4);
        return l;
    }
    // The batch's policies (nb_scenes_set_policy): `weights` holds 1 or scenes() policies of
    // nb_policy_floats(features, hidden) floats each -- w1[f * H + j], b1[j], w2[k * H + j] for k = 0, 1, b2[k] --, scene s using
    // policy s (or all policy 0).  accel_limit >= 0 clamps the two outputs; infinity: no limit.  May be called again.
    void set_policy(const std::vector<float> &weights, uint32_t features, uint32_t hidden, float accel_limit = INFINITY)
    {
        const size_t one = nb_policy_floats(features, hidden);
        if (one == 0 || weights.empty() || weights.size() % one != 0)
            throw std::invalid_argument("weights must hold whole policies of nb_policy_floats(features, hidden) floats");
        check_sc(nb_scenes_set_policy(ctx_, features, hidden, (uint32_t)(weights.size() / one), weights.data(), accel_limit));
        features_ = features;
    }
    // k steps of every scene under its policy (nb_scenes_step_policy): the pooled eye row through the two-layer network, thrust and
    // turn along the eye's own axes; one fused launch per step.  width must be a multiple of the policy's features.
    void step_policy(uint32_t k, const Mat4 &cp, uint32_t width = 1024, const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        check_sc(nb_scenes_step_policy(ctx_, k, up.data(), cp[0].data(), width));
    }
    // What that step computes in front of the actuation (nb_scenes_eyes_policy) for scenes [first_scene, first_scene + scene_count):
    // per eye s * n + i the policy's features and the two outputs behind the limit.
    struct PolicyObservation {
        uint32_t features = 0;
        std::vector<float> feat, act;
    };
    PolicyObservation policy_observe(const Mat4 &cp, uint32_t width = 1024, uint32_t first_scene = 0, uint32_t scene_count = UINT32_MAX,
                                     const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (scene_count == UINT32_MAX) scene_count = first_scene <= scenes_ ? scenes_ - first_scene : 0;
        PolicyObservation o;
        o.features = features_;
        const size_t eyes = (size_t)scene_count * n_, cells = eyes * features_;
        o.feat.resize(cells ? cells : 1), o.act.resize(eyes ? eyes * 2 : 2);
        check_sc(nb_scenes_eyes_policy(ctx_, first_scene, scene_count, up.data(), cp[0].data(), width, o.feat.data(), o.act.data()));
        o.feat.resize(cells), o.act.resize(eyes * 2);
        return o;
    }
    // The batch's policies, recurrent (nb_scenes_set_policy_recurrent): `weights` holds 1 or scenes() policies of
    // nb_policy_recurrent_floats(features, hidden) floats each -- w1[f * H + j], wr[r * H + j], b1[j], w2[k * H + j], b2[k].  Every body
    // gets `hidden` words of memory, cleared to +0 here; memory_limit >= 0 clamps what a step writes to it; infinity: no limit.
    // step_policy, step_policy_scored and policy_observe then run the recurrent kernel until set_policy sets a feedforward policy.
    void set_policy_recurrent(const std::vector<float> &weights, uint32_t features, uint32_t hidden, float accel_limit = INFINITY,
                              float memory_limit = INFINITY)
    {
        const size_t one = nb_policy_recurrent_floats(features, hidden);
        if (one == 0 || weights.empty() || weights.size() % one != 0)
            throw std::invalid_argument("weights must hold whole policies of nb_policy_recurrent_floats(features, hidden) floats");
        check_sc(nb_scenes_set_policy_recurrent(ctx_, features, hidden, (uint32_t)(weights.size() / one), weights.data(), accel_limit,
                                                memory_limit));
        features_ = features, hidden_ = hidden;
    }
    // The memory of scenes [first_scene, first_scene + scene_count) (nb_scenes_memory): n * hidden floats a scene.  Waits for the stream.
    std::vector<float> memory(uint32_t first_scene = 0, uint32_t scene_count = UINT32_MAX)
    {
        if (scene_count == UINT32_MAX) scene_count = first_scene <= scenes_ ? scenes_ - first_scene : 0;
        const size_t words = (size_t)scene_count * n_ * hidden_;
        std::vector<float> out(words ? words : 1);
        check_sc(nb_scenes_memory(ctx_, first_scene, scene_count, out.data()));
        out.resize(words);
        return out;
    }
    // The memory of the whole batch from the host (nb_scenes_set_memory): scenes * n * hidden floats, any bit patterns.
    void set_memory(const std::vector<float> &memory)
    {
        if (memory.empty() || memory.size() != (size_t)scenes_ * n_ * hidden_)
            throw std::invalid_argument("memory must hold scenes * n * hidden floats");
        check_sc(nb_scenes_set_memory(ctx_, memory.data()));
    }
    // The memory of every body set to +0 (nb_scenes_memory_reset), asynchronous.  An upload, keep and rewind do not touch the memory.
    void memory_reset() { check_sc(nb_scenes_memory_reset(ctx_)); }
    // policy_observe for a recurrent policy with the memory the step would write (nb_scenes_eyes_policy_memory); the memory is left
    // as it is.
    struct PolicyMemoryObservation {
        uint32_t features = 0, hidden = 0;
        std::vector<float> feat, act, mem;
    };
    PolicyMemoryObservation policy_observe_memory(const Mat4 &cp, uint32_t width = 1024, uint32_t first_scene = 0,
                                                  uint32_t scene_count = UINT32_MAX, const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        if (scene_count == UINT32_MAX) scene_count = first_scene <= scenes_ ? scenes_ - first_scene : 0;
        PolicyMemoryObservation o;
        o.features = features_, o.hidden = hidden_;
        const size_t eyes = (size_t)scene_count * n_, cells = eyes * features_, words = eyes * hidden_;
        o.feat.resize(cells ? cells : 1), o.act.resize(eyes ? eyes * 2 : 2), o.mem.resize(words ? words : 1);
        check_sc(nb_scenes_eyes_policy_memory(ctx_, first_scene, scene_count, up.data(), cp[0].data(), width, o.feat.data(), o.act.data(),
                                              o.mem.data()));
        o.feat.resize(cells), o.act.resize(eyes * 2), o.mem.resize(words);
        return o;
    }
    // The batch's score (nb_scenes_set_score): radius_sq >= 0 is the squared radius below which a pair counts
    // as near (infinity: every pair), goal the point whose squared distance is summed.  Allocates one record a scene on first use
    // and clears the records.  May be called again.
    void set_score(float radius_sq, const Vec3 &goal = Vec3{0.0f, 0.0f, 0.0f})
    {
        const nb_score_params sp = {radius_sq, {goal[0], goal[1], goal[2]}};
        check_sc(nb_scenes_set_score(ctx_, &sp));
    }
    // The current snapshot of every scene added to its record (nb_scenes_score): one kernel, asynchronous.
    void score() { check_sc(nb_scenes_score(ctx_)); }
    // The records cleared (nb_scenes_score_reset), asynchronous.  An upload does not clear them.
    void score_reset() { check_sc(nb_scenes_score_reset(ctx_)); }
    // The records of scenes [first_scene, first_scene + scene_count) (nb_scenes_scores), 32 bytes a scene.  Waits for the stream.
    std::vector<nb_scene_score> scores(uint32_t first_scene = 0, uint32_t scene_count = UINT32_MAX)
    {
        if (scene_count == UINT32_MAX) scene_count = first_scene <= scenes_ ? scenes_ - first_scene : 0;
        std::vector<nb_scene_score> out(scene_count ? scene_count : 1);
        check_sc(nb_scenes_scores(ctx_, first_scene, scene_count, out.data()));
        out.resize(scene_count);
        return out;
    }
    // k times step_policy(1) then score() (nb_scenes_step_policy_scored): a rollout scored where it runs.
    void step_policy_scored(uint32_t k, const Mat4 &cp, uint32_t width = 1024, const Vec3 &up = Vec3{0.0f, 0.0f, 1.0f})
    {
        check_sc(nb_scenes_step_policy_scored(ctx_, k, up.data(), cp[0].data(), width));
    }
    // The batch's search (nb_scenes_es_set): mean, nb_policy_floats(features, hidden) floats, is the policy the
    // population -- one policy a scene, at most NB_ES_MAX_POPULATION scenes -- is drawn around; ep holds the draw's scale, the update's
    // step, the fitness's six coefficients and the seed.  The generation starts at 0.
    void es_set(const std::vector<float> &mean, uint32_t features, uint32_t hidden, const nb_es_params &ep,
                float accel_limit = INFINITY)
    {
        if (mean.size() != nb_policy_floats(features, hidden) || mean.empty())
            throw std::invalid_argument("mean must hold nb_policy_floats(features, hidden) floats");
        check_sc(nb_scenes_es_set(ctx_, features, hidden, mean.data(), accel_limit, &ep));
        es_floats_ = mean.size();
        features_ = features;
    }
    // es_set over a recurrent policy (nb_scenes_es_set_recurrent): mean holds nb_policy_recurrent_floats(features, hidden) floats.  A
    // generation is rewind, memory_reset, score_reset, es_perturb, step_policy_scored, es_update: rewind does not touch the memory.
    void es_set_recurrent(const std::vector<float> &mean, uint32_t features, uint32_t hidden, const nb_es_params &ep,
                          float accel_limit = INFINITY, float memory_limit = INFINITY)
    {
        if (mean.size() != nb_policy_recurrent_floats(features, hidden) || mean.empty())
            throw std::invalid_argument("mean must hold nb_policy_recurrent_floats(features, hidden) floats");
        check_sc(nb_scenes_es_set_recurrent(ctx_, features, hidden, mean.data(), accel_limit, memory_limit, &ep));
        es_floats_ = mean.size();
        features_ = features, hidden_ = hidden;
    }
    // The batch's policies become the population of the current generation (nb_scenes_es_perturb), asynchronous.
    void es_perturb() { check_sc(nb_scenes_es_perturb(ctx_)); }
    // The score records ranked, the mean updated in place and the generation incremented (nb_scenes_es_update), asynchronous.
    void es_update() { check_sc(nb_scenes_es_update(ctx_)); }
    // The mean (nb_scenes_es_mean).  Waits for the stream.
    std::vector<float> es_mean()
    {
        std::vector<float> out(es_floats_ ? es_floats_ : 1);
        check_sc(nb_scenes_es_mean(ctx_, out.data()));
        out.resize(es_floats_);
        return out;
    }
    // What the last es_update left (nb_scenes_es_result): the report, the fitnesses and the ranks, 0 the worst.  Waits for the stream.
    struct EsResult {
        nb_es_report report;
        std::vector<float> fitness;
        std::vector<uint32_t> rank;
    };
    EsResult es_result()
    {
        EsResult o{};
        o.fitness.resize(scenes_), o.rank.resize(scenes_);
        check_sc(nb_scenes_es_result(ctx_, &o.report, o.fitness.data(), o.rank.data()));
        return o;
    }
    uint32_t es_generation() const { return nb_scenes_es_generation(ctx_); }
    // Positions, velocities and the step counter copied to buffers the batch keeps (nb_scenes_keep), on the device; rewind copies them
    // back (nb_scenes_rewind), asynchronous.  An upload does not drop the kept state.
    void keep() { check_sc(nb_scenes_keep(ctx_)); }
    void rewind() { check_sc(nb_scenes_rewind(ctx_)); }
    void sync() { check_sc(nb_scenes_sync(ctx_)); }
    uint64_t steps_done() const { return nb_scenes_steps(ctx_); }
    void download(std::vector<Vec3> &positions, std::vector<Vec3> &velocities, std::vector<Mat4> &instances)
    {
        const size_t total = (size_t)scenes_ * n_;
        positions.resize(total), velocities.resize(total), instances.resize(total);
        check_sc(nb_scenes_download(ctx_, positions[0].data(), velocities[0].data(), instances[0][0].data()));
    }
    // the batch's device records (nb_scenes_device_state): scene s starts s * n records behind each pointer
    struct DeviceState {
        const void *pos, *vel, *inst;
    };
    DeviceState device_state()
    {
        DeviceState d{};
        check_sc(nb_scenes_device_state(ctx_, &d.pos, &d.vel, &d.inst));
        return d;
    }

private:
    void check_sc(int rc)
    {
        if (rc != NB_OK) throw Error(rc, nb_scenes_last_error(ctx_));
    }
    void create(const std::vector<Vec3> &pos, const std::vector<Vec3> &vel, const nb_params &params)
    {
        const int rc = nb_scenes_create(scenes_, n_, &params, &ctx_);
        if (rc != NB_OK) throw Error(rc, nb_scenes_last_error(nullptr));
        const int up = nb_scenes_upload(ctx_, pos[0].data(), vel[0].data());
        if (up != NB_OK) {
            const std::string msg = nb_scenes_last_error(ctx_);
            nb_scenes_destroy(ctx_);
            ctx_ = nullptr;
            throw Error(up, msg);
        }
    }
    nb_scenes *ctx_ = nullptr;
    uint32_t scenes_ = 0, n_ = 0;
    uint32_t features_ = 0;   // F of the policy set last; 0: none
    uint32_t hidden_ = 0;     // H of the recurrent policy set last; 0: none
    size_t es_floats_ = 0;    // the floats of the search's mean; 0: none
};

// One rank's share of a scene on a multi-GPU host (one process or thread per GPU): nb_shard_* of nenbody.h.  Every rank
// passes the same full state; the rank keeps its index range and a replica of all positions, and each step ends with
// one exchange (RCCL when constructed with a comm id from Shard::comm_id(), else the host's nb_gather_fn).
class Shard {
public:
    static std::array<char, NB_COMM_ID_BYTES> comm_id()
    {
        std::array<char, NB_COMM_ID_BYTES> id{};
        check(nb_comm_id(id.data()), nullptr);
        return id;
    }
    Shard(const std::vector<Vec3> &positions, const std::vector<Vec3> &velocities, int rank, int world, const nb_params &params,
          const void *rccl_id = nullptr, nb_gather_fn gather = nullptr, void *gather_user = nullptr, nb_ring_fn ring = nullptr,
          void *ring_user = nullptr)
    {
        check_abi();
        if (positions.empty() || positions.size() != velocities.size())
            throw std::invalid_argument("positions and velocities must be non-empty and equally long");
        check(nb_shard_create((uint32_t)positions.size(), rank, world, &params, &sh_), nullptr);
        n_ = (uint32_t)positions.size();
        try {
            check_sh(nb_shard_range(sh_, &first_, &count_));
            if (rccl_id) check_sh(nb_shard_use_rccl(sh_, rccl_id));
            else if (gather) check_sh(nb_shard_use_gather(sh_, gather, gather_user));
            // FAST on equal ranks: every unordered pair once, with a second exchange per step (include/nenbody.h); RCCL brings
            // it along, a host exchange needs `ring` beside `gather` (else the ordered fold stays)
            if (ring) check_sh(nb_shard_use_ring(sh_, ring, ring_user));
            check_sh(nb_shard_upload(sh_, positions[0].data(), velocities[0].data()));
        } catch (...) {
            nb_shard_destroy(sh_);
            throw;
        }
    }
    Shard(const Shard &) = delete;
    Shard &operator=(const Shard &) = delete;
    ~Shard() { nb_shard_destroy(sh_); }

    uint32_t first() const { return first_; }
    uint32_t count() const { return count_; }
    int pairs_partners() const { return nb_shard_pairs_partners(sh_); }  // D of the pairs form a step will take; 0: the ordered fold
    bool pairs_overlapped() const { return nb_shard_pairs_overlapped(sh_) == 1; }  // the pairs form in phases, both exchanges on the second stream (set_overlap)
    void step(uint32_t k = 1) { check_sh(nb_shard_step(sh_, k)); }
    void step_boids(uint32_t k = 1, const nb_boids_params *params = nullptr) { check_sh(nb_shard_step_boids(sh_, k, params)); }
    // FAST only (a STRICT shard ignores it): fold the rank's own slot while the exchange of the others is in flight
    void set_overlap(bool on) { check_sh(nb_shard_set_overlap(sh_, on ? 1 : 0)); }
    // both exchanges once on a known pattern, checked on every rank, with fallbacks (collective).  gather: 0 in place, 1 from a copy;
    // ring: -1 no pairs form, 0 one group, 1 one group per distance, 2 dropped for the ordered fold
    struct ExchangePaths {
        int gather, ring;
    };
    ExchangePaths verify_exchanges()  // (gather 2 / ring 3: pulled over xGMI, see peer_import)
    {
        ExchangePaths p{0, -1};
        check_sh(nb_shard_verify_exchanges(sh_, &p.gather, &p.ring));
        return p;
    }
    // every form a FAST step can take timed on this machine (slowest rank; collective), the fastest kept, the state put back:
    // 0 the ordered fold, 1 the pairs form, 2 the pairs form in phases; ms_per_step[form] < 0: not offered
    struct FormChoice {
        int chosen;
        double ms_per_step[3];
    };
    FormChoice choose_form(uint32_t steps = 4)
    {
        FormChoice c{};
        check_sh(nb_shard_choose_form(sh_, steps, &c.chosen, c.ms_per_step));
        return c;
    }
    void set_pairs(bool on) { check_sh(nb_shard_set_pairs(sh_, on ? 1 : 0)); }  // name the form (run-to-run identical FAST bits)
    // both exchanges as pulls over xGMI, no collective library (include/nenbody.h): every rank's peer_blob() travels to every rank by the
    // host's own channel, rank-major, into peer_import(); all ranks in processes of one node
    std::vector<unsigned char> peer_blob()
    {
        std::vector<unsigned char> b(nb_peers_blob_bytes());
        check_sh(nb_shard_peer_export(sh_, b.data()));
        return b;
    }
    void peer_import(const std::vector<unsigned char> &all_blobs_rank_major) { check_sh(nb_shard_peer_import(sh_, all_blobs_rank_major.data())); }
    void use_peers(bool on) { check_sh(nb_shard_use_peers(sh_, on ? 1 : 0)); }
    // waits; throws Error(NB_ERR_STATE) if a kernel of this shard reported a failure (a block-chain wave gave up waiting)
    void sync() { check_sh(nb_shard_sync(sh_)); }
    // all n positions (the replica); this rank's velocities and model matrices
    void download(std::vector<Vec3> &positions, std::vector<Vec3> &velocities_local, std::vector<Mat4> &instances_local)
    {
        positions.resize(n_);
        velocities_local.resize(count_);
        instances_local.resize(count_);
        check_sh(nb_shard_download(sh_, positions[0].data(), count_ ? velocities_local[0].data() : nullptr,
                                   count_ ? instances_local[0][0].data() : nullptr));
    }

private:
    void check_sh(int rc)
    {
        if (rc != NB_OK) throw Error(rc, nb_shard_last_error(sh_));
    }
    nb_shard *sh_ = nullptr;
    uint32_t n_ = 0, first_ = 0, count_ = 0;
};

// Drop-ins for the reference's free functions, src/main.rs:404-410 and 443-449: same five arguments, updated in place,
// one FFI call each (nb_update_instance_nbody / nb_update_instance_boids keep the device context between calls).
// A length mismatch is where copy_from_slice panics (src/main.rs:415-416): std::invalid_argument here.
namespace detail {
inline void update_status(int rc)
{
    if (rc == NB_ERR_INVALID) throw std::invalid_argument(nb_last_error(nullptr));
    check(rc, nullptr);
}
inline float *ptr(std::vector<Vec3> &v) { return v.empty() ? nullptr : v[0].data(); }
inline float *ptr(std::vector<Mat4> &v) { return v.empty() ? nullptr : v[0][0].data(); }
}  // namespace detail

inline void update_instance_nbody(std::vector<Mat4> &instances, std::vector<Vec3> &positions, std::vector<Vec3> &old_positions,
                                  std::vector<Vec3> &velocities, std::vector<Vec3> &old_velocities,
                                  const nb_params *params = nullptr)
{
    check_abi();
    detail::update_status(nb_update_instance_nbody(detail::ptr(instances), instances.size(), detail::ptr(positions),
                                                   positions.size(), detail::ptr(old_positions), old_positions.size(),
                                                   detail::ptr(velocities), velocities.size(), detail::ptr(old_velocities),
                                                   old_velocities.size(), params));
}

inline void update_instance_boids(std::vector<Mat4> &instances, std::vector<Vec3> &positions, std::vector<Vec3> &old_positions,
                                  std::vector<Vec3> &velocities, std::vector<Vec3> &old_velocities,
                                  const nb_boids_params *params = nullptr)
{
    check_abi();
    detail::update_status(nb_update_instance_boids(detail::ptr(instances), instances.size(), detail::ptr(positions),
                                                   positions.size(), detail::ptr(old_positions), old_positions.size(),
                                                   detail::ptr(velocities), velocities.size(), detail::ptr(old_velocities),
                                                   old_velocities.size(), params));
}

// update_instance_random(instances, positions, velocities) (src/main.rs:381-385): the third controller, its own three
// arguments; the library keeps the seed and counts the calls (nb_update_random_seed restarts the stream)
inline void update_instance_random(std::vector<Mat4> &instances, std::vector<Vec3> &positions, std::vector<Vec3> &velocities)
{
    check_abi();
    detail::update_status(nb_update_instance_random(detail::ptr(instances), instances.size(), detail::ptr(positions), positions.size(),
                                                    detail::ptr(velocities), velocities.size()));
}

// the same step at a stream position the caller names: `step` = the frame number
inline void update_instance_random(std::vector<Mat4> &instances, std::vector<Vec3> &positions, std::vector<Vec3> &velocities,
                                   uint64_t seed, uint64_t step)
{
    check_abi();
    detail::update_status(nb_update_instance_random_seeded(detail::ptr(instances), instances.size(), detail::ptr(positions),
                                                           positions.size(), detail::ptr(velocities), velocities.size(), seed, step));
}

}  // namespace nenbody
