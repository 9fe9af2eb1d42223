// frame_msaa_check.cpp -- drives the frame through 8 samples per pixel (Scene::camera_at, Scene::frame_msaa of
// include/nenbody_scene.hpp) and dumps the four outputs, so that tests/test_cpp_frame_msaa.py can compare them with the rule's
// restatement.
// usage: frame_msaa_check STATE.bin N CAM.bin W H SKIN.bin TW TH OUT.bin
//   STATE.bin: N positions then N velocities, 3 floats each; CAM.bin: eye, direction, up (3 floats each), then the camera
//   constant (16 floats, column-major); SKIN.bin: TW * TH * 4 linear floats, row 0 first ("-": the white skin)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nenbody_scene.hpp"

int main(int argc, char **argv)
{
    if (argc < 10) return 2;
    const uint32_t n = (uint32_t)std::atoi(argv[2]), width = (uint32_t)std::atoi(argv[4]), height = (uint32_t)std::atoi(argv[5]);
    const uint32_t tw = (uint32_t)std::atoi(argv[7]), th = (uint32_t)std::atoi(argv[8]);
    // the host-only helpers need no device
    float o[16] = {};
    if (nb_frame_msaa_scratch_bytes(width, height) != (size_t)width * height * 64 || nb_frame_msaa_scratch_bytes(0, height) != 0 ||
        nb_frame_msaa_scratch_bytes(width, NB_FRAME_MSAA_MAX_DIM + 1u) != 0 || nb_frame_sample_offsets(o) != NB_OK || o[0] != 0.5625f ||
        o[8] != 0.3125f || o[15] != 0.0625f)
        return 3;
    std::printf("scratch ok\n");
    std::fflush(stdout);
    try {
        std::vector<nenbody::Vec3> pos(n), vel(n);
        float cam_in[25] = {};
        nenbody::Mat4 cp{};
        if (std::strcmp(argv[1], "-") != 0) {
            FILE *f = std::fopen(argv[1], "rb");
            if (!f || std::fread(pos.data(), sizeof(pos[0]), n, f) != n || std::fread(vel.data(), sizeof(vel[0]), n, f) != n) return 4;
            std::fclose(f);
            f = std::fopen(argv[3], "rb");
            if (!f || std::fread(cam_in, sizeof(float), 25, f) != 25) return 4;
            std::fclose(f);
            std::memcpy(cp[0].data(), cam_in + 9, 16 * sizeof(float));
        }
        std::vector<std::array<float, 4>> skin;
        if (std::strcmp(argv[6], "-") != 0) {
            skin.resize((size_t)tw * th);
            FILE *f = std::fopen(argv[6], "rb");
            if (!f || std::fread(skin.data(), sizeof(skin[0]), skin.size(), f) != skin.size()) return 4;
            std::fclose(f);
        }
        const nb_params prm = nenbody::default_params();
        nenbody::Scene scene(pos, vel, prm);
        scene.set_skin(skin, tw, th);
        const nenbody::Mat4 cam = scene.camera_at({cam_in[0], cam_in[1], cam_in[2]}, {cam_in[3], cam_in[4], cam_in[5]},
                                                  {cam_in[6], cam_in[7], cam_in[8]}, cp);
        const nenbody::Scene::FrameMsaa fr = scene.frame_msaa(cam, width, height);
        const size_t cells = (size_t)width * height;
        if (fr.width != width || fr.height != height || fr.ids8.size() != cells || fr.depth8.size() != cells || fr.rgba.size() != cells ||
            fr.bgra8.size() != cells)
            return 5;
        // an invalid extent is refused, as an Error: 0, and nb_frame's maximum, which is above this one's
        int refused = 0;
        for (uint32_t w : {0u, (uint32_t)NB_FRAME_MAX_DIM}) try {
                (void)scene.frame_msaa(cam, w, height);
            } catch (const nenbody::Error &e) {
                refused += e.status == NB_ERR_INVALID;
            }
        if (refused != 2) return 6;
        FILE *f = std::fopen(argv[9], "wb");
        if (!f) return 4;
        std::fwrite(cam[0].data(), sizeof(float), 16, f);
        std::fwrite(fr.ids8.data(), sizeof(fr.ids8[0]), cells, f);
        std::fwrite(fr.depth8.data(), sizeof(fr.depth8[0]), cells, f);
        std::fwrite(fr.rgba.data(), sizeof(fr.rgba[0]), cells, f);
        std::fwrite(fr.bgra8.data(), sizeof(uint32_t), cells, f);
        std::fclose(f);
        std::printf("ok\n");
    } catch (const nenbody::Error &e) {
        std::fprintf(stderr, "nenbody error %d: %s\n", e.status, e.what());
        return 10;
    }
    return 0;
}
