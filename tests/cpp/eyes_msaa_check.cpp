// eyes_msaa_check.cpp -- drives the 8-sample eye rows (Scene::eyes_msaa of include/nenbody_scene.hpp) and dumps the four outputs,
// so that tests/test_cpp_eyes_msaa.py can compare them with the rule's restatement.
// usage: eyes_msaa_check N WIDTH SKIN.bin TW TH OUT.bin   (SKIN.bin: TW * TH * 4 linear floats, row 0 first; "-": the white skin)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nenbody_scene.hpp"

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const uint32_t n = (uint32_t)std::atoi(argv[1]), width = (uint32_t)std::atoi(argv[2]);
    const uint32_t tw = (uint32_t)std::atoi(argv[4]), th = (uint32_t)std::atoi(argv[5]);
    // the sample offsets need no device: sixteenths, each odd one once
    float o[NB_EYES_SAMPLES];
    const float want[NB_EYES_SAMPLES] = {0.5625f, 0.4375f, 0.8125f, 0.3125f, 0.1875f, 0.0625f, 0.6875f, 0.9375f};
    if (nb_eyes_sample_offsets(o) != NB_OK || nb_eyes_sample_offsets(nullptr) != NB_ERR_INVALID) return 3;
    for (uint32_t k = 0; k < NB_EYES_SAMPLES; ++k)
        if (o[k] != want[k]) return 3;
    std::printf("offsets ok\n");
    std::fflush(stdout);
    try {
        std::vector<std::array<float, 4>> skin;
        if (std::strcmp(argv[3], "-") != 0) {
            skin.resize((size_t)tw * th);
            FILE *f = std::fopen(argv[3], "rb");
            if (!f || std::fread(skin.data(), sizeof(skin[0]), skin.size(), f) != skin.size()) return 4;
            std::fclose(f);
        }
        nenbody::Mat4 cp;
        nenbody::check(nb_camera_constant(90.0f / (float)width, (float)width / 1.0f, 1.0f, 10000.0f, cp[0].data()), nullptr);
        const nb_params prm = nenbody::default_params();
        nenbody::Scene scene(n, prm, 1234);
        scene.set_skin(skin, tw, th);
        const nenbody::Scene::EyesMsaa all = scene.eyes_msaa(cp, width);
        if (all.ids8.size() != (size_t)n * width || all.depth8.size() != (size_t)n * width || all.rgba.size() != (size_t)n * width ||
            all.bgra8.size() != (size_t)n * width) {
            std::fprintf(stderr, "Scene::eyes_msaa: wrong sizes\n");
            return 5;
        }
        // a slice with the eye's own body drawn, and an empty one
        const nenbody::Scene::EyesMsaa part = scene.eyes_msaa(cp, width, n / 2, 1, true);
        if (part.bgra8.size() != width || !scene.eyes_msaa(cp, width, 0, 0).bgra8.empty()) return 6;
        FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 4;
        std::fwrite(all.ids8.data(), sizeof(all.ids8[0]), all.ids8.size(), f);
        std::fwrite(all.depth8.data(), sizeof(all.depth8[0]), all.depth8.size(), f);
        std::fwrite(all.rgba.data(), sizeof(all.rgba[0]), all.rgba.size(), f);
        std::fwrite(all.bgra8.data(), sizeof(uint32_t), all.bgra8.size(), f);
        std::fwrite(part.bgra8.data(), sizeof(uint32_t), part.bgra8.size(), f);
        std::fclose(f);
        std::printf("ok\n");
    } catch (const nenbody::Error &e) {
        std::fprintf(stderr, "nenbody error %d: %s\n", e.status, e.what());
        return 10;
    }
    return 0;
}
