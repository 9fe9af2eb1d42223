// eyes_check.cpp -- drives the eye view (Scene::eyes, Scene::eyes_colour, Scene::set_skin of include/nenbody_scene.hpp) and dumps
// the four rows, so that tests/test_cpp_eyes.py can compare them with the rule's restatement.
// usage: eyes_check N WIDTH SKIN.bin TW TH OUT.bin   (SKIN.bin: TW * TH * 4 linear floats, row 0 first; "-": the white skin)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nenbody_scene.hpp"

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const uint32_t n = (uint32_t)std::atoi(argv[1]), width = (uint32_t)std::atoi(argv[2]);
    const uint32_t tw = (uint32_t)std::atoi(argv[4]), th = (uint32_t)std::atoi(argv[5]);
    // the host-only helpers need no device: D[0] = 0, D[255] = 1, encode(D[b]) = b, a NaN gives 0
    float D[256];
    uint8_t back[256];
    if (nb_srgb_decode_table(D) != NB_OK || nb_srgb_encode(D, 256, back) != NB_OK || D[0] != 0.0f || D[255] != 1.0f) return 3;
    for (int b = 0; b < 256; ++b)
        if (back[b] != b) return 3;
    std::printf("tables ok\n");
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
        const nenbody::Scene::Eyes plain = scene.eyes(cp, width);
        const nenbody::Scene::EyesColour col = scene.eyes_colour(cp, width);
        if (plain.ids != col.ids || std::memcmp(plain.depth.data(), col.depth.data(), plain.depth.size() * sizeof(float)) != 0 ||
            col.rgba.size() != (size_t)n * width || col.bgra8.size() != (size_t)n * width) {
            std::fprintf(stderr, "Scene::eyes and Scene::eyes_colour disagree\n");
            return 5;
        }
        // a slice with the eye's own body drawn, and an empty one
        const nenbody::Scene::EyesColour part = scene.eyes_colour(cp, width, n / 2, 1, true);
        if (part.bgra8.size() != width || !scene.eyes_colour(cp, width, 0, 0).bgra8.empty()) return 6;
        FILE *f = std::fopen(argv[6], "wb");
        if (!f) return 4;
        std::fwrite(col.ids.data(), sizeof(uint32_t), col.ids.size(), f);
        std::fwrite(col.depth.data(), sizeof(float), col.depth.size(), f);
        std::fwrite(col.rgba.data(), sizeof(col.rgba[0]), col.rgba.size(), f);
        std::fwrite(col.bgra8.data(), sizeof(uint32_t), col.bgra8.size(), f);
        std::fwrite(part.bgra8.data(), sizeof(uint32_t), part.bgra8.size(), f);
        std::fclose(f);
        std::printf("ok\n");
    } catch (const nenbody::Error &e) {
        std::fprintf(stderr, "nenbody error %d: %s\n", e.status, e.what());
        return 10;
    }
    return 0;
}
