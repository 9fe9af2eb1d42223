// located_check.cpp -- drives the located seen sets and the vision-only gravity step of the C++ host mirror (Scene::located,
// Scene::step_nbody_located of include/nenbody_scene.hpp) and dumps the lists, the located rows and the state after one step, so that
// tests/test_gpu_located.py can compare them with the restatement.
// usage: located_check N WIDTH OUT.bin
#include <cstdio>
#include <cstdlib>

#include "nenbody_scene.hpp"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const uint32_t n = (uint32_t)std::atoi(argv[1]), width = (uint32_t)std::atoi(argv[2]);
    try {
        nenbody::Mat4 cp;
        nenbody::check(nb_camera_constant(90.0f / (float)width, (float)width / 1.0f, 1.0f, 10000.0f, cp[0].data()), nullptr);
        const nb_params prm = nenbody::default_params();
        nenbody::Scene scene(n, prm, 1234);
        const nenbody::Scene::Located s = scene.located(cp, width);
        if (s.count.size() != n || s.ids.size() != (size_t)n * width || s.depth.size() != s.ids.size() || s.cols.size() != s.ids.size() ||
            s.col.size() != s.ids.size() || s.rel.size() != s.ids.size())
            return 5;
        if (!scene.located(cp, width, 0, 0).rel.empty() || scene.located(cp, width, n / 2, 1, true).count.size() != 1) return 6;
        scene.step_nbody_located(cp, width);
        FILE *f = std::fopen(argv[3], "wb");
        if (!f) return 4;
        std::fwrite(s.count.data(), sizeof(uint32_t), s.count.size(), f);
        std::fwrite(s.ids.data(), sizeof(uint32_t), s.ids.size(), f);
        std::fwrite(s.depth.data(), sizeof(float), s.depth.size(), f);
        std::fwrite(s.cols.data(), sizeof(uint32_t), s.cols.size(), f);
        std::fwrite(s.col.data(), sizeof(uint32_t), s.col.size(), f);
        std::fwrite(s.rel.data(), sizeof(s.rel[0]), s.rel.size(), f);
        std::fwrite(scene.positions.data(), sizeof(scene.positions[0]), n, f);
        std::fwrite(scene.velocities.data(), sizeof(scene.velocities[0]), n, f);
        std::fclose(f);
        std::printf("ok\n");
    } catch (const nenbody::Error &e) {
        std::fprintf(stderr, "nenbody error %d: %s\n", e.status, e.what());
        return 10;
    }
    return 0;
}
