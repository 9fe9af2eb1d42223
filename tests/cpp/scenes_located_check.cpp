// scenes_located_check.cpp -- drives gravity from located vision of a scene batch through the C++ host mirror
// (SceneBatch::located, SceneBatch::step_nbody_located of include/nenbody_scene.hpp) and dumps the located sets of the initial state
// and the state after K steps, so that tests/test_gpu_scenes_located.py can compare them with the restatement.
// usage: scenes_located_check SCENES N WIDTH K OUT.bin      The batch starts from seeds 1100, 1101, ...
#include <cstdio>
#include <cstdlib>

#include "nenbody_scene.hpp"

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const uint32_t scenes = (uint32_t)std::atoi(argv[1]), n = (uint32_t)std::atoi(argv[2]), width = (uint32_t)std::atoi(argv[3]);
    const uint32_t k = (uint32_t)std::atoi(argv[4]);
    try {
        nenbody::Mat4 cp;
        nenbody::check(nb_camera_constant(90.0f / (float)width, (float)width / 1.0f, 1.0f, 10000.0f, cp[0].data()), nullptr);
        const nb_params prm = nenbody::default_params();
        nenbody::SceneBatch batch(scenes, n, 1100, prm);
        const nenbody::SceneBatch::Located l = batch.located(cp, width);
        const size_t cells = l.count.size() * width;
        if (l.count.size() != (size_t)scenes * n || l.ids.size() != cells || l.depth.size() != cells || l.col.size() != cells ||
            l.rel.size() != cells * 4)
            return 5;
        if (!batch.located(cp, width, 0, 0).rel.empty() || batch.located(cp, width, scenes - 1, 1).count.size() != n) return 6;
        batch.step_nbody_located(k, cp, width);
        std::vector<nenbody::Vec3> p, v;
        std::vector<nenbody::Mat4> inst;
        batch.download(p, v, inst);
        if (batch.steps_done() != (uint64_t)k) return 3;
        FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 4;
        std::fwrite(l.count.data(), sizeof(uint32_t), l.count.size(), f);
        std::fwrite(l.ids.data(), sizeof(uint32_t), l.ids.size(), f);
        std::fwrite(l.depth.data(), sizeof(float), l.depth.size(), f);
        std::fwrite(l.col.data(), sizeof(uint32_t), l.col.size(), f);
        std::fwrite(l.rel.data(), sizeof(float), l.rel.size(), f);
        std::fwrite(p.data(), sizeof(nenbody::Vec3), p.size(), f);
        std::fwrite(v.data(), sizeof(nenbody::Vec3), v.size(), f);
        std::fclose(f);
        std::printf("ok steps=%llu\n", (unsigned long long)batch.steps_done());
    } catch (const nenbody::Error &e) {
        std::fprintf(stderr, "nenbody error %d: %s\n", e.status, e.what());
        return 10;
    }
    return 0;
}
