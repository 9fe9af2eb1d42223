// scenes_seen_check.cpp -- drives the seen boids step of a scene batch through the C++ host mirror (SceneBatch::seen,
// SceneBatch::step_boids_seen of include/nenbody_scene.hpp) and dumps the seen sets of the initial state and the state after K steps,
// so that tests/test_gpu_scenes_seen.py can compare them with the restatement.
// usage: scenes_seen_check SCENES N WIDTH K OUT.bin      The batch starts from seeds 1100, 1101, ...
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
        const nenbody::SceneBatch::Seen s = batch.seen(cp, width);
        if (s.count.size() != (size_t)scenes * n || s.ids.size() != s.count.size() * width) return 5;
        if (!batch.seen(cp, width, 0, 0).ids.empty() || batch.seen(cp, width, scenes - 1, 1).count.size() != n) return 6;
        batch.step_boids_seen(k, cp, width);
        std::vector<nenbody::Vec3> p, v;
        std::vector<nenbody::Mat4> inst;
        batch.download(p, v, inst);
        if (batch.steps_done() != (uint64_t)k) return 3;
        FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 4;
        std::fwrite(s.count.data(), sizeof(uint32_t), s.count.size(), f);
        std::fwrite(s.ids.data(), sizeof(uint32_t), s.ids.size(), f);
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
