// scenes_check.cpp -- drives a scene batch through the C++ host mirror (nenbody::SceneBatch of include/nenbody_scene.hpp) and dumps
// the state, so that tests/test_gpu_scenes.py can compare it with the restatement.  usage: scenes_check SCENES N K OUT.bin
// The batch starts from seeds 1234, 1235, ...; it takes K gravity steps, one boids step and one more gravity step.
#include <cstdio>
#include <cstdlib>

#include "nenbody_scene.hpp"

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const uint32_t scenes = (uint32_t)std::atoi(argv[1]);
    const uint32_t n = (uint32_t)std::atoi(argv[2]);
    const uint32_t k = (uint32_t)std::atoi(argv[3]);
    try {
        const nb_params prm = nenbody::default_params();
        nenbody::SceneBatch batch(scenes, n, 1234, prm);
        batch.step(k);
        batch.step_boids();
        batch.step();
        std::vector<nenbody::Vec3> p, v;
        std::vector<nenbody::Mat4> inst;
        batch.download(p, v, inst);
        const nenbody::SceneBatch::DeviceState d = batch.device_state();
        if (!d.pos || !d.vel || !d.inst || batch.steps_done() != (uint64_t)k + 2) {
            std::fprintf(stderr, "device_state or steps_done wrong\n");
            return 3;
        }
        FILE *f = std::fopen(argv[4], "wb");
        if (!f) return 4;
        std::fwrite(p.data(), sizeof(nenbody::Vec3), p.size(), f);
        std::fwrite(v.data(), sizeof(nenbody::Vec3), v.size(), f);
        std::fwrite(inst.data(), sizeof(nenbody::Mat4), inst.size(), f);
        std::fclose(f);
        std::printf("ok steps=%llu\n", (unsigned long long)batch.steps_done());
    } catch (const nenbody::Error &e) {
        std::fprintf(stderr, "nenbody error %d: %s\n", e.status, e.what());
        return 10;
    }
    return 0;
}
