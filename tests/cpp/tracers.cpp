// tracers.cpp -- the tracer recorder (gpe_tracers_*) driven through the C++ host mirror
// (gpu-physics-engine_amd/host/gpe_host.hpp): a host in a compiled language records the path of some particles during
// its steps and reads what a twin that looks them up after every step sees.  Runs on the GPU box:
//   g++ -std=c++17 tests/cpp/tracers.cpp -Lgpu-physics-engine_amd -lgpe -o tests/cpp/tracers
// Exit code 0 = all passed; `--list` prints the test names (used by the CPU-side compile check).
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "../../gpu-physics-engine_amd/host/gpe_host.hpp"

using namespace gpe;

static int g_failed = 0;
#define ASSERT_TRUE(a)                                                                                    \
    do {                                                                                                  \
        if (!(a)) {                                                                                       \
            std::printf("    ASSERT_TRUE failed at %s:%d: %s\n", __FILE__, __LINE__, #a);                  \
            throw std::runtime_error("assertion failed");                                                 \
        }                                                                                                 \
    } while (0)

static const Vec2 kWorld{200.0f, 120.0f};

static void make_scene(size_t n, std::vector<Vec2> *pos, std::vector<float> *rad)
{
    std::mt19937 rng(20241018u);
    std::uniform_real_distribution<float> ux(1.0f, kWorld.x - 1.0f), uy(1.0f, kWorld.y - 1.0f);
    pos->resize(n);
    rad->assign(n, 0.5f);
    for (auto &p : *pos) p = {ux(rng), uy(rng)};
}

// 12 steps with two re-sorts on an armed State; a twin makes the same steps and calls find_uids after each
static void frames_equal_a_twin_that_looks_up_after_every_step()
{
    std::vector<Vec2> pos;
    std::vector<float> rad;
    make_scene(3000, &pos, &rad);
    State a(pos, rad, kWorld), b(pos, rad, kWorld);
    a.particles().enable_uids();
    b.particles().enable_uids();
    const std::vector<uint32_t> uids = {2999, 7, 1234, 5000, 0};                  // 5000 names nobody
    const size_t k = uids.size();
    a.particles().tracers_begin(uids, 2, 4, true, true);
    a.particles().tracers_sample();
    std::vector<ParticleSystem::UidLookup> want = {b.particles().find_uids(uids)};
    for (int s = 0; s < 12; ++s) {
        const bool resort = s == 0 || s == 6;
        a.update(1.0f / 60.0f, resort);
        b.update(1.0f / 60.0f, resort);
        want.push_back(b.particles().find_uids(uids));
    }
    const ParticleSystem::TracerFrames f = a.particles().tracers_read();
    // 7 frames were taken (steps 0, 2, .. 12), the ring holds the newest 4
    ASSERT_TRUE(f.recorded == 7 && f.k == k);
    ASSERT_TRUE((f.step == std::vector<uint64_t>{6, 8, 10, 12}));
    ASSERT_TRUE(f.pos.size() == 4 * k && f.prev.size() == 4 * k && f.index.size() == 4 * k);
    for (size_t r = 0; r < 4; ++r) {
        const ParticleSystem::UidLookup &w = want[f.step[r]];
        ASSERT_TRUE(std::memcmp(&f.pos[r * k], w.pos.data(), k * sizeof(Vec2)) == 0);
        ASSERT_TRUE(std::memcmp(&f.prev[r * k], w.prev.data(), k * sizeof(Vec2)) == 0);
        ASSERT_TRUE(std::memcmp(&f.index[r * k], w.index.data(), k * sizeof(uint32_t)) == 0);
    }
    ASSERT_TRUE(f.index[3] == GPE_UID_ABSENT && f.pos[3].x != f.pos[3].x);        // the row of uid 5000
    ASSERT_TRUE(f.index[0] != 2999u || f.index[1] != 7u);                         // the re-sorts moved them
    ASSERT_TRUE(a.particles().tracers_read(true).step.size() == 4);
    ASSERT_TRUE(a.particles().tracers_read().step.empty());
    a.particles().tracers_end();
    bool refused = false;
    try {
        a.particles().tracers_sample();
    } catch (const Error &e) {
        refused = e.status == GPE_ERR_STATE;
    }
    ASSERT_TRUE(refused);
}

int main(int argc, char **argv)
{
    const std::vector<std::pair<std::string, std::function<void()>>> tests = {
        {"frames_equal_a_twin_that_looks_up_after_every_step", frames_equal_a_twin_that_looks_up_after_every_step},
    };
    if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
        for (auto &t : tests) std::printf("%s\n", t.first.c_str());
        return 0;
    }
    for (auto &t : tests) {
        try {
            t.second();
            std::printf("test %s ... ok\n", t.first.c_str());
        } catch (const std::exception &e) {
            std::printf("test %s ... FAILED: %s\n", t.first.c_str(), e.what());
            ++g_failed;
        }
    }
    std::printf("test result: %s. %zu passed; %d failed\n", g_failed ? "FAILED" : "ok", tests.size() - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
