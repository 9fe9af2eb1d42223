// plan_table.cpp -- the step planner (nenbody_amd/csrc/nb_plan.h) against tests/golden/plan_table.txt, without the library and without HIP.
//
// usage: plan_table <table>.  For every line of the table the case columns (in front of " => ") are read, the knobs are set in a
// DebugOverrides directly, and the line is printed again with the result columns as this planner gives them: the return code or the
// error, the launcher and its scalar arguments (through nb_plan.h's own visit_launch), the plan-derived argument words (through its
// plan_step_args; zero words are left out), the scratch size, nb_diag_plan's string, nb_diag_step_clock's verdict and, where the case
// has a (jlo, jhi), the two-phase plan.  tests/test_plan_table.py asserts that the output equals the table.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../nenbody_amd/csrc/nb_plan.h"

using namespace nbp;

// The kernels' layout arithmetic, restated (nb_launch.inc: strict_bc_scratch_bytes; nb_nbody_sym.inc: fast_pairs_*): the table's scratch
// columns were recorded from the real functions, and test_plan_table.py holds them against the built library as well.
struct Sizes {
    size_t planes_bytes(uint32_t n) const { return 256u + 3u * (size_t)((n + 63u) / 64u * 64u) * sizeof(float) + 64u; }
    uint32_t pairs_chunk(uint32_t n, uint32_t chunk) const { return chunk ? chunk : n <= 262144u ? n : 131072u; }
    uint32_t pairs_rows(uint32_t n, uint32_t w, uint32_t np) const { return (n + 128u * np * w - 1u) / (128u * np * w); }
    size_t pairs_scratch_floats(uint32_t n, uint32_t w, uint32_t np, uint32_t chunk) const
    {
        const uint32_t c = pairs_chunk(n, chunk), super = 128u * np * w;
        const size_t rows = (size_t)3 * ((c + super - 1u) / super) * c;
        return c >= n ? rows : (size_t)3 * n + 2 * rows;
    }
};

struct Words {
    uint32_t lo_bits, hi_bits, force_ieee, force_3d, j_chunk, no_packed, spin_budget, bc_prio;
};

static std::string call(const char *name, std::initializer_list<uint32_t> args)
{
    std::string s = std::string(name) + "(";
    for (uint32_t v : args) s += (s.back() == '(' ? "" : ",") + std::to_string(v);
    return s + ")";
}
struct Names {
    std::string strict(uint32_t tile, uint32_t unroll, uint32_t lanes) const { return call("launch_strict", {tile, unroll, lanes}); }
    std::string strict_pc(uint32_t producers) const { return call("launch_strict_pc", {producers}); }
    std::string strict_bc() const { return call("launch_strict_bc", {}); }
    std::string strict_sl(uint32_t shape) const { return call("launch_strict_sl", {shape}); }
    std::string fast(uint32_t tile, uint32_t ib, uint32_t groups, uint32_t slices) const { return call("launch_fast", {tile, ib, groups, slices}); }
    std::string fast_wave(uint32_t tile, uint32_t ib, uint32_t waves, uint32_t slices) const { return call("launch_fast_wave", {tile, ib, waves, slices}); }
    std::string fast_sl(uint32_t ib, uint32_t slices) const { return call("launch_fast_sl", {ib, slices}); }
    std::string fast_pairs(uint32_t w, uint32_t np, uint32_t chunk) const { return call("launch_fast_pairs", {w, np, chunk}); }
};

static Knob *knob(DebugOverrides &d, const std::string &name)
{
    for (const KnobName &k : kKnobNames)
        if (name == k.name) return &(d.*k.knob);
    return nullptr;
}

static float from_bits(const std::string &hex)
{
    const uint32_t u = (uint32_t)std::stoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static std::string failure(int rc, const std::string &err) { return "rc=" + std::to_string(rc) + " err=\"" + err + "\""; }

static std::string results(const nb_params &p, uint32_t n, uint32_t count, const DebugOverrides &dbg, bool with_phase, uint32_t j_lo, uint32_t j_hi)
{
    const Sizes sz;
    std::string s, err;
    Plan pl;
    int rc = make_plan(p, n, count, dbg, &pl, &err);
    if (rc != NB_OK) {
        s = failure(rc, err);
    } else {
        s = "rc=0 launch=" + visit_launch(pl, Names{});
        Words w{};
        plan_step_args(pl, &w);
        const struct {
            const char *name;
            uint32_t v;
            bool hex;
        } words[] = {{"lo", w.lo_bits, true}, {"hi", w.hi_bits, true}, {"ieee", w.force_ieee, false}, {"f3d", w.force_3d, false}, {"jchunk", w.j_chunk, false},
                     {"nopk", w.no_packed, false}, {"spin", w.spin_budget, false}, {"prio", w.bc_prio, false}};
        char buf[64];
        for (const auto &x : words)
            if (x.v) {
                std::snprintf(buf, sizeof buf, x.hex ? " %s=%08x" : " %s=%u", x.name, x.v);
                s += buf;
            }
        s += " scratch=" + std::to_string(plan_scratch_bytes(pl, count, sz)) + " plan=" + plan_kernels(pl, sz);
        s += " clock=" + (count != n ? std::string("-") : !pl.stamped ? std::string("refused") : std::to_string(stamp_groups(pl, n, sz)));
    }
    if (with_phase) {
        PhasePlan pp;
        err.clear();
        rc = make_phase_plan(p, n, count, j_lo, j_hi, dbg, &pp, &err);
        if (rc != NB_OK) {
            s += " | phase " + failure(rc, err);
        } else {
            char buf[256];
            std::snprintf(buf, sizeof buf, " | phase rc=0 sl=%u groups=%u,%u slices=%u,%u chunk=%u,%u scratch=%zu", phase_sl(pp) ? 1u : 0u, pp.groups[0], pp.groups[1],
                          pp.slices[0], pp.slices[1], pp.chunk[0], pp.chunk[1], phase_scratch_bytes(pp, count, sz));
            s += buf;
        }
    }
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: plan_table <table>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "plan_table: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(in, line)) {
        const size_t arrow = line.find(" => ");
        if (arrow == std::string::npos) {
            std::fprintf(stderr, "plan_table: no ' => ' in: %s\n", line.c_str());
            return 2;
        }
        const std::string columns = line.substr(0, arrow);
        std::istringstream tokens(columns);
        nb_params p{};
        p.dt = 0.1f;
        DebugOverrides dbg;
        uint32_t n = 0, count = 0, j_lo = 0, j_hi = 0;
        bool with_phase = false;
        for (std::string t; tokens >> t;) {
            const size_t eq = t.find('=');
            const std::string key = t.substr(0, eq), value = t.substr(eq + 1);
            if (key == "G") {
                p.G = from_bits(value);
            } else if (key == "bias") {
                p.bias = from_bits(value);
            } else {
                const uint32_t v = (uint32_t)std::stoul(value, nullptr, 10);
                if (key == "mode") p.mode = v;
                else if (key == "n") n = v;
                else if (key == "count") count = v;
                else if (key == "tile") p.tile = v;
                else if (key == "jlo") j_lo = v, with_phase = true;
                else if (key == "jhi") j_hi = v;
                else if (Knob *k = knob(dbg, key)) k->set = true, k->v = v;
                else {
                    std::fprintf(stderr, "plan_table: unknown column %s\n", key.c_str());
                    return 2;
                }
            }
        }
        std::cout << columns << " => " << results(p, n, count, dbg, with_phase, j_lo, j_hi) << "\n";
    }
    return 0;
}
