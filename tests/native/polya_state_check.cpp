// The per-graph state of the Pólya urn edge-index codec (ans_polya.hpp State, Coder, push_graph,
// pop_graph: the functions the kernels of ans_polya.hip and the host codec run) behind the checked
// accessor of state_check.hpp.  Ws::at is called with a region's start alone, in the order urn, orb,
// ord, rop, por, head, next; a region ends where the next begins, the last at ws_entries.  Run by
// tests/test_polya_state.py.
#include <numeric>

#include "ans_polya.hpp"
#include "state_check.hpp"

namespace pu = shuffle_coding::polya;
using namespace state_check;
using Coder = pu::Coder<Msg>;

namespace {

constexpr uint32_t kMaxNodes = 40, kMaxEdges = 120;
const char* const kRegionName[] = {"urn", "orb", "ord", "rop", "por", "head", "next"};

struct Checker : Common {
    pu::State<CheckedAcc> st;
    uint64_t zero_mass = 0, arg = 0;

    explicit Checker(bool shorter) : Common(20260219), st(make(shorter)) {}
    pu::State<CheckedAcc> make(bool shorter) {
        const uint64_t entries = pu::ws_entries(kMaxNodes, kMaxEdges);
        sh.resize(entries);
        auto state = pu::State<CheckedAcc>::make(CheckedWs{&sh}, kMaxNodes, kMaxEdges);
        CheckedWs{&sh}.close(entries);
        if (shorter) sh.shorten();
        return state;
    }
    // The shared drivers take a codec that returns a perm and a count.  This one is given the number of
    // pairs and keeps the nodes' labels, so the adapters below report E pairs and the identity: the
    // drivers' checks of the count and of the perm are vacuous here, those of the pairs, the message
    // and the words past the pairs' end are not.
    auto popper(uint32_t n, bool loops, bool redraws) {
        return [this, n, loops, redraws](Coder& c, uint32_t* out, uint64_t E, uint64_t* count) {
            *count = E;
            return pu::pop_graph(c, st, n, loops, redraws, out, static_cast<uint32_t>(E));
        };
    }

    void roundtrip(uint32_t n, const Pairs& g, bool loops, bool redraws) {
        int rc = 0;
        std::vector<uint32_t> perm;
        if (!Common::roundtrip<Coder>(
                n, g, g.empty(), false,
                [&](Coder& c, const uint32_t* e, uint32_t E, uint32_t* p) {
                    std::iota(p, p + n, 0u);
                    return pu::push_graph(c, st, n, loops, redraws, e, E);
                },
                popper(n, loops, redraws), rc, perm)) {
            ++roundtrip_fail;
            std::fprintf(stderr, "round trip failed: n=%u E=%zu loops=%d redraws=%d rc=%d\n", n, g.size(), loops, redraws, rc);
        }
    }

    // bytes no push wrote
    void hostile_pop(bool loops, bool redraws) {
        const uint32_t n = 1 + static_cast<uint32_t>(below(kMaxNodes)), E = static_cast<uint32_t>(below(kMaxEdges + 1));
        switch (const int rc = Common::hostile_pop<Coder>(n, E, 300, loops, popper(n, loops, redraws))) {
        case ANS_OK: break;
        case ANS_E_EXHAUSTED: ++exhausted; break;
        case ANS_E_ZERO_MASS: ++zero_mass; break;
        case ANS_E_SYMBOL: ++symbol; break;
        case ANS_E_ARG: ++arg; break;
        default: bad_status(rc);
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    Checker ck(short_run(argc, argv));
    auto run = [&](uint32_t n, const Pairs& g, bool loops, bool redraws) {
        ck.roundtrip(n, g, loops, redraws);
        ck.hostile_pop(loops, redraws);
    };
    // the named shapes
    uint64_t named = 0;
    for (int setting = 0; setting < 4; ++setting) {
        const bool loops = setting & 1, redraws = setting & 2;
        for (uint32_t E : {0u, 1u, 11u, 12u, 13u}) {
            run(8, ck.random_graph(8, E, loops), loops, redraws);
            ++named;
        }
        Pairs path;
        for (uint32_t v = 0; v + 1 < kMaxNodes; ++v) path.emplace_back(v, v + 1);
        run(kMaxNodes, path, loops, redraws);
        ++named;
        if (!redraws) {  // the norms go down to 1; 16 nodes: 120 pairs, max_edges exactly
            run(16, ck.alphabet(16, false), loops, redraws);
            ++named;
        }
        if (!loops) {  // the hub's exclusion list: itself and its E neighbours, orb's entries 0 .. E
            Pairs star;
            for (uint32_t v = 1; v < kMaxNodes; ++v) star.emplace_back(0, v);
            run(kMaxNodes, star, loops, redraws);
            ++named;
        }
    }
    const uint64_t named_graphs = ck.graphs;
    // the random graphs, the four settings in turn
    for (uint32_t k = 0; k < 4000; ++k) {
        const bool loops = k & 1, redraws = k & 2;
        uint32_t n = 1 + static_cast<uint32_t>(ck.below(kMaxNodes)), E = static_cast<uint32_t>(ck.below(kMaxEdges + 1));
        if (k % 50 == 49) n = kMaxNodes, E = kMaxEdges;
        run(n, ck.random_graph(n, E, loops), loops, redraws);
    }
    std::printf("polya_state_check:");
    Common::field("graphs", ck.graphs - named_graphs);
    Common::field("named", named);
    Common::field("roundtrip_fail", ck.roundtrip_fail);
    Common::field("hostile", ck.hostile);
    Common::field("hostile_ok", ck.hostile_ok);
    Common::field("hostile_status", ck.exhausted + ck.zero_mass + ck.symbol + ck.arg);
    Common::field("exhausted", ck.exhausted);
    Common::field("zero_mass", ck.zero_mass);
    Common::field("symbol", ck.symbol);
    Common::field("arg", ck.arg);
    Common::field("hostile_bad", ck.hostile_bad);
    Common::field("oob", ck.oob());
    Common::field("stale", ck.stale());
    ck.print_regions(kRegionName);
    return 0;
}
