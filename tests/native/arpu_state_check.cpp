// The per-graph states of the autoregressive Pólya urn codecs (ans_arpu.hpp PushState, PopState: the
// recursion of ans_rgraph.hpp over PuSlices and the counts per class) behind the checked accessor of
// state_check.hpp, under each orbits value.  Run by tests/test_arpu_state.py.
#include "ans_arpu.hpp"
#include "state_check.hpp"

namespace ar = shuffle_coding::arer;
namespace ap = shuffle_coding::arpu;
namespace rg = shuffle_coding::rgraph;
using namespace state_check;
using Coder = shuffle_coding::polya::Coder<Msg>;

namespace {

constexpr uint32_t kMaxNodes = 40, kMaxEdges = 200;
constexpr int kPushRegions = 13;  // push's, then pop's over the same entries
const char* const kRegionName[] = {"pos_of", "node_at", "off", "nbr", "urn", "sl", "ord", "rop", "por", "ids", "orb", "rk",
                                   "cnt", "pop_urn", "pop_sl", "pop_ord", "pop_rop", "pop_por", "pop_ids", "pop_orb",
                                   "deg", "pop_cnt"};

struct Checker : Common {
    std::vector<uint32_t> rank;
    ap::PushState<CheckedAcc, CheckedRank> push;
    ap::PopState<CheckedAcc, CheckedRank> pop;

    explicit Checker(bool shorter) : push(make_push()), pop(make_pop(shorter)) {}
    CheckedRank ranks() { return CheckedRank{rank.data(), kMaxNodes + 1, &sh}; }
    ap::PushState<CheckedAcc, CheckedRank> make_push() {
        sh.resize(ap::push_entries(kMaxNodes, kMaxEdges));
        if (!ar::build_degree_ranks(kMaxNodes, rank)) std::exit(2);
        auto state = ap::PushState<CheckedAcc, CheckedRank>::make(CheckedWs{&sh}, kMaxNodes, kMaxEdges, 0, ranks(), kMaxNodes + 1);
        return state;
    }
    ap::PopState<CheckedAcc, CheckedRank> make_pop(bool shorter) {
        auto state = ap::PopState<CheckedAcc, CheckedRank>::make(CheckedWs{&sh}, kMaxNodes, 0, 0, ranks(), kMaxNodes + 1);
        if (sh.regions[kPushRegions - 1].end != sh.value.size() || sh.regions.back().end != ap::pop_entries(kMaxNodes))
            std::exit(2);
        if (shorter) sh.shorten();
        return state;
    }
    auto popper(uint32_t n, bool loops, int orbits) {
        pop.orb.orbits = orbits;
        return [this, n, loops](Coder& c, uint32_t* out, uint64_t cap, uint64_t* count) {
            return rg::pop_graph(c, pop, n, loops, out, cap, count);
        };
    }

    static bool identity(const std::vector<uint32_t>& perm, uint32_t n) {
        for (uint32_t p = 0; p < n; ++p)
            if (perm[p] != p) return false;
        return true;
    }
    void roundtrip(uint32_t n, const Pairs& g, bool loops, int orbits) {
        push.orb.orbits = orbits;
        int rc = 0;
        std::vector<uint32_t> perm;
        if (!Common::roundtrip<Coder>(
                n, g, n == 0, true,  // no node, no step: every slice pushes its size; v ascending, within v w ascending
                [&](Coder& c, const uint32_t* e, uint32_t E, uint32_t* p) { return rg::push_graph(c, push, n, loops, e, E, p); },
                popper(n, loops, orbits), rc, perm) ||
            (orbits == ANS_ORBITS_NONE && !identity(perm, n))) {  // (the labelled codec moves no node)
            ++roundtrip_fail;
            std::fprintf(stderr, "round trip failed: n=%u E=%zu loops=%d orbits=%d rc=%d\n", n, g.size(), loops, orbits, rc);
        }
    }

    // bytes no push wrote: a graph of the alphabet, exhaustion, a slice size above its alphabet's, or
    // more pairs than the capacity
    void hostile_pop(bool loops, int orbits) {
        const uint32_t n = static_cast<uint32_t>(below(kMaxNodes + 1));
        const uint64_t cap = below(60);
        switch (const int rc = Common::hostile_pop<Coder>(n, cap, 40, loops, popper(n, loops, orbits))) {
        case ANS_OK: break;
        case ANS_E_EXHAUSTED: ++exhausted; break;
        case ANS_E_LEN: ++len; break;
        case ANS_E_SYMBOL: ++symbol; break;
        default: bad_status(rc);
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    Checker ck(short_run(argc, argv));
    auto run = [&](uint32_t n, const Pairs& g, bool loops, int orbits) {
        ck.roundtrip(n, g, loops, orbits);
        ck.hostile_pop(loops, orbits);
    };
    // the named shapes
    uint64_t named = 0;
    for (int orbits = 0; orbits < 3; ++orbits) {
        auto shape = [&](uint32_t n, const Pairs& g, bool loops) {
            run(n, g, loops, orbits);
            ++named;
        };
        Pairs cycle, star, path, star_first, star_last, matching;
        for (uint32_t v = 0; v < kMaxNodes; ++v) star_first.emplace_back(0, v);  // a slice of max_nodes pairs
        for (uint32_t v = 0; v < kMaxNodes; ++v) star_last.emplace_back(v, kMaxNodes - 1);
        for (uint32_t v = 0; v + 1 < 12; v += 2) matching.emplace_back(v, v + 1);
        for (uint32_t v = 0; v < 8; ++v) cycle.emplace_back(std::min(v, (v + 1) % 8), std::max(v, (v + 1) % 8));
        for (uint32_t v = 1; v < 8; ++v) star.emplace_back(0, v);
        for (uint32_t v = 0; v + 1 < 6; ++v) path.emplace_back(v, v + 1);
        shape(0, {}, false);
        shape(1, {}, false);
        shape(1, {{0, 0}}, true);
        shape(2, {{0, 1}}, false);
        shape(8, cycle, false);
        shape(8, star, false);
        shape(6, path, false);
        shape(6, ck.alphabet(6, false), false);
        shape(5, {}, false);
        shape(kMaxNodes, ck.random_graph(kMaxNodes, 90, false), false);
        shape(9, ck.random_graph(9, 20, true), true);
        shape(kMaxNodes, ck.random_graph(kMaxNodes, kMaxEdges, false), false);  // nbr's last entry
        shape(20, ck.alphabet(20, false), false);  // every degree the largest
        shape(kMaxNodes, star_first, true);  // the slice scratch's last entries, the joint layer
        shape(kMaxNodes, star_last, true);   // one pair a slice
        shape(12, matching, false);
        shape(14, ck.alphabet(14, true), true);  // slices of 14 .. 1 pairs: joint and plain
        shape(13, Pairs(star_first.begin() + 1, star_first.begin() + 13), false);  // 12 pairs: the first joint size
        shape(12, Pairs(star_first.begin() + 1, star_first.begin() + 12), false);  // 11 pairs: the last plain size
    }
    const uint64_t named_graphs = ck.graphs;
    // the random graphs, the settings in turn
    for (uint32_t k = 0; k < 3000; ++k) {
        const bool loops = (k / 3) & 1;
        uint32_t n = static_cast<uint32_t>(ck.below(kMaxNodes + 1)), E = static_cast<uint32_t>(ck.below(kMaxEdges + 1));
        if (k % 50 == 49) n = kMaxNodes, E = kMaxEdges;
        run(n, ck.random_graph(n, E, loops), loops, static_cast<int>(k % 3));
    }
    std::printf("arpu_state_check:");
    Common::field("graphs", ck.graphs - named_graphs);
    Common::field("named", named);
    Common::field("roundtrip_fail", ck.roundtrip_fail);
    Common::field("hostile", ck.hostile);
    Common::field("hostile_ok", ck.hostile_ok);
    Common::field("exhausted", ck.exhausted);
    Common::field("len", ck.len);
    Common::field("symbol", ck.symbol);
    Common::field("hostile_bad", ck.hostile_bad);
    Common::field("rank_oob", ck.sh.rank_oob);
    Common::field("oob", ck.oob());
    Common::field("stale", ck.stale());
    ck.print_regions(kRegionName);
    return 0;
}
