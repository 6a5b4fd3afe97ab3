// The per-graph states of graph shuffle coding with Weisfeiler-Lehman orbits (ans_wl.hpp ErPush,
// ErPop, PuPush, PuPop: the recursion of ans_rgraph.hpp over either slice model and the WL ids) behind
// the checked accessor of state_check.hpp, on one workspace of fixed bounds (40 nodes, 200 pairs), for
// both slice models, wl_iter 0 .. 3 and both settings of the half iteration.  Run by
// tests/test_wl_state.py.
#include <map>
#include <memory>
#include <string>

#include "ans_wl.hpp"
#include "state_check.hpp"

namespace ar = shuffle_coding::arer;
namespace rg = shuffle_coding::rgraph;
namespace wl = shuffle_coding::wl;
using namespace state_check;
using Coder = shuffle_coding::polya::Coder<Msg>;

namespace {

constexpr uint32_t kMaxNodes = 40, kMaxEdges = 200;

// the regions of a state in the order its make() takes them: the prefix graph (a push), the slice
// model's, the decoded adjacency (a pop), the ids
const std::vector<std::string> kCsr = {"pos_of", "node_at", "off", "nbr"};
const std::vector<std::string> kAdj = {"head", "next", "deg"};
const std::vector<std::string> kOrbit = {"ids", "ord", "inv", "dirty", "stamp", "sort"};
const std::vector<std::string> kSlice = {"urn", "sl", "s_ord", "rop", "por", "s_ids", "s_orb"};
std::vector<std::string> names_of(const std::string& state, bool push, const std::vector<std::string>& model) {
    std::vector<std::string> names = push ? kCsr : model;
    const std::vector<std::string>& then = push ? model : kAdj;
    names.insert(names.end(), then.begin(), then.end());
    names.insert(names.end(), kOrbit.begin(), kOrbit.end());
    for (auto& n : names) n = state + "." + n;
    return names;
}

// what the run adds up per region name, over the settings
struct Tally {
    uint64_t states = 0, unfilled = 0, oob = 0, stale = 0, size = 0;  // size: at the largest wl_iter
};

struct Checker : Common {
    bool shorter = false;
    uint64_t fill_tries = 0;
};

// one model at one setting: its two states over the workspace
template <bool kPolya>
struct Setting {
    using Push = std::conditional_t<kPolya, wl::PuPush<CheckedAcc>, wl::ErPush<CheckedAcc>>;
    using Pop = std::conditional_t<kPolya, wl::PuPop<CheckedAcc>, wl::ErPop<CheckedAcc>>;
    Checker& ck;
    uint32_t wl_iter;
    bool half;
    int first_region, push_regions, pop_regions;
    Push push;
    Pop pop;

    Setting(Checker& c, uint32_t w, bool h)
        : ck(c), wl_iter(w), half(h), first_region(static_cast<int>(c.sh.regions.size())),
          push(Push::make(CheckedWs{&c.sh}, kMaxNodes, kMaxEdges, w, h)),
          pop((push_regions = static_cast<int>(c.sh.regions.size()) - first_region,
               Pop::make(CheckedWs{&c.sh}, kMaxNodes, kMaxEdges, w, h))) {
        pop_regions = static_cast<int>(c.sh.regions.size()) - first_region - push_regions;
        const uint64_t pe = kPolya ? wl::pu_push_entries(kMaxNodes, kMaxEdges, w) : wl::er_push_entries(kMaxNodes, kMaxEdges, w);
        const uint64_t qe = kPolya ? wl::pu_pop_entries(kMaxNodes, kMaxEdges, w) : wl::er_pop_entries(kMaxNodes, kMaxEdges, w);
        // the published sizes are what make() takes
        if (c.sh.regions[first_region + push_regions - 1].end != pe || c.sh.regions.back().end != qe) std::exit(2);
        if (c.sh.value.size() < std::max(pe, qe)) std::exit(2);
        if (c.shorter) c.sh.shorten(first_region);
        if constexpr (!kPolya) push.bern = pop.bern = ar::bern_of(900, 100);
    }
    auto popper(uint32_t n, bool loops) {
        return [this, n, loops](Coder& c, uint32_t* out, uint64_t cap, uint64_t* count) {
            return rg::pop_graph(c, pop, n, loops, out, cap, count);
        };
    }

    void roundtrip(uint32_t n, const Pairs& g, bool loops) {
        int rc = 0;
        std::vector<uint32_t> perm;
        if (!ck.roundtrip<Coder>(
                n, g, n == 0, false,  // no node, no step
                [&](Coder& c, const uint32_t* e, uint32_t E, uint32_t* p) { return rg::push_graph(c, push, n, loops, e, E, p); },
                popper(n, loops), rc, perm)) {
            ++ck.roundtrip_fail;
            std::fprintf(stderr, "round trip failed: polya=%d wl_iter=%u half=%d n=%u E=%zu loops=%d rc=%d\n", kPolya, wl_iter,
                         half, n, g.size(), loops, rc);
        }
    }

    // bytes no push wrote: a graph of the alphabet, exhaustion, or more pairs than the capacity
    void hostile_pop(bool loops) {
        const uint32_t n = static_cast<uint32_t>(ck.below(kMaxNodes + 1));
        const uint64_t cap = ck.below(60);
        switch (const int rc = ck.hostile_pop<Coder>(n, cap, 40, loops, popper(n, loops))) {
        case ANS_OK: break;
        case ANS_E_EXHAUSTED: ++ck.exhausted; break;
        case ANS_E_LEN: ++ck.len; break;
        case ANS_E_SYMBOL:  // the urn's slices alone: a decoded slice size above the alphabet's
            if (kPolya) ++ck.symbol;
            else ++ck.hostile_bad;
            break;
        default: ck.bad_status(rc);
        }
    }
    void run(uint32_t n, const Pairs& g, bool loops) {
        roundtrip(n, g, loops);
        hostile_pop(loops);
    }

    bool filled() const {
        for (int r = first_region; r < first_region + push_regions + pop_regions; ++r) {
            if (!ck.sh.regions[r].filled()) return false;
        }
        return true;
    }

    uint64_t named() {
        uint64_t count = 0;
        auto shape = [&](uint32_t n, const Pairs& g, bool loops) {
            run(n, g, loops);
            ++count;
        };
        Pairs cycle, star, path, star_loop;
        for (uint32_t v = 0; v < 8; ++v) cycle.emplace_back(std::min(v, (v + 1) % 8), std::max(v, (v + 1) % 8));
        for (uint32_t v = 1; v < kMaxNodes; ++v) star.emplace_back(0, v);
        for (uint32_t v = 0; v < kMaxNodes; ++v) star_loop.emplace_back(0, v);
        for (uint32_t v = 0; v + 1 < 6; ++v) path.emplace_back(v, v + 1);
        shape(0, {}, false);
        shape(1, {}, false);
        shape(1, {{0, 0}}, true);
        shape(2, {{0, 1}}, false);
        shape(8, cycle, false);
        shape(6, path, false);
        shape(kMaxNodes, star, false);      // one node of degree n - 1
        shape(kMaxNodes, star_loop, true);  // ... and its loop: the sort scratch is full
        shape(20, ck.alphabet(20, false), false);  // complete: every id changes every step, one class
        shape(14, ck.alphabet(14, true), true);
        shape(kMaxNodes, {}, false);        // empty
        shape(9, ck.random_graph(9, 20, true), true);
        shape(kMaxNodes, ck.random_graph(kMaxNodes, 90, false), false);
        shape(kMaxNodes, ck.random_graph(kMaxNodes, kMaxEdges, false), false);  // E = max_edges exactly
        // The dirty list (at wl_iter = 0) and the urn's slice scratch are full only when a node with
        // its loop and every other node for a neighbour ends at position 0, every other node unknown.
        // The message decides that; with one class (wl_iter = 0 without the half iteration) it is input
        // node 1 that ends there whatever the message.  So: a star around node 1 with its loop, and a
        // few pairs between the leaves (more classes: without them and without the half iteration the
        // centre never came last in thousands of seeds), from fresh seeds until it has happened, a few
        // in a hundred pushes (the generator is seeded, so the count is the same every run).
        Pairs filler;
        for (uint32_t v = 0; v < kMaxNodes; ++v) filler.emplace_back(std::min(1u, v), std::max(1u, v));
        for (uint32_t k = 0; k < 30; ++k) {
            const std::pair<uint32_t, uint32_t> pair{2 + k % 18, 21 + (k * 7) % 18};
            if (std::find(filler.begin(), filler.end(), pair) == filler.end()) filler.push_back(pair);
        }
        for (int tries = 0; tries < 4000 && !filled(); ++tries) {
            roundtrip(kMaxNodes, filler, true);
            --ck.graphs;
            ++ck.fill_tries;
        }
        return count;
    }
};

}  // namespace

int main(int argc, char** argv) {
    Checker ck;
    ck.shorter = short_run(argc, argv);
    ck.sh.resize(std::max(wl::pu_push_entries(kMaxNodes, kMaxEdges, wl::kMaxIter),
                          wl::pu_pop_entries(kMaxNodes, kMaxEdges, wl::kMaxIter)));
    std::vector<std::unique_ptr<Setting<false>>> er;
    std::vector<std::unique_ptr<Setting<true>>> pu_;
    for (uint32_t w = 0; w <= wl::kMaxIter; ++w)
        for (int h = 0; h < 2; ++h) {
            er.push_back(std::make_unique<Setting<false>>(ck, w, h != 0));
            pu_.push_back(std::make_unique<Setting<true>>(ck, w, h != 0));
        }
    uint64_t named = 0;
    for (size_t s = 0; s < er.size(); ++s) named += er[s]->named() + pu_[s]->named();
    const uint64_t named_graphs = ck.graphs;
    // the random graphs, the settings and the models in turn
    for (uint32_t k = 0; k < 3000; ++k) {
        const bool loops = (k / 16) & 1;
        uint32_t n = static_cast<uint32_t>(ck.below(kMaxNodes + 1)), E = static_cast<uint32_t>(ck.below(kMaxEdges + 1));
        if (k % 50 == 49) n = kMaxNodes, E = kMaxEdges;
        const Pairs g = ck.random_graph(n, E, loops);
        if (k & 1) pu_[(k / 2) % pu_.size()]->run(n, g, loops);
        else er[(k / 2) % er.size()]->run(n, g, loops);
    }
    // per region name over the settings
    std::vector<std::string> order;
    std::map<std::string, Tally> tally;
    auto add = [&](const std::vector<std::string>& names, int first) {
        for (size_t k = 0; k < names.size(); ++k) {
            const Region& r = ck.sh.regions[first + k];
            if (!tally.count(names[k])) order.push_back(names[k]);
            Tally& t = tally[names[k]];
            t.oob += r.oob;
            t.stale += r.stale;
            t.size = r.declared_end - r.begin;
            if (r.end == r.begin) continue;  // (the sort scratch at wl_iter = 0)
            ++t.states;
            if (!r.filled()) ++t.unfilled;
        }
    };
    for (size_t s = 0; s < er.size(); ++s) {
        add(names_of("er_push", true, {"mark"}), er[s]->first_region);
        add(names_of("er_pop", false, {}), er[s]->first_region + er[s]->push_regions);
        add(names_of("pu_push", true, kSlice), pu_[s]->first_region);
        add(names_of("pu_pop", false, kSlice), pu_[s]->first_region + pu_[s]->push_regions);
    }
    uint64_t unfilled = 0;
    for (auto& [name, t] : tally) unfilled += t.unfilled;
    std::printf("wl_state_check:");
    Common::field("graphs", ck.graphs - named_graphs);
    Common::field("named", named);
    Common::field("fill_tries", ck.fill_tries);
    Common::field("roundtrip_fail", ck.roundtrip_fail);
    Common::field("hostile", ck.hostile);
    Common::field("hostile_ok", ck.hostile_ok);
    Common::field("exhausted", ck.exhausted);
    Common::field("len", ck.len);
    Common::field("symbol", ck.symbol);
    Common::field("hostile_bad", ck.hostile_bad);
    Common::field("oob", ck.oob());
    Common::field("stale", ck.stale());
    Common::field("unfilled", unfilled);
    for (auto& name : order) {
        const Tally& t = tally[name];
        std::printf(" %s:size=%llu,states=%llu,unfilled=%llu,oob=%llu,stale=%llu", name.c_str(), (unsigned long long)t.size,
                    (unsigned long long)t.states, (unsigned long long)t.unfilled, (unsigned long long)t.oob,
                    (unsigned long long)t.stale);
    }
    std::printf("\n");
    return 0;
}
