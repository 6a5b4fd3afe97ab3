// The per-graph states of joint shuffle coding of graphs (ans_joint.hpp ErPush, ErPop, PuPush, PuPop:
// the prefix graph or the decoded adjacency, the orbit stage of ans_wl.hpp, and over it the ordered
// urn's arrays) behind the checked accessor of state_check.hpp, on one workspace of fixed bounds (40
// nodes, 200 pairs), for both ordered codecs, wl_iter 0 .. 3, both settings of the half iteration and,
// for the urn, of redraws.  The urn's arrays lie over the orbit stage's: a read of an entry the current
// call has not written is what a wrong overlap shows as.  Run by tests/test_joint_state.py.
#include <map>
#include <memory>
#include <string>

#include "ans_joint.hpp"
#include "state_check.hpp"

namespace ar = shuffle_coding::arer;
namespace jt = shuffle_coding::joint;
namespace wl = shuffle_coding::wl;
using namespace state_check;
using Coder = shuffle_coding::polya::Coder<Msg>;

namespace {

constexpr uint32_t kMaxNodes = 40, kMaxEdges = 200;

// the regions of a state in the order its make() takes them
const std::vector<std::string> kCsr = {"pos_of", "node_at", "off", "nbr"};
const std::vector<std::string> kAdj = {"head", "next", "deg"};
const std::vector<std::string> kOrbit = {"ids", "ord", "inv", "dirty", "stamp", "sort"};
const std::vector<std::string> kUrn = {"u_urn", "u_orb", "u_ord", "u_rop", "u_por", "u_head", "u_next"};
std::vector<std::string> names_of(const std::string& state, bool push, bool polya) {
    std::vector<std::string> names = push ? kCsr : kAdj;
    names.insert(names.end(), kOrbit.begin(), kOrbit.end());
    if (push) names.push_back("scr");
    if (polya) names.insert(names.end(), kUrn.begin(), kUrn.end());
    for (auto& n : names) n = state + "." + n;
    return names;
}

struct Tally {
    uint64_t states = 0, unfilled = 0, oob = 0, stale = 0, size = 0;  // size: at the largest wl_iter
};

struct Checker : Common {
    bool shorter = false;
};

// one ordered codec at one setting: its two states over the workspace
template <bool kPolya>
struct Setting {
    using Push = std::conditional_t<kPolya, jt::PuPush<CheckedAcc>, jt::ErPush<CheckedAcc>>;
    using Pop = std::conditional_t<kPolya, jt::PuPop<CheckedAcc>, jt::ErPop<CheckedAcc>>;
    Checker& ck;
    uint32_t wl_iter;
    bool half;
    int first_region, push_regions, pop_regions;
    Push push;
    Pop pop;

    uint64_t end_of(int first, int count) const {
        uint64_t end = 0;
        for (int r = first; r < first + count; ++r) end = std::max(end, ck.sh.regions[r].end);
        return end;
    }
    Setting(Checker& c, uint32_t w, bool h)
        : ck(c), wl_iter(w), half(h), first_region(static_cast<int>(c.sh.regions.size())),
          push(Push::make(CheckedWs{&c.sh}, kMaxNodes, kMaxEdges, w, h)),
          pop((push_regions = static_cast<int>(c.sh.regions.size()) - first_region,
               Pop::make(CheckedWs{&c.sh}, kMaxNodes, kMaxEdges, w, h))) {
        pop_regions = static_cast<int>(c.sh.regions.size()) - first_region - push_regions;
        const uint64_t pe = kPolya ? jt::pu_push_entries(kMaxNodes, kMaxEdges, w) : jt::er_push_entries(kMaxNodes, kMaxEdges, w);
        const uint64_t qe = kPolya ? jt::pu_pop_entries(kMaxNodes, kMaxEdges, w) : jt::er_pop_entries(kMaxNodes, kMaxEdges, w);
        // the published sizes are where the furthest region of make() ends
        if (end_of(first_region, push_regions) != pe || end_of(first_region + push_regions, pop_regions) != qe) std::exit(2);
        if (c.sh.value.size() < std::max(pe, qe)) std::exit(2);
        if (c.shorter) c.sh.shorten(first_region);
        if constexpr (!kPolya) push.bern = pop.bern = ar::bern_of(900, 100);
    }
    void redraws(bool r) {
        if constexpr (kPolya) push.redraws = pop.redraws = r;
    }
    auto popper(uint32_t n, bool loops) {
        return [this, n, loops](Coder& c, uint32_t* out, uint64_t cap, uint64_t* count) {
            return jt::pop_joint(c, pop, n, loops, out, cap, count);
        };
    }

    void roundtrip(uint32_t n, const Pairs& g, bool loops) {
        int rc = 0;
        std::vector<uint32_t> perm;
        if (!ck.roundtrip<Coder>(
                n, g, n == 0 && g.empty(), false,  // no node, no step
                [&](Coder& c, const uint32_t* e, uint32_t E, uint32_t* p) { return jt::push_joint(c, push, n, loops, e, E, p); },
                popper(n, loops), rc, perm)) {
            ++ck.roundtrip_fail;
            std::fprintf(stderr, "round trip failed: polya=%d wl_iter=%u half=%d n=%u E=%zu loops=%d rc=%d\n", kPolya, wl_iter,
                         half, n, g.size(), loops, rc);
        }
    }

    // bytes no push wrote: a graph of the alphabet, exhaustion, more pairs than the capacity; under the
    // urn also a pair decoded twice (ANS_E_SYMBOL), an urn with no mass left (ANS_E_ZERO_MASS) and two
    // decoded pairs with one orbit id (ANS_E_ARG), as ans_polya_pop has them
    void hostile_pop(bool loops) {
        const uint32_t n = static_cast<uint32_t>(ck.below(kMaxNodes + 1));
        const uint64_t cap = ck.below(60);
        switch (const int rc = ck.hostile_pop<Coder>(n, cap, 40, loops, popper(n, loops))) {
        case ANS_OK: break;
        case ANS_E_EXHAUSTED: ++ck.exhausted; break;
        case ANS_E_LEN:
            if (kPolya) ++ck.hostile_bad;
            else ++ck.len;
            break;
        case ANS_E_SYMBOL:
        case ANS_E_ZERO_MASS:
        case ANS_E_ARG:
            if (kPolya) ++ck.symbol;
            else ++ck.hostile_bad;
            break;
        default: ck.bad_status(rc);
        }
    }
    void run(uint32_t n, const Pairs& g, bool loops, bool r) {
        redraws(r);
        roundtrip(n, g, loops);
        hostile_pop(loops);
    }

    uint64_t named() {
        uint64_t count = 0;
        auto shape = [&](uint32_t n, const Pairs& g, bool loops) {
            run(n, g, loops, false);
            run(n, g, loops, true);
            count += 2;
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
        shape(kMaxNodes, star, false);      // one node of degree n - 1: every node is within distance 1 of it
        shape(kMaxNodes, star_loop, true);  // ... and its loop: the sort scratch is full
        shape(20, ck.alphabet(20, false), false);  // complete: one class
        shape(14, ck.alphabet(14, true), true);
        shape(kMaxNodes, {}, false);        // empty
        for (uint32_t E = 11; E <= 13; ++E) shape(8, ck.random_graph(8, E, false), false);  // the urn's plain / joint switch
        shape(9, ck.random_graph(9, 20, true), true);
        shape(kMaxNodes, ck.random_graph(kMaxNodes, 90, false), false);
        shape(kMaxNodes, ck.random_graph(kMaxNodes, kMaxEdges, false), false);  // E = max_edges exactly
        return count;
    }
};

}  // namespace

int main(int argc, char** argv) {
    Checker ck;
    ck.shorter = short_run(argc, argv);
    ck.sh.resize(std::max({jt::pu_push_entries(kMaxNodes, kMaxEdges, wl::kMaxIter), jt::pu_pop_entries(kMaxNodes, kMaxEdges, wl::kMaxIter),
                           jt::er_push_entries(kMaxNodes, kMaxEdges, wl::kMaxIter)}));
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
    // the random graphs, the settings and the codecs in turn
    for (uint32_t k = 0; k < 3000; ++k) {
        const bool loops = (k / 16) & 1, redraws = (k / 32) & 1;
        uint32_t n = static_cast<uint32_t>(ck.below(kMaxNodes + 1)), E = static_cast<uint32_t>(ck.below(kMaxEdges + 1));
        if (k % 50 == 49) n = kMaxNodes, E = kMaxEdges;
        const Pairs g = ck.random_graph(n, E, loops);
        if (k & 1) pu_[(k / 2) % pu_.size()]->run(n, g, loops, redraws);
        else er[(k / 2) % er.size()]->run(n, g, loops, redraws);
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
            // (the urn's Fenwick tree and its orbit counts keep one entry more than they use, as the
            // ordered urn's own state does: DESIGN.md 3.9)
            const bool spare = names[k].size() > 6 && (names[k].compare(names[k].size() - 6, 6, ".u_urn") == 0 ||
                                                        names[k].compare(names[k].size() - 6, 6, ".u_orb") == 0);
            if (spare ? r.highest < static_cast<int64_t>(r.size()) - 2 : !r.filled()) ++t.unfilled;
        }
    };
    for (size_t s = 0; s < er.size(); ++s) {
        add(names_of("er_push", true, false), er[s]->first_region);
        add(names_of("er_pop", false, false), er[s]->first_region + er[s]->push_regions);
        add(names_of("pu_push", true, true), pu_[s]->first_region);
        add(names_of("pu_pop", false, true), pu_[s]->first_region + pu_[s]->push_regions);
    }
    uint64_t unfilled = 0;
    for (auto& [name, t] : tally) unfilled += t.unfilled;
    std::printf("joint_state_check:");
    Common::field("graphs", ck.graphs - named_graphs);
    Common::field("named", named);
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
