// The per-graph states of graph shuffle coding with node and edge labels (ans_wl.hpp ErPush, ErPop,
// PuPush, PuPop under a label policy: the recursion of ans_rgraph.hpp over either slice model, the WL
// ids that hash the labels, and the labels' own arrays) behind the checked accessor of
// state_check.hpp, on one workspace of fixed bounds (40 nodes, 200 pairs), for the four label
// policies, both slice models, wl_iter 0 .. 3 and both settings of the half iteration.  Run by
// tests/test_labelled_state.py.
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

// the tables: cdf(0 .. nsym) with the norm last; a symbol of mass 0 in each
const uint64_t kNodeCum[] = {0, 50, 80, 90, 97, 97, 99, 100};
const uint64_t kEdgeCum[] = {0, 6, 9, 9, 10};
const rg::Cat kNode{kNodeCum, nullptr, 100, 7, 0}, kEdge{kEdgeCum, nullptr, 10, 4, 0};
const uint32_t kNodeAlphabet[] = {0, 1, 2, 3, 5, 6}, kEdgeAlphabet[] = {0, 1, 3};

// the regions of a state in the order its make() takes them: the prefix graph (a push), the slice
// model's, the decoded adjacency (a pop), the ids, the labels' arrays (a push under a policy with a label)
const std::vector<std::string> kCsr = {"pos_of", "node_at", "off", "nbr"};
const std::vector<std::string> kAdj = {"head", "next", "deg"};
const std::vector<std::string> kOrbit = {"ids", "ord", "inv", "dirty", "stamp", "sort"};
const std::vector<std::string> kSlice = {"urn", "sl", "s_ord", "rop", "por", "s_ids", "s_orb"};
const std::vector<std::string> kLabels = {"elab", "spos", "slab"};
std::vector<std::string> names_of(const std::string& state, bool push, bool labels, const std::vector<std::string>& model) {
    std::vector<std::string> names = push ? kCsr : model;
    const std::vector<std::string>& then = push ? model : kAdj;
    names.insert(names.end(), then.begin(), then.end());
    names.insert(names.end(), kOrbit.begin(), kOrbit.end());
    if (push && labels) names.insert(names.end(), kLabels.begin(), kLabels.end());
    for (auto& n : names) n = state + "." + n;
    return names;
}

struct Tally {
    uint64_t states = 0, unfilled = 0, oob = 0, stale = 0, size = 0;  // size: at the largest wl_iter
};

struct Checker : Common {
    bool shorter = false;
    uint64_t fill_tries = 0, order_bad = 0;
};

// a graph with its labels (unread under a policy without them)
struct Graph {
    uint32_t n;
    Pairs pairs;
    std::vector<uint32_t> nl, el;
};
Graph labelled(Checker& ck, uint32_t n, Pairs pairs, bool equal_labels = false) {
    Graph g{n, std::move(pairs), {}, {}};
    for (uint32_t v = 0; v < n; ++v) g.nl.push_back(equal_labels ? 0 : kNodeAlphabet[ck.below(6)]);
    for (size_t k = 0; k < g.pairs.size(); ++k) g.el.push_back(equal_labels ? 0 : kEdgeAlphabet[ck.below(3)]);
    return g;
}

// one model under one policy at one setting: its two states over the workspace
template <bool kPolya, class L>
struct Setting {
    using Push = std::conditional_t<kPolya, wl::PuPush<CheckedAcc, L>, wl::ErPush<CheckedAcc, L>>;
    using Pop = std::conditional_t<kPolya, wl::PuPop<CheckedAcc, L>, wl::ErPop<CheckedAcc, L>>;
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
        const uint64_t pe = kPolya ? wl::pu_push_entries(kMaxNodes, kMaxEdges, w, L::edge) : wl::er_push_entries(kMaxNodes, kMaxEdges, w, L::edge);
        const uint64_t qe = kPolya ? wl::pu_pop_entries(kMaxNodes, kMaxEdges, w, L::edge) : wl::er_pop_entries(kMaxNodes, kMaxEdges, w, L::edge);
        // the published sizes are what make() takes
        if (c.sh.regions[first_region + push_regions - 1].end != pe || c.sh.regions.back().end != qe) std::exit(2);
        if (c.sh.value.size() < std::max(pe, qe)) std::exit(2);
        if (c.shorter) c.sh.shorten(first_region);
        if constexpr (!kPolya) push.bern = pop.bern = ar::bern_of(900, 100);
        if constexpr (L::any) {
            push.lab.node = kNode;
            push.lab.edge = kEdge;
        }
    }
    int run_pop(Coder& c, uint32_t n, bool loops, uint32_t* out, uint64_t cap, uint64_t* count, uint32_t* nl, uint32_t* el) {
        pop.lab = rg::PopLabels{kNode, kEdge, nl, el};
        return rg::pop_graph(c, pop, n, loops, out, cap, count);
    }

    // Push g onto a seed message, pop from what the push left, the state junk before either.  True
    // when the pop gave g under the push's perm with every label in its place, a node's pairs
    // ascending as they came, the seed came back and nothing was written past an array's end.
    bool roundtrip_ok(const Graph& g, bool loops, int& rc) {
        const uint32_t n = g.n, E = static_cast<uint32_t>(g.pairs.size());
        std::vector<uint8_t> seed(400);
        for (auto& b : seed) b = static_cast<uint8_t>(ck.rng());
        seed.back() |= 1;
        std::vector<uint32_t> e(2 * size_t(E) + 2, 0xDEADBEEFu), out(2 * size_t(E) + 2, 0xDEADBEEFu), perm(n + 1, 0xDEADBEEFu);
        std::vector<uint32_t> nl_out(n + 1, 0xDEADBEEFu), el_out(E + 1, 0xDEADBEEFu);
        for (uint32_t k = 0; k < E; ++k) e[2 * k] = g.pairs[k].first, e[2 * k + 1] = g.pairs[k].second;
        ++ck.graphs;
        Msg m;
        m.tail = seed;
        Coder c{m, ANS_OK};
        if constexpr (L::any) {
            push.lab.nl = g.nl.data();
            push.lab.el = g.el.data();
        }
        ck.fresh();
        rc = rg::push_graph(c, push, n, loops, e.data(), E, perm.data());
        Msg m2;
        m2.tail = m.flatten();
        Coder c2{m2, ANS_OK};
        uint64_t count = 0;
        ck.fresh();
        if (!rc) rc = run_pop(c2, n, loops, out.data(), E, &count, nl_out.data(), el_out.data());
        if (rc != ANS_OK || count != E || perm[n] != 0xDEADBEEFu || out[2 * size_t(E)] != 0xDEADBEEFu ||
            nl_out[n] != 0xDEADBEEFu || el_out[E] != 0xDEADBEEFu)
            return false;
        std::vector<uint32_t> pos(n);
        for (uint32_t p = 0; p < n; ++p) {
            if (perm[p] >= n) return false;
            pos[perm[p]] = p;
            if (L::node && nl_out[p] != g.nl[perm[p]]) return false;
        }
        std::vector<std::pair<std::pair<uint32_t, uint32_t>, uint32_t>> want, got;
        for (uint32_t k = 0; k < E; ++k) {
            const auto [i, j] = g.pairs[k];
            want.push_back({{std::min(pos[i], pos[j]), std::max(pos[i], pos[j])}, L::edge ? g.el[k] : 0});
            got.push_back({{out[2 * k], out[2 * k + 1]}, L::edge ? el_out[k] : 0});
        }
        std::sort(want.begin(), want.end());
        // v ascending, within v w ascending: the order EdgesIID::pop's sort gives (not sorted here)
        if (!std::is_sorted(got.begin(), got.end())) ++ck.order_bad;
        if (n == 0) seed.insert(seed.end(), 2, 0);  // no step: each call is flatten(unflatten(B)) = B ++ [0]
        return got == want && m2.flatten() == seed;
    }
    void roundtrip(const Graph& g, bool loops) {
        int rc = 0;
        if (!roundtrip_ok(g, loops, rc)) {
            ++ck.roundtrip_fail;
            std::fprintf(stderr, "round trip failed: polya=%d node=%d edge=%d wl_iter=%u half=%d n=%u E=%zu loops=%d rc=%d\n", kPolya,
                         L::node, L::edge, wl_iter, half, g.n, g.pairs.size(), loops, rc);
        }
    }

    // bytes no push wrote: a graph of the alphabet, exhaustion, or more pairs than the capacity
    void hostile_pop(bool loops) {
        const uint32_t n = static_cast<uint32_t>(ck.below(kMaxNodes + 1));
        const uint64_t cap = ck.below(60);
        std::vector<uint32_t> nl(n + 1, 0xDEADBEEFu), el(cap + 1, 0xDEADBEEFu);
        const int rc = ck.hostile_pop<Coder>(n, cap, 40, loops, [&](Coder& c, uint32_t* out, uint64_t room, uint64_t* count) {
            return run_pop(c, n, loops, out, room, count, nl.data(), el.data());
        });
        if (nl[n] != 0xDEADBEEFu || el[cap] != 0xDEADBEEFu) ++ck.hostile_bad;
        switch (rc) {
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
    void run(const Graph& g, bool loops) {
        roundtrip(g, loops);
        hostile_pop(loops);
    }

    // (the sort scratch of wl_iter = 0 serves the half iteration alone)
    bool idle(int r) const { return wl_iter == 0 && !half && r == first_region + push_regions - (L::any ? 4 : 1); }
    bool idle_pop(int r) const { return wl_iter == 0 && !half && r == first_region + push_regions + pop_regions - 1; }
    bool filled() const {
        for (int r = first_region; r < first_region + push_regions + pop_regions; ++r)
            if (!ck.sh.regions[r].filled() && !idle(r) && !idle_pop(r)) return false;
        return true;
    }

    uint64_t named() {
        uint64_t count = 0;
        auto shape = [&](uint32_t n, const Pairs& g, bool loops) {
            run(labelled(ck, n, g), loops);
            ++count;
        };
        Pairs star, star_loop;
        for (uint32_t v = 1; v < kMaxNodes; ++v) star.emplace_back(0, v);
        for (uint32_t v = 0; v < kMaxNodes; ++v) star_loop.emplace_back(0, v);
        shape(0, {}, false);
        shape(1, {}, false);
        shape(1, {{0, 0}}, true);
        shape(2, {{0, 1}}, false);
        shape(kMaxNodes, star, false);      // one node of degree n - 1
        shape(kMaxNodes, star_loop, true);  // ... and its loop: the sort scratch is full
        shape(20, ck.alphabet(20, false), false);
        shape(14, ck.alphabet(14, true), true);
        shape(kMaxNodes, {}, false);
        shape(kMaxNodes, ck.random_graph(kMaxNodes, kMaxEdges, false), false);  // E = max_edges exactly
        // wl_state_check.cpp's filler: the dirty list, the urn's slice scratch and here the slice's
        // positions are full only when a node with its loop and every other node for a neighbour ends
        // at position 0.  Its labels are all equal, so that the classes are those of the graph alone.
        Pairs filler;
        for (uint32_t v = 0; v < kMaxNodes; ++v) filler.emplace_back(std::min(1u, v), std::max(1u, v));
        for (uint32_t k = 0; k < 30; ++k) {
            const std::pair<uint32_t, uint32_t> pair{2 + k % 18, 21 + (k * 7) % 18};
            if (std::find(filler.begin(), filler.end(), pair) == filler.end()) filler.push_back(pair);
        }
        const Graph fill = labelled(ck, kMaxNodes, filler, true);
        for (int tries = 0; tries < 4000 && !filled(); ++tries) {
            roundtrip(fill, true);
            --ck.graphs;
            ++ck.fill_tries;
        }
        return count;
    }
};

// a policy's settings of both models
template <class L>
struct Policy {
    std::vector<std::unique_ptr<Setting<false, L>>> er;
    std::vector<std::unique_ptr<Setting<true, L>>> pu;
    explicit Policy(Checker& ck) {
        for (uint32_t w = 0; w <= wl::kMaxIter; ++w)
            for (int h = 0; h < 2; ++h) {
                er.push_back(std::make_unique<Setting<false, L>>(ck, w, h != 0));
                pu.push_back(std::make_unique<Setting<true, L>>(ck, w, h != 0));
            }
    }
    uint64_t named() {
        uint64_t count = 0;
        for (size_t s = 0; s < er.size(); ++s) count += er[s]->named() + pu[s]->named();
        return count;
    }
    void random(Checker& ck, uint32_t graphs) {
        for (uint32_t k = 0; k < graphs; ++k) {
            const bool loops = (k / 16) & 1;
            uint32_t n = static_cast<uint32_t>(ck.below(kMaxNodes + 1)), E = static_cast<uint32_t>(ck.below(kMaxEdges + 1));
            if (k % 50 == 49) n = kMaxNodes, E = kMaxEdges;
            const Graph g = labelled(ck, n, ck.random_graph(n, E, loops));
            if (k & 1) pu[(k / 2) % pu.size()]->run(g, loops);
            else er[(k / 2) % er.size()]->run(g, loops);
        }
    }
    void tally(Checker& ck, const std::string& tag, std::vector<std::string>& order, std::map<std::string, Tally>& out) {
        auto add = [&](const std::vector<std::string>& names, int first, auto&& idle) {
            for (size_t k = 0; k < names.size(); ++k) {
                const Region& r = ck.sh.regions[first + k];
                const std::string name = tag + "." + names[k];
                if (!out.count(name)) order.push_back(name);
                Tally& t = out[name];
                t.oob += r.oob;
                t.stale += r.stale;
                t.size = r.declared_end - r.begin;
                if (r.end == r.begin || idle(first + static_cast<int>(k))) continue;  // (no such array at this setting)
                ++t.states;
                if (!r.filled()) ++t.unfilled;
            }
        };
        for (size_t s = 0; s < er.size(); ++s) {
            auto& e = *er[s];
            auto& p = *pu[s];
            add(names_of("er_push", true, L::any, {"mark"}), e.first_region, [&](int r) { return e.idle(r); });
            add(names_of("er_pop", false, L::any, {}), e.first_region + e.push_regions, [&](int r) { return e.idle_pop(r); });
            add(names_of("pu_push", true, L::any, kSlice), p.first_region, [&](int r) { return p.idle(r); });
            add(names_of("pu_pop", false, L::any, kSlice), p.first_region + p.push_regions, [&](int r) { return p.idle_pop(r); });
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    Checker ck;
    ck.shorter = short_run(argc, argv);
    ck.sh.resize(std::max(wl::pu_push_entries(kMaxNodes, kMaxEdges, wl::kMaxIter, true),
                          wl::pu_pop_entries(kMaxNodes, kMaxEdges, wl::kMaxIter, true)));
    Policy<rg::Labels<true, true>> both(ck);
    Policy<rg::Labels<true, false>> node(ck);
    Policy<rg::Labels<false, true>> edge(ck);
    Policy<rg::Labels<false, false, true>> none(ck);
    const uint64_t named = both.named() + node.named() + edge.named() + none.named();
    const uint64_t named_graphs = ck.graphs;
    both.random(ck, 600);
    node.random(ck, 300);
    edge.random(ck, 300);
    none.random(ck, 300);
    std::vector<std::string> order;
    std::map<std::string, Tally> tally;
    both.tally(ck, "ne", order, tally);
    node.tally(ck, "n", order, tally);
    edge.tally(ck, "e", order, tally);
    none.tally(ck, "none", order, tally);
    uint64_t unfilled = 0;
    for (auto& [name, t] : tally) unfilled += t.unfilled;
    std::printf("labelled_state_check:");
    Common::field("graphs", ck.graphs - named_graphs);
    Common::field("named", named);
    Common::field("fill_tries", ck.fill_tries);
    Common::field("roundtrip_fail", ck.roundtrip_fail);
    Common::field("order_bad", ck.order_bad);
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
