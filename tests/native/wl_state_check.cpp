// The per-graph states of graph shuffle coding with Weisfeiler-Lehman orbits (ans_wl.hpp ErPush,
// ErPop, PuPush, PuPop) behind a checked accessor: one workspace of fixed bounds (40 nodes, 200
// pairs) reused for every graph, full of junk before every push and every pop, as a lane's entries
// of the device workspace are.  The shared templates (the functions the kernels of ans_wl.hip and the
// host codec run) are instantiated, for both slice models, wl_iter 0 .. 3 and both settings of the
// half iteration, with
//   * an accessor that knows its region of the workspace (Ws::at names its start and its length)
//     and counts every access at or past the region's end (not performed: the load gives kOobValue,
//     the store is dropped) and every load of an entry that the current call has not stored (a stale
//     read: on the device another graph's leftovers);
//   * a message that is a head and a byte vector, with the renorm of src/ans.rs:233-253 under the
//     Empty generator.
// Built with ASan + UBSan and run by tests/test_wl_state.py, which parses the summary line.
// --short declares every region one entry shorter than it is: the run must then report accesses
// out of range (the check of the checker).  Those entries exist, so in that run an access to one
// is counted and performed all the same, and the codec's results still hold.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "ans_wl.hpp"

namespace ar = shuffle_coding::arer;
namespace pu = shuffle_coding::polya;
namespace wl = shuffle_coding::wl;

namespace {

constexpr uint32_t kMaxNodes = 40, kMaxEdges = 200;
constexpr uint32_t kOobValue = 0;  // what a load out of range gives (a value every caller survives)

// the regions of a state in the order its make() takes them
const std::vector<std::string> kOrbit = {"ids", "ord", "inv", "dirty", "stamp", "sort"};
const std::vector<std::string> kSlice = {"urn", "sl", "s_ord", "rop", "por", "s_ids", "s_orb"};
std::vector<std::string> names_of(const std::string& state, std::vector<std::string> own, bool slice) {
    if (slice) own.insert(own.end(), kSlice.begin(), kSlice.end());
    own.insert(own.end(), kOrbit.begin(), kOrbit.end());
    for (auto& n : own) n = state + "." + n;
    return own;
}

struct Region {
    uint64_t begin = 0, end = 0, declared_end = 0, oob = 0, stale = 0;
    int64_t highest = -1;
};
struct Shadow {
    std::vector<uint32_t> value, stamp;
    uint32_t epoch = 0;
    std::vector<Region> regions;
};

struct CheckedAcc {
    Shadow* s;
    int region;
    bool in_range(uint32_t i) const {
        Region& r = s->regions[region];
        const uint64_t at = r.begin + i;
        if (at >= r.declared_end) ++r.oob;
        if (at >= r.end) return false;
        r.highest = std::max<int64_t>(r.highest, i);
        return true;
    }
    uint32_t load(uint32_t i) const {
        if (!in_range(i)) return kOobValue;
        Region& r = s->regions[region];
        const uint64_t at = r.begin + i;
        if (s->stamp[at] != s->epoch) ++r.stale;
        return s->value[at];
    }
    void store(uint32_t i, uint32_t v) {
        if (!in_range(i)) return;
        const uint64_t at = s->regions[region].begin + i;
        s->value[at] = v;
        s->stamp[at] = s->epoch;
    }
};
struct CheckedWs {
    Shadow* s;
    CheckedAcc at(uint64_t o, uint64_t count) const {
        Region r;
        r.begin = o;
        r.end = r.declared_end = o + count;
        s->regions.push_back(r);
        return CheckedAcc{s, static_cast<int>(s->regions.size()) - 1};
    }
};

// Message::unflatten(bytes) with the Empty generator: head 0, the bytes as the tail
struct Msg {
    uint64_t head = 0;
    std::vector<uint8_t> tail;
    bool renorm(uint64_t min_head) {
        while (head < min_head) {
            if (tail.empty()) return false;  // src/ans.rs:144
            head = (head << 8) | tail.back();
            tail.pop_back();
        }
        while ((head >> 8) >= min_head) {
            tail.push_back(static_cast<uint8_t>(head));
            head >>= 8;
        }
        return true;
    }
    std::vector<uint8_t> flatten() const {  // src/ans.rs:255-260
        std::vector<uint8_t> b = tail;
        uint64_t h = head;
        while ((h >> 8) >= 1) {
            b.push_back(static_cast<uint8_t>(h));
            h >>= 8;
        }
        b.push_back(static_cast<uint8_t>(h));
        return b;
    }
};

using Pairs = std::vector<std::pair<uint32_t, uint32_t>>;

// what the run adds up per region name, over the settings
struct Tally {
    uint64_t states = 0, unfilled = 0, oob = 0, stale = 0, size = 0;  // size: at the largest wl_iter
};

struct Common {
    std::mt19937_64 rng{20261021};
    Shadow sh;
    bool shorter = false;
    uint64_t graphs = 0, roundtrip_fail = 0, hostile = 0, hostile_ok = 0, hostile_bad = 0, exhausted = 0, len = 0,
             symbol = 0, fill_tries = 0;
    uint64_t below(uint64_t n) { return rng() % n; }
    // what a lane finds: every entry holds something, none of it this call's
    void fresh() {
        ++sh.epoch;
        for (auto& v : sh.value) v = static_cast<uint32_t>(rng());
    }
    Pairs alphabet(uint32_t n, bool loops) {
        Pairs all;
        for (uint32_t j = 0; j < n; ++j)
            for (uint32_t i = 0; i < (loops ? j + 1 : j); ++i) all.emplace_back(i, j);
        return all;
    }
    Pairs random_graph(uint32_t n, uint32_t want, bool loops) {
        Pairs all = alphabet(n, loops);
        const size_t E = std::min<size_t>(want, all.size());
        for (size_t k = 0; k < E; ++k) std::swap(all[k], all[k + below(all.size() - k)]);
        all.resize(E);
        return all;
    }
};

// one model at one setting: its two states over the workspace
template <bool kPolya>
struct Setting {
    using Push = std::conditional_t<kPolya, wl::PuPush<CheckedAcc>, wl::ErPush<CheckedAcc>>;
    using Pop = std::conditional_t<kPolya, wl::PuPop<CheckedAcc>, wl::ErPop<CheckedAcc>>;
    Common& ck;
    uint32_t wl_iter;
    bool half;
    int first_region, push_regions, pop_regions;
    Push push;
    Pop pop;
    const ar::Bern bern = ar::bern_of(900, 100);

    Setting(Common& c, uint32_t w, bool h)
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
        if (c.shorter)
            for (size_t r = first_region; r < c.sh.regions.size(); ++r)
                if (c.sh.regions[r].end > c.sh.regions[r].begin) --c.sh.regions[r].declared_end;
    }
    int do_push(pu::Coder<Msg>& c, uint32_t n, bool loops, const uint32_t* e, uint32_t E, uint32_t* perm) {
        if constexpr (kPolya) return wl::pu_push_graph(c, push, n, loops, e, E, perm);
        else return wl::er_push_graph(c, push, bern, n, loops, e, E, perm);
    }
    int do_pop(pu::Coder<Msg>& c, uint32_t n, bool loops, uint32_t* out, uint64_t cap, uint64_t* count) {
        if constexpr (kPolya) return wl::pu_pop_graph(c, pop, n, loops, out, cap, count);
        else return wl::er_pop_graph(c, pop, bern, n, loops, out, cap, count);
    }

    // push onto the seed, pop from what the push left; the state is junk before either
    void roundtrip(uint32_t n, const Pairs& g, bool loops) {
        const uint32_t E = static_cast<uint32_t>(g.size());
        std::vector<uint8_t> seed(400);
        for (auto& b : seed) b = static_cast<uint8_t>(ck.rng());
        seed.back() |= 1;  // a nonzero top byte: the seed comes back byte for byte
        std::vector<uint32_t> e(2 * size_t(E) + 2, 0xDEADBEEFu), out(2 * size_t(E) + 2, 0xDEADBEEFu), perm(n + 1, 0xDEADBEEFu);
        for (uint32_t k = 0; k < E; ++k) {
            e[2 * k] = g[k].first;
            e[2 * k + 1] = g[k].second;
        }
        ++ck.graphs;
        Msg m;
        m.tail = seed;
        pu::Coder<Msg> c{m, ANS_OK};
        ck.fresh();
        int rc = do_push(c, n, loops, e.data(), E, perm.data());
        Msg m2;
        m2.tail = m.flatten();
        pu::Coder<Msg> c2{m2, ANS_OK};
        uint64_t count = 0;
        ck.fresh();
        if (!rc) rc = do_pop(c2, n, loops, out.data(), E, &count);
        bool ok = rc == ANS_OK && count == E && perm[n] == 0xDEADBEEFu && out[2 * size_t(E)] == 0xDEADBEEFu;
        if (ok) {
            std::vector<uint32_t> pos(n);
            for (uint32_t p = 0; p < n; ++p) {
                if (perm[p] >= n) return fail(n, E, loops, rc);
                pos[perm[p]] = p;
            }
            Pairs want, got;
            for (auto& [i, j] : g) want.emplace_back(std::min(pos[i], pos[j]), std::max(pos[i], pos[j]));
            for (uint32_t k = 0; k < E; ++k) got.emplace_back(out[2 * k], out[2 * k + 1]);
            std::sort(want.begin(), want.end());
            std::sort(got.begin(), got.end());
            std::vector<uint8_t> rest = seed;
            if (n == 0) rest.insert(rest.end(), 2, 0);  // without a step each call is flatten(unflatten(B)) = B ++ [0]
            ok = got == want && m2.flatten() == rest;
        }
        if (!ok) fail(n, E, loops, rc);
    }
    void fail(uint32_t n, uint32_t E, bool loops, int rc) {
        ++ck.roundtrip_fail;
        std::fprintf(stderr, "round trip failed: polya=%d wl_iter=%u half=%d n=%u E=%u loops=%d rc=%d\n", kPolya, wl_iter,
                     half, n, E, loops, rc);
    }

    // bytes no push wrote: a graph of the alphabet, exhaustion, or more pairs than the capacity
    void hostile_pop(bool loops) {
        const uint32_t n = static_cast<uint32_t>(ck.below(kMaxNodes + 1));
        const uint64_t cap = ck.below(60);
        Msg m;
        m.tail.resize(1 + ck.below(40));
        for (auto& b : m.tail) b = static_cast<uint8_t>(ck.rng());
        std::vector<uint32_t> out(2 * cap + 2, 0xDEADBEEFu);
        pu::Coder<Msg> c{m, ANS_OK};
        uint64_t count = 0;
        ck.fresh();
        const int rc = do_pop(c, n, loops, out.data(), cap, &count);
        ++ck.hostile;
        if (out[2 * cap] != 0xDEADBEEFu) ++ck.hostile_bad;
        switch (rc) {
        case ANS_OK:
            ++ck.hostile_ok;
            for (uint64_t k = 0; k < count; ++k) {
                const uint32_t i = out[2 * k], j = out[2 * k + 1];
                if (count > cap || i > j || j >= n || (i == j && !loops)) {
                    ++ck.hostile_bad;
                    std::fprintf(stderr, "hostile pop: pair (%u, %u) outside the alphabet, n=%u\n", i, j, n);
                    break;
                }
            }
            break;
        case ANS_E_EXHAUSTED: ++ck.exhausted; break;
        case ANS_E_LEN: ++ck.len; break;
        case ANS_E_SYMBOL:  // the urn's slices alone: a decoded slice size above the alphabet's
            if (kPolya) ++ck.symbol;
            else ++ck.hostile_bad;
            break;
        default:
            ++ck.hostile_bad;
            std::fprintf(stderr, "hostile pop: status %d\n", rc);
        }
    }
    void run(uint32_t n, const Pairs& g, bool loops) {
        roundtrip(n, g, loops);
        hostile_pop(loops);
    }

    bool filled() const {
        for (int r = first_region; r < first_region + push_regions + pop_regions; ++r) {
            const Region& reg = ck.sh.regions[r];
            if (reg.end > reg.begin && reg.highest != static_cast<int64_t>(reg.end - reg.begin) - 1) return false;
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
    Common ck;
    ck.shorter = argc > 1 && std::strcmp(argv[1], "--short") == 0;
    const uint64_t entries = std::max(wl::pu_push_entries(kMaxNodes, kMaxEdges, wl::kMaxIter),
                                      wl::pu_pop_entries(kMaxNodes, kMaxEdges, wl::kMaxIter));
    ck.sh.value.assign(entries, 0);
    ck.sh.stamp.assign(entries, 0);
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
            if (r.highest != static_cast<int64_t>(r.end - r.begin) - 1) ++t.unfilled;
        }
    };
    for (size_t s = 0; s < er.size(); ++s) {
        add(names_of("er_push", {"pos_of", "node_at", "off", "nbr", "mark"}, false), er[s]->first_region);
        add(names_of("er_pop", {"head", "next", "deg"}, false), er[s]->first_region + er[s]->push_regions);
        add(names_of("pu_push", {"pos_of", "node_at", "off", "nbr"}, true), pu_[s]->first_region);
        add(names_of("pu_pop", {"head", "next", "deg"}, true), pu_[s]->first_region + pu_[s]->push_regions);
    }
    uint64_t oob = 0, stale = 0, unfilled = 0;
    for (auto& [name, t] : tally) oob += t.oob, stale += t.stale, unfilled += t.unfilled;
    std::printf("wl_state_check: graphs=%llu named=%llu fill_tries=%llu roundtrip_fail=%llu hostile=%llu hostile_ok=%llu "
                "exhausted=%llu len=%llu symbol=%llu hostile_bad=%llu oob=%llu stale=%llu unfilled=%llu",
                (unsigned long long)(ck.graphs - named_graphs), (unsigned long long)named, (unsigned long long)ck.fill_tries,
                (unsigned long long)ck.roundtrip_fail, (unsigned long long)ck.hostile, (unsigned long long)ck.hostile_ok,
                (unsigned long long)ck.exhausted, (unsigned long long)ck.len, (unsigned long long)ck.symbol,
                (unsigned long long)ck.hostile_bad, (unsigned long long)oob, (unsigned long long)stale,
                (unsigned long long)unfilled);
    for (auto& name : order) {
        const Tally& t = tally[name];
        std::printf(" %s:size=%llu,states=%llu,unfilled=%llu,oob=%llu,stale=%llu", name.c_str(), (unsigned long long)t.size,
                    (unsigned long long)t.states, (unsigned long long)t.unfilled, (unsigned long long)t.oob,
                    (unsigned long long)t.stale);
    }
    std::printf("\n");
    return 0;
}
