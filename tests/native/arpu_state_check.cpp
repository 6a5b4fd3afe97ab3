// The per-graph states of the autoregressive Pólya urn codecs (ans_arpu.hpp PushState, PopState)
// behind a checked accessor: one workspace of fixed bounds reused for every graph, full of junk
// before every push and every pop, as a lane's entries of the device workspace are.  The shared
// templates (PushState, PopState, push_graph, pop_graph: the functions the kernels of ans_arpu.hip
// and the host codec run) are instantiated with
//   * an accessor that knows its region of the workspace (Ws::at names its start and its length)
//     and counts every access at or past the region's end (not performed: the load gives kOobValue,
//     the store is dropped) and every load of an entry that the current call has not stored (a stale
//     read: on the device another graph's leftovers);
//   * a rank table that counts a read past its max_nodes + 1 entries;
//   * a message that is a head and a byte vector, with the renorm of src/ans.rs:233-253 under the
//     Empty generator.
// Built with ASan + UBSan and run by tests/test_arpu_state.py, which parses the summary line.
// --short declares every region one entry shorter than it is: the run must then report accesses
// out of range (the check of the checker).  Those entries exist, so in that run an access to one
// is counted and performed all the same, and the codec's results still hold.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "ans_arpu.hpp"

namespace ar = shuffle_coding::arer;
namespace ap = shuffle_coding::arpu;
namespace pu = shuffle_coding::polya;

namespace {

constexpr uint32_t kMaxNodes = 40, kMaxEdges = 200;
constexpr int kPushRegions = 13, kRegions = 22;  // push's, then pop's over the same entries
const char* const kRegionName[kRegions] = {"pos_of", "node_at", "off", "nbr", "rk", "cnt", "urn", "sl", "ord", "rop", "por",
                                           "ids", "orb", "deg", "pop_cnt", "pop_urn", "pop_sl", "pop_ord", "pop_rop",
                                           "pop_por", "pop_ids", "pop_orb"};
constexpr uint32_t kOobValue = 0;  // what a load out of range gives (a value every caller survives)

struct Shadow {
    std::vector<uint32_t> value, stamp;
    uint32_t epoch = 0;
    std::array<uint64_t, kRegions> begin{}, end{}, declared_end{}, oob{}, stale{};
    std::array<int64_t, kRegions> highest;
    int regions = 0;
    uint64_t rank_oob = 0;
    Shadow() { highest.fill(-1); }
};

struct CheckedAcc {
    Shadow* s;
    int region;
    bool in_range(uint32_t i) const {
        const uint64_t at = s->begin[region] + i;
        if (at >= s->declared_end[region]) ++s->oob[region];
        if (at >= s->end[region]) return false;
        s->highest[region] = std::max<int64_t>(s->highest[region], i);
        return true;
    }
    uint32_t load(uint32_t i) const {
        if (!in_range(i)) return kOobValue;
        const uint64_t at = s->begin[region] + i;
        if (s->stamp[at] != s->epoch) ++s->stale[region];
        return s->value[at];
    }
    void store(uint32_t i, uint32_t v) {
        if (!in_range(i)) return;
        const uint64_t at = s->begin[region] + i;
        s->value[at] = v;
        s->stamp[at] = s->epoch;
    }
};
struct CheckedWs {
    Shadow* s;
    CheckedAcc at(uint64_t o, uint64_t count) const {
        const int r = s->regions++;
        s->begin[r] = o;
        s->end[r] = o + count;
        return CheckedAcc{s, r};
    }
};
struct CheckedRank {
    const uint32_t* p;
    uint32_t entries;
    Shadow* s;
    uint32_t operator[](uint32_t d) const {
        if (d < entries) return p[d];
        ++s->rank_oob;
        return 0;
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

struct Checker {
    std::mt19937_64 rng{20261021};
    Shadow sh;
    std::vector<uint32_t> rank;
    ap::PushState<CheckedAcc> push;
    ap::PopState<CheckedAcc> pop;
    uint64_t graphs = 0, roundtrip_fail = 0, hostile = 0, hostile_ok = 0, hostile_bad = 0, exhausted = 0, len = 0, symbol = 0;

    explicit Checker(bool shorter) : push(make_push()), pop(make_pop(shorter)) {}
    ap::PushState<CheckedAcc> make_push() {
        const uint64_t entries = ap::push_entries(kMaxNodes, kMaxEdges);
        sh.value.assign(entries, 0);
        sh.stamp.assign(entries, 0);
        if (!ar::build_degree_ranks(kMaxNodes, rank)) std::exit(2);
        return ap::PushState<CheckedAcc>::make(CheckedWs{&sh}, kMaxNodes, kMaxEdges);
    }
    ap::PopState<CheckedAcc> make_pop(bool shorter) {
        auto state = ap::PopState<CheckedAcc>::make(CheckedWs{&sh}, kMaxNodes);
        if (sh.regions != kRegions || sh.end[kPushRegions - 1] != sh.value.size() ||
            sh.end[kRegions - 1] != ap::pop_entries(kMaxNodes))
            std::exit(2);
        sh.declared_end = sh.end;
        if (shorter)
            for (auto& e : sh.declared_end) --e;
        return state;
    }
    // what a lane finds: every entry holds something, none of it this call's
    void fresh() {
        ++sh.epoch;
        for (auto& v : sh.value) v = static_cast<uint32_t>(rng());
    }
    uint64_t below(uint64_t n) { return rng() % n; }
    CheckedRank ranks() { return CheckedRank{rank.data(), kMaxNodes + 1, &sh}; }

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

    // push onto the seed, pop from what the push left; the state is junk before either
    void roundtrip(uint32_t n, const Pairs& g, bool loops, int orbits) {
        const uint32_t E = static_cast<uint32_t>(g.size());
        std::vector<uint8_t> seed(400);
        for (auto& b : seed) b = static_cast<uint8_t>(rng());
        seed.back() |= 1;  // a nonzero top byte: the seed comes back byte for byte
        std::vector<uint32_t> e(2 * size_t(E) + 2, 0xDEADBEEFu), out(2 * size_t(E) + 2, 0xDEADBEEFu), perm(n + 1, 0xDEADBEEFu);
        for (uint32_t k = 0; k < E; ++k) {
            e[2 * k] = g[k].first;
            e[2 * k + 1] = g[k].second;
        }
        ++graphs;
        Msg m;
        m.tail = seed;
        pu::Coder<Msg> c{m, ANS_OK};
        fresh();
        int rc = ap::push_graph(c, push, n, loops, orbits, ranks(), kMaxNodes + 1, e.data(), E, perm.data());
        Msg m2;
        m2.tail = m.flatten();
        pu::Coder<Msg> c2{m2, ANS_OK};
        uint64_t count = 0;
        fresh();
        if (!rc) rc = ap::pop_graph(c2, pop, n, loops, orbits, ranks(), kMaxNodes + 1, out.data(), E, &count);
        bool ok = rc == ANS_OK && count == E && perm[n] == 0xDEADBEEFu;
        if (ok) {
            std::vector<uint32_t> pos(n);
            for (uint32_t p = 0; p < n; ++p) {
                if (perm[p] >= n) return fail(n, E, loops, orbits, rc);
                pos[perm[p]] = p;
            }
            Pairs want, got;
            for (auto& [i, j] : g) want.emplace_back(std::min(pos[i], pos[j]), std::max(pos[i], pos[j]));
            for (uint32_t k = 0; k < E; ++k) got.emplace_back(out[2 * k], out[2 * k + 1]);
            std::sort(want.begin(), want.end());
            // the pairs come v ascending, within v by w ascending: sorted as they are
            std::vector<uint8_t> rest = seed;
            // without a step (no node: every slice pushes its size) each call is flatten(unflatten(B)) = B ++ [0]
            if (n == 0) rest.insert(rest.end(), 2, 0);
            bool identity = true;
            for (uint32_t p = 0; p < n; ++p) identity = identity && perm[p] == p;
            ok = got == want && m2.flatten() == rest && (orbits != ANS_ORBITS_NONE || identity);
        }
        if (!ok) fail(n, E, loops, orbits, rc);
    }
    void fail(uint32_t n, uint32_t E, bool loops, int orbits, int rc) {
        ++roundtrip_fail;
        std::fprintf(stderr, "round trip failed: n=%u E=%u loops=%d orbits=%d rc=%d\n", n, E, loops, orbits, rc);
    }

    // bytes no push wrote: a graph of the alphabet, exhaustion, a slice size above its alphabet's, or
    // more pairs than the capacity
    void hostile_pop(bool loops, int orbits) {
        const uint32_t n = static_cast<uint32_t>(below(kMaxNodes + 1));
        const uint64_t cap = below(60);
        Msg m;
        m.tail.resize(1 + below(40));
        for (auto& b : m.tail) b = static_cast<uint8_t>(rng());
        std::vector<uint32_t> out(2 * cap + 2, 0xDEADBEEFu);
        pu::Coder<Msg> c{m, ANS_OK};
        uint64_t count = 0;
        fresh();
        const int rc = ap::pop_graph(c, pop, n, loops, orbits, ranks(), kMaxNodes + 1, out.data(), cap, &count);
        ++hostile;
        if (out[2 * cap] != 0xDEADBEEFu) ++hostile_bad;
        switch (rc) {
        case ANS_OK:
            ++hostile_ok;
            for (uint64_t k = 0; k < count; ++k) {
                const uint32_t i = out[2 * k], j = out[2 * k + 1];
                if (count > cap || i > j || j >= n || (i == j && !loops)) {
                    ++hostile_bad;
                    std::fprintf(stderr, "hostile pop: pair (%u, %u) outside the alphabet, n=%u\n", i, j, n);
                    break;
                }
            }
            break;
        case ANS_E_EXHAUSTED: ++exhausted; break;
        case ANS_E_LEN: ++len; break;
        case ANS_E_SYMBOL: ++symbol; break;
        default:
            ++hostile_bad;
            std::fprintf(stderr, "hostile pop: status %d\n", rc);
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    const bool shorter = argc > 1 && std::strcmp(argv[1], "--short") == 0;
    Checker ck(shorter);
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
    const Shadow& sh = ck.sh;
    uint64_t oob = 0, stale = 0;
    for (int r = 0; r < kRegions; ++r) oob += sh.oob[r], stale += sh.stale[r];
    std::printf("arpu_state_check: graphs=%llu named=%llu roundtrip_fail=%llu hostile=%llu hostile_ok=%llu "
                "exhausted=%llu len=%llu symbol=%llu hostile_bad=%llu rank_oob=%llu oob=%llu stale=%llu",
                (unsigned long long)(ck.graphs - named_graphs), (unsigned long long)named,
                (unsigned long long)ck.roundtrip_fail, (unsigned long long)ck.hostile, (unsigned long long)ck.hostile_ok,
                (unsigned long long)ck.exhausted, (unsigned long long)ck.len, (unsigned long long)ck.symbol,
                (unsigned long long)ck.hostile_bad,
                (unsigned long long)sh.rank_oob, (unsigned long long)oob, (unsigned long long)stale);
    for (int r = 0; r < kRegions; ++r)
        std::printf(" %s:size=%llu,highest=%lld,oob=%llu,stale=%llu", kRegionName[r],
                    (unsigned long long)(sh.declared_end[r] - sh.begin[r]), (long long)sh.highest[r],
                    (unsigned long long)sh.oob[r], (unsigned long long)sh.stale[r]);
    std::printf("\n");
    return 0;
}
