// The per-graph state of the Pólya urn codec (ans_polya.hpp State) behind a checked accessor:
// one workspace of fixed bounds reused for every graph, full of junk before every call, as a
// lane's entries of the device workspace are.  The shared templates (State, Coder, push_graph,
// pop_graph: the functions the kernels of ans_polya.hip and the host codec run) are instantiated
// with
//   * an accessor that knows its region of the workspace (Ws::at is called in the order urn, orb,
//     ord, rop, por, head, next; a region ends where the next begins, the last at ws_entries) and
//     counts every access at or past the region's end (not performed: the load gives kOobValue,
//     the store is dropped) and every load of an entry that the current call has not stored
//     (a stale read: on the device another graph's leftovers);
//   * a message that is a head and a byte vector, with the renorm of src/ans.rs:233-253 under the
//     Empty generator.
// Built with ASan + UBSan and run by tests/test_polya_state.py, which parses the summary line.
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

#include "ans_polya.hpp"

namespace pu = shuffle_coding::polya;

namespace {

constexpr uint32_t kMaxNodes = 40, kMaxEdges = 120;
constexpr int kRegions = 7;
const char* const kRegionName[kRegions] = {"urn", "orb", "ord", "rop", "por", "head", "next"};
constexpr uint32_t kOobValue = 0;  // what a load out of range gives (a value every caller survives)

struct Shadow {
    std::vector<uint32_t> value, stamp;
    uint32_t epoch = 0;
    std::array<uint64_t, kRegions> begin{}, end{}, declared_end{}, oob{}, stale{};
    std::array<int64_t, kRegions> highest;
    int regions = 0;
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
    CheckedAcc at(uint64_t o) const {
        const int r = s->regions++;
        s->begin[r] = o;
        if (r) s->end[r - 1] = o;
        return CheckedAcc{s, r};
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
    std::mt19937_64 rng{20260219};
    Shadow sh;
    pu::State<CheckedAcc> st;
    uint64_t graphs = 0, roundtrip_fail = 0;
    uint64_t hostile = 0, hostile_ok = 0, hostile_bad = 0;
    uint64_t exhausted = 0, zero_mass = 0, symbol = 0, arg = 0;

    explicit Checker(bool shorter) : st(make(shorter)) {}
    pu::State<CheckedAcc> make(bool shorter) {
        const uint64_t entries = pu::ws_entries(kMaxNodes, kMaxEdges);
        sh.value.assign(entries, 0);
        sh.stamp.assign(entries, 0);
        auto state = pu::State<CheckedAcc>::make(CheckedWs{&sh}, kMaxNodes, kMaxEdges);
        sh.end[kRegions - 1] = entries;
        if (sh.regions != kRegions) std::exit(2);
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
    void roundtrip(uint32_t n, const Pairs& g, bool loops, bool redraws) {
        const uint32_t E = static_cast<uint32_t>(g.size());
        std::vector<uint8_t> seed(400);
        for (auto& b : seed) b = static_cast<uint8_t>(rng());
        seed.back() |= 1;  // a nonzero top byte: the seed comes back byte for byte
        std::vector<uint32_t> e(2 * size_t(E) + 2, 0xDEADBEEFu), out(2 * size_t(E) + 2, 0xDEADBEEFu);
        for (uint32_t k = 0; k < E; ++k) {
            e[2 * k] = g[k].first;
            e[2 * k + 1] = g[k].second;
        }
        ++graphs;
        Msg m;
        m.tail = seed;
        pu::Coder<Msg> c{m, ANS_OK};
        fresh();
        int rc = pu::push_graph(c, st, n, loops, redraws, e.data(), E);
        Msg m2;
        m2.tail = m.flatten();
        pu::Coder<Msg> c2{m2, ANS_OK};
        fresh();
        if (!rc) rc = pu::pop_graph(c2, st, n, loops, redraws, out.data(), E);
        bool ok = rc == ANS_OK;
        if (ok) {
            Pairs got;
            for (uint32_t k = 0; k < E; ++k) got.emplace_back(out[2 * k], out[2 * k + 1]);
            Pairs a = g;
            std::sort(a.begin(), a.end());
            std::sort(got.begin(), got.end());
            std::vector<uint8_t> want = seed;
            if (E == 0) want.insert(want.end(), 2, 0);  // each call is flatten(unflatten(B)) = B ++ [0]
            ok = got == a && m2.flatten() == want;
        }
        if (!ok) {
            ++roundtrip_fail;
            std::fprintf(stderr, "round trip failed: n=%u E=%u loops=%d redraws=%d rc=%d\n", n, E, loops, redraws, rc);
        }
    }

    // bytes no push wrote
    void hostile_pop(bool loops, bool redraws) {
        const uint32_t n = 1 + static_cast<uint32_t>(below(kMaxNodes)), E = static_cast<uint32_t>(below(kMaxEdges + 1));
        Msg m;
        m.tail.resize(1 + below(300));
        for (auto& b : m.tail) b = static_cast<uint8_t>(rng());
        std::vector<uint32_t> out(2 * size_t(E) + 2, 0xDEADBEEFu);
        pu::Coder<Msg> c{m, ANS_OK};
        fresh();
        const int rc = pu::pop_graph(c, st, n, loops, redraws, out.data(), E);
        ++hostile;
        switch (rc) {
        case ANS_OK:
            ++hostile_ok;
            for (uint32_t k = 0; k < E; ++k) {
                const uint32_t i = out[2 * k], j = out[2 * k + 1];
                if (i > j || j >= n || (i == j && !loops)) {
                    ++hostile_bad;
                    std::fprintf(stderr, "hostile pop: pair (%u, %u) outside the alphabet, n=%u\n", i, j, n);
                    break;
                }
            }
            break;
        case ANS_E_EXHAUSTED: ++exhausted; break;
        case ANS_E_ZERO_MASS: ++zero_mass; break;
        case ANS_E_SYMBOL: ++symbol; break;
        case ANS_E_ARG: ++arg; break;
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
    const Shadow& sh = ck.sh;
    uint64_t oob = 0, stale = 0;
    for (int r = 0; r < kRegions; ++r) oob += sh.oob[r], stale += sh.stale[r];
    std::printf("polya_state_check: graphs=%llu named=%llu roundtrip_fail=%llu hostile=%llu hostile_ok=%llu "
                "hostile_status=%llu exhausted=%llu zero_mass=%llu symbol=%llu arg=%llu hostile_bad=%llu oob=%llu stale=%llu",
                (unsigned long long)(ck.graphs - named_graphs), (unsigned long long)named,
                (unsigned long long)ck.roundtrip_fail, (unsigned long long)ck.hostile, (unsigned long long)ck.hostile_ok,
                (unsigned long long)(ck.exhausted + ck.zero_mass + ck.symbol + ck.arg), (unsigned long long)ck.exhausted,
                (unsigned long long)ck.zero_mass, (unsigned long long)ck.symbol, (unsigned long long)ck.arg,
                (unsigned long long)ck.hostile_bad, (unsigned long long)oob, (unsigned long long)stale);
    for (int r = 0; r < kRegions; ++r)
        std::printf(" %s:size=%llu,highest=%lld,oob=%llu,stale=%llu", kRegionName[r],
                    (unsigned long long)(sh.declared_end[r] - sh.begin[r]), (long long)sh.highest[r],
                    (unsigned long long)sh.oob[r], (unsigned long long)sh.stale[r]);
    std::printf("\n");
    return 0;
}
