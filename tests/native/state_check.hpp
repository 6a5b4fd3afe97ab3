// What the state checks (arer_, arpu_, wl_, polya_state_check.cpp) share.  A per-graph state is put
// behind a checked accessor: one workspace of fixed bounds reused for every graph, full of junk
// before every push and every pop, as a lane's entries of the device workspace are.  The templates
// the kernels and the host codec run are instantiated with
//   * an accessor that knows its region of the workspace (Ws::at names its start and its length; with
//     the start alone a region ends where the next begins) and counts every access at or past the
//     region's end (not performed: the load gives kOobValue, the store is dropped) and every load of
//     an entry that the current call has not stored (a stale read: on the device another graph's
//     leftovers);
//   * a rank table that counts a read past its entries;
//   * a message that is a head and a byte vector, with the renorm of src/ans.rs:233-253 under the
//     Empty generator.
// Built with ASan + UBSan and run by tests/test_*_state.py, which parse the summary line.
// --short declares every region one entry shorter than it is: the run must then report accesses
// out of range (the check of the checker).  Those entries exist, so in that run an access to one
// is counted and performed all the same, and the codec's results still hold.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

namespace state_check {

constexpr uint32_t kOobValue = 0;  // what a load out of range gives (a value every caller survives)

struct Region {
    uint64_t begin = 0, end = 0, declared_end = 0, oob = 0, stale = 0;
    int64_t highest = -1;
    uint64_t size() const { return end - begin; }
    bool filled() const { return highest == static_cast<int64_t>(size()) - 1; }
};
struct Shadow {
    std::vector<uint32_t> value, stamp;
    uint32_t epoch = 0;
    std::vector<Region> regions;
    uint64_t rank_oob = 0;
    void resize(uint64_t entries) {
        value.assign(entries, 0);
        stamp.assign(entries, 0);
    }
    // --short: the regions from `first` on, one entry shorter (an empty one stays)
    void shorten(size_t first = 0) {
        for (size_t r = first; r < regions.size(); ++r)
            if (regions[r].end > regions[r].begin) --regions[r].declared_end;
    }
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
    // the start alone: the region before ends here, the last where close() says
    CheckedAcc at(uint64_t o) const {
        close(o);
        return at(o, 0);
    }
    void close(uint64_t end) const {
        if (!s->regions.empty()) s->regions.back().end = s->regions.back().declared_end = end;
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

// the generator, the workspace and the counts every program reports
struct Common {
    std::mt19937_64 rng;
    Shadow sh;
    uint64_t graphs = 0, roundtrip_fail = 0, hostile = 0, hostile_ok = 0, hostile_bad = 0, exhausted = 0, len = 0,
             symbol = 0;
    explicit Common(uint64_t seed = 20261021) : rng(seed) {}
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
    // Push g onto a seed message (400 random bytes, a nonzero top byte: it comes back byte for byte),
    // pop from what the push left; the state is junk before either.  push(coder, pairs, E, perm) and
    // pop(coder, out, cap, &count) return a status.  True when the pop gave g's pairs under the push's
    // perm (as they came if `ascending`, else in any order), the seed came back (with `no_step`
    // followed by two zero bytes: each call is then flatten(unflatten(B)) = B ++ [0]) and nothing was
    // written past the perm's or the pairs' end.
    template <class Coder, class Push, class Pop>
    bool roundtrip(uint32_t n, const Pairs& g, bool no_step, bool ascending, Push&& push, Pop&& pop, int& rc,
                   std::vector<uint32_t>& perm) {
        const uint32_t E = static_cast<uint32_t>(g.size());
        std::vector<uint8_t> seed(400);
        for (auto& b : seed) b = static_cast<uint8_t>(rng());
        seed.back() |= 1;
        std::vector<uint32_t> e(2 * size_t(E) + 2, 0xDEADBEEFu), out(2 * size_t(E) + 2, 0xDEADBEEFu);
        perm.assign(n + 1, 0xDEADBEEFu);
        for (uint32_t k = 0; k < E; ++k) {
            e[2 * k] = g[k].first;
            e[2 * k + 1] = g[k].second;
        }
        ++graphs;
        Msg m;
        m.tail = seed;
        Coder c{m, ANS_OK};
        fresh();
        rc = push(c, e.data(), E, perm.data());
        Msg m2;
        m2.tail = m.flatten();
        Coder c2{m2, ANS_OK};
        uint64_t count = 0;
        fresh();
        if (!rc) rc = pop(c2, out.data(), E, &count);
        if (rc != ANS_OK || count != E || perm[n] != 0xDEADBEEFu || out[2 * size_t(E)] != 0xDEADBEEFu) return false;
        std::vector<uint32_t> pos(n);
        for (uint32_t p = 0; p < n; ++p) {
            if (perm[p] >= n) return false;
            pos[perm[p]] = p;
        }
        Pairs want, got;
        for (auto& [i, j] : g) want.emplace_back(std::min(pos[i], pos[j]), std::max(pos[i], pos[j]));
        for (uint32_t k = 0; k < E; ++k) got.emplace_back(out[2 * k], out[2 * k + 1]);
        std::sort(want.begin(), want.end());
        if (!ascending) std::sort(got.begin(), got.end());
        if (no_step) seed.insert(seed.end(), 2, 0);
        return got == want && m2.flatten() == seed;
    }

    // Bytes no push wrote, at most max_bytes of them, popped as a graph of n nodes and at most cap
    // pairs.  Counts the call, a write past the pairs' end, and under ANS_OK a pair outside the
    // alphabet; returns the status for the caller to count.
    template <class Coder, class Pop>
    int hostile_pop(uint32_t n, uint64_t cap, uint64_t max_bytes, bool loops, Pop&& pop) {
        Msg m;
        m.tail.resize(1 + below(max_bytes));
        for (auto& b : m.tail) b = static_cast<uint8_t>(rng());
        std::vector<uint32_t> out(2 * cap + 2, 0xDEADBEEFu);
        Coder c{m, ANS_OK};
        uint64_t count = 0;
        fresh();
        const int rc = pop(c, out.data(), cap, &count);
        ++hostile;
        if (out[2 * cap] != 0xDEADBEEFu) ++hostile_bad;
        if (rc != ANS_OK) return rc;
        ++hostile_ok;
        for (uint64_t k = 0; k < count; ++k) {
            const uint32_t i = out[2 * k], j = out[2 * k + 1];
            if (count > cap || i > j || j >= n || (i == j && !loops)) {
                ++hostile_bad;
                std::fprintf(stderr, "hostile pop: pair (%u, %u) outside the alphabet, n=%u\n", i, j, n);
                break;
            }
        }
        return rc;
    }
    void bad_status(int rc) {
        ++hostile_bad;
        std::fprintf(stderr, "hostile pop: status %d\n", rc);
    }

    // the summary's fields
    static void field(const char* name, uint64_t v) { std::printf(" %s=%llu", name, (unsigned long long)v); }
    uint64_t oob() const {
        uint64_t n = 0;
        for (auto& r : sh.regions) n += r.oob;
        return n;
    }
    uint64_t stale() const {
        uint64_t n = 0;
        for (auto& r : sh.regions) n += r.stale;
        return n;
    }
    // ... and a region each, in the order the states took them
    template <size_t N>
    void print_regions(const char* const (&name)[N]) const {
        if (sh.regions.size() != N) std::exit(2);
        for (size_t r = 0; r < N; ++r) {
            const Region& reg = sh.regions[r];
            std::printf(" %s:size=%llu,highest=%lld,oob=%llu,stale=%llu", name[r],
                        (unsigned long long)(reg.declared_end - reg.begin), (long long)reg.highest,
                        (unsigned long long)reg.oob, (unsigned long long)reg.stale);
        }
        std::printf("\n");
    }
};

inline bool short_run(int argc, char** argv) { return argc > 1 && std::strcmp(argv[1], "--short") == 0; }

}  // namespace state_check
