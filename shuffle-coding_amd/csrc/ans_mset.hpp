// ans_mset.hpp — the arithmetic of recursive multiset shuffle coding that is not the coder's own:
// ShuffleCodec<IIDVecSliceCodecs<Categorical>, VecOrbitCodecs> (src/recursive/mod.rs:117-148,
// src/recursive/multiset.rs:13-91,139-141).  The orbit id of a value, the rank of every symbol of
// an alphabet among the orbit ids, and the counts of the current prefix per rank with the queries
// of the orbit distribution (a MutCategorical keyed by orbit id, src/codec.rs:145-181: norm =
// the prefix's length, pmf = the rank's count, cdf = the counts below it, icdf by cumulative
// count).  Plain C++, host and device alike, so that the host codec (ans_capi.cpp), the kernels
// (ans_mset.hip) and the CPU tests (g++, tests/test_mset_host.py) run the same functions.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#ifdef __HIPCC__
#define ANS_MSET_HD __host__ __device__
#else
#define ANS_MSET_HD
#endif

namespace shuffle_coding {
namespace mset {

// hash(x) of src/recursive/prefix_orbit.rs:132-136 for a usize x: std's DefaultHasher::new(),
// SipHash-1-3 with keys (0, 0), fed the value's 8 native-endian (little-endian) bytes; the final
// block carries the length, 8 << 56.
constexpr uint64_t rotl(uint64_t v, int s) { return (v << s) | (v >> (64 - s)); }
constexpr void sip_round(uint64_t& v0, uint64_t& v1, uint64_t& v2, uint64_t& v3) {
    v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
    v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
    v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
    v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
}
constexpr uint64_t orbit_id(uint64_t x) {
    uint64_t v0 = 0x736f6d6570736575ull, v1 = 0x646f72616e646f6dull, v2 = 0x6c7967656e657261ull,
             v3 = 0x7465646279746573ull;
    v3 ^= x;
    sip_round(v0, v1, v2, v3);
    v0 ^= x;
    const uint64_t tail = 8ull << 56;
    v3 ^= tail;
    sip_round(v0, v1, v2, v3);
    v0 ^= tail;
    v2 ^= 0xff;
    sip_round(v0, v1, v2, v3);
    sip_round(v0, v1, v2, v3);
    sip_round(v0, v1, v2, v3);
    return v0 ^ v1 ^ v2 ^ v3;
}

constexpr uint32_t kMaxSymbols = 65536;  // alphabets the multiset codec takes

// The rank tables of the alphabet 0 .. nsym-1: rank[s] is symbol s's position when the alphabet
// is sorted by ascending orbit id, sym_of_rank its inverse.  They depend on nsym alone.  False
// when two symbols share an id (the orbit distribution could not tell them apart).
inline bool build_ranks(uint32_t nsym, std::vector<uint32_t>& rank, std::vector<uint32_t>& sym_of_rank) {
    std::vector<uint64_t> id(nsym);
    for (uint32_t s = 0; s < nsym; ++s) id[s] = orbit_id(s);
    sym_of_rank.resize(nsym);
    std::iota(sym_of_rank.begin(), sym_of_rank.end(), 0u);
    std::sort(sym_of_rank.begin(), sym_of_rank.end(), [&](uint32_t a, uint32_t b) { return id[a] < id[b]; });
    rank.resize(nsym);
    for (uint32_t r = 0; r < nsym; ++r) {
        if (r && id[sym_of_rank[r]] == id[sym_of_rank[r - 1]]) return false;
        rank[sym_of_rank[r]] = r;
    }
    return true;
}

// The counts per rank as a Fenwick tree: node i (1 .. nsym, stored at index i - 1) holds the
// counts of ranks (i - lowbit(i), i], as 0-based ranks i - lowbit(i) .. i - 1.  Acc says how a
// node is read and written (uint32_t load(uint32_t index), void store(uint32_t index, uint32_t)):
// lane-interleaved LDS or global memory in the kernels, a vector on the host.
//   find   walks down from the top: ceil(log2(nsym + 1)) loads, each address depending on the
//          last comparison (the chain of the push step);
//   prefix, count and add touch nodes whose addresses depend on the rank alone (independent
//          loads, off the chain).
struct Found {
    uint32_t rank;
    uint32_t count;  // the rank's count
    uint64_t cum;    // the counts of the ranks below it
};
template <class Acc>
struct Counts {
    Acc a;
    uint32_t nsym;

    ANS_MSET_HD void clear() {
        for (uint32_t i = 0; i < nsym; ++i) a.store(i, 0);
    }
    // the histogram: plain per-rank counts in the nodes' places, then build() once
    ANS_MSET_HD void tally(uint32_t rank) { a.store(rank, a.load(rank) + 1); }
    ANS_MSET_HD void build() {
        for (uint32_t i = 1; i <= nsym; ++i) {
            const uint32_t j = i + (i & (0u - i));
            if (j <= nsym) a.store(j - 1, a.load(j - 1) + a.load(i - 1));
        }
    }
    // icdf: the rank r with prefix(r) <= cf < prefix(r + 1) (ranks of count 0 are skipped), its
    // count and prefix(r); cf must be below the total.  The count comes from the walk itself: the
    // last node that did not fit is node r + 1, which holds the counts of ranks
    // (r + 1 - lowbit(r + 1)) .. r, and every step after it went right, over the ranks below r of
    // that range: count = that node - what those steps took.
    ANS_MSET_HD Found find(uint64_t cf) const {
        uint32_t top = 1;
        while (top <= nsym / 2) top <<= 1;
        uint32_t pos = 0;
        uint64_t rem = cf, miss_node = 0, miss_rem = 0;
        for (uint32_t step = top; step; step >>= 1) {
            const uint32_t nxt = pos + step;
            if (nxt > nsym) continue;
            const uint64_t v = a.load(nxt - 1);
            if (v <= rem) {
                pos = nxt;
                rem -= v;
            } else {
                miss_node = v;
                miss_rem = rem;
            }
        }
        return Found{pos, static_cast<uint32_t>(miss_node - (miss_rem - rem)), cf - rem};
    }
    // the counts of the ranks below rank
    ANS_MSET_HD uint64_t prefix(uint32_t rank) const {
        uint64_t s = 0;
        for (uint32_t i = rank; i; i &= i - 1) s += a.load(i - 1);
        return s;
    }
    ANS_MSET_HD uint32_t count(uint32_t rank) const {
        const uint32_t i = rank + 1, stop = i & (i - 1);
        uint32_t c = a.load(i - 1);
        for (uint32_t j = i - 1; j != stop; j &= j - 1) c -= a.load(j - 1);
        return c;
    }
    ANS_MSET_HD void add(uint32_t rank, int32_t d) {
        for (uint32_t i = rank + 1; i <= nsym; i += i & (0u - i))
            a.store(i - 1, a.load(i - 1) + static_cast<uint32_t>(d));
    }
};

// Bytes a message can grow by between two steps of a pop of n values (ans_gpu_mset_pop_slack):
// step k takes the value's bits under the table out and puts log2((k + 1) / count) <=
// log2(n) bits of its rank back, so the message is never more than n ceil(log2(n + 1)) bits above
// where it began; 16 more for the head's bytes at flatten.
constexpr uint64_t pop_slack(uint64_t n) {
    uint64_t bits = 0;
    while (bits < 64 && (n >> bits)) ++bits;  // ceil(log2(n + 1))
    return (n / 8 + 1) * bits + 16;
}

}  // namespace mset
}  // namespace shuffle_coding
