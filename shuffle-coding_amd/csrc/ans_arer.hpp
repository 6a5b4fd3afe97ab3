// ans_arer.hpp — undirected, unlabelled graphs under the autoregressive Erdős–Rényi model, as a
// labelled graph (Autoregressive(ErdosRenyiSliceCodecs), src/recursive/mod.rs:190-216,
// src/recursive/graph/slice.rs:16-59) or up to the order of its nodes (ShuffleCodec<
// ErdosRenyiSliceCodecs, WLOrbitCodecs<GraphPrefix>> with wl_iter = 0, src/recursive/mod.rs:117-148,
// src/recursive/graph/incomplete.rs:189-236), one graph on one message.  Plain C++ templated on the
// message and on how a per-graph array is read and written, host and device alike, so that the host
// codec (ans_capi.cpp), the kernels (ans_arer.hip) and the CPU tests (g++, tests/native/
// arer_state_check.cpp) run the same functions.  The recursion is ans_rgraph.hpp's; this header has
// its Erdős–Rényi slice model (ErSlices) and the orbit stage of wl_iter = 0 (CountPush / CountPop),
// which ans_arpu.hpp uses too.  DESIGN.md §3.10 has the restatement with its sources; the comments
// here say which reference line a step is.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/ans_capi.h"
#include "ans_polya.hpp"
#include "ans_rgraph.hpp"

namespace shuffle_coding {
namespace arer {

constexpr uint64_t kMaxEdges = rgraph::kMaxEdges;

// The class of a known node of degree d (a loop counts once): at wl_iter = 0 with the extra half
// iteration, hash((h0, vec![&(); d])) with h0 = hash(((), None::<usize>))
// (incomplete.rs:49-51, 193-199).  h0 hashes the 8 zero bytes of None's isize discriminant,
// mset::orbit_id(0); the tuple feeds h0 and the vector's usize length prefix (the units hash
// nothing), 16 bytes, polya::edge_id(h0, d).
constexpr uint64_t kH0 = mset::orbit_id(0);
constexpr uint64_t class_id(uint64_t degree) { return polya::edge_id(kH0, degree); }

// rank[d] = the position of class_id(d) among class_id(0 .. max_nodes) in ascending order (the
// MutCategorical of src/codec.rs:145-181 orders its symbols so; only the order of the classes
// present matters, so any max_nodes >= the graph's gives the same bytes).  Built once per call on
// the host, read-only afterwards.  False when two degrees share an id.
inline bool build_degree_ranks(uint32_t max_nodes, std::vector<uint32_t>& rank) {
    const uint32_t count = max_nodes + 1;
    std::vector<uint64_t> id(count);
    for (uint32_t d = 0; d < count; ++d) id[d] = class_id(d);
    std::vector<uint32_t> by_id(count);
    std::iota(by_id.begin(), by_id.end(), 0u);
    std::sort(by_id.begin(), by_id.end(), [&](uint32_t a, uint32_t b) { return id[a] < id[b]; });
    rank.resize(count);
    for (uint32_t r = 0; r < count; ++r) {
        if (r && id[by_id[r]] == id[by_id[r - 1]]) return false;
        rank[by_id[r]] = r;
    }
    return true;
}

// Bernoulli::new(mass, norm) = Categorical[norm - mass, mass] (src/codec.rs:125-128) with what a
// step needs beside the masses: the renorm bounds p * (2^56 / norm) and norm * (2^56 / norm)
// (src/ans.rs:100, 109), so that a step divides once, by one of the two masses or by the norm.
struct Bern {
    uint64_t mass[2], lim[2], norm, pop_lim;
};
constexpr Bern bern_of(uint64_t mass0, uint64_t mass1) {
    const uint64_t norm = mass0 + mass1, k = norm ? polya::kK / norm : 0;
    return Bern{{mass0, mass1}, {mass0 * k, mass1 * k}, norm, norm * k};
}
template <class M>
ANS_MSET_HD void push_bit(polya::Coder<M>& c, const Bern& b, uint32_t x) {  // src/ans.rs:97-104
    const uint64_t p = b.mass[x];
    if (p == 0 && !c.err) c.err = ANS_E_ZERO_MASS;  // src/ans.rs:98
    if (!c.renorm(b.lim[x])) return;
    const uint64_t h = c.m.head, q = h / p;
    c.m.head = b.norm * q + (x ? b.mass[0] : 0) + (h - q * p);
}
template <class M>
ANS_MSET_HD uint32_t pop_bit(polya::Coder<M>& c, const Bern& b) {  // src/ans.rs:107-116
    if (!c.renorm(b.pop_lim)) return 0;
    const uint64_t h = c.m.head, q = h / b.norm, cf = h - q * b.norm;
    const uint32_t x = cf >= b.mass[0];
    c.m.head = b.mass[x] * q + (x ? cf - b.mass[0] : cf);
    return x;
}

// ---- the slice model: IID<Bernoulli> over a node's pairs (slice.rs:16-59).  mark (a push alone):
// per position, the stamp of the step whose slice holds it; before the first step the stamps that
// find a pair given twice.  bern is the caller's to set.
template <class Acc>
struct ErSlices {
    Acc mark;
    Bern bern;
    template <class T>
    ANS_MSET_HD static ErSlices make(T& take, uint64_t max_nodes, bool push) {
        ErSlices s{push ? take(max_nodes) : Acc{}, Bern{}};
        return s;
    }
    ANS_MSET_HD Acc& scratch() { return mark; }
    ANS_MSET_HD void start_push(uint32_t n) {
        for (uint32_t v = 0; v < n; ++v) mark.store(v, 0);
    }
    ANS_MSET_HD void gather(uint32_t, uint32_t p, uint32_t L) { mark.store(p, L); }
    // IID<Bernoulli>::push over (L-1, L) .. (L-1, n-1), then the loop: last entry first
    template <class M, class G>
    ANS_MSET_HD int push(polya::Coder<M>& c, const G&, uint32_t n, bool loops, uint32_t last, uint32_t) {
        const uint32_t L = last + 1;
        if (loops) push_bit(c, bern, mark.load(last) == L);
        for (uint32_t j = n; j-- > L;) push_bit(c, bern, mark.load(j) == L);
        return c.err;
    }
    ANS_MSET_HD void start_pop(uint32_t, bool) {}
    // ... and its pop: the pairs in pop order, the loop last
    template <class M, class F>
    ANS_MSET_HD int pop(polya::Coder<M>& c, uint32_t n, bool loops, uint32_t v, uint64_t room, uint32_t& len, F&& emit) {
        for (uint32_t j = v + 1; j < n + (loops ? 1u : 0u); ++j) {
            const uint32_t x = pop_bit(c, bern);
            if (c.err) return c.err;
            if (!x) continue;
            if (len >= room) return ANS_E_LEN;
            emit(j < n ? j : v);
            ++len;
        }
        return ANS_OK;
    }
};

// ---- the orbit stage at wl_iter = 0 as counts per class (WLOrbitCodecs::apply, incomplete.rs:
// 193-210): `orbits` says which classes (ANS_ORBITS_NONE: nothing is coded, the labelled codec;
// ONE_CLASS: every known node has id h0, incomplete.rs:193-196 without the half iteration; DEGREE: a
// class per degree).  rank: build_degree_ranks of some max_nodes >= n, nranks = max_nodes + 1 its
// entries (DEGREE alone reads it; the counts span its ranks, one rank otherwise).  The kernels give
// `orbits` as a constant, so a step carries no test of it.
//   rk    the class rank of the node at a position;  cnt the orbit counts per rank (a Fenwick tree)
template <class Acc, class Rank>
struct CountPush {
    Acc rk;
    mset::Counts<Acc> cnt;
    int orbits;
    Rank rank;
    uint32_t nranks;
    template <class T>
    ANS_MSET_HD static CountPush make(T& take, uint64_t max_nodes, uint64_t, int orbits, Rank rank, uint32_t nranks) {
        CountPush o{take(max_nodes), {take(max_nodes + 1), 0}, orbits, rank, nranks};
        return o;
    }
    ANS_MSET_HD bool coded() const { return orbits != ANS_ORBITS_NONE; }
    ANS_MSET_HD uint32_t class_rank(uint32_t degree) const { return orbits == ANS_ORBITS_DEGREE ? rank[degree] : 0; }
    template <class G>
    ANS_MSET_HD void apply_full(const G& g, uint32_t n) {
        if (!coded()) return;
        cnt.nsym = orbits == ANS_ORBITS_DEGREE ? nranks : 1;
        cnt.clear();
        for (uint32_t v = 0; v < n; ++v) {
            const uint32_t r = class_rank(g.degree(v));
            rk.store(v, r);
            cnt.tally(r);
        }
        cnt.build();
    }
    // the blanket pop under norm L, then the class's smallest position (prefix_orbit.rs:117-119), by
    // a scan
    template <class M>
    ANS_MSET_HD int pop_element(polya::Coder<M>& c, uint32_t L, uint32_t& index, uint32_t& cls) {
        uint64_t q = 0, cf = 0;
        if (!c.pop_begin(L, q, cf)) return c.err;
        const mset::Found f = cnt.find(cf);
        c.pop_end(f.count, q, cf - f.cum);
        cls = f.rank;
        for (index = 0; index < L - 1 && rk.load(index) != cls;) ++index;
        return ANS_OK;
    }
    // the orbits' swap of the positions index and last, then pop_id (prefix_orbit.rs:59-70)
    ANS_MSET_HD void pop_id(uint32_t index, uint32_t last, uint32_t cls) {
        rk.store(index, rk.load(last));
        cnt.add(cls, -1);
    }
    // a class is a degree in the whole graph: a slice that leaves changes none
    ANS_MSET_HD void touch(uint32_t) {}
    template <class G>
    ANS_MSET_HD void after_pop_slice(const G&, uint32_t) {}
};
//   deg   the degree so far per position
template <class Acc, class Rank>
struct CountPop {
    Acc deg;
    mset::Counts<Acc> cnt;
    int orbits;
    Rank rank;
    uint32_t nranks;
    template <class T>
    ANS_MSET_HD static CountPop make(T& take, uint64_t max_nodes, uint64_t, int orbits, Rank rank, uint32_t nranks) {
        CountPop o{take(max_nodes), {take(max_nodes + 1), 0}, orbits, rank, nranks};
        return o;
    }
    ANS_MSET_HD void start_pop(uint32_t n, const uint32_t*) {
        if (orbits == ANS_ORBITS_NONE) return;
        cnt.nsym = orbits == ANS_ORBITS_DEGREE ? nranks : 1;
        cnt.clear();
        for (uint32_t v = 0; v < n; ++v) deg.store(v, 0);
    }
    ANS_MSET_HD void add_pair(uint32_t v, uint32_t w, uint32_t) {
        if (orbits != ANS_ORBITS_NONE && w != v) deg.store(w, deg.load(w) + 1);
    }
    // push_id, update_around_slice, push_element (recursive/mod.rs:143-145): v's slice held len pairs
    template <class M>
    ANS_MSET_HD int push_element(polya::Coder<M>& c, uint32_t v, uint32_t len) {
        if (orbits == ANS_ORBITS_NONE) return ANS_OK;
        const uint32_t r = orbits == ANS_ORBITS_DEGREE ? rank[deg.load(v) + len] : 0;
        cnt.add(r, 1);
        c.push(cnt.count(r), uint64_t(v) + 1, cnt.prefix(r));
        return c.err;
    }
};
constexpr uint64_t count_entries(uint64_t max_nodes) { return 2 * max_nodes + 1; }

// The per-graph states (ans_rgraph.hpp lays them out): the prefix graph, the stamps, the counts; a
// pop holds nothing sized by the edges.
constexpr uint64_t push_entries(uint64_t max_nodes, uint64_t max_edges) {
    return rgraph::graph_entries(max_nodes, max_edges) + max_nodes + count_entries(max_nodes);
}
constexpr uint64_t pop_entries(uint64_t max_nodes) { return count_entries(max_nodes); }
template <class Acc, class Rank>
using PushState = rgraph::PushState<Acc, ErSlices<Acc>, CountPush<Acc, Rank>>;
template <class Acc, class Rank>
using PopState = rgraph::PopState<Acc, ErSlices<Acc>, CountPop<Acc, Rank>>;

// Bytes a message can grow by during a push or a pop of a graph of at most max_nodes nodes
// (ans_gpu_ar_er_slack; DESIGN.md §3.10 derives it): a push adds n(n-1)/2 + n*loops indicators of
// at most log2(norm / pmin) < bitlen(norm / pmin) bits each, pmin the smaller nonzero mass, and a
// bit more each when the norm is above 2^36 (the quotient's floor costs log2(1 + 1 / (2^56 / norm)));
// a pop puts back at most bitlen(n) bits per node; a byte per 2^20 steps for the floors otherwise,
// and 16 for the head's bytes at flatten and a renorm in flight.
constexpr uint64_t slack(const Bern& b, uint64_t max_nodes, bool loops) {
    const uint64_t m0 = b.mass[0], m1 = b.mass[1];
    const uint64_t pmin = m0 && (m0 < m1 || !m1) ? m0 : m1;
    const uint64_t steps = max_nodes * (max_nodes - (max_nodes ? 1 : 0)) / 2 + (loops ? max_nodes : 0);
    const uint64_t push_bits = steps * (polya::bit_len(pmin ? b.norm / pmin : 1) + ((b.norm >> 36) ? 1 : 0));
    const uint64_t pop_bits = max_nodes * polya::bit_len(max_nodes);
    return (push_bits > pop_bits ? push_bits : pop_bits) / 8 + 1 + ((steps + max_nodes) >> 20) + 16;
}

}  // namespace arer
}  // namespace shuffle_coding
