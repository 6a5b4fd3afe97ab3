// ans_arer.hpp — undirected, unlabelled graphs under the autoregressive Erdős–Rényi model, as a
// labelled graph (Autoregressive(ErdosRenyiSliceCodecs), src/recursive/mod.rs:190-216,
// src/recursive/graph/slice.rs:16-59) or up to the order of its nodes (ShuffleCodec<
// ErdosRenyiSliceCodecs, WLOrbitCodecs<GraphPrefix>> with wl_iter = 0, src/recursive/mod.rs:117-148,
// src/recursive/graph/incomplete.rs:189-236), one graph on one message.  Plain C++ templated on the
// message and on how a per-graph array is read and written, host and device alike, so that the host
// codec (ans_capi.cpp), the kernels (ans_arer.hip) and the CPU tests (g++, tests/native/
// arer_state_check.cpp) run the same functions.  DESIGN.md §3.10 has the restatement with its
// sources; the comments here say which reference line a step is.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/ans_capi.h"
#include "ans_polya.hpp"

namespace shuffle_coding {
namespace arer {

constexpr uint64_t kMaxEdges = polya::kMaxEdges;  // the adjacency entries 2e, 2e + 1 stay below 2^32

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

// The per-graph state of a push, u32 entries: Ws::at(offset, count) is an accessor (load / store, as
// mset::Counts takes) of `count` entries from `offset` on.
//   pos_of   the position of an input node;  node_at its inverse (the result is perm = node_at)
//   off, nbr the adjacency in input labels as a CSR built from the pairs: node v's neighbours are
//            nbr[off[v] .. off[v + 1]) (a loop names v once)
//   mark     per node, the stamp that finds a pair given twice; then per position, the stamp of the
//            step whose slice holds it
//   rk       the class rank of the node at a position;  cnt the orbit counts per rank (a Fenwick tree)
constexpr uint64_t push_entries(uint64_t max_nodes, uint64_t max_edges) { return 6 * max_nodes + 2 * max_edges + 2; }
template <class Acc>
struct PushState {
    Acc pos_of, node_at, off, nbr, mark, rk;
    mset::Counts<Acc> cnt;
    template <class Ws>
    ANS_MSET_HD static PushState make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges) {
        uint64_t o = 0;
        auto take = [&](uint64_t n) {
            const uint64_t at = o;
            o += n;
            return ws.at(at, n);
        };
        PushState s{take(max_nodes),     take(max_nodes), take(max_nodes + 1),     take(2 * max_edges),
                    take(max_nodes),     take(max_nodes), {take(max_nodes + 1), 0}};
        return s;
    }
};
// ... and of a pop: the degree so far per position and the orbit counts, nothing sized by the edges
constexpr uint64_t pop_entries(uint64_t max_nodes) { return 2 * max_nodes + 1; }
template <class Acc>
struct PopState {
    Acc deg;
    mset::Counts<Acc> cnt;
    template <class Ws>
    ANS_MSET_HD static PopState make(const Ws& ws, uint64_t max_nodes) {
        PopState s{ws.at(0, max_nodes), {ws.at(max_nodes, max_nodes + 1), 0}};
        return s;
    }
};

// The class rank of a known node of degree d under `orbits` (ONE_CLASS: every known node has id h0,
// incomplete.rs:193-196 without the half iteration); the counts span nranks ranks (the table's
// entries) under DEGREE and one otherwise.
template <class Rank>
ANS_MSET_HD uint32_t class_rank(int orbits, const Rank& rank, uint32_t degree) {
    return orbits == ANS_ORBITS_DEGREE ? rank[degree] : 0;
}

// ---- push.  e: the E pairs; n nodes; rank: build_degree_ranks of some max_nodes >= n, nranks =
// max_nodes + 1 its entries (DEGREE alone reads it; the counts span its ranks); perm: null, or n
// entries out, perm[position] = input node.  Returns a status.
template <class M, class Acc, class Rank>
ANS_MSET_HD int push_graph(polya::Coder<M>& c, PushState<Acc>& st, const Bern& b, uint32_t n, bool loops, int orbits,
                           const Rank& rank, uint32_t nranks, const uint32_t* e, uint32_t E, uint32_t* perm) {
    // the adjacency: degrees into off, their running sums (off[v] = v's end), the fill moves each
    // off[v] down to v's start
    for (uint32_t v = 0; v <= n; ++v) st.off.store(v, 0);
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t i = e[2 * uint64_t(k)], j = e[2 * uint64_t(k) + 1];
        if (i > j || j >= n || (i == j && !loops)) return ANS_E_SYMBOL;  // src/graph_codec.rs:136
        st.off.store(i, st.off.load(i) + 1);
        if (i != j) st.off.store(j, st.off.load(j) + 1);
    }
    uint32_t sum = 0;
    for (uint32_t v = 0; v < n; ++v) {
        sum += st.off.load(v);
        st.off.store(v, sum);
    }
    st.off.store(n, sum);
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t i = e[2 * uint64_t(k)], j = e[2 * uint64_t(k) + 1];
        uint32_t at = st.off.load(i) - 1;
        st.off.store(i, at);
        st.nbr.store(at, j);
        if (i != j) {
            at = st.off.load(j) - 1;
            st.off.store(j, at);
            st.nbr.store(at, i);
        }
    }
    // a pair given twice names a neighbour twice (Graph::new's insert asserts, src/graph.rs)
    for (uint32_t v = 0; v < n; ++v) st.mark.store(v, 0);
    for (uint32_t v = 0; v < n; ++v)
        for (uint32_t a = st.off.load(v), end = st.off.load(v + 1); a < end; ++a) {
            const uint32_t w = st.nbr.load(a);
            if (st.mark.load(w) == v + 1) return ANS_E_SYMBOL;
            st.mark.store(w, v + 1);
        }
    // Prefix::from_full: position p holds input node p, every node known (graph/mod.rs:97-99);
    // WLOrbitCodecs::apply (incomplete.rs:193-210): a class per degree in the whole graph
    st.cnt.nsym = orbits == ANS_ORBITS_DEGREE ? nranks : 1;
    if (orbits != ANS_ORBITS_NONE) st.cnt.clear();
    for (uint32_t v = 0; v < n; ++v) {
        st.pos_of.store(v, v);
        st.node_at.store(v, v);
        st.mark.store(v, 0);
        if (orbits != ANS_ORBITS_NONE) {
            const uint32_t r = class_rank(orbits, rank, st.off.load(v + 1) - st.off.load(v));
            st.rk.store(v, r);
            st.cnt.tally(r);
        }
    }
    if (orbits != ANS_ORBITS_NONE) st.cnt.build();
    for (uint32_t L = n; L > 0; --L) {
        const uint32_t last = L - 1;
        if (orbits != ANS_ORBITS_NONE) {
            // orbit_codec.pop_element (recursive/mod.rs:123): the blanket pop under norm L, then the
            // class's smallest position (prefix_orbit.rs:117-119), by a scan
            uint64_t q = 0, cf = 0;
            if (!c.pop_begin(L, q, cf)) return c.err;
            const mset::Found f = st.cnt.find(cf);
            c.pop_end(f.count, q, cf - f.cum);
            uint32_t index = 0;
            while (index < last && st.rk.load(index) != f.rank) ++index;
            // x.swap(index, last_index) (graph.rs:304-331: the two nodes change labels)
            const uint32_t a = st.node_at.load(index), z = st.node_at.load(last);
            st.node_at.store(index, z);
            st.node_at.store(last, a);
            st.pos_of.store(z, index);
            st.pos_of.store(a, last);
            st.rk.store(index, st.rk.load(last));
            st.cnt.add(f.rank, -1);  // pop_id (prefix_orbit.rs:59-70)
        }
        // pop_slice (graph/mod.rs:57-66): the node's edges to positions >= L - 1
        const uint32_t u = st.node_at.load(last);
        for (uint32_t a = st.off.load(u), end = st.off.load(u + 1); a < end; ++a) {
            const uint32_t p = st.pos_of.load(st.nbr.load(a));
            if (p >= last) st.mark.store(p, L);
        }
        // IID<Bernoulli>::push over (L-1, L) .. (L-1, n-1), then the loop: last entry first
        if (loops) push_bit(c, b, st.mark.load(last) == L);
        for (uint32_t j = n; j-- > L;) push_bit(c, b, st.mark.load(j) == L);
        if (c.err) return c.err;
    }
    if (perm)
        for (uint32_t p = 0; p < n; ++p) perm[p] = st.node_at.load(p);
    return ANS_OK;
}

// ---- pop.  out receives the pairs (position, position) in pop order, at most cap of them
// (ANS_E_LEN beyond); *count their number.
template <class M, class Acc, class Rank>
ANS_MSET_HD int pop_graph(polya::Coder<M>& c, PopState<Acc>& st, const Bern& b, uint32_t n, bool loops, int orbits,
                          const Rank& rank, uint32_t nranks, uint32_t* out, uint64_t cap, uint64_t* count) {
    uint64_t E = 0;
    *count = 0;
    st.cnt.nsym = orbits == ANS_ORBITS_DEGREE ? nranks : 1;
    if (orbits != ANS_ORBITS_NONE) st.cnt.clear();
    for (uint32_t v = 0; v < n; ++v) st.deg.store(v, 0);
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t d = st.deg.load(v);
        for (uint32_t j = v + 1; j < n + (loops ? 1u : 0u); ++j) {
            const uint32_t w = j < n ? j : v;  // the loop comes last
            const uint32_t x = pop_bit(c, b);
            if (c.err) return c.err;
            if (!x) continue;
            if (E >= cap) return ANS_E_LEN;
            out[2 * E] = v;
            out[2 * E + 1] = w;
            ++E;
            ++d;
            if (w != v) st.deg.store(w, st.deg.load(w) + 1);
        }
        if (orbits != ANS_ORBITS_NONE) {
            // push_id, update_around_slice, push_element (recursive/mod.rs:143-145)
            const uint32_t r = class_rank(orbits, rank, d);
            st.cnt.add(r, 1);
            c.push(st.cnt.count(r), uint64_t(v) + 1, st.cnt.prefix(r));
            if (c.err) return c.err;
        }
    }
    *count = E;
    return ANS_OK;
}

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
