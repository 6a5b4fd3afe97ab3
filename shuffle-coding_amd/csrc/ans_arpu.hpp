// ans_arpu.hpp — undirected, unlabelled graphs under the autoregressive Pólya urn model, as a
// labelled graph (Autoregressive(PolyaUrnSliceCodecs), src/recursive/mod.rs:190-216,
// src/recursive/graph/slice.rs:61-230; the harness's ord_AP) or up to the order of its nodes
// (ShuffleCodec<PolyaUrnSliceCodecs, WLOrbitCodecs<GraphPrefix>> with wl_iter = 0,
// src/recursive/mod.rs:117-148, src/recursive/graph/incomplete.rs:189-236; wl0r_AP / wl0-r_AP), one
// graph on one message.  Plain C++ templated on the message and on how a per-graph array is read and
// written, host and device alike, so that the host codec (ans_capi.cpp), the kernels (ans_arpu.hip)
// and the CPU tests (g++, tests/native/arpu_state_check.cpp) run the same functions.  The orbit stage
// is ans_arer.hpp's (it does not depend on the slice model), the outer layers of a slice's multiset
// codec are ans_polya.hpp's.  DESIGN.md §3.11 has the restatement with its sources; the comments
// here say which reference line a step is.
#pragma once
#include <cstdint>

#include "../../include/ans_capi.h"
#include "ans_arer.hpp"
#include "ans_polya.hpp"

namespace shuffle_coding {
namespace arpu {

constexpr uint64_t kMaxEdges = polya::kMaxEdges;  // the adjacency entries 2e, 2e + 1 stay below 2^32

// What a slice's multiset codec works in, sized by max_nodes (a slice holds at most num_nodes pairs):
//   sl    the slice's positions j (element k of the multiset is the pair (v, sl[k]))
//   ord, rop, por, orb   as polya::State names them (polya::rank_elements / shuffle_push /
//         shuffle_pop); the ordered codec, which runs while orb is idle, parks the masses it took out
//         of the urn in orb's entries
//   ids   the 64-bit orbit ids (low, high) the joint layer's sort compares
template <class Acc>
struct Slice {
    Acc sl, ord, rop, por, ids;
    mset::Counts<Acc> orb;
};
constexpr uint64_t slice_entries(uint64_t max_nodes) { return 7 * max_nodes; }

// The per-graph state of a push, u32 entries: Ws::at(offset, count) is an accessor (load / store, as
// mset::Counts takes) of `count` entries from `offset` on.
//   pos_of, node_at, off, nbr, rk, cnt   as arer::PushState has them (the adjacency in input labels
//         as a CSR, the positions, the class ranks and their counts)
//   urn   the urn of the unknown positions, a Fenwick tree over the positions 0 .. n-1 in ascending
//         order (a position outside the urn has mass 0), total its norm
//   s     the slice scratch; before the first step s.sl holds the stamps that find a pair given twice
constexpr uint64_t push_entries(uint64_t max_nodes, uint64_t max_edges) {
    return 6 * max_nodes + 2 * max_edges + 2 + slice_entries(max_nodes);
}
template <class Acc>
struct PushState {
    Acc pos_of, node_at, off, nbr, rk;
    mset::Counts<Acc> cnt, urn;
    Slice<Acc> s;
    uint64_t total;
    template <class Ws>
    ANS_MSET_HD static PushState make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges) {
        uint64_t o = 0;
        auto take = [&](uint64_t n) {
            const uint64_t at = o;
            o += n;
            return ws.at(at, n);
        };
        PushState st{take(max_nodes),
                     take(max_nodes),
                     take(max_nodes + 1),
                     take(2 * max_edges),
                     take(max_nodes),
                     {take(max_nodes + 1), 0},
                     {take(max_nodes), 0},
                     {take(max_nodes), take(max_nodes), take(max_nodes), take(max_nodes), take(2 * max_nodes),
                      {take(max_nodes), 0}},
                     0};
        return st;
    }
};
// ... and of a pop: the degree so far per position, the orbit counts, the urn and the slice scratch
// (the joint layer's pop does not read por, so it holds a plain slice's entries); nothing sized by
// the edges
constexpr uint64_t pop_por_entries(uint64_t max_nodes) { return max_nodes < polya::kPlainMax ? max_nodes : polya::kPlainMax; }
constexpr uint64_t pop_entries(uint64_t max_nodes) {
    return 3 * max_nodes + 1 + slice_entries(max_nodes) - max_nodes + pop_por_entries(max_nodes);
}
template <class Acc>
struct PopState {
    Acc deg;
    mset::Counts<Acc> cnt, urn;
    Slice<Acc> s;
    uint64_t total;
    template <class Ws>
    ANS_MSET_HD static PopState make(const Ws& ws, uint64_t max_nodes) {
        uint64_t o = 0;
        auto take = [&](uint64_t n) {
            const uint64_t at = o;
            o += n;
            return ws.at(at, n);
        };
        PopState st{take(max_nodes),
                    {take(max_nodes + 1), 0},
                    {take(max_nodes), 0},
                    {take(max_nodes), take(max_nodes), take(max_nodes), take(pop_por_entries(max_nodes)),
                     take(2 * max_nodes), {take(max_nodes), 0}},
                    0};
        return st;
    }
};

template <class St>
ANS_MSET_HD void urn_add(St& st, uint32_t j, uint32_t mass) {
    st.urn.add(j, static_cast<int32_t>(mass));
    st.total += mass;
}
template <class St>
ANS_MSET_HD void urn_sub(St& st, uint32_t j, uint32_t mass) {
    st.urn.add(j, -static_cast<int32_t>(mass));
    st.total -= mass;
}

// The ranks of the slice's len pairs (v, sl[k]): as tuples they order by sl[k]; the joint layer's
// orbit id is hash((v, j)) (src/recursive/prefix_orbit.rs:132-136).
template <class Acc>
ANS_MSET_HD int rank_slice(Slice<Acc>& s, uint32_t v, uint32_t len, bool joint) {
    const Acc& sl = s.sl;
    return polya::rank_elements(
        s, s.ids, len, joint, [&](uint32_t k) { return polya::edge_id(v, sl.load(k)); },
        [&](uint32_t a, uint32_t b) { return sl.load(a) < sl.load(b); },
        [&](uint32_t a, uint32_t b) { return sl.load(a) == sl.load(b); });
}

// LogUniform::new(bitlen(s_v) + 1) of the slice's size (slice.rs:72-76, codec.rs:566-611): the
// number of bits b under Uniform(bitlen(s_v) + 2), below it the value without its top bit under
// Uniform(2^(b-1)) (Uniform(1) for b = 1: a renorm and nothing else, kept)
template <class M>
ANS_MSET_HD void push_len(polya::Coder<M>& c, uint32_t alphabet, uint32_t len) {
    const uint64_t b = polya::bit_len(len);
    if (b) c.push_uniform(1ull << (b - 1), len - (1ull << (b - 1)));
    c.push_uniform(polya::bit_len(alphabet) + 2, b);
}
template <class M>
ANS_MSET_HD uint64_t pop_len(polya::Coder<M>& c, uint32_t alphabet) {
    const uint64_t b = c.pop_uniform(polya::bit_len(alphabet) + 2);
    if (c.err || b == 0) return 0;
    return c.pop_uniform(1ull << (b - 1)) | (1ull << (b - 1));
}

// PolyaUrnSliceCodec::push (slice.rs:102-108) of the slice s.sl[0 .. len) of position v.  The urn
// ends as it began.
template <class M, class St>
ANS_MSET_HD int push_slice(polya::Coder<M>& c, St& st, uint32_t v, uint32_t alphabet, uint32_t len) {
    auto& s = st.s;
    if (len > 0) {
        // multiset_shuffle_codec (src/recursive/multiset.rs:126-136): the order the ordered codec sees
        const bool joint = len > polya::kPlainMax;
        if (const int rc = rank_slice(s, v, len, joint)) return rc;
        if (const int rc = polya::shuffle_push(c, s, len, joint)) return rc;
        // PolyaUrnSliceEdgeIndicesCodec::push (slice.rs:140-152): every element leaves the urn, then,
        // last first, each comes back and is pushed under the urn as it then stands
        for (uint32_t p = 0; p < len; ++p) {
            const uint32_t j = s.sl.load(s.rop.load(p)), mass = st.urn.count(j);
            s.orb.a.store(p, mass);
            urn_sub(st, j, mass);
        }
        for (uint32_t p = len; p-- > 0;) {
            const uint32_t j = s.sl.load(s.rop.load(p)), mass = s.orb.a.load(p);
            urn_add(st, j, mass);
            if (mass == 0 && !c.err) c.err = ANS_E_ZERO_MASS;  // src/ans.rs:98 (not reached from a valid slice)
            else c.push(mass, st.total, st.urn.prefix(j));
        }
        if (c.err) return c.err;
    }
    push_len(c, alphabet, len);
    return c.err;
}

// PolyaUrnSliceCodec::pop (slice.rs:110-117): the slice's positions ascending in s.sl[0 .. *len)
// (EdgesIID::pop sorts, src/graph_codec.rs:67-72).  A length above the alphabet's is ANS_E_SYMBOL
// before any urn step (bytes no push wrote; the reference panics in the urn).
template <class M, class St>
ANS_MSET_HD int pop_slice(polya::Coder<M>& c, St& st, uint32_t v, uint32_t alphabet, uint32_t* len_out) {
    auto& s = st.s;
    *len_out = 0;
    const uint64_t len64 = pop_len(c, alphabet);
    if (c.err) return c.err;
    if (len64 > alphabet) return ANS_E_SYMBOL;
    const uint32_t len = static_cast<uint32_t>(len64);
    if (len == 0) return ANS_OK;
    // PolyaUrnSliceEdgeIndicesCodec::pop (slice.rs:154-170): sampling without replacement
    for (uint32_t p = 0; p < len; ++p) {
        uint64_t q = 0, cf = 0;
        if (st.total == 0) return ANS_E_ZERO_MASS;  // (not reached: len <= the urn's positions)
        if (!c.pop_begin(st.total, q, cf)) return c.err;
        const mset::Found f = st.urn.find(cf);
        c.pop_end(f.count, q, cf - f.cum);
        s.sl.store(p, f.rank);
        s.orb.a.store(p, f.count);
        urn_sub(st, f.rank, f.count);
    }
    for (uint32_t p = 0; p < len; ++p) urn_add(st, s.sl.load(p), s.orb.a.load(p));
    const bool joint = len > polya::kPlainMax;
    if (const int rc = rank_slice(s, v, len, joint)) return rc;
    if (const int rc = polya::shuffle_pop(c, s, len, joint)) return rc;
    polya::heapsort(s.sl, len, [](uint32_t a, uint32_t b) { return a < b; });
    *len_out = len;
    return ANS_OK;
}

// ---- push.  e: the E pairs; n nodes; rank: arer::build_degree_ranks of some max_nodes >= n, nranks
// = max_nodes + 1 its entries (DEGREE alone reads it; the counts span its ranks); perm: null, or n
// entries out, perm[position] = input node.  Returns a status.
template <class M, class Acc, class Rank>
ANS_MSET_HD int push_graph(polya::Coder<M>& c, PushState<Acc>& st, uint32_t n, bool loops, int orbits, const Rank& rank,
                           uint32_t nranks, const uint32_t* e, uint32_t E, uint32_t* perm) {
    // the adjacency: degrees into off, their running sums (off[v] = v's end), the fill moves each
    // off[v] down to v's start
    for (uint32_t v = 0; v <= n; ++v) st.off.store(v, 0);
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t i = e[2 * uint64_t(k)], j = e[2 * uint64_t(k) + 1];
        if (i > j || j >= n || (i == j && !loops)) return ANS_E_SYMBOL;
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
    Acc& mark = st.s.sl;
    for (uint32_t v = 0; v < n; ++v) mark.store(v, 0);
    for (uint32_t v = 0; v < n; ++v)
        for (uint32_t a = st.off.load(v), end = st.off.load(v + 1); a < end; ++a) {
            const uint32_t w = st.nbr.load(a);
            if (mark.load(w) == v + 1) return ANS_E_SYMBOL;
            mark.store(w, v + 1);
        }
    // Prefix::from_full: position p holds input node p, every node known (graph/mod.rs:97-99);
    // WLOrbitCodecs::apply (incomplete.rs:193-210): a class per degree in the whole graph;
    // PolyaUrnSliceCodec::from_graph (slice.rs:78-86) of the full prefix: an empty urn
    st.cnt.nsym = orbits == ANS_ORBITS_DEGREE ? nranks : 1;
    if (orbits != ANS_ORBITS_NONE) st.cnt.clear();
    st.urn.nsym = n;
    st.urn.clear();
    st.total = 0;
    for (uint32_t v = 0; v < n; ++v) {
        st.pos_of.store(v, v);
        st.node_at.store(v, v);
        if (orbits != ANS_ORBITS_NONE) {
            const uint32_t r = arer::class_rank(orbits, rank, st.off.load(v + 1) - st.off.load(v));
            st.rk.store(v, r);
            st.cnt.tally(r);
        }
    }
    if (orbits != ANS_ORBITS_NONE) st.cnt.build();
    const uint32_t skip = loops ? 0u : 1u;
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
            // x.swap(index, last_index) (graph.rs:304-331: the two nodes change labels); the urn
            // holds unknown positions only and is invariant to it (slice.rs:223)
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
        uint32_t len = 0;
        for (uint32_t a = st.off.load(u), end = st.off.load(u + 1); a < end; ++a) {
            const uint32_t p = st.pos_of.load(st.nbr.load(a));
            if (p >= last) st.s.sl.store(len++, p);
        }
        // update_after_pop_slice (slice.rs:194-210): position last + !loops enters with 1 + its
        // degree in the prefix graph as it now stands (its edges to the positions below last), every
        // other position of the slice loses the edge that left
        const uint32_t fresh = last + skip;
        if (fresh < n) {
            uint32_t mass = 1;
            if (loops) {
                mass += st.off.load(u + 1) - st.off.load(u) - len;
            } else {
                const uint32_t w = st.node_at.load(fresh);
                for (uint32_t a = st.off.load(w), end = st.off.load(w + 1); a < end; ++a)
                    if (st.pos_of.load(st.nbr.load(a)) < last) ++mass;
            }
            urn_add(st, fresh, mass);
        }
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t j = st.s.sl.load(k);
            if (j != fresh) urn_sub(st, j, 1);
        }
        // EdgesIID::push (src/graph_codec.rs:61-65; the labels are units)
        if (const int rc = push_slice(c, st, last, n - last - 1 + (loops ? 1u : 0u), len)) return rc;
    }
    if (perm)
        for (uint32_t p = 0; p < n; ++p) perm[p] = st.node_at.load(p);
    return ANS_OK;
}

// ---- pop.  out receives the pairs (position, position): v ascending, within v the other end
// ascending (the loop first), at most cap of them (ANS_E_LEN beyond); *count their number.
template <class M, class Acc, class Rank>
ANS_MSET_HD int pop_graph(polya::Coder<M>& c, PopState<Acc>& st, uint32_t n, bool loops, int orbits, const Rank& rank,
                          uint32_t nranks, uint32_t* out, uint64_t cap, uint64_t* count) {
    uint64_t E = 0;
    *count = 0;
    st.cnt.nsym = orbits == ANS_ORBITS_DEGREE ? nranks : 1;
    if (orbits != ANS_ORBITS_NONE) st.cnt.clear();
    // from_graph of the empty prefix (slice.rs:78-86): all ones over [!loops, n)
    const uint32_t skip = loops ? 0u : 1u;
    st.urn.nsym = n;
    for (uint32_t v = 0; v < n; ++v) {
        st.deg.store(v, 0);
        st.urn.a.store(v, v >= skip ? 1 : 0);
    }
    st.urn.build();
    st.total = n > skip ? n - skip : 0;
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t len = 0;
        if (const int rc = pop_slice(c, st, v, n - v - 1 + (loops ? 1u : 0u), &len)) return rc;
        if (len > cap - E) return ANS_E_LEN;
        // push_slice (graph/mod.rs:82-95), update_after_push_slice (slice.rs:212-221)
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t w = st.s.sl.load(k);
            out[2 * E] = v;
            out[2 * E + 1] = w;
            ++E;
            if (w != v) st.deg.store(w, st.deg.load(w) + 1);
            urn_add(st, w, 1);
        }
        if (v + skip < n) urn_sub(st, v + skip, st.urn.count(v + skip));
        if (orbits != ANS_ORBITS_NONE) {
            // push_id, update_around_slice, push_element (recursive/mod.rs:143-145)
            const uint32_t r = arer::class_rank(orbits, rank, st.deg.load(v) + len);
            st.cnt.add(r, 1);
            c.push(st.cnt.count(r), uint64_t(v) + 1, st.cnt.prefix(r));
            if (c.err) return c.err;
        }
    }
    *count = E;
    return ANS_OK;
}

// Bytes a message can grow by during a push or a pop of a graph of at most max_nodes nodes and
// max_edges edges (ans_gpu_ar_polya_slack; DESIGN.md §3.11 derives it): a push adds a slice length
// per node, fewer than bitlen(bitlen(max_nodes) + 2) + bitlen(max_nodes) bits, and an urn symbol per
// edge under a norm <= max_nodes + max_edges and a mass >= 1; a pop puts back an orbit per node and a
// permutation step per edge, each under a norm <= max_nodes; a byte per 2^20 steps for the
// quotients' floors, and 16 for the head's bytes at flatten and a renorm in flight.
constexpr uint64_t slack(uint64_t max_nodes, uint64_t max_edges) {
    const uint64_t bn = polya::bit_len(max_nodes);
    const uint64_t push_bits = max_nodes * (polya::bit_len(bn + 2) + bn) + max_edges * polya::bit_len(max_nodes + max_edges);
    const uint64_t pop_bits = (max_nodes + max_edges) * bn;
    return (push_bits > pop_bits ? push_bits : pop_bits) / 8 + 1 + ((2 * max_nodes + 2 * max_edges) >> 20) + 16;
}

}  // namespace arpu
}  // namespace shuffle_coding
