// ans_rgraph.hpp — recursive shuffle coding of an undirected graph, with or without node and edge
// labels, one graph on one message: ShuffleCodec<SliceCodecs, OrbitCodecs>
// (src/recursive/mod.rs:117-148), written once over a slice model and an orbit stage, and with the
// stage that codes nothing Autoregressive(SliceCodecs) (src/recursive/mod.rs:190-216).  The slice
// models are ans_arer.hpp's ErSlices and ans_arpu.hpp's PuSlices; the orbit stages are ans_arer.hpp's
// counts per degree class (CountPush / CountPop: none, one class, a class per degree) and ans_wl.hpp's
// Weisfeiler-Lehman ids (Orbits / PopOrbits).  Plain C++ templated on the message and on how a
// per-graph array is read and written, host and device alike, so that the host codec (ans_capi.cpp),
// the kernels (ans_arer.hip, ans_arpu.hip, ans_wl.hip, ans_wl_labelled.hip) and the CPU tests (g++,
// tests/native/*_state_check.cpp) run the same functions.  DESIGN.md §3.10 has the restatement with
// its sources; the comments here say which reference line a step is.
//
// What the recursion asks of its parts (all compile-time types: a step has no indirect call):
//   a slice model, on push   scratch()  n entries free until start_push (build_csr's stamps)
//                            start_push(n)                    from_graph of the full prefix
//                            gather(k, p, L)                  position p is the k-th of step L's slice
//                            push(c, g, n, loops, last, len)  update_after_pop_slice, then the slice
//                  on pop    start_pop(n, loops)              from_graph of the empty prefix
//                            pop(c, n, loops, v, room, len, emit)  the slice of v: emit(w) per pair, at
//                                                             most room of them (ANS_E_LEN beyond)
//   an orbit stage, on push  apply_full(g, n)                 WLOrbitCodecs::apply of the full prefix
//                            coded()                          false: no element is coded, no node moves
//                            pop_element(c, L, index, cls)    the blanket pop: a class and its position
//                            pop_id(index, last, cls)         the orbits' swap, then pop_id
//                            touch(p), after_pop_slice(g, last)  update_after_pop_slice
//                  on pop    start_pop(n, out), add_pair(v, w, k), push_element(c, v, len)
// Labels (Graph<N, E, Undirected> with N, E = usize or (), graph/mod.rs:53-104) are a compile-time
// policy, Labels<node, edge>: the recursion codes them around the slice model's step and hands the
// stage the state (its `lab` member) to hash them; under NoLabels nothing of it exists.
#pragma once
#include <cstdint>

#include "../../include/ans_capi.h"
#include "ans_polya.hpp"

namespace shuffle_coding {
namespace rgraph {

constexpr uint64_t kMaxEdges = polya::kMaxEdges;  // the adjacency entries 2e, 2e + 1 stay below 2^32

// A state's arrays, one after the other: Ws::at(offset, count) is an accessor (load / store, as
// mset::Counts takes) of `count` u32 entries from `offset` on.
template <class Ws>
struct Take {
    const Ws& ws;
    uint64_t o;
    ANS_MSET_HD auto operator()(uint64_t n) {
        const uint64_t at = o;
        o += n;
        return ws.at(at, n);
    }
};

// ---- labels.  Labels<node, edge>: which of the two a graph carries; kSorted: a pop gives a node's
// pairs with the other end ascending (EdgesIID::pop's sort, src/graph_codec.rs:67-72), which the
// labelled entries promise whatever the slice model and whichever labels are present.
template <bool kNode, bool kEdge, bool kSorted = kNode || kEdge>
struct Labels {
    static constexpr bool node = kNode, edge = kEdge, any = kNode || kEdge, sorted = kSorted;
};
using NoLabels = Labels<false, false>;

// Categorical::new(masses) (src/codec.rs:58-80) as a step of a Coder: cum holds cdf(0 .. nsym), the
// last the norm; bkt, when given, icdf(j << shift) per bucket j and one more entry (nsym - 1).
struct Cat {
    const uint64_t* cum;
    const uint32_t* bkt;
    uint64_t norm;
    uint32_t nsym, shift;
};
ANS_MSET_HD inline int cat_check(const Cat& t, uint32_t x) {
    if (x >= t.nsym) return ANS_E_SYMBOL;                      // src/codec.rs:63
    return t.cum[x + 1] == t.cum[x] ? ANS_E_ZERO_MASS : ANS_OK;  // src/ans.rs:98
}
template <class M>
ANS_MSET_HD int push_cat(polya::Coder<M>& c, const Cat& t, uint32_t x) {
    if (const int rc = cat_check(t, x)) return rc;
    c.push(t.cum[x + 1] - t.cum[x], t.norm, t.cum[x]);
    return c.err;
}
template <class M>
ANS_MSET_HD uint32_t pop_cat(polya::Coder<M>& c, const Cat& t) {
    uint64_t q = 0, cf = 0;
    if (!c.pop_begin(t.norm, q, cf)) return 0;
    // icdf (src/codec.rs:65-68): the last x with cdf(x) <= cf, within its bucket when there are buckets.
    // (nsym >= 1: a norm of 0 is refused before a table gets here, by check_norm on the host and by
    // ans_tableset_build for a set, and pop_begin has a norm > 0 to divide by.)
    uint32_t lo = 0, hi = t.nsym - 1;
    if (t.bkt) lo = t.bkt[cf >> t.shift], hi = t.bkt[(cf >> t.shift) + 1];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (t.cum[mid] <= cf) lo = mid;
        else hi = mid - 1;
    }
    c.pop_end(t.cum[lo + 1] - t.cum[lo], q, cf - t.cum[lo]);
    return lo;
}

// Bytes the labels add to what a message can grow by (ans_gpu_ar_er_wl_labelled_slack; DESIGN.md
// §3.13 derives it): a push of a symbol of mass p under norm adds log2(norm / p) < bitlen(norm / pmin)
// bits, pmin the table's smallest non-zero mass, and a bit more when the norm is above 2^36 (the
// quotient's floor, as arer::slack has it); a graph pushes at most max_nodes node labels and max_edges
// edge labels; a byte per 2^20 steps for the floors otherwise.  A pop takes labels off and adds none.
constexpr uint64_t label_push_bits(uint64_t norm, uint64_t pmin) {
    return norm && pmin ? polya::bit_len(norm / pmin) + ((norm >> 36) ? 1 : 0) : 0;
}
constexpr uint64_t label_slack(uint64_t node_bits, uint64_t edge_bits, uint64_t max_nodes, uint64_t max_edges) {
    return (max_nodes * node_bits + max_edges * edge_bits) / 8 + 1 + ((max_nodes + max_edges) >> 20);
}

// What a labelled push holds beside the prefix graph, u32 entries (none without edge labels):
//   elab  the label of each entry of the CSR (2 max_edges)
//   spos  the positions of the step's slice;  slab[p] the label of its pair (last, p) (max_nodes each)
// and reads: nl[v] the label of input node v, el[k] that of pair k, under the tables node and edge.
constexpr uint64_t push_label_entries(uint64_t max_nodes, uint64_t max_edges, bool edge) {
    return edge ? 2 * max_edges + 2 * max_nodes : 0;
}
template <class Acc, class L>
struct PushLabels {
    Acc elab, spos, slab;
    Cat node, edge;
    const uint32_t *nl, *el;
    template <class T>
    ANS_MSET_HD static PushLabels make(T& take, uint64_t max_nodes, uint64_t max_edges) {
        PushLabels s{take(L::edge ? 2 * max_edges : 0), take(L::edge ? max_nodes : 0), take(L::edge ? max_nodes : 0),
                     Cat{}, Cat{}, nullptr, nullptr};
        return s;
    }
    // every label has a mass, before a byte moves (Categorical::pmf and the blanket push assert)
    ANS_MSET_HD int check(uint32_t n, uint32_t E) const {
        if constexpr (L::node)
            for (uint32_t v = 0; v < n; ++v)
                if (const int rc = cat_check(node, nl[v])) return rc;
        if constexpr (L::edge)
            for (uint32_t k = 0; k < E; ++k)
                if (const int rc = cat_check(edge, el[k])) return rc;
        return ANS_OK;
    }
    ANS_MSET_HD void gather(uint32_t k, uint32_t p, uint32_t at) {
        spos.store(k, p);
        slab.store(p, elab.load(at));
    }
    // IID<EdgeC>::push over the slice's labels in the order of the edge index (last, j)
    // (EdgesIID::split, src/graph_codec.rs:82-85; src/codec.rs:415-420: the last first)
    template <class M>
    ANS_MSET_HD int push_edges(polya::Coder<M>& c, uint32_t len) {
        polya::heapsort(spos, len, [](uint32_t a, uint32_t b) { return a < b; });
        for (uint32_t k = len; k-- > 0;)
            if (const int rc = push_cat(c, edge, slab.load(spos.load(k)))) return rc;
        return ANS_OK;
    }
};
template <class Acc, bool kSorted>
struct PushLabels<Acc, Labels<false, false, kSorted>> {
    template <class T>
    ANS_MSET_HD static PushLabels make(T&, uint64_t, uint64_t) {
        return PushLabels{};
    }
};
// ... and a labelled pop writes: nl[p] the label of position p, el[k] that of pair k of out
struct PopLabels {
    Cat node, edge;
    uint32_t *nl, *el;
};

// The pairs into a CSR in input labels: degrees into off, their running sums (off[v] = v's end), the
// fill moves each off[v] down to v's start.  The alphabet and a pair given twice are checked (mark: n
// entries of scratch).  placed(at, k): entry `at` of the CSR is an end of pair k.
struct NotPlaced {
    ANS_MSET_HD void operator()(uint32_t, uint32_t) const {}
};
template <class Acc, class Placed = NotPlaced>
ANS_MSET_HD int build_csr(Acc& off, Acc& nbr, Acc& mark, uint32_t n, bool loops, const uint32_t* e, uint32_t E,
                          Placed&& placed = Placed{}) {
    for (uint32_t v = 0; v <= n; ++v) off.store(v, 0);
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t i = e[2 * uint64_t(k)], j = e[2 * uint64_t(k) + 1];
        if (i > j || j >= n || (i == j && !loops)) return ANS_E_SYMBOL;  // src/graph_codec.rs:136
        off.store(i, off.load(i) + 1);
        if (i != j) off.store(j, off.load(j) + 1);
    }
    uint32_t sum = 0;
    for (uint32_t v = 0; v < n; ++v) {
        sum += off.load(v);
        off.store(v, sum);
    }
    off.store(n, sum);
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t i = e[2 * uint64_t(k)], j = e[2 * uint64_t(k) + 1];
        uint32_t at = off.load(i) - 1;
        off.store(i, at);
        nbr.store(at, j);
        placed(at, k);
        if (i != j) {
            at = off.load(j) - 1;
            off.store(j, at);
            nbr.store(at, i);
            placed(at, k);
        }
    }
    for (uint32_t v = 0; v < n; ++v) mark.store(v, 0);
    for (uint32_t v = 0; v < n; ++v)
        for (uint32_t a = off.load(v), end = off.load(v + 1); a < end; ++a) {
            const uint32_t w = nbr.load(a);
            if (mark.load(w) == v + 1) return ANS_E_SYMBOL;  // Graph::new's insert asserts (src/graph.rs)
            mark.store(w, v + 1);
        }
    return ANS_OK;
}

// The prefix graph of a push, u32 entries:
//   pos_of   the position of an input node;  node_at its inverse (the result is perm = node_at)
//   off, nbr the adjacency in input labels as a CSR: node v's neighbours are nbr[off[v] .. off[v + 1])
//            (a loop names v once)
constexpr uint64_t graph_entries(uint64_t max_nodes, uint64_t max_edges) { return 3 * max_nodes + 1 + 2 * max_edges; }
template <class Acc>
struct PushGraph {
    Acc pos_of, node_at, off, nbr;
    template <class T>
    ANS_MSET_HD static PushGraph make(T& take, uint64_t max_nodes, uint64_t max_edges) {
        PushGraph g{take(max_nodes), take(max_nodes), take(max_nodes + 1), take(2 * max_edges)};
        return g;
    }
    // x.swap(index, last) (graph.rs:304-331): the two nodes change labels
    ANS_MSET_HD void swap(uint32_t index, uint32_t last) {
        const uint32_t a = node_at.load(index), z = node_at.load(last);
        node_at.store(index, z);
        node_at.store(last, a);
        pos_of.store(z, index);
        pos_of.store(a, last);
    }
    ANS_MSET_HD uint32_t degree(uint32_t node) const { return off.load(node + 1) - off.load(node); }
    // the positions of node's neighbours
    template <class F>
    ANS_MSET_HD void each(uint32_t node, F&& f) const {
        for (uint32_t a = off.load(node), end = off.load(node + 1); a < end; ++a) f(pos_of.load(nbr.load(a)));
    }
    // ... each with its entry of the CSR
    template <class F>
    ANS_MSET_HD void each_at(uint32_t node, F&& f) const {
        for (uint32_t a = off.load(node), end = off.load(node + 1); a < end; ++a) f(pos_of.load(nbr.load(a)), a);
    }
};

// (the labels' arrays come last: a state without labels is laid out as it was before there were any)
template <class Acc, class Slices, class Orbits, class L = NoLabels>
struct PushState : PushGraph<Acc>, Slices {
    Orbits orb;
    PushLabels<Acc, L> lab;
    template <class Ws, class... OrbitArgs>
    ANS_MSET_HD static PushState make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, OrbitArgs... args) {
        Take<Ws> take{ws, 0};
        PushState s{PushGraph<Acc>::make(take, max_nodes, max_edges), Slices::make(take, max_nodes, true),
                    Orbits::make(take, max_nodes, max_edges, args...), PushLabels<Acc, L>::make(take, max_nodes, max_edges)};
        return s;
    }
};
template <class Acc, class Slices, class Orbits, class L = NoLabels>
struct PopState : Slices {
    Orbits orb;
    PopLabels lab;  // (unread without labels)
    template <class Ws, class... OrbitArgs>
    ANS_MSET_HD static PopState make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, OrbitArgs... args) {
        Take<Ws> take{ws, 0};
        PopState s{Slices::make(take, max_nodes, false), Orbits::make(take, max_nodes, max_edges, args...), PopLabels{}};
        return s;
    }
};

// ---- push.  e: the E pairs; n nodes; perm: null, or n entries out, perm[position] = input node.
// Returns a status.  A slice is the tuple (N, Multiset<Edge<E>>) under (NodeC, EdgesIID<EdgeC, indices>)
// (graph/mod.rs:55, slice.rs:33-51, 185-192): the tuple pushes .1 first (src/codec.rs:468-479), and
// EdgesIID the labels before the indices (src/graph_codec.rs:61-65).
template <class M, class Acc, class Slices, class Orbits, class L>
ANS_MSET_HD int push_graph(polya::Coder<M>& c, PushState<Acc, Slices, Orbits, L>& st, uint32_t n, bool loops,
                           const uint32_t* e, uint32_t E, uint32_t* perm) {
    PushGraph<Acc>& g = st;
    if constexpr (L::edge) {
        if (const int rc = build_csr(g.off, g.nbr, st.scratch(), n, loops, e, E,
                                     [&](uint32_t at, uint32_t k) { st.lab.elab.store(at, st.lab.el[k]); }))
            return rc;
    } else {
        if (const int rc = build_csr(g.off, g.nbr, st.scratch(), n, loops, e, E)) return rc;
    }
    if constexpr (L::any)
        if (const int rc = st.lab.check(n, E)) return rc;
    // Prefix::from_full: position p holds input node p, every node known (graph/mod.rs:97-99)
    for (uint32_t v = 0; v < n; ++v) {
        g.pos_of.store(v, v);
        g.node_at.store(v, v);
    }
    st.start_push(n);
    st.orb.apply_full(st, n);
    for (uint32_t known = n; known > 0; --known) {
        const uint32_t last = known - 1;
        if (st.orb.coded()) {
            // orbit_codec.pop_element, x.swap(index, last), the orbits' swap and pop_id
            // (recursive/mod.rs:123-127)
            uint32_t index = last, cls = 0;
            if (const int rc = st.orb.pop_element(c, known, index, cls)) return rc;
            g.swap(index, last);
            st.orb.pop_id(index, last, cls);
        }
        // pop_slice (graph/mod.rs:57-66): the node's edges to positions >= last, then the stage's
        // update_after_pop_slice (incomplete.rs:212-221, 87-95)
        uint32_t len = 0;
        const auto gather = [&](uint32_t p, auto... at) {
            if (p < last) return;
            if constexpr (L::edge) st.lab.gather(len, p, at...);
            st.gather(len++, p, known);
            st.orb.touch(p);
        };
        if constexpr (L::edge) g.each_at(g.node_at.load(last), gather);
        else g.each(g.node_at.load(last), gather);
        st.orb.after_pop_slice(st, last);
        if constexpr (L::edge)
            if (const int rc = st.lab.push_edges(c, len)) return rc;
        if (const int rc = st.push(c, g, n, loops, last, len)) return rc;
        // ... and .0 last; pop_slice takes the label out (mem::take): the position is unknown from here on
        if constexpr (L::node)
            if (const int rc = push_cat(c, st.lab.node, st.lab.nl[g.node_at.load(last)])) return rc;
    }
    if (perm)
        for (uint32_t p = 0; p < n; ++p) perm[p] = g.node_at.load(p);
    return ANS_OK;
}

// ---- pop.  out receives the pairs (position, position), v ascending, within v in the slice model's
// order (ascending under L::sorted), at most cap of them (ANS_E_LEN beyond); *count their number.
template <class M, class Acc, class Slices, class Orbits, class L>
ANS_MSET_HD int pop_graph(polya::Coder<M>& c, PopState<Acc, Slices, Orbits, L>& st, uint32_t n, bool loops, uint32_t* out,
                          uint64_t cap, uint64_t* count) {
    uint64_t E = 0;
    *count = 0;
    st.start_pop(n, loops);
    if constexpr (L::any) st.orb.start_pop(n, out, st.lab.nl, st.lab.el);
    else st.orb.start_pop(n, out);
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t len = 0;
        // the tuple pops .0 first (src/codec.rs:468-479): the node's label
        if constexpr (L::node) {
            const uint32_t x = pop_cat(c, st.lab.node);
            if (c.err) return c.err;
            st.lab.nl[v] = x;
        }
        // push_slice (graph/mod.rs:82-95)
        const uint64_t first = E;
        if (const int rc = st.pop(c, n, loops, v, cap - E, len, [&](uint32_t w) {
                out[2 * E] = v;
                out[2 * E + 1] = w;
                if constexpr (!L::sorted) st.orb.add_pair(v, w, static_cast<uint32_t>(E));
                ++E;
            }))
            return rc;
        if constexpr (L::sorted) {
            // EdgesIID::pop (src/graph_codec.rs:67-72): the indices sorted, then a label each.  (An
            // insertion sort: both slice models give the other ends ascending but for the Erdős–Rényi
            // model's loop at the end, so it moves that one entry or none.)
            for (uint64_t k = first + 1; k < E; ++k) {
                const uint32_t w = out[2 * k + 1];
                uint64_t at = k;
                for (; at > first && out[2 * at - 1] > w; --at) out[2 * at + 1] = out[2 * at - 1];
                out[2 * at + 1] = w;
            }
            for (uint64_t k = first; k < E; ++k) {
                if constexpr (L::edge) {
                    const uint32_t x = pop_cat(c, st.lab.edge);
                    if (c.err) return c.err;
                    st.lab.el[k] = x;
                }
                st.orb.add_pair(v, out[2 * k + 1], static_cast<uint32_t>(k));
            }
        }
        // push_id, update_around_slice, push_element (recursive/mod.rs:143-145)
        if (const int rc = st.orb.push_element(c, v, len)) return rc;
    }
    *count = E;
    return ANS_OK;
}

}  // namespace rgraph
}  // namespace shuffle_coding
