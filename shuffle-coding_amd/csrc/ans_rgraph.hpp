// ans_rgraph.hpp — recursive shuffle coding of an undirected, unlabelled graph, one graph on one
// message: ShuffleCodec<SliceCodecs, OrbitCodecs> (src/recursive/mod.rs:117-148), written once over a
// slice model and an orbit stage, and with the stage that codes nothing Autoregressive(SliceCodecs)
// (src/recursive/mod.rs:190-216).  The slice models are ans_arer.hpp's ErSlices and ans_arpu.hpp's
// PuSlices; the orbit stages are ans_arer.hpp's counts per degree class (CountPush / CountPop: none,
// one class, a class per degree) and ans_wl.hpp's Weisfeiler-Lehman ids (Orbits / PopOrbits).  Plain
// C++ templated on the message and on how a per-graph array is read and written, host and device
// alike, so that the host codec (ans_capi.cpp), the kernels (ans_arer.hip, ans_arpu.hip, ans_wl.hip)
// and the CPU tests (g++, tests/native/*_state_check.cpp) run the same functions.  DESIGN.md §3.10
// has the restatement with its sources; the comments here say which reference line a step is.
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

// The pairs into a CSR in input labels: degrees into off, their running sums (off[v] = v's end), the
// fill moves each off[v] down to v's start.  The alphabet and a pair given twice are checked (mark: n
// entries of scratch).
template <class Acc>
ANS_MSET_HD int build_csr(Acc& off, Acc& nbr, Acc& mark, uint32_t n, bool loops, const uint32_t* e, uint32_t E) {
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
        if (i != j) {
            at = off.load(j) - 1;
            off.store(j, at);
            nbr.store(at, i);
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
};

template <class Acc, class Slices, class Orbits>
struct PushState : PushGraph<Acc>, Slices {
    Orbits orb;
    template <class Ws, class... OrbitArgs>
    ANS_MSET_HD static PushState make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, OrbitArgs... args) {
        Take<Ws> take{ws, 0};
        PushState s{PushGraph<Acc>::make(take, max_nodes, max_edges), Slices::make(take, max_nodes, true),
                    Orbits::make(take, max_nodes, max_edges, args...)};
        return s;
    }
};
template <class Acc, class Slices, class Orbits>
struct PopState : Slices {
    Orbits orb;
    template <class Ws, class... OrbitArgs>
    ANS_MSET_HD static PopState make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, OrbitArgs... args) {
        Take<Ws> take{ws, 0};
        PopState s{Slices::make(take, max_nodes, false), Orbits::make(take, max_nodes, max_edges, args...)};
        return s;
    }
};

// ---- push.  e: the E pairs; n nodes; perm: null, or n entries out, perm[position] = input node.
// Returns a status.
template <class M, class Acc, class Slices, class Orbits>
ANS_MSET_HD int push_graph(polya::Coder<M>& c, PushState<Acc, Slices, Orbits>& st, uint32_t n, bool loops,
                           const uint32_t* e, uint32_t E, uint32_t* perm) {
    PushGraph<Acc>& g = st;
    if (const int rc = build_csr(g.off, g.nbr, st.scratch(), n, loops, e, E)) return rc;
    // Prefix::from_full: position p holds input node p, every node known (graph/mod.rs:97-99)
    for (uint32_t v = 0; v < n; ++v) {
        g.pos_of.store(v, v);
        g.node_at.store(v, v);
    }
    st.start_push(n);
    st.orb.apply_full(g, n);
    for (uint32_t L = n; L > 0; --L) {
        const uint32_t last = L - 1;
        if (st.orb.coded()) {
            // orbit_codec.pop_element, x.swap(index, last), the orbits' swap and pop_id
            // (recursive/mod.rs:123-127)
            uint32_t index = last, cls = 0;
            if (const int rc = st.orb.pop_element(c, L, index, cls)) return rc;
            g.swap(index, last);
            st.orb.pop_id(index, last, cls);
        }
        // pop_slice (graph/mod.rs:57-66): the node's edges to positions >= L - 1, then the stage's
        // update_after_pop_slice (incomplete.rs:212-221, 87-95)
        uint32_t len = 0;
        g.each(g.node_at.load(last), [&](uint32_t p) {
            if (p < last) return;
            st.gather(len++, p, L);
            st.orb.touch(p);
        });
        st.orb.after_pop_slice(g, last);
        if (const int rc = st.push(c, g, n, loops, last, len)) return rc;
    }
    if (perm)
        for (uint32_t p = 0; p < n; ++p) perm[p] = g.node_at.load(p);
    return ANS_OK;
}

// ---- pop.  out receives the pairs (position, position), v ascending, within v in the slice model's
// order, at most cap of them (ANS_E_LEN beyond); *count their number.
template <class M, class Acc, class Slices, class Orbits>
ANS_MSET_HD int pop_graph(polya::Coder<M>& c, PopState<Acc, Slices, Orbits>& st, uint32_t n, bool loops, uint32_t* out,
                          uint64_t cap, uint64_t* count) {
    uint64_t E = 0;
    *count = 0;
    st.start_pop(n, loops);
    st.orb.start_pop(n, out);
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t len = 0;
        // push_slice (graph/mod.rs:82-95)
        if (const int rc = st.pop(c, n, loops, v, cap - E, len, [&](uint32_t w) {
                out[2 * E] = v;
                out[2 * E + 1] = w;
                st.orb.add_pair(v, w, static_cast<uint32_t>(E));
                ++E;
            }))
            return rc;
        // push_id, update_around_slice, push_element (recursive/mod.rs:143-145)
        if (const int rc = st.orb.push_element(c, v, len)) return rc;
    }
    *count = E;
    return ANS_OK;
}

}  // namespace rgraph
}  // namespace shuffle_coding
