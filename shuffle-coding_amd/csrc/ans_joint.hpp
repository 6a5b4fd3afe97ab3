// ans_joint.hpp — joint shuffle coding of an undirected, unlabelled graph, one graph on one message:
// ShuffleCodec<JointSliceCodecs<C>, WLOrbitCodecs<JointPrefix<Graph>>> (src/recursive/joint.rs,
// src/recursive/mod.rs:117-148, src/recursive/graph/incomplete.rs:154-187), as
// src/graph_codec.rs:405-450 runs it.  The graph is coded whole by an ordered codec C and the order of
// its nodes is taken back bits-back through the orbit stage of ans_wl.hpp, which is used as it is.  C is
// either the dense Erdős–Rényi indicator (GraphIID<EmptyCodec, EmptyCodec, ErdosRenyi<Undirected>>,
// src/graph_codec.rs:104-139, 184-199) or the ordered Pólya urn (polya_urn, ans_polya.hpp).  Plain C++
// templated on the message and on how a per-graph array is read and written, host and device alike, so
// that the host codec (ans_capi.cpp), the kernels (ans_joint.hip) and the CPU tests (g++,
// tests/native/joint_state_check.cpp) run the same functions.  DESIGN.md §3.14 has the restatement
// with its sources; the comments here say which reference line a step is.
//
// What differs from the recursion of ans_rgraph.hpp: a slice is empty, so the prefix graph keeps every
// edge (a neighbour counts even when both ends are unknown, the degree is the full degree), and an
// update has the node that changed sides alone at distance 0.
//
// Include this header before ans_lane.hpp: its loops call rgraph::push_graph / pop_graph by qualified
// name, and the overloads for the joint states at the end of this file must be declared by then.
#pragma once
#include <cstdint>

#include "../../include/ans_capi.h"
#include "ans_arer.hpp"
#include "ans_polya.hpp"
#include "ans_rgraph.hpp"
#include "ans_wl.hpp"

namespace shuffle_coding {
namespace joint {

// ---- the full graph as the orbit stage reads it on a push: the CSR in input labels and the positions
// (JointPrefix::full under the swaps so far), every neighbour whatever `len`
template <class Acc>
struct FullAdj {
    const Acc &pos_of, &node_at, &off, &nbr;
    template <class F>
    ANS_MSET_HD void each(uint32_t p, uint32_t, F&& f) const {
        const uint32_t u = node_at.load(p);
        for (uint32_t a = off.load(u), end = off.load(u + 1); a < end; ++a) f(pos_of.load(nbr.load(a)));
    }
    ANS_MSET_HD uint32_t degree(uint32_t p, uint32_t) const {
        const uint32_t u = node_at.load(p);
        return off.load(u + 1) - off.load(u);
    }
};

// ---- PrefixShuffleCodec::push (recursive/mod.rs:117-134) over JointPrefix up to the ordered codec:
// the n orbit pops.  st: a PushGraph with the members orb (wl::Orbits) and scr (n entries free until the
// ordered codec).  perm: null, or n entries out, perm[position] = input node.
template <class M, class Acc, class St>
ANS_MSET_HD int push_orbits(polya::Coder<M>& c, St& st, uint32_t n, bool loops, const uint32_t* e, uint32_t E, uint32_t* perm) {
    rgraph::PushGraph<Acc>& g = st;
    if (const int rc = rgraph::build_csr(g.off, g.nbr, st.scr, n, loops, e, E)) return rc;
    for (uint32_t v = 0; v < n; ++v) {  // JointPrefix::from_full (joint.rs:26-28)
        g.pos_of.store(v, v);
        g.node_at.store(v, v);
    }
    const FullAdj<Acc> adj{g.pos_of, g.node_at, g.off, g.nbr};
    st.orb.apply(adj, n, n);  // incomplete.rs:158-162
    st.orb.begin();
    for (uint32_t known = n; known > 0; --known) {
        const uint32_t last = known - 1;
        // pop_element, x.swap(index, last), the orbits' swap (recursive/mod.rs:123-127, joint.rs:40-44)
        uint32_t index = last, cls = 0;
        if (const int rc = st.orb.pop_element(c, known, index, cls)) return rc;
        g.swap(index, last);
        // pop_slice is len -= 1; update_after_pop_slice: pop_id, update_around(full, [len])
        // (incomplete.rs:164-172)
        st.orb.swap_and_pop(index);
        st.orb.touch(last);
        st.orb.around(adj);
        st.orb.begin();
    }
    if (perm)
        for (uint32_t p = 0; p < n; ++p) perm[p] = g.node_at.load(p);
    return ANS_OK;
}

// ---- PrefixShuffleCodec::pop (recursive/mod.rs:136-148) after the ordered codec: out holds the E
// decoded pairs of positions.  apply with every position unknown, then n times push_slice (len += 1),
// push_id, update_around(full, [len - 1]), push_element (incomplete.rs:174-182).
template <class M, class Acc>
ANS_MSET_HD int pop_orbits(polya::Coder<M>& c, wl::PopOrbits<Acc>& o, uint32_t n, const uint32_t* out, uint32_t E) {
    o.adj.out = out;
    o.adj.clear(n);
    for (uint32_t k = 0; k < E; ++k) o.adj.add(k);
    o.orb.apply(o.adj, n, 0);
    o.orb.begin();
    for (uint32_t v = 0; v < n; ++v)
        if (const int rc = o.push_element(c, v, 0)) return rc;
    return ANS_OK;
}

// ---- the ordered codecs.  Erdős–Rényi: IID<Bernoulli> over AllEdgeIndices (src/graph_codec.rs:104-139,
// 184-199): the loops first, then (i, j) by j, then by i; IID pushes the last slot first
// (src/codec.rs:415-420).  stamp: n entries; a row's indicator is the stamp of its neighbours' positions.
// (one indicator; the symbol is a constant on either side of the branch, so that the masses are named
// and not indexed: an index a value chooses kept the whole state in scratch memory on the device)
template <class M>
ANS_MSET_HD void push_indicator(polya::Coder<M>& c, const arer::Bern& bern, bool x) {
    if (x) arer::push_bit(c, bern, 1u);
    else arer::push_bit(c, bern, 0u);
}
template <class M, class Acc>
ANS_MSET_HD int push_dense(polya::Coder<M>& c, const rgraph::PushGraph<Acc>& g, Acc& stamp, const arer::Bern& bern, uint32_t n,
                           bool loops) {
    for (uint32_t p = 0; p < n; ++p) stamp.store(p, 0);
    for (uint32_t j = n; j-- > 0;) {
        g.each(g.node_at.load(j), [&](uint32_t q) { stamp.store(q, j + 1); });
        for (uint32_t i = j; i-- > 0;) push_indicator(c, bern, stamp.load(i) == j + 1);
        if (c.err) return c.err;
    }
    if (loops)
        for (uint32_t i = n; i-- > 0;) {
            bool has = false;
            g.each(g.node_at.load(i), [&](uint32_t q) { has = has || q == i; });
            push_indicator(c, bern, has);
        }
    return c.err;
}
// ... and its pop: the pairs in the alphabet's order, at most room of them (ANS_E_LEN beyond)
template <class M>
ANS_MSET_HD int pop_dense(polya::Coder<M>& c, const arer::Bern& bern, uint32_t n, bool loops, uint32_t* out, uint64_t room,
                          uint64_t& E) {
    E = 0;
    const auto take = [&](uint32_t i, uint32_t j) {
        const uint32_t x = arer::pop_bit(c, bern);
        if (c.err) return c.err;
        if (!x) return static_cast<int>(ANS_OK);
        if (E >= room) return static_cast<int>(ANS_E_LEN);
        out[2 * E] = i;
        out[2 * E + 1] = j;
        ++E;
        return static_cast<int>(ANS_OK);
    };
    if (loops)
        for (uint32_t i = 0; i < n; ++i)
            if (const int rc = take(i, i)) return rc;
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t i = 0; i < j; ++i)
            if (const int rc = take(i, j)) return rc;
    return ANS_OK;
}

// Pólya urn: polya::push_graph on the pairs relabelled to positions.  pair_at(k, i, j): pair k as
// positions, i <= j.  (polya::push_graph reads a pair list in memory; this is its body over a functor,
// kept here so that the ordered urn's own kernels stay as they are.  The alphabet and the duplicates are
// build_csr's checks by now.)
template <class M, class Acc, class PairAt>
ANS_MSET_HD int push_urn(polya::Coder<M>& c, polya::State<Acc>& st, uint32_t n, bool loops, bool redraws, PairAt&& pair_at,
                         uint32_t E) {
    const bool joint = E > polya::kPlainMax;
    const auto pair = [&](uint32_t k) {
        uint32_t i = 0, j = 0;
        pair_at(k, i, j);
        return (uint64_t(i) << 32) | j;
    };
    if (const int rc = polya::rank_elements(
            st, st.next, E, joint,
            [&](uint32_t k) {
                const uint64_t p = pair(k);
                return polya::edge_id(p >> 32, p & 0xFFFFFFFFu);
            },
            [&](uint32_t a, uint32_t b) { return pair(a) < pair(b); }, [&](uint32_t a, uint32_t b) { return pair(a) == pair(b); }))
        return rc;
    if (const int rc = polya::shuffle_push(c, st, E, joint)) return rc;
    // PolyaUrnEdgeIndicesCodec::push (src/graph_codec.rs:318-326) of the permuted vector
    auto edge_at = [&](uint32_t p, uint32_t& i, uint32_t& j) { pair_at(st.rop.load(p), i, j); };
    polya::graph_empty(st, n, redraws);
    for (uint32_t p = 0; p < E; ++p) {
        uint32_t i = 0, j = 0;
        edge_at(p, i, j);
        st.urn.tally(i);
        if (i != j) st.urn.tally(j);
        st.total += i != j ? 2 : 1;
        if (!redraws) polya::link_edge(st, p, i, j);
    }
    st.urn.build();
    for (uint32_t p = E; p-- > 0;) {
        uint32_t i = 0, j = 0;
        edge_at(p, i, j);
        if (!redraws) polya::unlink_edge(st, p, i, j);
        polya::urn_edge(st, i, j, -1);
        polya::push_edge(c, st, i, j, loops, redraws, edge_at);
        if (c.err) return c.err;
    }
    return ANS_OK;
}

// ---- the per-graph states, u32 entries.  The orbit stage and the ordered codec never run at the same
// time (a push runs the ordered codec after the last orbit step, a pop before the first), so the
// ordered codec's arrays lie over the orbit stage's:
//   Erdős–Rényi push   the prefix graph | the orbit stage; scr (build_csr's marks, then the rows' stamps)
//                      over the stage's first max_nodes entries
//   Erdős–Rényi pop    the decoded adjacency | the orbit stage (the dense pop keeps nothing)
//   Pólya urn push     the prefix graph | the orbit stage, and over it the ordered urn's state; scr
//                      (build_csr's marks) over the stage's first max_nodes entries
//   Pólya urn pop      the decoded adjacency | the orbit stage, and over both the ordered urn's state
// The orbit stage is wl::Orbits with its arrays as ans_wl.hpp lists them, but for the dirty list: an
// update starts from one position, so at wl_iter = 0 the list holds that one (a slice's update lists
// the slice).
constexpr uint64_t max2(uint64_t a, uint64_t b) { return a > b ? a : b; }
constexpr uint64_t dirty_entries(uint64_t max_nodes, uint32_t wl_iter) { return wl_iter || !max_nodes ? max_nodes : 1; }
constexpr uint64_t orbit_entries(uint64_t max_nodes, uint32_t wl_iter) {
    return wl::orbit_entries(max_nodes, wl_iter) - max_nodes + dirty_entries(max_nodes, wl_iter);
}
template <class Acc, class T>
ANS_MSET_HD wl::Orbits<Acc> orbit_stage(T& take, uint64_t max_nodes, uint32_t wl_iter, bool half_iter) {
    wl::Orbits<Acc> o{take(2 * (uint64_t(wl_iter) + 1) * max_nodes),
                      take(max_nodes),
                      take(max_nodes),
                      take(dirty_entries(max_nodes, wl_iter)),
                      take(max_nodes),
                      take(wl::sort_entries(max_nodes, wl_iter, false)),
                      wl_iter + 1,
                      half_iter ? 1u : 0u,
                      0,
                      0,
                      0,
                      0,
                      0};
    return o;
}
template <class Acc, class T>
ANS_MSET_HD wl::PopOrbits<Acc> pop_stage(T& take, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
    wl::PopOrbits<Acc> o{{take(max_nodes), take(2 * max_edges), take(max_nodes), nullptr, {}},
                         orbit_stage<Acc>(take, max_nodes, wl_iter, half_iter)};
    return o;
}
constexpr uint64_t er_push_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter) {
    return rgraph::graph_entries(max_nodes, max_edges) + orbit_entries(max_nodes, wl_iter);
}
constexpr uint64_t er_pop_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter) {
    return wl::pop_adj_entries(max_nodes, max_edges) + orbit_entries(max_nodes, wl_iter);
}
// polya::State's arrays from `take` (State::make names no lengths; these are ws_entries' terms).  A pop
// reads por in the plain shuffle alone, of at most kPlainMax pairs.
constexpr uint64_t por_entries(uint64_t max_edges, bool push) {
    return push || max_edges < polya::kPlainMax ? max_edges : polya::kPlainMax;
}
constexpr uint64_t urn_entries(uint64_t max_nodes, uint64_t max_edges, bool push) {
    return polya::ws_entries(max_nodes, max_edges) - max_edges + por_entries(max_edges, push);
}
template <class Acc, class T>
ANS_MSET_HD polya::State<Acc> urn_state(T& take, uint64_t max_nodes, uint64_t max_edges, bool push) {
    polya::State<Acc> s{{take(max_nodes + 1), 0},
                        {take(max_edges + 1), 0},
                        take(max_edges),
                        take(max_edges),
                        take(por_entries(max_edges, push)),
                        take(max_nodes),
                        take(2 * max_edges),
                        0};
    return s;
}
constexpr uint64_t pu_push_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter) {
    return rgraph::graph_entries(max_nodes, max_edges) +
           max2(orbit_entries(max_nodes, wl_iter), urn_entries(max_nodes, max_edges, true));
}
constexpr uint64_t pu_pop_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter) {
    return max2(wl::pop_adj_entries(max_nodes, max_edges) + orbit_entries(max_nodes, wl_iter),
                urn_entries(max_nodes, max_edges, false));
}

template <class Acc>
struct ErPush : rgraph::PushGraph<Acc> {
    wl::Orbits<Acc> orb;
    Acc scr;
    arer::Bern bern;
    template <class Ws>
    ANS_MSET_HD static ErPush make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        rgraph::Take<Ws> take{ws, 0};
        auto g = rgraph::PushGraph<Acc>::make(take, max_nodes, max_edges);
        rgraph::Take<Ws> over{ws, take.o};
        ErPush s{g, orbit_stage<Acc>(take, max_nodes, wl_iter, half_iter), over(max_nodes), arer::Bern{}};
        return s;
    }
};
template <class Acc>
struct ErPop {
    wl::PopOrbits<Acc> orb;
    arer::Bern bern;
    uint64_t max_edges;
    template <class Ws>
    ANS_MSET_HD static ErPop make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        rgraph::Take<Ws> take{ws, 0};
        ErPop s{pop_stage<Acc>(take, max_nodes, max_edges, wl_iter, half_iter), arer::Bern{}, max_edges};
        return s;
    }
};
template <class Acc>
struct PuPush : rgraph::PushGraph<Acc> {
    wl::Orbits<Acc> orb;
    Acc scr;
    polya::State<Acc> urn;
    bool redraws;
    template <class Ws>
    ANS_MSET_HD static PuPush make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        rgraph::Take<Ws> take{ws, 0};
        auto g = rgraph::PushGraph<Acc>::make(take, max_nodes, max_edges);
        rgraph::Take<Ws> over{ws, take.o}, urn{ws, take.o};
        PuPush s{g, orbit_stage<Acc>(take, max_nodes, wl_iter, half_iter), over(max_nodes),
                 urn_state<Acc>(urn, max_nodes, max_edges, true), false};
        return s;
    }
};
template <class Acc>
struct PuPop {
    wl::PopOrbits<Acc> orb;
    polya::State<Acc> urn;
    bool redraws;
    uint64_t max_edges;
    template <class Ws>
    ANS_MSET_HD static PuPop make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        rgraph::Take<Ws> take{ws, 0}, urn{ws, 0};
        PuPop s{pop_stage<Acc>(take, max_nodes, max_edges, wl_iter, half_iter), urn_state<Acc>(urn, max_nodes, max_edges, false),
                false, max_edges};
        return s;
    }
};

// ---- the whole codecs
template <class M, class Acc>
ANS_MSET_HD int push_joint(polya::Coder<M>& c, ErPush<Acc>& st, uint32_t n, bool loops, const uint32_t* e, uint32_t E,
                           uint32_t* perm) {
    if (const int rc = push_orbits<M, Acc>(c, st, n, loops, e, E, perm)) return rc;
    return push_dense(c, st, st.scr, st.bern, n, loops);  // EmptyJointPrefixCodec::push (joint.rs:87-89)
}
template <class M, class Acc>
ANS_MSET_HD int push_joint(polya::Coder<M>& c, PuPush<Acc>& st, uint32_t n, bool loops, const uint32_t* e, uint32_t E,
                           uint32_t* perm) {
    if (const int rc = push_orbits<M, Acc>(c, st, n, loops, e, E, perm)) return rc;
    return push_urn(c, st.urn, n, loops, st.redraws,
                    [&](uint32_t k, uint32_t& i, uint32_t& j) {
                        const uint32_t a = st.pos_of.load(e[2 * uint64_t(k)]), b = st.pos_of.load(e[2 * uint64_t(k) + 1]);
                        i = a < b ? a : b;
                        j = a < b ? b : a;
                    },
                    E);
}
// out receives the pairs (position, position): under the Erdős–Rényi codec in the alphabet's order, at
// most cap of them and at most the state's max_edges (ANS_E_LEN beyond), *count their number; under the
// urn the cap pairs the graph has (the codec's parameter; more than the state's max_edges is ANS_E_ARG),
// as polya::pop_graph gives them.
template <class M, class Acc>
ANS_MSET_HD int pop_joint(polya::Coder<M>& c, ErPop<Acc>& st, uint32_t n, bool loops, uint32_t* out, uint64_t cap,
                          uint64_t* count) {
    *count = 0;
    uint64_t E = 0;
    if (const int rc = pop_dense(c, st.bern, n, loops, out, cap < st.max_edges ? cap : st.max_edges, E)) return rc;
    if (const int rc = pop_orbits(c, st.orb, n, out, static_cast<uint32_t>(E))) return rc;
    *count = E;
    return ANS_OK;
}
template <class M, class Acc>
ANS_MSET_HD int pop_joint(polya::Coder<M>& c, PuPop<Acc>& st, uint32_t n, bool loops, uint32_t* out, uint64_t cap,
                          uint64_t* count) {
    *count = 0;
    if (cap > st.max_edges) return ANS_E_ARG;
    const uint32_t E = static_cast<uint32_t>(cap);
    if (const int rc = polya::pop_graph(c, st.urn, n, loops, st.redraws, out, E)) return rc;
    if (const int rc = pop_orbits(c, st.orb, n, out, E)) return rc;
    *count = E;
    return ANS_OK;
}

// Bytes a message can grow by during a push or a pop (ans_gpu_joint_er_slack, ans_gpu_joint_polya_slack;
// DESIGN.md §3.14 derives them).  A push's n orbit pops add nothing and its ordered push adds what the
// ordered codec's bound says; a pop's ordered pop adds what that bound says (nothing for the dense
// indicators) and its n orbit pushes at most bitlen(max_nodes) bits each.  Under the Erdős–Rényi codec
// that is arer::slack as it stands: the same n (n - 1) / 2 + n loops indicators on a push, the same n
// orbit pushes on a pop.  Under the urn the orbit pushes come on top of polya::slack, whose pop side the
// ordered pop's own shuffle uses up.
constexpr uint64_t er_slack(const arer::Bern& b, uint64_t max_nodes, bool loops) { return arer::slack(b, max_nodes, loops); }
constexpr uint64_t pu_slack(uint64_t max_nodes, uint64_t max_edges) {
    return polya::slack(max_nodes, max_edges) + max_nodes * polya::bit_len(max_nodes) / 8 + 1 + (max_nodes >> 20);
}

}  // namespace joint

// ans_lane.hpp's loops code a graph by these names
namespace rgraph {
template <class M, class Acc>
ANS_MSET_HD int push_graph(polya::Coder<M>& c, joint::ErPush<Acc>& st, uint32_t n, bool loops, const uint32_t* e, uint32_t E,
                           uint32_t* perm) {
    return joint::push_joint(c, st, n, loops, e, E, perm);
}
template <class M, class Acc>
ANS_MSET_HD int push_graph(polya::Coder<M>& c, joint::PuPush<Acc>& st, uint32_t n, bool loops, const uint32_t* e, uint32_t E,
                           uint32_t* perm) {
    return joint::push_joint(c, st, n, loops, e, E, perm);
}
template <class M, class Acc>
ANS_MSET_HD int pop_graph(polya::Coder<M>& c, joint::ErPop<Acc>& st, uint32_t n, bool loops, uint32_t* out, uint64_t cap,
                          uint64_t* count) {
    return joint::pop_joint(c, st, n, loops, out, cap, count);
}
template <class M, class Acc>
ANS_MSET_HD int pop_graph(polya::Coder<M>& c, joint::PuPop<Acc>& st, uint32_t n, bool loops, uint32_t* out, uint64_t cap,
                          uint64_t* count) {
    return joint::pop_joint(c, st, n, loops, out, cap, count);
}
}  // namespace rgraph

}  // namespace shuffle_coding
