// ans_polya.hpp — the Pólya urn model of a graph's edge set:
// multiset_shuffle_codec(PolyaUrnEdgeIndicesCodec<Undirected>{num_nodes, num_edges, loops, redraws})
// (src/graph_codec.rs:210-375, src/recursive/multiset.rs:126-136), one graph on one message.
// Plain C++ templated on the message and on how a per-graph array is read and written, host and
// device alike, so that the host codec (ans_capi.cpp), the kernels (ans_polya.hip) and the CPU
// tests (g++, tests/test_polya_host.py) run the same functions.  DESIGN.md §3.9 has the
// restatement with its sources; the comments here say which reference line a step is.
#pragma once
#include <cstdint>

#include "../../include/ans_capi.h"
#include "ans_mset.hpp"

namespace shuffle_coding {
namespace polya {

constexpr uint32_t kNil = 0xFFFFFFFFu;
constexpr uint64_t kK = 1ull << 56;            // MAX_MIN_HEAD, src/ans.rs:19
constexpr uint32_t kPlainMax = 11;             // src/recursive/multiset.rs:131
constexpr uint64_t kMaxEdges = 0x7FFFFFFFull;  // the adjacency slots 2e, 2e + 1 stay below kNil

// hash((i, j)) of src/recursive/prefix_orbit.rs:132-136 for a pair of usizes: the tuple feeds
// DefaultHasher (SipHash-1-3, keys 0, 0) its two fields in turn, 16 little-endian bytes in all,
// two whole blocks; the final block carries the length, 16 << 56.
constexpr uint64_t edge_id(uint64_t i, uint64_t j) {
    uint64_t v0 = 0x736f6d6570736575ull, v1 = 0x646f72616e646f6dull, v2 = 0x6c7967656e657261ull,
             v3 = 0x7465646279746573ull;
    v3 ^= i;
    mset::sip_round(v0, v1, v2, v3);
    v0 ^= i;
    v3 ^= j;
    mset::sip_round(v0, v1, v2, v3);
    v0 ^= j;
    const uint64_t tail = 16ull << 56;
    v3 ^= tail;
    mset::sip_round(v0, v1, v2, v3);
    v0 ^= tail;
    v2 ^= 0xff;
    mset::sip_round(v0, v1, v2, v3);
    mset::sip_round(v0, v1, v2, v3);
    mset::sip_round(v0, v1, v2, v3);
    return v0 ^ v1 ^ v2 ^ v3;
}

// The per-graph state, u32 entries: Ws::at(offset) is an accessor (uint32_t load(uint32_t),
// void store(uint32_t, uint32_t), as mset::Counts takes) of the entries from `offset` on.
//   urn   the node urn, a Fenwick tree over the nodes in ascending index (mass = degree + 1)
//   orb   the 0/1 orbit counts per rank (joint codec); the ordered codec, which runs while orb is
//         idle, keeps the masses use_codec_without took out in it; the plain pop keeps its js there
//   ord   ord[r] = the edge of rank r (by orbit id; by tuple for E <= 11)
//   rop   rank of the edge at a position | the Fisher-Yates p | (push) the edge at a position
//   por   position of a rank | p's inverse
//   head, next   the adjacency stacks: head[v] = v's newest slot, next[slot] the one before;
//         edge p's slots are 2p (in i's stack, naming j) and 2p + 1 (in j's, naming i; none for a
//         loop).  Edges leave in the reverse of the order they came, so push and pop of a stack
//         suffice.  Before the ordered stage of a push / after that of a pop, next holds the
//         64-bit orbit ids (low, high) the sort compares.
constexpr uint64_t ws_entries(uint64_t max_nodes, uint64_t max_edges) { return 2 * max_nodes + 6 * max_edges + 2; }
template <class Acc>
struct State {
    mset::Counts<Acc> urn, orb;
    Acc ord, rop, por, head, next;
    uint64_t total;  // the urn's norm
    template <class Ws>
    ANS_MSET_HD static State make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges) {
        uint64_t o = 0;
        auto take = [&](uint64_t n) {
            const uint64_t at = o;
            o += n;
            return ws.at(at);
        };
        State s{{take(max_nodes + 1), 0}, {take(max_edges + 1), 0}, take(max_edges), take(max_edges), take(max_edges),
                take(max_nodes),       take(2 * max_edges),        0};
        return s;
    }
};

// The blanket push / pop (src/ans.rs:96-116) on a message M: uint64_t head, and
// bool renorm(uint64_t min_head) (src/ans.rs:233-253), false when the tail's generator is Empty
// and the pull ran past the stream's start (src/ans.rs:144).  The first failure sticks.
template <class M>
struct Coder {
    M& m;
    int err;
    ANS_MSET_HD bool renorm(uint64_t min_head) {
        if (err) return false;
        if (!m.renorm(min_head)) err = ANS_E_EXHAUSTED;
        return !err;
    }
    ANS_MSET_HD bool pop_begin(uint64_t norm, uint64_t& q, uint64_t& cf) {  // src/ans.rs:108-111
        if (!renorm(norm * (kK / norm))) return false;
        q = m.head / norm;
        cf = m.head - q * norm;
        return true;
    }
    ANS_MSET_HD void pop_end(uint64_t p, uint64_t q, uint64_t r) { m.head = p * q + r; }  // src/ans.rs:114
    ANS_MSET_HD void push(uint64_t p, uint64_t norm, uint64_t c) {                       // src/ans.rs:97-104
        if (!renorm(p * (kK / norm))) return;
        m.head = norm * (m.head / p) + c + m.head % p;
    }
    // Uniform (src/codec.rs:13-49): pmf 1, cdf x.  Uniform(1) is renorm(2^56) and nothing else;
    // it is kept wherever the reference has it.
    ANS_MSET_HD uint64_t pop_uniform(uint64_t size) {
        uint64_t q = 0, cf = 0;
        if (pop_begin(size, q, cf)) pop_end(1, q, 0);
        return cf;
    }
    ANS_MSET_HD void push_uniform(uint64_t size, uint64_t x) { push(1, size, x); }
};

template <class Acc, class Less>
ANS_MSET_HD void sift_down(Acc& a, uint32_t root, uint32_t n, Less& less) {
    const uint32_t v = a.load(root);
    for (;;) {
        uint32_t child = 2 * root + 1;
        if (child >= n) break;
        uint32_t c = a.load(child);
        if (child + 1 < n) {
            const uint32_t c2 = a.load(child + 1);
            if (less(c, c2)) {
                ++child;
                c = c2;
            }
        }
        if (!less(v, c)) break;
        a.store(root, c);
        root = child;
    }
    a.store(root, v);
}
// a[0 .. n) ascending under less (heapsort: in place, no recursion, O(n log n) whatever the input)
template <class Acc, class Less>
ANS_MSET_HD void heapsort(Acc& a, uint32_t n, Less less) {
    for (uint32_t s = n / 2; s-- > 0;) sift_down(a, s, n, less);
    for (uint32_t end = n; end-- > 1;) {
        const uint32_t top = a.load(0);
        a.store(0, a.load(end));
        a.store(end, top);
        sift_down(a, 0, end, less);
    }
}

// ---- the outer layers of multiset_shuffle_codec over E distinct elements (src/recursive/
// multiset.rs:126-136): plain_shuffle_codec for E <= 11, the joint recursive codec with singleton
// orbits beyond.  Shared by this codec (the elements are the graph's pairs) and ans_arpu.hpp (the
// pairs of one slice).  St has the members orb, ord, rop, por as State names them; ids is an accessor
// of 2 E entries, idle outside rank_elements for the caller's other uses.

// ord = the elements 0 .. E-1 in ascending order: by orbit id when joint (id_of(k), kept in ids as
// (low, high)), else as tuples (tuple_less(a, b)).  ANS_E_SYMBOL when an element occurs twice
// (same(a, b); insert_plain_edge asserts, src/graph_codec.rs:257), ANS_E_ARG when two different
// elements share an orbit id (they would share an orbit; not built).
template <class St, class Ids, class IdOf, class Less, class Same>
ANS_MSET_HD int rank_elements(St& st, Ids& ids, uint32_t E, bool joint, IdOf id_of, Less tuple_less, Same same) {
    for (uint32_t k = 0; k < E; ++k) st.ord.store(k, k);
    if (joint) {
        for (uint32_t k = 0; k < E; ++k) {
            const uint64_t id = id_of(k);
            ids.store(2 * k, static_cast<uint32_t>(id));
            ids.store(2 * k + 1, static_cast<uint32_t>(id >> 32));
        }
        const Ids& rd = ids;
        heapsort(st.ord, E, [&](uint32_t a, uint32_t b) {
            const uint32_t ha = rd.load(2 * a + 1), hb = rd.load(2 * b + 1);
            return ha != hb ? ha < hb : rd.load(2 * a) < rd.load(2 * b);
        });
    } else {
        heapsort(st.ord, E, tuple_less);
    }
    for (uint32_t r = 1; r < E; ++r) {
        const uint32_t a = st.ord.load(r - 1), b = st.ord.load(r);
        if (same(a, b)) return ANS_E_SYMBOL;
        if (joint && ids.load(2 * a) == ids.load(2 * b) && ids.load(2 * a + 1) == ids.load(2 * b + 1))
            return ANS_E_ARG;
    }
    return ANS_OK;
}
template <class Acc>
ANS_MSET_HD int rank_edges(State<Acc>& st, const uint32_t* e, uint32_t E, bool joint) {
    return rank_elements(
        st, st.next, E, joint, [&](uint32_t k) { return edge_id(e[2 * uint64_t(k)], e[2 * uint64_t(k) + 1]); },
        [&](uint32_t a, uint32_t b) {
            const uint32_t ia = e[2 * uint64_t(a)], ib = e[2 * uint64_t(b)];
            return ia != ib ? ia < ib : e[2 * uint64_t(a) + 1] < e[2 * uint64_t(b) + 1];
        },
        [&](uint32_t a, uint32_t b) {
            return e[2 * uint64_t(a)] == e[2 * uint64_t(b)] && e[2 * uint64_t(a) + 1] == e[2 * uint64_t(b) + 1];
        });
}

// The push side, after rank_elements: pops the order the ordered codec will see; rop[p] = the
// element at position p of the permuted vector.  Returns a status.
template <class M, class St>
ANS_MSET_HD int shuffle_push(Coder<M>& c, St& st, uint32_t E, bool joint) {
    if (!joint) {
        // plain_shuffle_codec (src/plain/mod.rs:111-116): canonized() sorts; the group is trivial,
        // so RCosetUniform::pop is PermutationUniform{E}::pop and E Uniform(1) pushes
        for (uint32_t k = 0; k < E; ++k) st.por.store(k, k);
        for (uint32_t k = E; k-- > 0;) {
            const uint32_t x = static_cast<uint32_t>(c.pop_uniform(k + 1));
            const uint32_t a = st.por.load(k), b = st.por.load(x);
            st.por.store(k, b);
            st.por.store(x, a);
        }
        for (uint32_t k = 0; k < E; ++k) c.push_uniform(1, 0);
        if (c.err) return c.err;
        // perm * x (_permuted_from_swap, src/permutable.rs:26-41): the k-th smallest goes to perm[k]
        for (uint32_t k = 0; k < E; ++k) st.rop.store(st.por.load(k), st.ord.load(k));
    } else {
        // PrefixShuffleCodec::push (src/recursive/mod.rs:117-134) with unit slices (joint.rs) and
        // singleton orbits (multiset.rs:105-124): position p starts with the element of rank p
        st.orb.nsym = E;
        for (uint32_t r = 0; r < E; ++r) {
            st.orb.a.store(r, 1);
            st.rop.store(r, r);
            st.por.store(r, r);
        }
        st.orb.build();
        for (uint32_t L = E; L > 0; --L) {
            uint64_t q = 0, cf = 0;
            if (!c.pop_begin(L, q, cf)) return c.err;
            const uint32_t r = st.orb.find(cf).rank;
            c.pop_end(1, q, 0);
            const uint32_t at = st.por.load(r), last = L - 1, r2 = st.rop.load(last);
            st.rop.store(at, r2);
            st.por.store(r2, at);
            st.rop.store(last, r);
            st.por.store(r, last);
            st.orb.add(r, -1);
        }
        for (uint32_t p = 0; p < E; ++p) st.rop.store(p, st.ord.load(st.rop.load(p)));
    }
    return ANS_OK;
}

// The pop side, after the ordered codec's pop and rank_elements of what it returned (element k =
// the k-th popped): pushes the order back.  Returns a status.
template <class M, class St>
ANS_MSET_HD int shuffle_pop(Coder<M>& c, St& st, uint32_t E, bool joint) {
    if (!joint) {
        // plain_shuffle_codec's pop (src/plain/mod.rs:118-123): canon^-1 = ord; RCosetUniform::push
        // is E Uniform(1) pops and PermutationUniform{E}::push (src/permutable.rs:184-200)
        for (uint32_t k = 0; k < E; ++k) c.pop_uniform(1);
        for (uint32_t k = 0; k < E; ++k) {
            st.rop.store(k, k);
            st.por.store(k, k);
        }
        for (uint32_t k = E; k-- > 0;) {
            const uint32_t xi = st.ord.load(k), x = st.por.load(xi), pk = st.rop.load(k);
            const uint32_t a = st.por.load(pk);  // p_inv.swap(p * k, xi)
            st.por.store(pk, x);
            st.por.store(xi, a);
            const uint32_t b = st.rop.load(x);  // p.swap(k, x)
            st.rop.store(x, pk);
            st.rop.store(k, b);
            st.orb.a.store(k, x);
        }
        for (uint32_t k = 0; k < E; ++k) c.push_uniform(k + 1, st.orb.a.load(k));
    } else {
        // PrefixShuffleCodec::pop (src/recursive/mod.rs:136-148): element k joins, its orbit is pushed
        for (uint32_t r = 0; r < E; ++r) st.rop.store(st.ord.load(r), r);
        st.orb.nsym = E;
        st.orb.clear();
        for (uint32_t k = 0; k < E; ++k) {
            const uint32_t r = st.rop.load(k);
            st.orb.add(r, 1);
            c.push(1, uint64_t(k) + 1, st.orb.prefix(r));
            if (c.err) return c.err;
        }
    }
    return c.err;
}

// ---- the graph the ordered codec keeps: PlainGraph + MutCategorical (src/graph_codec.rs:211-264)
template <class Acc>
ANS_MSET_HD void graph_empty(State<Acc>& st, uint32_t n, bool redraws) {  // :224 on the empty graph
    st.urn.nsym = n;
    for (uint32_t v = 0; v < n; ++v) st.urn.a.store(v, 1);
    st.total = n;
    if (!redraws)
        for (uint32_t v = 0; v < n; ++v) st.head.store(v, kNil);
}
template <class Acc>
ANS_MSET_HD void link_edge(State<Acc>& st, uint32_t p, uint32_t i, uint32_t j) {
    st.next.store(2 * p, st.head.load(i));
    st.head.store(i, 2 * p);
    if (i != j) {
        st.next.store(2 * p + 1, st.head.load(j));
        st.head.store(j, 2 * p + 1);
    }
}
template <class Acc>
ANS_MSET_HD void unlink_edge(State<Acc>& st, uint32_t p, uint32_t i, uint32_t j) {  // p is the newest edge
    st.head.store(i, st.next.load(2 * p));
    if (i != j) st.head.store(j, st.next.load(2 * p + 1));
}
// insert_edge / remove_edge's urn side (:250-253, 259-262): a loop counts once
template <class Acc>
ANS_MSET_HD void urn_edge(State<Acc>& st, uint32_t i, uint32_t j, int32_t d) {
    st.urn.add(i, d);
    if (i != j) st.urn.add(j, d);
    st.total += static_cast<uint64_t>(static_cast<int64_t>(d) * (i != j ? 2 : 1));
}

// use_codec_without (:229-245): the masses of `node` itself when !loops and of its neighbours in
// the graph as it stands when !redraws leave the urn (kept in orb's entries, in walk order);
// returns what left.  include() walks the same way and puts them back.  EdgeAt: the pair at a
// position of the vector being coded, p -> (i, j).
template <class Acc, class EdgeAt>
ANS_MSET_HD uint64_t exclude(State<Acc>& st, uint32_t node, bool loops, bool redraws, EdgeAt& edge_at) {
    uint64_t gone = 0;
    uint32_t t = 0;
    auto drop = [&](uint32_t v) {
        const uint32_t c = st.urn.count(v);
        st.orb.a.store(t++, c);
        if (c) st.urn.add(v, -static_cast<int32_t>(c));
        gone += c;
    };
    if (!loops) drop(node);
    if (!redraws)
        for (uint32_t s = st.head.load(node); s != kNil; s = st.next.load(s)) {
            uint32_t i = 0, j = 0;
            edge_at(s >> 1, i, j);
            drop((s & 1) ? i : j);
        }
    return gone;
}
template <class Acc, class EdgeAt>
ANS_MSET_HD void include(State<Acc>& st, uint32_t node, bool loops, bool redraws, EdgeAt& edge_at) {
    uint32_t t = 0;
    auto back = [&](uint32_t v) {
        const uint32_t c = st.orb.a.load(t++);
        if (c) st.urn.add(v, static_cast<int32_t>(c));
    };
    if (!loops) back(node);
    if (!redraws)
        for (uint32_t s = st.head.load(node); s != kNil; s = st.next.load(s)) {
            uint32_t i = 0, j = 0;
            edge_at(s >> 1, i, j);
            back((s & 1) ? i : j);
        }
}

// ---- one edge: plain_shuffle_codec(PolyaUrnEdgeIndexCodec) on the 2-vector [i, j], i <= j
// (src/plain/mod.rs:111-116, src/graph_codec.rs:269-276).  The edge is out of the graph already.
template <class M, class Acc, class EdgeAt>
ANS_MSET_HD void push_edge(Coder<M>& c, State<Acc>& st, uint32_t i, uint32_t j, bool loops, bool redraws,
                           EdgeAt& edge_at) {
    // RCosetUniform::pop (plain/mod.rs:258-263): PermutationUniform{2}::pop (permutable.rs:202-212)
    const uint64_t j1 = c.pop_uniform(2);
    c.pop_uniform(1);
    // ... then AutomorphismUniform::push down the stabiliser chain, last base first
    // (plain/mod.rs:209-214): orbits {0}, {1} for i != j; {0, 1}, {1} for i == j, whose min element
    // under the popped permutation is 0 for the identity (j1 = 1) and 1 for the swap (:334-337)
    c.push_uniform(1, 0);
    if (i != j) c.push_uniform(1, 0);
    else c.push_uniform(2, 1 - j1);
    // coset_min * x: the swap (j1 = 0) turns [i, j] round; [i, i] stays
    const uint32_t node = (i == j || j1 == 1) ? i : j, node_ = (i == j || j1 == 1) ? j : i;
    if (c.err) return;
    const uint64_t gone = exclude(st, node, loops, redraws, edge_at);  // graph_codec.rs:271
    const uint64_t p = st.urn.count(node_);
    if (p == 0) c.err = ANS_E_ZERO_MASS;  // src/ans.rs:98 (not reached from a valid edge list)
    else c.push(p, st.total - gone, st.urn.prefix(node_));
    include(st, node, loops, redraws, edge_at);
    if (c.err) return;
    c.push(st.urn.count(node), st.total, st.urn.prefix(node));  // :272
}

// pop (src/plain/mod.rs:118-123, src/graph_codec.rs:278-282): the pair comes back sorted
template <class M, class Acc, class EdgeAt>
ANS_MSET_HD void pop_edge(Coder<M>& c, State<Acc>& st, uint32_t& i, uint32_t& j, bool loops, bool redraws,
                          EdgeAt& edge_at) {
    i = j = 0;
    uint64_t q = 0, cf = 0;
    if (st.total == 0) {  // a graph without nodes has no edge to decode
        c.err = ANS_E_ZERO_MASS;
        return;
    }
    if (!c.pop_begin(st.total, q, cf)) return;
    mset::Found f = st.urn.find(cf);
    c.pop_end(f.count, q, cf - f.cum);
    const uint32_t node = f.rank;
    const uint64_t gone = exclude(st, node, loops, redraws, edge_at);
    const uint64_t norm = st.total - gone;
    uint32_t node_ = 0;
    if (norm == 0) c.err = ANS_E_ZERO_MASS;  // every node excluded: the reference divides by zero
    else if (c.pop_begin(norm, q, cf)) {
        f = st.urn.find(cf);
        c.pop_end(f.count, q, cf - f.cum);
        node_ = f.rank;
    }
    include(st, node, loops, redraws, edge_at);
    if (c.err) return;
    // canonized(), then RCosetUniform::push of canon^-1 (plain/mod.rs:251-256): AutomorphismUniform::pop
    // up the chain (:216-223), then PermutationUniform{2}::push (permutable.rs:184-200)
    if (node != node_) {
        c.pop_uniform(1);
        c.pop_uniform(1);
        c.push_uniform(1, 0);
        c.push_uniform(2, node < node_ ? 1 : 0);
    } else {
        const uint64_t e = c.pop_uniform(2);
        c.pop_uniform(1);
        c.push_uniform(1, 0);
        c.push_uniform(2, 1 - e);
    }
    i = node < node_ ? node : node_;
    j = node < node_ ? node_ : node;
}

// ---- the whole codec.  e: the E pairs; n nodes.  Returns a status; the message is c.m.
template <class M, class Acc>
ANS_MSET_HD int push_graph(Coder<M>& c, State<Acc>& st, uint32_t n, bool loops, bool redraws, const uint32_t* e,
                           uint32_t E) {
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t i = e[2 * uint64_t(k)], j = e[2 * uint64_t(k) + 1];
        if (i > j || j >= n || (i == j && !loops)) return ANS_E_SYMBOL;
    }
    const bool joint = E > kPlainMax;
    if (const int rc = rank_edges(st, e, E, joint)) return rc;
    if (const int rc = shuffle_push(c, st, E, joint)) return rc;
    // PolyaUrnEdgeIndicesCodec::push (src/graph_codec.rs:318-326) of the permuted vector
    auto edge_at = [&](uint32_t p, uint32_t& i, uint32_t& j) {
        const uint64_t k = st.rop.load(p);
        i = e[2 * k];
        j = e[2 * k + 1];
    };
    graph_empty(st, n, redraws);
    for (uint32_t p = 0; p < E; ++p) {
        uint32_t i = 0, j = 0;
        edge_at(p, i, j);
        st.urn.tally(i);
        if (i != j) st.urn.tally(j);
        st.total += i != j ? 2 : 1;
        if (!redraws) link_edge(st, p, i, j);
    }
    st.urn.build();
    for (uint32_t p = E; p-- > 0;) {
        uint32_t i = 0, j = 0;
        edge_at(p, i, j);
        if (!redraws) unlink_edge(st, p, i, j);
        urn_edge(st, i, j, -1);
        push_edge(c, st, i, j, loops, redraws, edge_at);
        if (c.err) return c.err;
    }
    return ANS_OK;
}

// out receives the E pairs: sorted for E <= 11, in pop order beyond
template <class M, class Acc>
ANS_MSET_HD int pop_graph(Coder<M>& c, State<Acc>& st, uint32_t n, bool loops, bool redraws, uint32_t* out, uint32_t E) {
    auto edge_at = [&](uint32_t p, uint32_t& i, uint32_t& j) {
        i = out[2 * uint64_t(p)];
        j = out[2 * uint64_t(p) + 1];
    };
    // PolyaUrnEdgeIndicesCodec::pop (src/graph_codec.rs:328-342)
    graph_empty(st, n, redraws);
    st.urn.build();
    for (uint32_t p = 0; p < E; ++p) {
        uint32_t i = 0, j = 0;
        pop_edge(c, st, i, j, loops, redraws, edge_at);
        if (c.err) return c.err;
        out[2 * uint64_t(p)] = i;
        out[2 * uint64_t(p) + 1] = j;
        if (!redraws) link_edge(st, p, i, j);
        urn_edge(st, i, j, 1);
    }
    const bool joint = E > kPlainMax;
    // (an edge decoded twice, possible with redraws alone, is found here, not at its insert: the
    // urn and the stacks hold a multigraph as well as a graph)
    if (const int rc = rank_edges(st, out, E, joint)) return rc;
    if (const int rc = shuffle_pop(c, st, E, joint)) return rc;
    if (!joint) {  // the pairs come back sorted
        for (uint32_t k = 0; k < 2 * E; ++k) st.next.store(k, out[k]);
        for (uint32_t r = 0; r < E; ++r) {
            const uint32_t k = st.ord.load(r);
            out[2 * r] = st.next.load(2 * k);
            out[2 * r + 1] = st.next.load(2 * k + 1);
        }
    }
    return ANS_OK;
}

// Bytes a message can grow by during a push or a pop of a graph of at most max_nodes nodes and
// max_edges edges (ans_gpu_polya_slack; DESIGN.md §3.9 derives it): a push adds two urn symbols
// per edge under norms <= max_nodes + 2 max_edges, a pop puts back an orbit (norm <= max_edges) and
// an orientation bit per edge; a byte per 2^20 edges for the quotients' floors, and 16 more for the
// head's bytes at flatten and a renorm in flight.
constexpr uint64_t bit_len(uint64_t x) {
    uint64_t b = 0;
    while (b < 64 && (x >> b)) ++b;
    return b;
}
constexpr uint64_t slack(uint64_t max_nodes, uint64_t max_edges) {
    const uint64_t push_bits = 2 * bit_len(max_nodes + 2 * max_edges), pop_bits = bit_len(max_edges) + 1;
    return (max_edges / 8 + 1) * (push_bits > pop_bits ? push_bits : pop_bits) + (max_edges >> 20) + 16;
}

}  // namespace polya
}  // namespace shuffle_coding
