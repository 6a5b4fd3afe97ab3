// ans_wl.hpp — the orbit stage of recursive shuffle coding on graphs at any wl_iter: the
// Weisfeiler-Lehman ids of WLOrbitCodecs<GraphPrefix> (src/recursive/graph/incomplete.rs:45-57,
// 87-151, 189-236) and the PrefixOrbitCodec over them (src/recursive/prefix_orbit.rs), with the
// autoregressive Erdős–Rényi slices of ans_arer.hpp and the Pólya urn slices of ans_arpu.hpp on top,
// one graph on one message.  Plain C++ templated on the message and on how a per-graph array is read
// and written, host and device alike, so that the host codec (ans_capi.cpp), the kernels
// (ans_wl.hip) and the CPU tests (g++, tests/native/wl_state_check.cpp) run the same functions.
// DESIGN.md §3.12 has the restatement with its sources; the comments here say which reference line
// a step is.
#pragma once
#include <cstdint>

#include "../../include/ans_capi.h"
#include "ans_arer.hpp"
#include "ans_arpu.hpp"
#include "ans_polya.hpp"

namespace shuffle_coding {
namespace wl {

constexpr uint32_t kMaxIter = ANS_WL_MAX_ITER;
constexpr uint32_t kNil = 0xFFFFFFFFu;

// hash(x) of src/recursive/prefix_orbit.rs:132-136 over the 8-byte words x feeds DefaultHasher
// (SipHash-1-3, keys 0, 0), one word a block; the final block carries the byte count mod 256.
struct Sip {
    uint64_t v0 = 0x736f6d6570736575ull, v1 = 0x646f72616e646f6dull, v2 = 0x6c7967656e657261ull,
             v3 = 0x7465646279746573ull, words = 0;
    ANS_MSET_HD static uint64_t rotl(uint64_t v, int s) { return (v << s) | (v >> (64 - s)); }
    ANS_MSET_HD void round() {
        v0 += v1, v1 = rotl(v1, 13) ^ v0, v0 = rotl(v0, 32);
        v2 += v3, v3 = rotl(v3, 16) ^ v2;
        v0 += v3, v3 = rotl(v3, 21) ^ v0;
        v2 += v1, v1 = rotl(v1, 17) ^ v2, v2 = rotl(v2, 32);
    }
    ANS_MSET_HD void block(uint64_t w) {
        v3 ^= w;
        round();
        v0 ^= w;
    }
    ANS_MSET_HD void feed(uint64_t w) {
        block(w);
        ++words;
    }
    ANS_MSET_HD uint64_t finish() {
        block((8 * words) << 56);
        v2 ^= 0xFF;
        round();
        round();
        round();
        return v0 ^ v1 ^ v2 ^ v3;
    }
};
ANS_MSET_HD inline uint64_t hash2(uint64_t a, uint64_t b) {
    Sip s;
    s.feed(a);
    s.feed(b);
    return s.finish();
}

// a u64 in two u32 entries, low first
template <class Acc>
ANS_MSET_HD uint64_t load64(const Acc& a, uint32_t i) {
    return a.load(2 * i) | (uint64_t(a.load(2 * i + 1)) << 32);
}
template <class Acc>
ANS_MSET_HD void store64(Acc& a, uint32_t i, uint64_t v) {
    a.store(2 * i, static_cast<uint32_t>(v));
    a.store(2 * i + 1, static_cast<uint32_t>(v >> 32));
}
// a[0 .. n) of u64 ascending (heapsort: in place, no recursion, O(n log n) whatever the input)
template <class Acc>
ANS_MSET_HD void sift64(Acc& a, uint32_t root, uint32_t n) {
    const uint64_t v = load64(a, root);
    for (;;) {
        uint32_t child = 2 * root + 1;
        if (child >= n) break;
        uint64_t cv = load64(a, child);
        if (child + 1 < n) {
            const uint64_t c2 = load64(a, child + 1);
            if (c2 > cv) cv = c2, ++child;
        }
        if (cv <= v) break;
        store64(a, root, cv);
        root = child;
    }
    store64(a, root, v);
}
template <class Acc>
ANS_MSET_HD void heapsort64(Acc& a, uint32_t n) {
    for (uint32_t s = n / 2; s-- > 0;) sift64(a, s, n);
    for (uint32_t end = n; end-- > 1;) {
        const uint64_t top = load64(a, 0);
        store64(a, 0, load64(a, end));
        store64(a, end, top);
        sift64(a, 0, end);
    }
}

// The orbit stage's per-graph state, u32 entries (K = wl_iter + 1 levels):
//   ids    level t of position p, a u64, at entry pair p * K + t: every position's, known or not (a
//          known node's h_1 reads its unknown neighbours' h_0)
//   ord    the known positions ascending by (id, position), ids as vectors of unsigned words: a class
//          is a run of equal ids, its first entry the class's smallest position, its start the
//          cumulative count of the classes below it;  inv[p] = where position p stands in ord
//   dirty  the positions whose ids a step recomputes, in breadth-first order;  stamp[p] = the step
//          that listed p
//   sort   the neighbour hashes of one node, sorted (u64; none at wl_iter = 0)
// Insert, remove and change of one position move the entries behind it: O(n) u32 moves each, O(log n)
// id compares to find the place; the class questions scan the run, O(class size) id compares.
// An entry's index is a u32: the id store's 2 K max_nodes entries stay below 2^32.
constexpr bool nodes_ok(uint64_t max_nodes, uint32_t wl_iter) {
    return max_nodes <= 0x7FFFFFFFu && 2 * (uint64_t(wl_iter) + 1) * max_nodes <= 0xFFFFFFFFull;
}
constexpr uint64_t orbit_entries(uint64_t max_nodes, uint32_t wl_iter) {
    return (2 * (uint64_t(wl_iter) + 1) + 4 + (wl_iter ? 2 : 0)) * max_nodes;
}
struct Class {
    uint32_t count, cum, index;  // its members, the members of the classes below, its smallest position
};
template <class Acc>
struct Orbits {
    Acc ids, ord, inv, dirty, stamp, sort;
    uint32_t K, half, n, len, m, step, ndirty;  // len known positions, m of them in ord

    template <class Take>
    ANS_MSET_HD static Orbits make(Take& take, uint64_t max_nodes, uint32_t wl_iter, bool half_iter) {
        Orbits o{take(2 * (uint64_t(wl_iter) + 1) * max_nodes),
                 take(max_nodes),
                 take(max_nodes),
                 take(max_nodes),
                 take(max_nodes),
                 take(wl_iter ? 2 * max_nodes : 0),
                 wl_iter + 1,
                 half_iter ? 1u : 0u,
                 0,
                 0,
                 0,
                 0,
                 0};
        return o;
    }
    ANS_MSET_HD uint64_t id(uint32_t p, uint32_t t) const { return load64(ids, p * K + t); }
    // (id, position) of p below that of q
    ANS_MSET_HD bool below(uint32_t p, uint32_t q) const {
        for (uint32_t t = 0; t < K; ++t) {
            const uint64_t a = id(p, t), b = id(q, t);
            if (a != b) return a < b;
        }
        return p < q;
    }
    ANS_MSET_HD bool same(uint32_t p, uint32_t q) const {
        for (uint32_t t = K; t-- > 0;)  // the last level differs first
            if (id(p, t) != id(q, t)) return false;
        return true;
    }

    // level t of position p from level t - 1 (incomplete.rs:49-57, 114-124): g names p's neighbours
    // in the prefix graph
    template <class G>
    ANS_MSET_HD void level(const G& g, uint32_t p, uint32_t t) {
        if (t == 0) {
            // hash((n, if i < len { None } else { Some(i) })): () feeds nothing
            uint64_t h = p < len ? arer::kH0 : hash2(1, p);
            if (half) h = hash2(h, g.degree(p, len));  // half_wl_node_iter: h, the Vec<&()>'s length
            store64(ids, p * K, h);
            return;
        }
        uint32_t deg = 0;
        g.each(p, len, [&](uint32_t q) { store64(sort, deg++, id(q, t - 1)); });
        heapsort64(sort, deg);
        Sip s;  // hash((h, Vec<(usize, &())>)): h, the length, the hashes
        s.feed(id(p, t - 1));
        s.feed(deg);
        for (uint32_t k = 0; k < deg; ++k) s.feed(load64(sort, k));
        store64(ids, p * K + t, s.finish());
    }

    ANS_MSET_HD void remove(uint32_t p) {
        for (uint32_t i = inv.load(p) + 1; i < m; ++i) {
            const uint32_t q = ord.load(i);
            ord.store(i - 1, q);
            inv.store(q, i - 1);
        }
        --m;
    }
    ANS_MSET_HD void insert(uint32_t p) {
        uint32_t lo = 0, hi = m;  // the first entry above p
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (below(ord.load(mid), p)) lo = mid + 1;
            else hi = mid;
        }
        for (uint32_t i = m; i > lo; --i) {
            const uint32_t q = ord.load(i - 1);
            ord.store(i, q);
            inv.store(q, i);
        }
        ord.store(lo, p);
        inv.store(p, lo);
        ++m;
    }
    // the class the entry at `at` of ord stands in
    ANS_MSET_HD Class class_at(uint32_t at) const {
        const uint32_t p = ord.load(at);
        uint32_t lo = at, hi = at + 1;
        while (lo > 0 && same(ord.load(lo - 1), p)) --lo;
        while (hi < m && same(ord.load(hi), p)) ++hi;
        return Class{hi - lo, lo, ord.load(lo)};
    }
    ANS_MSET_HD Class class_of(uint32_t p) const { return class_at(inv.load(p)); }

    // WLOrbitCodecs::apply (incomplete.rs:193-210) of a prefix of `known` positions out of `nodes`:
    // every id afresh, level by level
    template <class G>
    ANS_MSET_HD void apply(const G& g, uint32_t nodes, uint32_t known) {
        n = nodes;
        len = known;
        m = 0;
        step = 0;
        ndirty = 0;
        for (uint32_t t = 0; t < K; ++t)
            for (uint32_t p = 0; p < n; ++p) level(g, p, t);
        for (uint32_t p = 0; p < n; ++p) stamp.store(p, 0);
        for (uint32_t p = 0; p < len; ++p) insert(p);
    }

    // update_around (incomplete.rs:97-151): touch() the indices, then around()
    ANS_MSET_HD void begin() {
        ++step;
        ndirty = 0;
    }
    ANS_MSET_HD void touch(uint32_t p) {
        if (stamp.load(p) == step) return;
        stamp.store(p, step);
        dirty.store(ndirty++, p);
        if (p < len) remove(p);
    }
    template <class G>
    ANS_MSET_HD void around(const G& g) {
        for (uint32_t k = 0; k < ndirty; ++k) level(g, dirty.load(k), 0);
        uint32_t from = 0;
        for (uint32_t t = 1; t < K; ++t) {
            // the positions at distance t (:103-111), then level t of everything within it (:127-145:
            // level t reads level t - 1 alone, which is final by now, so the ids are written in place)
            const uint32_t to = ndirty;
            for (uint32_t k = from; k < to; ++k) g.each(dirty.load(k), len, [&](uint32_t q) { touch(q); });
            from = to;
            for (uint32_t k = 0; k < ndirty; ++k) level(g, dirty.load(k), t);
        }
        for (uint32_t k = 0; k < ndirty; ++k) {
            const uint32_t p = dirty.load(k);
            if (p < len) insert(p);
        }
    }

    // push, one step (recursive/mod.rs:123-127): the class of cumulative frequency cf < len
    ANS_MSET_HD Class find(uint64_t cf) const { return class_at(static_cast<uint32_t>(cf)); }
    // ... the orbits' swap (prefix_orbit.rs:23-39) of the known positions index and last = len - 1,
    // then pop_id (:59-70): position last leaves with the class's id, index keeps last's
    ANS_MSET_HD void swap_and_pop(uint32_t index) {
        const uint32_t last = len - 1;
        remove(last);
        if (index != last) {
            remove(index);
            for (uint32_t t = 0; t < K; ++t) store64(ids, index * K + t, id(last, t));
            insert(index);
        }
        len = last;
    }
};

// ---- the prefix graph as the stage reads it
// On push: the CSR in input labels and the positions; a neighbour counts unless both ends are unknown
// (pop_slice took those edges out, graph/mod.rs:57-66).
template <class Acc>
struct PushAdj {
    const Acc &pos_of, &node_at, &off, &nbr;
    template <class F>
    ANS_MSET_HD void each(uint32_t p, uint32_t len, F&& f) const {
        const uint32_t u = node_at.load(p);
        for (uint32_t a = off.load(u), end = off.load(u + 1); a < end; ++a) {
            const uint32_t q = pos_of.load(nbr.load(a));
            if (p < len || q < len) f(q);
        }
    }
    ANS_MSET_HD uint32_t degree(uint32_t p, uint32_t len) const {
        const uint32_t u = node_at.load(p);
        if (p < len) return off.load(u + 1) - off.load(u);
        uint32_t d = 0;
        each(p, len, [&](uint32_t) { ++d; });
        return d;
    }
};
// On pop: a list per position over the decoded pairs.  Pair k's ends are the half-edges 2k (out[2k],
// whose neighbour is out[2k + 1]) and 2k + 1; a loop has the first alone.  Every decoded pair has a
// known end.
template <class Acc>
struct PopAdj {
    Acc head, next, deg;  // max_nodes, 2 * max_edges, max_nodes
    const uint32_t* out;
    ANS_MSET_HD void clear(uint32_t n) {
        for (uint32_t v = 0; v < n; ++v) {
            head.store(v, kNil);
            deg.store(v, 0);
        }
    }
    ANS_MSET_HD void link(uint32_t v, uint32_t half_edge) {
        next.store(half_edge, head.load(v));
        head.store(v, half_edge);
        deg.store(v, deg.load(v) + 1);
    }
    ANS_MSET_HD void add(uint32_t k) {  // pair k is in out
        const uint32_t v = out[2 * uint64_t(k)], w = out[2 * uint64_t(k) + 1];
        link(v, 2 * k);
        if (w != v) link(w, 2 * k + 1);
    }
    template <class F>
    ANS_MSET_HD void each(uint32_t p, uint32_t, F&& f) const {
        for (uint32_t e = head.load(p); e != kNil; e = next.load(e)) f(out[e ^ 1u]);
    }
    ANS_MSET_HD uint32_t degree(uint32_t p, uint32_t) const { return deg.load(p); }
};

// The pairs into a CSR in input labels (as arer::push_graph builds it), the alphabet and a pair given
// twice checked (mark: n entries of scratch).
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
            if (mark.load(w) == v + 1) return ANS_E_SYMBOL;  // Graph::new's insert asserts
            mark.store(w, v + 1);
        }
    return ANS_OK;
}

// One orbit step of a push (recursive/mod.rs:123-127): the blanket pop under norm L, the class's
// smallest position, x.swap(index, last) (graph.rs:304-331) and the orbits' swap and pop_id.
template <class M, class St>
ANS_MSET_HD int push_orbit(polya::Coder<M>& c, St& st, uint32_t L) {
    uint64_t q = 0, cf = 0;
    if (!c.pop_begin(L, q, cf)) return c.err;
    const Class f = st.orb.find(cf);
    c.pop_end(f.count, q, cf - f.cum);
    const uint32_t last = L - 1, a = st.node_at.load(f.index), z = st.node_at.load(last);
    st.node_at.store(f.index, z);
    st.node_at.store(last, a);
    st.pos_of.store(z, f.index);
    st.pos_of.store(a, last);
    st.orb.swap_and_pop(f.index);
    return ANS_OK;
}
// ... and of a pop (recursive/mod.rs:143-145) once update_around has run: push_element
template <class M, class St>
ANS_MSET_HD int pop_orbit(polya::Coder<M>& c, St& st, uint32_t v) {
    const Class f = st.orb.class_of(v);
    c.push(f.count, uint64_t(v) + 1, f.cum);
    return c.err;
}

// ================================================================ the Erdős–Rényi slices
//   pos_of, node_at, off, nbr   as arer::PushState has them;  mark the slice's stamps
constexpr uint64_t er_push_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter) {
    return 4 * max_nodes + 1 + 2 * max_edges + orbit_entries(max_nodes, wl_iter);
}
template <class Acc>
struct ErPush {
    Acc pos_of, node_at, off, nbr, mark;
    Orbits<Acc> orb;
    template <class Ws>
    ANS_MSET_HD static ErPush make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        uint64_t o = 0;
        auto take = [&](uint64_t n) {
            const uint64_t at = o;
            o += n;
            return ws.at(at, n);
        };
        ErPush s{take(max_nodes), take(max_nodes), take(max_nodes + 1), take(2 * max_edges), take(max_nodes),
                 Orbits<Acc>::make(take, max_nodes, wl_iter, half_iter)};
        return s;
    }
};
// ... of a pop: the decoded prefix's adjacency (head, next, deg), sized by max_edges
constexpr uint64_t er_pop_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter) {
    return 2 * max_nodes + 2 * max_edges + orbit_entries(max_nodes, wl_iter);
}
template <class Acc>
struct ErPop {
    PopAdj<Acc> adj;
    Orbits<Acc> orb;
    template <class Ws>
    ANS_MSET_HD static ErPop make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        uint64_t o = 0;
        auto take = [&](uint64_t n) {
            const uint64_t at = o;
            o += n;
            return ws.at(at, n);
        };
        ErPop s{{take(max_nodes), take(2 * max_edges), take(max_nodes), nullptr},
                Orbits<Acc>::make(take, max_nodes, wl_iter, half_iter)};
        return s;
    }
};

// ---- push, as arer::push_graph with the orbit stage replaced.  perm: null, or n entries out.
template <class M, class Acc>
ANS_MSET_HD int er_push_graph(polya::Coder<M>& c, ErPush<Acc>& st, const arer::Bern& b, uint32_t n, bool loops,
                              const uint32_t* e, uint32_t E, uint32_t* perm) {
    if (const int rc = build_csr(st.off, st.nbr, st.mark, n, loops, e, E)) return rc;
    // Prefix::from_full: position p holds input node p, every node known (graph/mod.rs:97-99)
    for (uint32_t v = 0; v < n; ++v) {
        st.pos_of.store(v, v);
        st.node_at.store(v, v);
        st.mark.store(v, 0);
    }
    const PushAdj<Acc> g{st.pos_of, st.node_at, st.off, st.nbr};
    st.orb.apply(g, n, n);
    for (uint32_t L = n; L > 0; --L) {
        const uint32_t last = L - 1;
        if (const int rc = push_orbit(c, st, L)) return rc;
        // pop_slice (graph/mod.rs:57-66), then update_after_pop_slice (incomplete.rs:212-221, 87-95)
        st.orb.begin();
        const uint32_t u = st.node_at.load(last);
        for (uint32_t a = st.off.load(u), end = st.off.load(u + 1); a < end; ++a) {
            const uint32_t p = st.pos_of.load(st.nbr.load(a));
            if (p >= last) {
                st.mark.store(p, L);
                st.orb.touch(p);
            }
        }
        st.orb.touch(last);
        st.orb.around(g);
        // IID<Bernoulli>::push over (L-1, L) .. (L-1, n-1), then the loop: last entry first
        if (loops) arer::push_bit(c, b, st.mark.load(last) == L);
        for (uint32_t j = n; j-- > L;) arer::push_bit(c, b, st.mark.load(j) == L);
        if (c.err) return c.err;
    }
    if (perm)
        for (uint32_t p = 0; p < n; ++p) perm[p] = st.node_at.load(p);
    return ANS_OK;
}

// ---- pop.  out receives the pairs in pop order, at most cap of them (ANS_E_LEN beyond; cap is
// at most the max_edges of the state); *count their number.
template <class M, class Acc>
ANS_MSET_HD int er_pop_graph(polya::Coder<M>& c, ErPop<Acc>& st, const arer::Bern& b, uint32_t n, bool loops,
                             uint32_t* out, uint64_t cap, uint64_t* count) {
    uint64_t E = 0;
    *count = 0;
    st.adj.out = out;
    st.adj.clear(n);
    st.orb.apply(st.adj, n, 0);
    for (uint32_t v = 0; v < n; ++v) {
        st.orb.begin();
        for (uint32_t j = v + 1; j < n + (loops ? 1u : 0u); ++j) {
            const uint32_t w = j < n ? j : v;  // the loop comes last
            const uint32_t x = arer::pop_bit(c, b);
            if (c.err) return c.err;
            if (!x) continue;
            if (E >= cap) return ANS_E_LEN;
            out[2 * E] = v;
            out[2 * E + 1] = w;
            st.adj.add(static_cast<uint32_t>(E));
            ++E;
            st.orb.touch(w);
        }
        // push_id, update_around_slice, push_element (recursive/mod.rs:143-145)
        st.orb.touch(v);
        st.orb.len = v + 1;
        st.orb.around(st.adj);
        if (const int rc = pop_orbit(c, st, v)) return rc;
    }
    *count = E;
    return ANS_OK;
}

// ================================================================ the Pólya urn slices
//   pos_of, node_at, off, nbr, urn, s, total   as arpu::PushState has them
constexpr uint64_t pu_push_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter) {
    return 4 * max_nodes + 1 + 2 * max_edges + arpu::slice_entries(max_nodes) + orbit_entries(max_nodes, wl_iter);
}
template <class Acc>
struct PuPush {
    Acc pos_of, node_at, off, nbr;
    mset::Counts<Acc> urn;
    arpu::Slice<Acc> s;
    uint64_t total;
    Orbits<Acc> orb;
    template <class Ws>
    ANS_MSET_HD static PuPush make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        uint64_t o = 0;
        auto take = [&](uint64_t n) {
            const uint64_t at = o;
            o += n;
            return ws.at(at, n);
        };
        PuPush st{take(max_nodes),
                  take(max_nodes),
                  take(max_nodes + 1),
                  take(2 * max_edges),
                  {take(max_nodes), 0},
                  {take(max_nodes), take(max_nodes), take(max_nodes), take(max_nodes), take(2 * max_nodes),
                   {take(max_nodes), 0}},
                  0,
                  Orbits<Acc>::make(take, max_nodes, wl_iter, half_iter)};
        return st;
    }
};
constexpr uint64_t pu_pop_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter) {
    return 3 * max_nodes + 2 * max_edges + arpu::slice_entries(max_nodes) - max_nodes + arpu::pop_por_entries(max_nodes) +
           orbit_entries(max_nodes, wl_iter);
}
template <class Acc>
struct PuPop {
    PopAdj<Acc> adj;
    mset::Counts<Acc> urn;
    arpu::Slice<Acc> s;
    uint64_t total;
    Orbits<Acc> orb;
    template <class Ws>
    ANS_MSET_HD static PuPop make(const Ws& ws, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        uint64_t o = 0;
        auto take = [&](uint64_t n) {
            const uint64_t at = o;
            o += n;
            return ws.at(at, n);
        };
        PuPop st{{take(max_nodes), take(2 * max_edges), take(max_nodes), nullptr},
                 {take(max_nodes), 0},
                 {take(max_nodes), take(max_nodes), take(max_nodes), take(arpu::pop_por_entries(max_nodes)),
                  take(2 * max_nodes), {take(max_nodes), 0}},
                 0,
                 Orbits<Acc>::make(take, max_nodes, wl_iter, half_iter)};
        return st;
    }
};

// ---- push, as arpu::push_graph with the orbit stage replaced
template <class M, class Acc>
ANS_MSET_HD int pu_push_graph(polya::Coder<M>& c, PuPush<Acc>& st, uint32_t n, bool loops, const uint32_t* e, uint32_t E,
                              uint32_t* perm) {
    if (const int rc = build_csr(st.off, st.nbr, st.s.sl, n, loops, e, E)) return rc;
    // PolyaUrnSliceCodec::from_graph (slice.rs:78-86) of the full prefix: an empty urn
    st.urn.nsym = n;
    st.urn.clear();
    st.total = 0;
    for (uint32_t v = 0; v < n; ++v) {
        st.pos_of.store(v, v);
        st.node_at.store(v, v);
    }
    const PushAdj<Acc> g{st.pos_of, st.node_at, st.off, st.nbr};
    st.orb.apply(g, n, n);
    const uint32_t skip = loops ? 0u : 1u;
    for (uint32_t L = n; L > 0; --L) {
        const uint32_t last = L - 1;
        if (const int rc = push_orbit(c, st, L)) return rc;
        // pop_slice (graph/mod.rs:57-66), then update_after_pop_slice (incomplete.rs:212-221, 87-95)
        st.orb.begin();
        const uint32_t u = st.node_at.load(last);
        uint32_t len = 0;
        for (uint32_t a = st.off.load(u), end = st.off.load(u + 1); a < end; ++a) {
            const uint32_t p = st.pos_of.load(st.nbr.load(a));
            if (p >= last) {
                st.s.sl.store(len++, p);
                st.orb.touch(p);
            }
        }
        st.orb.touch(last);
        st.orb.around(g);
        // the urn's update_after_pop_slice (slice.rs:194-210), as arpu::push_graph has it
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
            arpu::urn_add(st, fresh, mass);
        }
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t j = st.s.sl.load(k);
            if (j != fresh) arpu::urn_sub(st, j, 1);
        }
        if (const int rc = arpu::push_slice(c, st, last, n - last - 1 + (loops ? 1u : 0u), len)) return rc;
    }
    if (perm)
        for (uint32_t p = 0; p < n; ++p) perm[p] = st.node_at.load(p);
    return ANS_OK;
}

// ---- pop, as arpu::pop_graph with the orbit stage replaced (cap is at most the state's max_edges)
template <class M, class Acc>
ANS_MSET_HD int pu_pop_graph(polya::Coder<M>& c, PuPop<Acc>& st, uint32_t n, bool loops, uint32_t* out, uint64_t cap,
                             uint64_t* count) {
    uint64_t E = 0;
    *count = 0;
    const uint32_t skip = loops ? 0u : 1u;
    st.urn.nsym = n;
    for (uint32_t v = 0; v < n; ++v) st.urn.a.store(v, v >= skip ? 1 : 0);
    st.urn.build();
    st.total = n > skip ? n - skip : 0;
    st.adj.out = out;
    st.adj.clear(n);
    st.orb.apply(st.adj, n, 0);
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t len = 0;
        if (const int rc = arpu::pop_slice(c, st, v, n - v - 1 + (loops ? 1u : 0u), &len)) return rc;
        if (len > cap - E) return ANS_E_LEN;
        st.orb.begin();
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t w = st.s.sl.load(k);
            out[2 * E] = v;
            out[2 * E + 1] = w;
            st.adj.add(static_cast<uint32_t>(E));
            ++E;
            arpu::urn_add(st, w, 1);
            st.orb.touch(w);
        }
        if (v + skip < n) arpu::urn_sub(st, v + skip, st.urn.count(v + skip));
        st.orb.touch(v);
        st.orb.len = v + 1;
        st.orb.around(st.adj);
        if (const int rc = pop_orbit(c, st, v)) return rc;
    }
    *count = E;
    return ANS_OK;
}

}  // namespace wl
}  // namespace shuffle_coding
