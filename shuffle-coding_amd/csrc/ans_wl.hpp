// ans_wl.hpp — the orbit stage of recursive shuffle coding on graphs at any wl_iter: the
// Weisfeiler-Lehman ids of WLOrbitCodecs<GraphPrefix> (src/recursive/graph/incomplete.rs:45-57,
// 87-151, 189-236) and the PrefixOrbitCodec over them (src/recursive/prefix_orbit.rs), as a stage of
// the recursion of ans_rgraph.hpp under the autoregressive Erdős–Rényi slices of ans_arer.hpp and the
// Pólya urn slices of ans_arpu.hpp, one graph on one message.  Plain C++ templated on the message and
// on how a per-graph array is read and written, host and device alike, so that the host codec
// (ans_capi.cpp), the kernels (ans_wl.hip, ans_wl_labelled.hip) and the CPU tests (g++,
// tests/native/wl_state_check.cpp) run the same functions.  DESIGN.md §3.12 has the restatement with
// its sources, §3.13 the labels (the policy L = rgraph::Labels below); the comments here say which
// reference line a step is.
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
// ... and of (hash, label) keys, three entries each, ordered as the tuple (usize, &usize) is.  (Its
// own loops, not a parameter of the two above: a key of one word keeps the code it had.)
struct Key {
    uint64_t h;
    uint32_t l;
    ANS_MSET_HD bool operator>(const Key& k) const { return h != k.h ? h > k.h : l > k.l; }
};
template <class Acc>
ANS_MSET_HD Key load_key(const Acc& a, uint32_t i) {
    return Key{a.load(3 * i) | (uint64_t(a.load(3 * i + 1)) << 32), a.load(3 * i + 2)};
}
template <class Acc>
ANS_MSET_HD void store_key(Acc& a, uint32_t i, const Key& k) {
    a.store(3 * i, static_cast<uint32_t>(k.h));
    a.store(3 * i + 1, static_cast<uint32_t>(k.h >> 32));
    a.store(3 * i + 2, k.l);
}
template <class Acc>
ANS_MSET_HD void sift_keys(Acc& a, uint32_t root, uint32_t n) {
    const Key v = load_key(a, root);
    for (;;) {
        uint32_t child = 2 * root + 1;
        if (child >= n) break;
        Key cv = load_key(a, child);
        if (child + 1 < n) {
            const Key c2 = load_key(a, child + 1);
            if (c2 > cv) cv = c2, ++child;
        }
        if (!(cv > v)) break;
        store_key(a, root, cv);
        root = child;
    }
    store_key(a, root, v);
}
template <class Acc>
ANS_MSET_HD void heapsort_keys(Acc& a, uint32_t n) {
    for (uint32_t s = n / 2; s-- > 0;) sift_keys(a, s, n);
    for (uint32_t end = n; end-- > 1;) {
        const Key top = load_key(a, 0);
        store_key(a, 0, load_key(a, end));
        store_key(a, end, top);
        sift_keys(a, 0, end);
    }
}

// ---- the prefix graph as the stage reads it
// On push: the CSR in input labels and the positions; a neighbour counts unless both ends are unknown
// (pop_slice took those edges out, graph/mod.rs:57-66).
// With labels (L: rgraph::Labels) each() hands f the pair's label behind the neighbour, and
// node_label(p) is the label of the node at a known position; without, neither exists.
using rgraph::Labels;
using rgraph::NoLabels;
template <class Acc, class L>
struct PushAdjLabels {
    const Acc& elab;     // the label of each entry of nbr
    const uint32_t* nl;  // the label of an input node
};
template <class Acc, bool kSorted>
struct PushAdjLabels<Acc, Labels<false, false, kSorted>> {};
template <class Acc, class L = NoLabels>
struct PushAdj {
    const Acc &pos_of, &node_at, &off, &nbr;
    PushAdjLabels<Acc, L> lab;
    template <class F>
    ANS_MSET_HD void each(uint32_t p, uint32_t len, F&& f) const {
        const uint32_t u = node_at.load(p);
        for (uint32_t a = off.load(u), end = off.load(u + 1); a < end; ++a) {
            const uint32_t q = pos_of.load(nbr.load(a));
            if (p < len || q < len) {
                if constexpr (L::edge) f(q, lab.elab.load(a));
                else f(q);
            }
        }
    }
    ANS_MSET_HD uint32_t degree(uint32_t p, uint32_t len) const {
        const uint32_t u = node_at.load(p);
        if (p < len) return off.load(u + 1) - off.load(u);
        uint32_t d = 0;
        each(p, len, [&](uint32_t, auto...) { ++d; });
        return d;
    }
    ANS_MSET_HD uint32_t node_label(uint32_t p) const { return lab.nl[node_at.load(p)]; }
};
// On pop: a list per position over the decoded pairs.  Pair k's ends are the half-edges 2k (out[2k],
// whose neighbour is out[2k + 1]) and 2k + 1; a loop has the first alone.  Every decoded pair has a
// known end.
// The labels are the output arrays': nl[p] of position p, el[k] of pair k.
template <class L>
struct PopAdjLabels {
    const uint32_t *nl, *el;
};
template <bool kSorted>
struct PopAdjLabels<Labels<false, false, kSorted>> {};
template <class Acc, class L = NoLabels>
struct PopAdj {
    Acc head, next, deg;  // max_nodes, 2 * max_edges, max_nodes
    const uint32_t* out;
    PopAdjLabels<L> lab;
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
        for (uint32_t e = head.load(p); e != kNil; e = next.load(e)) {
            if constexpr (L::edge) f(out[e ^ 1u], lab.el[e >> 1]);
            else f(out[e ^ 1u]);
        }
    }
    ANS_MSET_HD uint32_t degree(uint32_t p, uint32_t) const { return deg.load(p); }
    ANS_MSET_HD uint32_t node_label(uint32_t p) const { return lab.nl[p]; }
};

// The orbit stage's per-graph state, u32 entries (K = wl_iter + 1 levels):
//   ids    level t of position p, a u64, at entry pair p * K + t: every position's, known or not (a
//          known node's h_1 reads its unknown neighbours' h_0)
//   ord    the known positions ascending by (id, position), ids as vectors of unsigned words: a class
//          is a run of equal ids, its first entry the class's smallest position, its start the
//          cumulative count of the classes below it;  inv[p] = where position p stands in ord
//   dirty  the positions whose ids a step recomputes, in breadth-first order;  stamp[p] = the step
//          that listed p
//   sort   the neighbour hashes of one node, sorted (u64; none at wl_iter = 0); with edge labels
//          the (hash, label) keys, three entries each, and at wl_iter = 0 the labels the half
//          iteration sorts, as u64
// Insert, remove and change of one position move the entries behind it: O(n) u32 moves each, O(log n)
// id compares to find the place; the class questions scan the run, O(class size) id compares.
// An entry's index is a u32: the id store's 2 K max_nodes entries stay below 2^32.
constexpr bool nodes_ok(uint64_t max_nodes, uint32_t wl_iter) {
    return max_nodes <= 0x7FFFFFFFu && 2 * (uint64_t(wl_iter) + 1) * max_nodes <= 0xFFFFFFFFull;
}
constexpr uint64_t sort_entries(uint64_t max_nodes, uint32_t wl_iter, bool edge_labels) {
    return (wl_iter ? (edge_labels ? 3 : 2) : (edge_labels ? 2 : 0)) * max_nodes;
}
constexpr uint64_t orbit_entries(uint64_t max_nodes, uint32_t wl_iter, bool edge_labels = false) {
    return (2 * (uint64_t(wl_iter) + 1) + 4) * max_nodes + sort_entries(max_nodes, wl_iter, edge_labels);
}
struct Class {
    uint32_t count, cum, index;  // its members, the members of the classes below, its smallest position
};
template <class Acc, class L = NoLabels>
struct Orbits {
    Acc ids, ord, inv, dirty, stamp, sort;
    uint32_t K, half, n, len, m, step, ndirty;  // len known positions, m of them in ord

    template <class Take>
    ANS_MSET_HD static Orbits make(Take& take, uint64_t max_nodes, uint64_t, uint32_t wl_iter, bool half_iter) {
        Orbits o{take(2 * (uint64_t(wl_iter) + 1) * max_nodes),
                 take(max_nodes),
                 take(max_nodes),
                 take(max_nodes),
                 take(max_nodes),
                 take(sort_entries(max_nodes, wl_iter, L::edge)),
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
        if constexpr (L::any) {
            labelled_level(g, p, t);
        } else {
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
    }
    // ... of a graph with labels: a usize label feeds a word where () feeds nothing.  Level 0 hashes
    // the node's label (an unknown position's is the default, 0: pop_slice took it out) before the
    // Option; the half iteration the sorted Vec<&usize> of the pairs' labels behind its length; a
    // level above the (hash, label) pairs sorted as tuples, two words each.
    template <class G>
    ANS_MSET_HD void labelled_level(const G& g, uint32_t p, uint32_t t) {
        if (t == 0) {
            uint64_t h = 0;
            if constexpr (L::node) {
                Sip s;
                s.feed(p < len ? g.node_label(p) : 0);
                s.feed(p < len ? 0 : 1);
                if (p >= len) s.feed(p);
                h = s.finish();
            } else {
                h = p < len ? arer::kH0 : hash2(1, p);
            }
            if (half) {
                if constexpr (L::edge) {
                    uint32_t deg = 0;
                    g.each(p, len, [&](uint32_t, uint32_t label) { store64(sort, deg++, label); });
                    heapsort64(sort, deg);
                    Sip s;
                    s.feed(h);
                    s.feed(deg);
                    for (uint32_t k = 0; k < deg; ++k) s.feed(load64(sort, k));
                    h = s.finish();
                } else {
                    h = hash2(h, g.degree(p, len));
                }
            }
            store64(ids, p * K, h);
            return;
        }
        uint32_t deg = 0;
        Sip s;
        if constexpr (L::edge) {
            g.each(p, len, [&](uint32_t q, uint32_t label) { store_key(sort, deg++, Key{id(q, t - 1), label}); });
            heapsort_keys(sort, deg);
        } else {
            g.each(p, len, [&](uint32_t q) { store64(sort, deg++, id(q, t - 1)); });
            heapsort64(sort, deg);
        }
        s.feed(id(p, t - 1));
        s.feed(deg);
        for (uint32_t k = 0; k < deg; ++k) {
            if constexpr (L::edge) {
                const Key key = load_key(sort, k);
                s.feed(key.h);
                s.feed(key.l);
            } else {
                s.feed(load64(sort, k));
            }
        }
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

    // update_around (incomplete.rs:97-151): touch() the indices, then around(); begin() opens the
    // next update (apply and around leave none open)
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
            for (uint32_t k = from; k < to; ++k) g.each(dirty.load(k), len, [&](uint32_t q, auto...) { touch(q); });
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
    // ---- what the recursion of ans_rgraph.hpp asks of an orbit stage on a push (g: its PushGraph)
    template <class G>
    ANS_MSET_HD static PushAdj<Acc, L> adj_of(const G& g) {
        if constexpr (L::any) return PushAdj<Acc, L>{g.pos_of, g.node_at, g.off, g.nbr, {g.lab.elab, g.lab.nl}};
        else return PushAdj<Acc, L>{g.pos_of, g.node_at, g.off, g.nbr, {}};
    }
    ANS_MSET_HD bool coded() const { return true; }
    template <class G>
    ANS_MSET_HD void apply_full(const G& g, uint32_t nodes) {
        apply(adj_of(g), nodes, nodes);
        begin();
    }
    // the blanket pop under norm `known` and the class's smallest position (recursive/mod.rs:123-127)
    template <class M>
    ANS_MSET_HD int pop_element(polya::Coder<M>& c, uint32_t known, uint32_t& index, uint32_t&) {
        uint64_t q = 0, cf = 0;
        if (!c.pop_begin(known, q, cf)) return c.err;
        const Class f = find(cf);
        c.pop_end(f.count, q, cf - f.cum);
        index = f.index;
        return ANS_OK;
    }
    ANS_MSET_HD void pop_id(uint32_t index, uint32_t, uint32_t) { swap_and_pop(index); }
    // update_after_pop_slice (incomplete.rs:212-221, 87-95): the slice's positions are touched by now
    template <class G>
    ANS_MSET_HD void after_pop_slice(const G& g, uint32_t last) {
        touch(last);
        around(adj_of(g));
        begin();
    }
};

// The stage of a pop: the decoded prefix's adjacency and the ids over it.  cap is at most the
// max_edges of the state.
template <class Acc, class L = NoLabels>
struct PopOrbits {
    PopAdj<Acc, L> adj;
    Orbits<Acc, L> orb;
    template <class Take>
    ANS_MSET_HD static PopOrbits make(Take& take, uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool half_iter) {
        PopOrbits o{{take(max_nodes), take(2 * max_edges), take(max_nodes), nullptr, {}},
                    Orbits<Acc, L>::make(take, max_nodes, max_edges, wl_iter, half_iter)};
        return o;
    }
    ANS_MSET_HD void start_pop(uint32_t n, const uint32_t* out, const uint32_t* nl, const uint32_t* el) {
        adj.lab = PopAdjLabels<L>{nl, el};
        start_pop(n, out);
    }
    ANS_MSET_HD void start_pop(uint32_t n, const uint32_t* out) {
        adj.out = out;
        adj.clear(n);
        orb.apply(adj, n, 0);
        orb.begin();
    }
    ANS_MSET_HD void add_pair(uint32_t, uint32_t w, uint32_t k) {  // pair k is in out
        adj.add(k);
        orb.touch(w);
    }
    // push_id, update_around_slice, push_element (recursive/mod.rs:143-145)
    template <class M>
    ANS_MSET_HD int push_element(polya::Coder<M>& c, uint32_t v, uint32_t) {
        orb.touch(v);
        orb.len = v + 1;
        orb.around(adj);
        const Class f = orb.class_of(v);
        c.push(f.count, uint64_t(v) + 1, f.cum);
        orb.begin();
        return c.err;
    }
};
constexpr uint64_t pop_adj_entries(uint64_t max_nodes, uint64_t max_edges) { return 2 * max_nodes + 2 * max_edges; }

using rgraph::build_csr;

// ---- the per-graph states (ans_rgraph.hpp lays them out: on a push the prefix graph, the slice
// model's arrays, the ids; on a pop the slice model's arrays, the decoded adjacency, the ids)
// Edge labels add to a push the label of each CSR entry and the slice's two arrays
// (rgraph::push_label_entries: 2 max_edges + 2 max_nodes), and to both a wider sort scratch
// (sort_entries: max_nodes more at wl_iter >= 1, 2 max_nodes at wl_iter = 0); node labels add nothing.
constexpr uint64_t er_push_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool edge_labels = false) {
    return rgraph::graph_entries(max_nodes, max_edges) + max_nodes + orbit_entries(max_nodes, wl_iter, edge_labels) +
           rgraph::push_label_entries(max_nodes, max_edges, edge_labels);
}
constexpr uint64_t er_pop_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool edge_labels = false) {
    return pop_adj_entries(max_nodes, max_edges) + orbit_entries(max_nodes, wl_iter, edge_labels);
}
constexpr uint64_t pu_push_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool edge_labels = false) {
    return rgraph::graph_entries(max_nodes, max_edges) + arpu::model_entries(max_nodes, true) +
           orbit_entries(max_nodes, wl_iter, edge_labels) + rgraph::push_label_entries(max_nodes, max_edges, edge_labels);
}
constexpr uint64_t pu_pop_entries(uint64_t max_nodes, uint64_t max_edges, uint32_t wl_iter, bool edge_labels = false) {
    return arpu::model_entries(max_nodes, false) + pop_adj_entries(max_nodes, max_edges) +
           orbit_entries(max_nodes, wl_iter, edge_labels);
}
template <class Acc, class L = NoLabels>
using ErPush = rgraph::PushState<Acc, arer::ErSlices<Acc>, Orbits<Acc, L>, L>;
template <class Acc, class L = NoLabels>
using ErPop = rgraph::PopState<Acc, arer::ErSlices<Acc>, PopOrbits<Acc, L>, L>;
template <class Acc, class L = NoLabels>
using PuPush = rgraph::PushState<Acc, arpu::PuSlices<Acc>, Orbits<Acc, L>, L>;
template <class Acc, class L = NoLabels>
using PuPop = rgraph::PopState<Acc, arpu::PuSlices<Acc>, PopOrbits<Acc, L>, L>;

}  // namespace wl
}  // namespace shuffle_coding
