// ans_arpu.hpp — undirected, unlabelled graphs under the autoregressive Pólya urn model, as a
// labelled graph (Autoregressive(PolyaUrnSliceCodecs), src/recursive/mod.rs:190-216,
// src/recursive/graph/slice.rs:61-230; the harness's ord_AP) or up to the order of its nodes
// (ShuffleCodec<PolyaUrnSliceCodecs, WLOrbitCodecs<GraphPrefix>> with wl_iter = 0,
// src/recursive/mod.rs:117-148, src/recursive/graph/incomplete.rs:189-236; wl0r_AP / wl0-r_AP), one
// graph on one message.  Plain C++ templated on the message and on how a per-graph array is read
// and written, host and device alike, so that the host codec (ans_capi.cpp), the kernels
// (ans_arpu.hip) and the CPU tests (g++, tests/native/arpu_state_check.cpp) run the same functions.
// The recursion is ans_rgraph.hpp's and the orbit stage ans_arer.hpp's (neither depends on the
// slice model); this header has the slice model (PuSlices); the outer layers of a slice's multiset
// codec are ans_polya.hpp's.  DESIGN.md §3.11 has the restatement with its sources; the comments
// here say which reference line a step is.
#pragma once
#include <cstdint>

#include "../../include/ans_capi.h"
#include "ans_arer.hpp"
#include "ans_polya.hpp"

namespace shuffle_coding {
namespace arpu {

constexpr uint64_t kMaxEdges = rgraph::kMaxEdges;

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

// ---- the slice model (PolyaUrnSliceCodecs, slice.rs:61-230):
//   urn   the urn of the unknown positions, a Fenwick tree over the positions 0 .. n-1 in ascending
//         order (a position outside the urn has mass 0), total its norm
//   s     the slice scratch; before the first step of a push s.sl holds the stamps that find a pair
//         given twice.  The joint layer's pop does not read por, so on a pop it holds a plain
//         slice's entries.
constexpr uint64_t pop_por_entries(uint64_t max_nodes) { return max_nodes < polya::kPlainMax ? max_nodes : polya::kPlainMax; }
constexpr uint64_t model_entries(uint64_t max_nodes, bool push) {
    return max_nodes + slice_entries(max_nodes) - (push ? 0 : max_nodes - pop_por_entries(max_nodes));
}
template <class Acc>
struct PuSlices {
    mset::Counts<Acc> urn;
    Slice<Acc> s;
    uint64_t total;
    template <class T>
    ANS_MSET_HD static PuSlices make(T& take, uint64_t max_nodes, bool push) {
        PuSlices m{{take(max_nodes), 0},
                   {take(max_nodes), take(max_nodes), take(max_nodes), take(push ? max_nodes : pop_por_entries(max_nodes)),
                    take(2 * max_nodes), {take(max_nodes), 0}},
                   0};
        return m;
    }
    ANS_MSET_HD void add(uint32_t j, uint32_t mass) {
        urn.add(j, static_cast<int32_t>(mass));
        total += mass;
    }
    ANS_MSET_HD void sub(uint32_t j, uint32_t mass) {
        urn.add(j, -static_cast<int32_t>(mass));
        total -= mass;
    }

    // PolyaUrnSliceCodec::push (slice.rs:102-108) of the slice s.sl[0 .. len) of position v.  The urn
    // ends as it began.
    template <class M>
    ANS_MSET_HD int push_slice(polya::Coder<M>& c, uint32_t v, uint32_t alphabet, uint32_t len) {
        if (len > 0) {
            // multiset_shuffle_codec (src/recursive/multiset.rs:126-136): the order the ordered codec sees
            const bool joint = len > polya::kPlainMax;
            if (const int rc = rank_slice(s, v, len, joint)) return rc;
            if (const int rc = polya::shuffle_push(c, s, len, joint)) return rc;
            // PolyaUrnSliceEdgeIndicesCodec::push (slice.rs:140-152): every element leaves the urn, then,
            // last first, each comes back and is pushed under the urn as it then stands
            for (uint32_t p = 0; p < len; ++p) {
                const uint32_t j = s.sl.load(s.rop.load(p)), mass = urn.count(j);
                s.orb.a.store(p, mass);
                sub(j, mass);
            }
            for (uint32_t p = len; p-- > 0;) {
                const uint32_t j = s.sl.load(s.rop.load(p)), mass = s.orb.a.load(p);
                add(j, mass);
                if (mass == 0 && !c.err) c.err = ANS_E_ZERO_MASS;  // src/ans.rs:98 (not reached from a valid slice)
                else c.push(mass, total, urn.prefix(j));
            }
            if (c.err) return c.err;
        }
        push_len(c, alphabet, len);
        return c.err;
    }
    // PolyaUrnSliceCodec::pop (slice.rs:110-117): the slice's positions ascending in s.sl[0 .. *len)
    // (EdgesIID::pop sorts, src/graph_codec.rs:67-72).  A length above the alphabet's is ANS_E_SYMBOL
    // before any urn step (bytes no push wrote; the reference panics in the urn).
    template <class M>
    ANS_MSET_HD int pop_slice(polya::Coder<M>& c, uint32_t v, uint32_t alphabet, uint32_t* len_out) {
        *len_out = 0;
        const uint64_t len64 = pop_len(c, alphabet);
        if (c.err) return c.err;
        if (len64 > alphabet) return ANS_E_SYMBOL;
        const uint32_t len = static_cast<uint32_t>(len64);
        if (len == 0) return ANS_OK;
        // PolyaUrnSliceEdgeIndicesCodec::pop (slice.rs:154-170): sampling without replacement
        for (uint32_t p = 0; p < len; ++p) {
            uint64_t q = 0, cf = 0;
            if (total == 0) return ANS_E_ZERO_MASS;  // (not reached: len <= the urn's positions)
            if (!c.pop_begin(total, q, cf)) return c.err;
            const mset::Found f = urn.find(cf);
            c.pop_end(f.count, q, cf - f.cum);
            s.sl.store(p, f.rank);
            s.orb.a.store(p, f.count);
            sub(f.rank, f.count);
        }
        for (uint32_t p = 0; p < len; ++p) add(s.sl.load(p), s.orb.a.load(p));
        const bool joint = len > polya::kPlainMax;
        if (const int rc = rank_slice(s, v, len, joint)) return rc;
        if (const int rc = polya::shuffle_pop(c, s, len, joint)) return rc;
        polya::heapsort(s.sl, len, [](uint32_t a, uint32_t b) { return a < b; });
        *len_out = len;
        return ANS_OK;
    }

    // ---- what the recursion of ans_rgraph.hpp asks of a slice model
    ANS_MSET_HD Acc& scratch() { return s.sl; }
    // PolyaUrnSliceCodec::from_graph (slice.rs:78-86) of the full prefix: an empty urn
    ANS_MSET_HD void start_push(uint32_t n) {
        urn.nsym = n;
        urn.clear();
        total = 0;
    }
    ANS_MSET_HD void gather(uint32_t k, uint32_t p, uint32_t) { s.sl.store(k, p); }
    // update_after_pop_slice (slice.rs:194-210): position last + !loops enters with 1 + its degree in
    // the prefix graph as it now stands (its edges to the positions below last), every other position
    // of the slice loses the edge that left (the urn holds unknown positions only and is invariant to
    // the orbits' swap, slice.rs:223); then EdgesIID::push (src/graph_codec.rs:61-65; the labels are
    // units)
    template <class M, class G>
    ANS_MSET_HD int push(polya::Coder<M>& c, const G& g, uint32_t n, bool loops, uint32_t last, uint32_t len) {
        const uint32_t fresh = last + (loops ? 0u : 1u);
        if (fresh < n) {
            uint32_t mass = 1;
            if (loops) mass += g.degree(g.node_at.load(last)) - len;
            else
                g.each(g.node_at.load(fresh), [&](uint32_t p) {
                    if (p < last) ++mass;
                });
            add(fresh, mass);
        }
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t j = s.sl.load(k);
            if (j != fresh) sub(j, 1);
        }
        return push_slice(c, last, n - last - 1 + (loops ? 1u : 0u), len);
    }
    // from_graph of the empty prefix (slice.rs:78-86): all ones over [!loops, n)
    ANS_MSET_HD void start_pop(uint32_t n, bool loops) {
        const uint32_t skip = loops ? 0u : 1u;
        urn.nsym = n;
        for (uint32_t v = 0; v < n; ++v) urn.a.store(v, v >= skip ? 1 : 0);
        urn.build();
        total = n > skip ? n - skip : 0;
    }
    // the slice of v, the other end ascending (the loop first); update_after_push_slice (slice.rs:212-221)
    template <class M, class F>
    ANS_MSET_HD int pop(polya::Coder<M>& c, uint32_t n, bool loops, uint32_t v, uint64_t room, uint32_t& len, F&& emit) {
        if (const int rc = pop_slice(c, v, n - v - 1 + (loops ? 1u : 0u), &len)) return rc;
        if (len > room) return ANS_E_LEN;
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t w = s.sl.load(k);
            emit(w);
            add(w, 1);
        }
        const uint32_t gone = v + (loops ? 0u : 1u);
        if (gone < n) sub(gone, urn.count(gone));
        return ANS_OK;
    }
};

// The per-graph states (ans_rgraph.hpp lays them out: the prefix graph, the urn and the slice scratch,
// the counts of arer::CountPush / CountPop); a pop holds nothing sized by the edges.
constexpr uint64_t push_entries(uint64_t max_nodes, uint64_t max_edges) {
    return rgraph::graph_entries(max_nodes, max_edges) + model_entries(max_nodes, true) + arer::count_entries(max_nodes);
}
constexpr uint64_t pop_entries(uint64_t max_nodes) { return model_entries(max_nodes, false) + arer::count_entries(max_nodes); }
template <class Acc, class Rank>
using PushState = rgraph::PushState<Acc, PuSlices<Acc>, arer::CountPush<Acc, Rank>>;
template <class Acc, class Rank>
using PopState = rgraph::PopState<Acc, PuSlices<Acc>, arer::CountPop<Acc, Rank>>;

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
