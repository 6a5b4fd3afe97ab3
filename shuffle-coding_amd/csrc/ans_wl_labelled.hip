// ans_wl_labelled.hip — graph shuffle coding with Weisfeiler-Lehman orbits of graphs that carry node
// and edge labels, in bulk, one graph per message, one lane per graph: ShuffleCodec<
// ErdosRenyiSliceCodecs<NodeC, EdgeC, _> | PolyaUrnSliceCodecs<NodeC, EdgeC, _>, WLOrbitCodecs<_, N, E, _>>
// (src/recursive/graph/mod.rs:53-104, slice.rs:33-51, 185-192, src/graph_codec.rs:58-94,
// incomplete.rs:45-57, 97-151, 193-210) under the resume contract of include/ans_capi.h 4b, as
// ans_wl.hip has the graphs without labels.  The codec is ans_rgraph.hpp's recursion under a label
// policy over either slice model and ans_wl.hpp's orbit stage, the same functions the host codec runs;
// the per-lane loops and the host staging are ans_lane.hpp's.  The label tables are Categoricals of
// a table set (ans_exact.hpp CatSetModel), its image staged in LDS when it fits as k_mset_push has
// it; a label step runs on the lane's polya::Coder (rgraph::push_cat / pop_cat).  The per-lane state
// lives in the context's workspace, entry i of lane l at i * lanes + l.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_hostio.hpp"
#include "ans_lane.hpp"
#include "ans_wl.hpp"

using namespace shuffle_coding::exact;
using namespace shuffle_coding::lane;
namespace ar = shuffle_coding::arer;
namespace ap = shuffle_coding::arpu;
namespace rg = shuffle_coding::rgraph;
namespace wl = shuffle_coding::wl;

namespace {

#define HIP_TRY(expr) ANS_HIP_TRY(expr)

// What the kernels take beside ans_lane.hpp's GraphArgs: the table set, the two label tables in it
// (ANS_NO_TABLE under a policy without that label) and the label arrays: node labels num_graphs x
// max_nodes, graph g's at g * max_nodes; edge labels beside the pairs, at the pairs' offsets.
struct LabelArgs {
    CatSetModel md;
    uint32_t t_node, t_edge;
    uint32_t *nl, *el;  // (read by a push, written by a pop)
};
__device__ rg::Cat cat_of(const CatSetModel& md, uint32_t t) {
    const TabHdr h = md.hdr[t];
    return rg::Cat{md.cum + h.cum_off, md.bkt + h.bkt_off, h.norm, h.nsym, h.shift};
}
template <class L, class Lab>
__device__ void set_tables(Lab& lab, const LabelArgs& la) {
    if constexpr (L::node) lab.node = cat_of(la.md, la.t_node);
    if constexpr (L::edge) lab.edge = cat_of(la.md, la.t_edge);
}

// ---- grid-stride over the graphs, lane = one graph at a time.  kEr: the Erdős–Rényi slices, else
// the Pólya urn's; L: the label policy.
template <bool kEr, class L>
__global__ __launch_bounds__(kThreads) void k_wll_push(GraphArgs a, LabelArgs la, const uint32_t* __restrict__ edges,
                                                        uint32_t* __restrict__ perm) {
    extern __shared__ __align__(16) unsigned char lds[];
    la.md.stage(lds);
    const Lane l = Lane::mine();
    using St = std::conditional_t<kEr, wl::ErPush<LaneAcc, L>, wl::PuPush<LaneAcc, L>>;
    auto st = St::make(l.ws(a.ws), a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    if constexpr (kEr) st.bern = a.bern;
    if constexpr (L::any) set_tables<L>(st.lab, la);
    push_loop(a, l, st, edges, perm, [&](uint64_t g, uint64_t e0) {
        if constexpr (L::node) st.lab.nl = la.nl + g * a.max_nodes;
        if constexpr (L::edge) st.lab.el = la.el + e0;
    });
}
// (edges and the edge labels are written by a pop and read back by its adjacency: not __restrict__)
template <bool kEr, class L>
__global__ __launch_bounds__(kThreads) void k_wll_pop(GraphArgs a, LabelArgs la, uint32_t* edges, uint32_t* __restrict__ num_edges) {
    extern __shared__ __align__(16) unsigned char lds[];
    la.md.stage(lds);
    const Lane l = Lane::mine();
    using St = std::conditional_t<kEr, wl::ErPop<LaneAcc, L>, wl::PuPop<LaneAcc, L>>;
    auto st = St::make(l.ws(a.ws), a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    if constexpr (kEr) st.bern = a.bern;
    set_tables<L>(st.lab, la);
    pop_loop<true>(a, l, st, edges, num_edges, [&](uint64_t g, uint64_t e0) {
        if constexpr (L::node) st.lab.nl = la.nl + g * a.max_nodes;
        if constexpr (L::edge) st.lab.el = la.el + e0;
    });
}

// ---- host side
bool wl_ok(int wl_iter) { return wl_iter >= 0 && wl_iter <= static_cast<int>(wl::kMaxIter); }

// The tables of a call, checked: t_bern a two-symbol table of the set (the Erdős–Rényi slices), or
// ANS_NO_TABLE for the Pólya urn's; a label table with its array and an array with its table.
struct Tables {
    ans_gpu_tableset* ts;
    uint32_t t_bern, t_node, t_edge;
    bool er() const { return t_bern != ANS_NO_TABLE; }
    bool in_set() const {
        if (!ts) return false;
        const std::vector<uint32_t>& nsym = ans_tableset_nsyms(ts);
        const auto ok = [&](uint32_t t) { return t == ANS_NO_TABLE || t < nsym.size(); };
        return ok(t_bern) && ok(t_node) && ok(t_edge) && (!er() || nsym[t_bern] == 2);
    }
    bool ok(const void* nl, const void* el) const {
        return in_set() && (t_node != ANS_NO_TABLE) == (nl != nullptr) && (t_edge != ANS_NO_TABLE) == (el != nullptr);
    }
    ar::Bern bern() const {
        if (!er()) return ar::Bern{};
        const ans_tab_info& b = ans_tableset_info(ts)[t_bern];
        return ar::bern_of(b.mass0, b.norm - b.mass0);
    }
    uint64_t slack(uint32_t max_nodes, uint64_t max_edges, bool loops) const {
        const std::vector<ans_tab_info>& info = ans_tableset_info(ts);
        const auto bits = [&](uint32_t t) { return t == ANS_NO_TABLE ? 0 : rg::label_push_bits(info[t].norm, info[t].pmin); };
        return (er() ? ar::slack(bern(), max_nodes, loops) : ap::slack(max_nodes, max_edges)) +
               rg::label_slack(bits(t_node), bits(t_edge), max_nodes, max_edges);
    }
};

template <class F>
void with_labels(bool node, bool edge, F&& f) {
    if (node) edge ? f(rg::Labels<true, true>{}) : f(rg::Labels<true, false>{});
    else edge ? f(rg::Labels<false, true>{}) : f(rg::Labels<false, false, true>{});
}

int dev_wll(bool push, const Tables& t, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
            const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_nl, uint32_t* d_el,
            uint32_t* d_aux, uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
            uint32_t* d_status, hipStream_t s) {
    ans_gpu* g = ans_tableset_gpu(t.ts);
    const uint32_t w = static_cast<uint32_t>(wl_iter);
    const bool nl = t.t_node != ANS_NO_TABLE, el = t.t_edge != ANS_NO_TABLE;
    if (!wl::nodes_ok(max_nodes, w) || max_edges > ar::kMaxEdges) return ANS_E_ARG;
    const uint64_t entries = t.er() ? (push ? wl::er_push_entries(max_nodes, max_edges, w, el) : wl::er_pop_entries(max_nodes, max_edges, w, el))
                                    : (push ? wl::pu_push_entries(max_nodes, max_edges, w, el) : wl::pu_pop_entries(max_nodes, max_edges, w, el));
    unsigned grid = 0;
    uint32_t* ws = nullptr;
    if (int rc = plan(g, num_graphs, entries, grid, ws)) return rc;
    const GraphArgs a{num_graphs, d_num_nodes, d_edge_offsets, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, ws,
                      loops, nullptr, t.bern(), w, half_iter != 0};
    const LabelArgs la{ans_tableset_model(t.ts), t.t_node, t.t_edge, d_nl, d_el};
    g->last.clear();
    g->last.add(t.er() ? (push ? kRecArerWllPush : kRecArerWllPop) : (push ? kRecArpuWllPush : kRecArpuWllPop), 0, wl_iter,
                rec_grid(grid), half_iter != 0, nl, el);
    const size_t lds = la.md.lds_bytes;
    with_labels(nl, el, [&](auto labels) {
        using L = decltype(labels);
        if (t.er()) {
            if (push) k_wll_push<true, L><<<grid, kThreads, lds, s>>>(a, la, d_edges, d_aux);
            else k_wll_pop<true, L><<<grid, kThreads, lds, s>>>(a, la, d_edges, d_aux);
        } else {
            if (push) k_wll_push<false, L><<<grid, kThreads, lds, s>>>(a, la, d_edges, d_aux);
            else k_wll_pop<false, L><<<grid, kThreads, lds, s>>>(a, la, d_edges, d_aux);
        }
    });
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}

int dev_entry(bool push, const Tables& t, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
              const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_nl, uint32_t* d_el,
              uint32_t* d_aux, uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
              uint32_t* d_status, void* stream) {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!t.ok(d_nl, d_el) || !dev_args_ok(wl_ok(wl_iter), num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status))
        return ANS_E_ARG;
    if (push ? (num_graphs && max_edges && !d_edges) : ((num_graphs && (!d_edges || !d_aux)) || slot_cap < 16)) return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    ans_gpu* g = ans_tableset_gpu(t.ts);
    HIP_TRY(hipSetDevice(g->device));
    return dev_wll(push, t, loops, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets, d_nl, d_el, d_aux,
                   max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
}

// host buffers in and out (ans_lane.hpp's staging; the labels staged here beside it).  node_labels:
// num_graphs x the largest num_nodes, as perm is laid out; edge_labels: one per pair of edges.
int host_wll(bool push, const Tables& t, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
             const uint32_t* num_nodes, uint32_t* edges, const uint64_t* edge_offsets, uint32_t* node_labels,
             uint32_t* edge_labels, uint32_t* aux, const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
             const uint64_t* in_lens, uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens, uint64_t* total) {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total) return ANS_E_ARG;
    *total = 0;
    if (!t.ok(node_labels, edge_labels) || !wl_ok(wl_iter)) return ANS_E_ARG;
    ans_gpu* g = ans_tableset_gpu(t.ts);
    DevBuf d_nl, d_el;
    uint64_t nl_entries = 0, el_entries = 0;
    const int rc = host_graphs(
        push, g, PopEdges::kBounded, num_graphs, num_nodes, edges, edge_offsets, aux, in, in_len, in_offsets, in_lens, out,
        out_cap, offsets, lens, total,
        [&](uint32_t max_nodes, uint64_t max_edges) { return t.slack(max_nodes, max_edges, loops != 0); },
        [&](const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_aux, uint32_t max_nodes,
            uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, hipStream_t s) {
            nl_entries = node_labels ? num_graphs * max_nodes : 0;
            el_entries = edge_labels ? edge_offsets[num_graphs] : 0;
            // (an array that is given has a device copy even when it holds nothing: the kernels' policy follows the pointers)
            if (node_labels) HIP_TRY(d_nl.alloc(4 * std::max<uint64_t>(nl_entries, 1)));
            if (edge_labels) HIP_TRY(d_el.alloc(4 * std::max<uint64_t>(el_entries, 1)));
            if (push && nl_entries) HIP_TRY(hipMemcpyAsync(d_nl.p, node_labels, 4 * nl_entries, hipMemcpyHostToDevice, s));
            if (push && el_entries) HIP_TRY(hipMemcpyAsync(d_el.p, edge_labels, 4 * el_entries, hipMemcpyHostToDevice, s));
            if (!push && nl_entries) HIP_TRY(hipMemsetAsync(d_nl.p, 0, 4 * nl_entries, s));  // (the entries past a graph's nodes)
            if (!push && el_entries) HIP_TRY(hipMemsetAsync(d_el.p, 0, 4 * el_entries, s));
            return dev_wll(push, t, loops, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets,
                           node_labels ? d_nl.as<uint32_t>() : nullptr, edge_labels ? d_el.as<uint32_t>() : nullptr, d_aux,
                           max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, s);
        });
    if (rc || push) return rc;
    if (nl_entries) HIP_TRY(hipMemcpy(node_labels, d_nl.p, 4 * nl_entries, hipMemcpyDeviceToHost));
    if (el_entries) HIP_TRY(hipMemcpy(edge_labels, d_el.p, 4 * el_entries, hipMemcpyDeviceToHost));
    return ANS_OK;
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

int ans_gpu_ar_er_wl_labelled_slack(const ans_gpu_tableset* ts, uint32_t bern_table, uint32_t node_table,
                                    uint32_t edge_table, uint32_t max_nodes, uint64_t max_edges, int loops,
                                    uint64_t* bytes) try {
    const Tables t{const_cast<ans_gpu_tableset*>(ts), bern_table, node_table, edge_table};
    if (!bytes || bern_table == ANS_NO_TABLE || !t.in_set() || max_nodes > 0x7FFFFFFFu || max_edges > ar::kMaxEdges)
        return ANS_E_ARG;
    *bytes = t.slack(max_nodes, max_edges, loops != 0);
    return ANS_OK;
} ANS_CATCH
int ans_gpu_ar_polya_wl_labelled_slack(const ans_gpu_tableset* ts, uint32_t node_table, uint32_t edge_table,
                                       uint32_t max_nodes, uint64_t max_edges, uint64_t* bytes) try {
    const Tables t{const_cast<ans_gpu_tableset*>(ts), ANS_NO_TABLE, node_table, edge_table};
    if (!bytes || !t.in_set() || max_nodes > 0x7FFFFFFFu || max_edges > ar::kMaxEdges)
        return ANS_E_ARG;
    *bytes = t.slack(max_nodes, max_edges, false);
    return ANS_OK;
} ANS_CATCH

int ans_dev_ar_er_wl_labelled_push(ans_gpu_tableset* ts, uint32_t bern_table, uint32_t node_table, uint32_t edge_table,
                                   int loops, int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t* d_num_nodes,
                                   const uint32_t* d_edges, const uint64_t* d_edge_offsets, const uint32_t* d_node_labels,
                                   const uint32_t* d_edge_labels, uint32_t max_nodes, uint64_t max_edges, uint32_t* d_perm,
                                   uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status,
                                   void* stream) try {
    if (bern_table == ANS_NO_TABLE) return ANS_E_ARG;
    return dev_entry(true, Tables{ts, bern_table, node_table, edge_table}, loops, wl_iter, half_iter, num_graphs, d_num_nodes,
                     const_cast<uint32_t*>(d_edges), d_edge_offsets, const_cast<uint32_t*>(d_node_labels),
                     const_cast<uint32_t*>(d_edge_labels), d_perm, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status,
                     stream);
} ANS_CATCH
int ans_dev_ar_er_wl_labelled_pop(ans_gpu_tableset* ts, uint32_t bern_table, uint32_t node_table, uint32_t edge_table,
                                  int loops, int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t* d_num_nodes,
                                  uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_num_edges,
                                  uint32_t* d_node_labels, uint32_t* d_edge_labels, uint32_t max_nodes, uint64_t max_edges,
                                  uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status,
                                  void* stream) try {
    if (bern_table == ANS_NO_TABLE) return ANS_E_ARG;
    return dev_entry(false, Tables{ts, bern_table, node_table, edge_table}, loops, wl_iter, half_iter, num_graphs,
                     d_num_nodes, d_edges, d_edge_offsets, d_node_labels, d_edge_labels, d_num_edges, max_nodes, max_edges,
                     d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH
int ans_dev_ar_polya_wl_labelled_push(ans_gpu_tableset* ts, uint32_t node_table, uint32_t edge_table, int loops,
                                      int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t* d_num_nodes,
                                      const uint32_t* d_edges, const uint64_t* d_edge_offsets,
                                      const uint32_t* d_node_labels, const uint32_t* d_edge_labels, uint32_t max_nodes,
                                      uint64_t max_edges, uint32_t* d_perm, uint8_t* d_slots, uint64_t slot_cap,
                                      uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    return dev_entry(true, Tables{ts, ANS_NO_TABLE, node_table, edge_table}, loops, wl_iter, half_iter, num_graphs,
                     d_num_nodes, const_cast<uint32_t*>(d_edges), d_edge_offsets, const_cast<uint32_t*>(d_node_labels),
                     const_cast<uint32_t*>(d_edge_labels), d_perm, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status,
                     stream);
} ANS_CATCH
int ans_dev_ar_polya_wl_labelled_pop(ans_gpu_tableset* ts, uint32_t node_table, uint32_t edge_table, int loops,
                                     int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t* d_num_nodes,
                                     uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_num_edges,
                                     uint32_t* d_node_labels, uint32_t* d_edge_labels, uint32_t max_nodes,
                                     uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                                     uint32_t* d_status, void* stream) try {
    return dev_entry(false, Tables{ts, ANS_NO_TABLE, node_table, edge_table}, loops, wl_iter, half_iter, num_graphs,
                     d_num_nodes, d_edges, d_edge_offsets, d_node_labels, d_edge_labels, d_num_edges, max_nodes, max_edges,
                     d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH

int ans_gpu_ar_er_wl_labelled_push_graphs(ans_gpu_tableset* ts, uint32_t bern_table, uint32_t node_table,
                                          uint32_t edge_table, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                          const uint32_t* num_nodes, const uint32_t* edges, const uint64_t* edge_offsets,
                                          const uint32_t* node_labels, const uint32_t* edge_labels, const uint8_t* in,
                                          uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens,
                                          uint32_t* perm, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                                          uint64_t* lens, uint64_t* total) try {
    if (bern_table == ANS_NO_TABLE) return ANS_E_ARG;
    return host_wll(true, Tables{ts, bern_table, node_table, edge_table}, loops, wl_iter, half_iter, num_graphs, num_nodes,
                    const_cast<uint32_t*>(edges), edge_offsets, const_cast<uint32_t*>(node_labels),
                    const_cast<uint32_t*>(edge_labels), perm, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens,
                    total);
} ANS_CATCH
int ans_gpu_ar_er_wl_labelled_pop_graphs(ans_gpu_tableset* ts, uint32_t bern_table, uint32_t node_table,
                                         uint32_t edge_table, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                         const uint32_t* num_nodes, const uint64_t* edge_offsets, const uint8_t* in,
                                         uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens,
                                         uint32_t* out_edges, uint32_t* out_num_edges, uint32_t* out_node_labels,
                                         uint32_t* out_edge_labels, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                                         uint64_t* lens, uint64_t* total) try {
    if (bern_table == ANS_NO_TABLE) return ANS_E_ARG;
    return host_wll(false, Tables{ts, bern_table, node_table, edge_table}, loops, wl_iter, half_iter, num_graphs, num_nodes,
                    out_edges, edge_offsets, out_node_labels, out_edge_labels, out_num_edges, in, in_len, in_offsets, in_lens,
                    out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_ar_polya_wl_labelled_push_graphs(ans_gpu_tableset* ts, uint32_t node_table, uint32_t edge_table, int loops,
                                             int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t* num_nodes,
                                             const uint32_t* edges, const uint64_t* edge_offsets,
                                             const uint32_t* node_labels, const uint32_t* edge_labels, const uint8_t* in,
                                             uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens,
                                             uint32_t* perm, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                                             uint64_t* lens, uint64_t* total) try {
    return host_wll(true, Tables{ts, ANS_NO_TABLE, node_table, edge_table}, loops, wl_iter, half_iter, num_graphs, num_nodes,
                    const_cast<uint32_t*>(edges), edge_offsets, const_cast<uint32_t*>(node_labels),
                    const_cast<uint32_t*>(edge_labels), perm, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens,
                    total);
} ANS_CATCH
int ans_gpu_ar_polya_wl_labelled_pop_graphs(ans_gpu_tableset* ts, uint32_t node_table, uint32_t edge_table, int loops,
                                            int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t* num_nodes,
                                            const uint64_t* edge_offsets, const uint8_t* in, uint64_t in_len,
                                            const uint64_t* in_offsets, const uint64_t* in_lens, uint32_t* out_edges,
                                            uint32_t* out_num_edges, uint32_t* out_node_labels, uint32_t* out_edge_labels,
                                            uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens,
                                            uint64_t* total) try {
    return host_wll(false, Tables{ts, ANS_NO_TABLE, node_table, edge_table}, loops, wl_iter, half_iter, num_graphs, num_nodes,
                    out_edges, edge_offsets, out_node_labels, out_edge_labels, out_num_edges, in, in_len, in_offsets, in_lens,
                    out, out_cap, offsets, lens, total);
} ANS_CATCH

}  // extern "C"
