// ans_wl.hip — graph shuffle coding with Weisfeiler-Lehman orbits at wl_iter >= 0 in bulk, one graph
// per message, one lane per graph: ShuffleCodec<ErdosRenyiSliceCodecs | PolyaUrnSliceCodecs,
// WLOrbitCodecs<GraphPrefix>> (src/recursive/mod.rs:117-148, src/recursive/graph/incomplete.rs:45-57,
// 87-151, 189-236) under the resume contract of include/ans_capi.h 4b, as ans_arer.hip and
// ans_arpu.hip have wl_iter = 0.  The codec is ans_wl.hpp's, the same functions the host codec runs,
// on the exact 64-bit message ops of ans_exact.hpp.  The per-lane state (ans_wl.hpp ErPush / ErPop /
// PuPush / PuPop: the slice model's, the ids, the ordered known positions, the dirty list, the sort
// scratch, on a pop the decoded prefix's adjacency) lives in the context's workspace, entry i of
// lane l at i * lanes + l, sized by the lanes resident; wl_iter and half_iter are runtime arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_hostio.hpp"
#include "ans_lane.hpp"
#include "ans_wl.hpp"

using namespace shuffle_coding::exact;
using namespace shuffle_coding::lane;
namespace ar = shuffle_coding::arer;
namespace ap = shuffle_coding::arpu;
namespace pu = shuffle_coding::polya;
namespace wl = shuffle_coding::wl;

namespace {

#define HIP_TRY(expr) ANS_HIP_TRY(expr)

struct WlArgs {
    uint64_t num_graphs;
    const uint32_t* num_nodes;
    const uint64_t* edge_offsets;
    uint32_t max_nodes;
    uint64_t max_edges;  // the bound of a graph's pairs (the state's nbr / next)
    uint8_t* slots;
    uint64_t slot_cap;
    uint32_t* lens;
    uint32_t* status;
    uint32_t* ws;
    ar::Bern bern;  // (the Erdős–Rényi slices alone)
    uint32_t wl_iter;
    int half_iter, loops;
};

// graph g's shape, checked: false (ANS_E_ARG / ANS_E_LEN raised, lens[g] = 0) when it is not coded.
// A push holds the graph's pairs in its state, so they are bounded; a pop's range is a capacity, of
// which the state holds max_edges pairs at the most.
template <bool kPush>
__device__ bool graph_shape(const WlArgs& a, uint64_t g, uint32_t& n, uint64_t& e0, uint64_t& room) {
    n = a.num_nodes[g];
    e0 = a.edge_offsets[g];
    const uint64_t e1 = a.edge_offsets[g + 1];
    int code = ANS_OK;
    if (e1 < e0 || (kPush && e1 - e0 > a.max_edges) || n > a.max_nodes) code = ANS_E_ARG;
    else if (a.lens[g] > a.slot_cap) code = ANS_E_LEN;
    if (code) {
        raise(a.status, code);
        a.lens[g] = 0;
        return false;
    }
    room = e1 - e0 < a.max_edges ? e1 - e0 : a.max_edges;
    return true;
}

template <class St>
__device__ void push_loop(const WlArgs& a, St& st, const uint32_t* edges, uint32_t* perm, uint64_t lane, uint64_t lanes) {
    for (uint64_t g = lane; g < a.num_graphs; g += lanes) {
        uint32_t n = 0;
        uint64_t e0 = 0, E = 0;
        if (!graph_shape<true>(a, g, n, e0, E)) continue;
        Sink sink(a.slots + g * a.slot_cap, a.slot_cap, a.lens[g]);
        SinkMsg m{0, &sink};  // Message::unflatten: head 0
        pu::Coder<SinkMsg> c{m, ANS_OK};
        uint32_t* const p = perm ? perm + g * a.max_nodes : nullptr;
        int rc;
        if constexpr (std::is_same_v<St, wl::ErPush<LaneAcc>>)
            rc = wl::er_push_graph(c, st, a.bern, n, a.loops != 0, edges + 2 * e0, static_cast<uint32_t>(E), p);
        else
            rc = wl::pu_push_graph(c, st, n, a.loops != 0, edges + 2 * e0, static_cast<uint32_t>(E), p);
        uint64_t len = 0;
        if (!rc) {
            flatten(m.head, [&](uint32_t byte) { sink.put(byte); });
            len = sink.finish();
            if (sink.overflow || len > 0xFFFFFFFFull) rc = ANS_E_LEN;
        }
        if (rc) {
            raise(a.status, rc);
            len = 0;
        }
        a.lens[g] = static_cast<uint32_t>(len);
    }
}

template <class St>
__device__ void pop_loop(const WlArgs& a, St& st, uint32_t* edges, uint32_t* num_edges, uint64_t lane, uint64_t lanes) {
    for (uint64_t g = lane; g < a.num_graphs; g += lanes) {
        uint32_t n = 0;
        uint64_t e0 = 0, cap = 0, count = 0;
        if (!graph_shape<false>(a, g, n, e0, cap)) {
            num_edges[g] = 0;
            continue;
        }
        RSource src{a.slots + g * a.slot_cap, a.slot_cap, a.lens[g], false, false};
        SourceMsg m{0, &src};  // Message::unflatten: head 0
        pu::Coder<SourceMsg> c{m, ANS_OK};
        int rc;
        if constexpr (std::is_same_v<St, wl::ErPop<LaneAcc>>)
            rc = wl::er_pop_graph(c, st, a.bern, n, a.loops != 0, edges + 2 * e0, cap, &count);
        else
            rc = wl::pu_pop_graph(c, st, n, a.loops != 0, edges + 2 * e0, cap, &count);
        if (!rc) {
            flatten(m.head, [&](uint32_t byte) { src.unpop(byte & 0xFFu); });
            if (src.overflow || src.pos > 0xFFFFFFFFull) rc = ANS_E_LEN;
        }
        if (rc) {
            raise(a.status, rc);
            src.pos = 0;
            count = 0;
        }
        a.lens[g] = static_cast<uint32_t>(src.pos);
        num_edges[g] = static_cast<uint32_t>(count);
    }
}

// ---- grid-stride over the graphs, lane = one graph at a time.  (edges is written by a pop and read
// back by its adjacency, so it is not __restrict__ there.)
__global__ __launch_bounds__(kThreads) void k_arer_wl_push(WlArgs a, const uint32_t* __restrict__ edges,
                                                            uint32_t* __restrict__ perm) {
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto st = wl::ErPush<LaneAcc>::make(LaneWs{a.ws + lane, lanes}, a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    push_loop(a, st, edges, perm, lane, lanes);
}
__global__ __launch_bounds__(kThreads) void k_arer_wl_pop(WlArgs a, uint32_t* edges, uint32_t* __restrict__ num_edges) {
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto st = wl::ErPop<LaneAcc>::make(LaneWs{a.ws + lane, lanes}, a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    pop_loop(a, st, edges, num_edges, lane, lanes);
}
__global__ __launch_bounds__(kThreads) void k_arpu_wl_push(WlArgs a, const uint32_t* __restrict__ edges,
                                                            uint32_t* __restrict__ perm) {
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto st = wl::PuPush<LaneAcc>::make(LaneWs{a.ws + lane, lanes}, a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    push_loop(a, st, edges, perm, lane, lanes);
}
__global__ __launch_bounds__(kThreads) void k_arpu_wl_pop(WlArgs a, uint32_t* edges, uint32_t* __restrict__ num_edges) {
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto st = wl::PuPop<LaneAcc>::make(LaneWs{a.ws + lane, lanes}, a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    pop_loop(a, st, edges, num_edges, lane, lanes);
}

// ---- host side.  gt: the Bernoulli of the Erdős–Rényi slices, null for the Pólya urn's.
bool table_ok(const ans_gpu_table* gt) { return gt && gt->g && gt->t.nsym == 2; }
bool wl_ok(int wl_iter) { return wl_iter >= 0 && wl_iter <= static_cast<int>(wl::kMaxIter); }

int dev_wl(bool push, ans_gpu* g, const ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
           const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_aux,
           uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
           uint32_t* d_status, hipStream_t s) {
    const uint32_t w = static_cast<uint32_t>(wl_iter);
    if (!wl::nodes_ok(max_nodes, w) || max_edges > ar::kMaxEdges) return ANS_E_ARG;
    const uint64_t entries = gt ? (push ? wl::er_push_entries(max_nodes, max_edges, w) : wl::er_pop_entries(max_nodes, max_edges, w))
                                : (push ? wl::pu_push_entries(max_nodes, max_edges, w) : wl::pu_pop_entries(max_nodes, max_edges, w));
    unsigned grid = 0;
    uint32_t* ws = nullptr;
    if (int rc = plan(g, num_graphs, entries, grid, ws)) return rc;
    const WlArgs a{num_graphs, d_num_nodes, d_edge_offsets, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, ws,
                   gt ? ar::bern_of(gt->mass2[0], gt->mass2[1]) : ar::Bern{}, w, half_iter != 0, loops};
    g->last.clear();
    g->last.add(gt ? (push ? kRecArerWlPush : kRecArerWlPop) : (push ? kRecArpuWlPush : kRecArpuWlPop), 0, wl_iter,
                rec_grid(grid), half_iter != 0);
    if (gt) {
        if (push) k_arer_wl_push<<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
        else k_arer_wl_pop<<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
    } else {
        if (push) k_arpu_wl_push<<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
        else k_arpu_wl_pop<<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
    }
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}

// host buffers in and out (as ans_gpu_ar_er_*_graphs / ans_gpu_ar_polya_*_graphs): the graphs' shapes
// checked on the host, the container expanded into slots with the slack of the largest graph (the
// wl_iter = 0 codecs' slack: an orbit step moves no more bits at any wl_iter), coded, packed.
int host_wl(bool push, ans_gpu* g, const ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
            const uint32_t* num_nodes, uint32_t* edges, const uint64_t* edge_offsets, uint32_t* aux, const uint8_t* in,
            uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out, uint64_t out_cap,
            uint64_t* offsets, uint64_t* lens, uint64_t* total) {
    *total = 0;
    if (!g || !wl_ok(wl_iter)) return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    if (!num_nodes || !edge_offsets || !in_offsets || !in_lens || (in_len && !in)) return ANS_E_ARG;
    if ((out && (!offsets || !lens)) || (!push && !aux)) return ANS_E_ARG;
    uint32_t max_nodes = 0;
    uint64_t max_edges = 0;
    for (uint64_t k = 0; k < num_graphs; ++k) {
        if (edge_offsets[k + 1] < edge_offsets[k]) return ANS_E_ARG;
        max_nodes = std::max(max_nodes, num_nodes[k]);
        max_edges = std::max(max_edges, edge_offsets[k + 1] - edge_offsets[k]);
    }
    const uint64_t num_edges = edge_offsets[num_graphs];
    if (max_nodes > 0x7FFFFFFFu || max_edges > ar::kMaxEdges || (num_edges && !edges)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    Stage st;
    const uint64_t slack = gt ? ar::slack(ar::bern_of(gt->mass2[0], gt->mass2[1]), max_nodes, loops != 0)
                              : ap::slack(max_nodes, max_edges);
    int rc = stage_in(g, edge_offsets, num_graphs, in, in_len, in_offsets, in_lens, slack, st);
    if (rc) return rc;
    const uint64_t aux_entries = push ? num_graphs * max_nodes : num_graphs;
    DevBuf d_nodes, d_edges, d_aux;
    HIP_TRY(d_nodes.alloc(4 * num_graphs));
    HIP_TRY(d_edges.alloc(8 * num_edges));
    if (aux) HIP_TRY(d_aux.alloc(4 * aux_entries));
    HIP_TRY(hipMemcpyAsync(d_nodes.p, num_nodes, 4 * num_graphs, hipMemcpyHostToDevice, s));
    if (push && num_edges) HIP_TRY(hipMemcpyAsync(d_edges.p, edges, 8 * num_edges, hipMemcpyHostToDevice, s));
    if (push && aux) HIP_TRY(hipMemsetAsync(d_aux.p, 0, 4 * aux_entries, s));  // (the entries past a graph's nodes)
    uint32_t* d_status = st.d.status.as<uint32_t>();
    rc = dev_wl(push, g, gt, loops, wl_iter, half_iter, num_graphs, d_nodes.as<uint32_t>(), d_edges.as<uint32_t>(),
                st.starts.as<uint64_t>(), aux ? d_aux.as<uint32_t>() : nullptr, max_nodes, max_edges,
                st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), d_status, s);
    if (rc || (rc = read_status(g, d_status, s))) return rc;
    if (!push && num_edges) HIP_TRY(hipMemcpy(edges, d_edges.p, 8 * num_edges, hipMemcpyDeviceToHost));
    if (aux && aux_entries) HIP_TRY(hipMemcpy(aux, d_aux.p, 4 * aux_entries, hipMemcpyDeviceToHost));
    return download_container(g, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), num_graphs, s, out, out_cap,
                              offsets, lens, total);
}

bool dev_args_ok(const ans_gpu* g, int wl_iter, uint64_t num_graphs, const uint32_t* d_num_nodes,
                 const uint64_t* d_edge_offsets, const uint8_t* d_slots, const uint32_t* d_lens, const uint32_t* d_status) {
    return g && wl_ok(wl_iter) && d_status && (!num_graphs || (d_num_nodes && d_edge_offsets && d_slots && d_lens));
}

int dev_push(ans_gpu* g, const ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
             const uint32_t* d_num_nodes, const uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t max_nodes,
             uint64_t max_edges, uint32_t* d_perm, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
             uint32_t* d_status, void* stream) {
    if (!dev_args_ok(g, wl_iter, num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status) ||
        (num_graphs && max_edges && !d_edges))
        return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return dev_wl(true, g, gt, loops, wl_iter, half_iter, num_graphs, d_num_nodes, const_cast<uint32_t*>(d_edges),
                  d_edge_offsets, d_perm, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
}
int dev_pop(ans_gpu* g, const ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
            const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_num_edges,
            uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
            uint32_t* d_status, void* stream) {
    if (!dev_args_ok(g, wl_iter, num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status) ||
        (num_graphs && (!d_edges || !d_num_edges)) || slot_cap < 16)
        return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return dev_wl(false, g, gt, loops, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets, d_num_edges,
                  max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

int ans_dev_ar_er_wl_push(ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                          const uint32_t* d_num_nodes, const uint32_t* d_edges, const uint64_t* d_edge_offsets,
                          uint32_t max_nodes, uint64_t max_edges, uint32_t* d_perm, uint8_t* d_slots, uint64_t slot_cap,
                          uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!table_ok(gt)) return ANS_E_ARG;
    return dev_push(gt->g, gt, loops, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets, max_nodes,
                    max_edges, d_perm, d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH
int ans_dev_ar_er_wl_pop(ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                         const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets,
                         uint32_t* d_num_edges, uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots,
                         uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!table_ok(gt)) return ANS_E_ARG;
    return dev_pop(gt->g, gt, loops, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets, d_num_edges,
                   max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH
int ans_dev_ar_polya_wl_push(ans_gpu* g, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                             const uint32_t* d_num_nodes, const uint32_t* d_edges, const uint64_t* d_edge_offsets,
                             uint32_t max_nodes, uint64_t max_edges, uint32_t* d_perm, uint8_t* d_slots,
                             uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    return dev_push(g, nullptr, loops, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets, max_nodes,
                    max_edges, d_perm, d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH
int ans_dev_ar_polya_wl_pop(ans_gpu* g, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                            const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets,
                            uint32_t* d_num_edges, uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots,
                            uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    return dev_pop(g, nullptr, loops, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets, d_num_edges,
                   max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH

int ans_gpu_ar_er_wl_push_graphs(ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                 const uint32_t* num_nodes, const uint32_t* edges, const uint64_t* edge_offsets,
                                 const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens,
                                 uint32_t* perm, uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens,
                                 uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total || !table_ok(gt)) return ANS_E_ARG;
    return host_wl(true, gt->g, gt, loops, wl_iter, half_iter, num_graphs, num_nodes, const_cast<uint32_t*>(edges),
                   edge_offsets, perm, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_ar_er_wl_pop_graphs(ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                const uint32_t* num_nodes, const uint64_t* edge_offsets, const uint8_t* in,
                                uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens, uint32_t* out_edges,
                                uint32_t* out_num_edges, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                                uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total || !table_ok(gt)) return ANS_E_ARG;
    return host_wl(false, gt->g, gt, loops, wl_iter, half_iter, num_graphs, num_nodes, out_edges, edge_offsets,
                   out_num_edges, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_ar_polya_wl_push_graphs(ans_gpu* g, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                    const uint32_t* num_nodes, const uint32_t* edges, const uint64_t* edge_offsets,
                                    const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
                                    const uint64_t* in_lens, uint32_t* perm, uint8_t* out, uint64_t out_cap,
                                    uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total) return ANS_E_ARG;
    return host_wl(true, g, nullptr, loops, wl_iter, half_iter, num_graphs, num_nodes, const_cast<uint32_t*>(edges),
                   edge_offsets, perm, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_ar_polya_wl_pop_graphs(ans_gpu* g, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                   const uint32_t* num_nodes, const uint64_t* edge_offsets, const uint8_t* in,
                                   uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens,
                                   uint32_t* out_edges, uint32_t* out_num_edges, uint8_t* out, uint64_t out_cap,
                                   uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total) return ANS_E_ARG;
    return host_wl(false, g, nullptr, loops, wl_iter, half_iter, num_graphs, num_nodes, out_edges, edge_offsets,
                   out_num_edges, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH

}  // extern "C"
