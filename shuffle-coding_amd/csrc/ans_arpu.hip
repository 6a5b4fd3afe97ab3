// ans_arpu.hip — the autoregressive Pólya urn graph codecs in bulk, one graph per message, one lane
// per graph: Autoregressive(PolyaUrnSliceCodecs) and ShuffleCodec<PolyaUrnSliceCodecs,
// WLOrbitCodecs<GraphPrefix>> with wl_iter = 0 (src/recursive/mod.rs:117-216, src/recursive/graph/
// slice.rs:61-230, incomplete.rs:189-236) under the resume contract of include/ans_capi.h 4b.
// Graph g's message is Message::unflatten(slot bytes) with the Empty tail; the codec is
// ans_arpu.hpp's, the same functions the host codec runs, on the exact 64-bit message ops of
// ans_exact.hpp.  A graph is a serial chain (two small uniform steps per node, an urn step and a
// permutation step per edge, an orbit step per node; Fenwick walks and a heapsort per large slice
// between them); the parallelism is across graphs.  The per-lane state (ans_arpu.hpp PushState /
// PopState) lives in the context's workspace, entry i of lane l at i * lanes + l, sized by the lanes
// resident; the degrees' class ranks are the context's read-only table (as ans_arer.hip's).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ans_arpu.hpp"
#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_hostio.hpp"
#include "ans_lane.hpp"

using namespace shuffle_coding::exact;
using namespace shuffle_coding::lane;
namespace ap = shuffle_coding::arpu;
namespace pu = shuffle_coding::polya;

namespace {

#define HIP_TRY(expr) ANS_HIP_TRY(expr)

struct ArpuArgs {
    uint64_t num_graphs;
    const uint32_t* num_nodes;
    const uint64_t* edge_offsets;
    uint32_t max_nodes;
    uint64_t max_edges;  // push: the bound of a graph's pairs (the state's nbr); pop: unused
    uint8_t* slots;
    uint64_t slot_cap;
    uint32_t* lens;
    uint32_t* status;
    uint32_t* ws;
    const uint32_t* rank;  // class ranks of the degrees 0 .. max_nodes
    int loops;
};

// graph g's shape, checked: false (ANS_E_ARG / ANS_E_LEN raised, lens[g] = 0) when it is not coded.
// A push holds the graph's pairs in its state, so they are bounded; a pop's range is a capacity.
template <bool kPush>
__device__ bool graph_shape(const ArpuArgs& a, uint64_t g, uint32_t& n, uint64_t& e0, uint64_t& room) {
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
    room = e1 - e0;
    return true;
}

// ---- push: grid-stride over the graphs, lane = one graph at a time
template <int kOrbits>
__global__ __launch_bounds__(kThreads) void k_arpu_push(ArpuArgs a, const uint32_t* __restrict__ edges,
                                                         uint32_t* __restrict__ perm) {
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto st = ap::PushState<LaneAcc>::make(LaneWs{a.ws + lane, lanes}, a.max_nodes, a.max_edges);
    for (uint64_t g = lane; g < a.num_graphs; g += lanes) {
        uint32_t n = 0;
        uint64_t e0 = 0, E = 0;
        if (!graph_shape<true>(a, g, n, e0, E)) continue;
        Sink sink(a.slots + g * a.slot_cap, a.slot_cap, a.lens[g]);
        SinkMsg m{0, &sink};  // Message::unflatten: head 0
        pu::Coder<SinkMsg> c{m, ANS_OK};
        int rc = ap::push_graph(c, st, n, a.loops != 0, kOrbits, a.rank, a.max_nodes + 1, edges + 2 * e0,
                                static_cast<uint32_t>(E), perm ? perm + g * a.max_nodes : nullptr);
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

// ---- pop: graph g's pairs from edge_offsets[g] of edges on, their number in num_edges[g]
template <int kOrbits>
__global__ __launch_bounds__(kThreads) void k_arpu_pop(ArpuArgs a, uint32_t* __restrict__ edges,
                                                        uint32_t* __restrict__ num_edges) {
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto st = ap::PopState<LaneAcc>::make(LaneWs{a.ws + lane, lanes}, a.max_nodes);
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
        int rc = ap::pop_graph(c, st, n, a.loops != 0, kOrbits, a.rank, a.max_nodes + 1, edges + 2 * e0, cap, &count);
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

// ---- host side
int dev_arpu(bool push, ans_gpu* g, int loops, int orbits, uint64_t num_graphs, const uint32_t* d_num_nodes,
             uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_aux, uint32_t max_nodes, uint64_t max_edges,
             uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, hipStream_t s) {
    if (max_nodes > 0x7FFFFFFFu || max_edges > ap::kMaxEdges) return ANS_E_ARG;
    unsigned grid = 0;
    uint32_t* ws = nullptr;
    const uint64_t entries = push ? ap::push_entries(max_nodes, max_edges) : ap::pop_entries(max_nodes);
    if (int rc = plan(g, num_graphs, entries, grid, ws)) return rc;
    if (orbits == ANS_ORBITS_DEGREE)
        if (int rc = degree_ranks(g, max_nodes)) return rc;
    const ArpuArgs a{num_graphs, d_num_nodes, d_edge_offsets, max_nodes, push ? max_edges : 0, d_slots,
                     slot_cap,   d_lens,      d_status,       ws,        g->d_degree_rank,     loops};
    g->last.clear();
    g->last.add(push ? kRecArpuPush : kRecArpuPop, 0, orbits, rec_grid(grid));
    if (push) {
        if (orbits == ANS_ORBITS_DEGREE) k_arpu_push<ANS_ORBITS_DEGREE><<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
        else if (orbits == ANS_ORBITS_ONE_CLASS) k_arpu_push<ANS_ORBITS_ONE_CLASS><<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
        else k_arpu_push<ANS_ORBITS_NONE><<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
    } else {
        if (orbits == ANS_ORBITS_DEGREE) k_arpu_pop<ANS_ORBITS_DEGREE><<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
        else if (orbits == ANS_ORBITS_ONE_CLASS) k_arpu_pop<ANS_ORBITS_ONE_CLASS><<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
        else k_arpu_pop<ANS_ORBITS_NONE><<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
    }
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}

// host buffers in and out (as ans_gpu_ar_er_*_graphs): the graphs' shapes checked on the host, the
// container expanded into slots with the slack of the largest graph, coded, packed.  max_edges: the
// largest graph's pairs on a push, its capacity on a pop (the slack's bound of what it can hold).
int host_arpu(bool push, ans_gpu* g, int loops, int orbits, uint64_t num_graphs, const uint32_t* num_nodes,
              uint32_t* edges, const uint64_t* edge_offsets, uint32_t* aux, const uint8_t* in, uint64_t in_len,
              const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
              uint64_t* lens, uint64_t* total) {
    *total = 0;
    if (!g || !orbits_ok(orbits)) return ANS_E_ARG;
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
    if (max_nodes > 0x7FFFFFFFu || max_edges > ap::kMaxEdges || (num_edges && !edges)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    Stage st;
    int rc = stage_in(g, edge_offsets, num_graphs, in, in_len, in_offsets, in_lens, ap::slack(max_nodes, max_edges), st);
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
    rc = dev_arpu(push, g, loops, orbits, num_graphs, d_nodes.as<uint32_t>(), d_edges.as<uint32_t>(),
                  st.starts.as<uint64_t>(), aux ? d_aux.as<uint32_t>() : nullptr, max_nodes, max_edges,
                  st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), d_status, s);
    if (rc || (rc = read_status(g, d_status, s))) return rc;
    if (!push && num_edges) HIP_TRY(hipMemcpy(edges, d_edges.p, 8 * num_edges, hipMemcpyDeviceToHost));
    if (aux && aux_entries) HIP_TRY(hipMemcpy(aux, d_aux.p, 4 * aux_entries, hipMemcpyDeviceToHost));
    return download_container(g, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), num_graphs, s, out, out_cap,
                              offsets, lens, total);
}

bool dev_args_ok(const ans_gpu* g, int orbits, uint64_t num_graphs, const uint32_t* d_num_nodes,
                 const uint64_t* d_edge_offsets, const uint8_t* d_slots, const uint32_t* d_lens,
                 const uint32_t* d_status) {
    return g && orbits_ok(orbits) && d_status && (!num_graphs || (d_num_nodes && d_edge_offsets && d_slots && d_lens));
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

int ans_gpu_ar_polya_slack(uint32_t max_nodes, uint64_t max_edges, uint64_t* bytes) try {
    if (!bytes || max_nodes > 0x7FFFFFFFu || max_edges > ap::kMaxEdges) return ANS_E_ARG;
    *bytes = ap::slack(max_nodes, max_edges);
    return ANS_OK;
} ANS_CATCH

int ans_dev_ar_polya_push(ans_gpu* g, int loops, int orbits, uint64_t num_graphs, const uint32_t* d_num_nodes,
                          const uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t max_nodes,
                          uint64_t max_edges, uint32_t* d_perm, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                          uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!dev_args_ok(g, orbits, num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status) ||
        (num_graphs && max_edges && !d_edges))
        return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return dev_arpu(true, g, loops, orbits, num_graphs, d_num_nodes, const_cast<uint32_t*>(d_edges), d_edge_offsets,
                    d_perm, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
} ANS_CATCH
int ans_dev_ar_polya_pop(ans_gpu* g, int loops, int orbits, uint64_t num_graphs, const uint32_t* d_num_nodes,
                         uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_num_edges, uint32_t max_nodes,
                         uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status,
                         void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!dev_args_ok(g, orbits, num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status) ||
        (num_graphs && (!d_edges || !d_num_edges)) || slot_cap < 16)
        return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return dev_arpu(false, g, loops, orbits, num_graphs, d_num_nodes, d_edges, d_edge_offsets, d_num_edges, max_nodes,
                    max_edges, d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
} ANS_CATCH

int ans_gpu_ar_polya_push_graphs(ans_gpu* g, int loops, int orbits, uint64_t num_graphs, const uint32_t* num_nodes,
                                 const uint32_t* edges, const uint64_t* edge_offsets, const uint8_t* in, uint64_t in_len,
                                 const uint64_t* in_offsets, const uint64_t* in_lens, uint32_t* perm, uint8_t* out,
                                 uint64_t out_cap, uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total) return ANS_E_ARG;
    return host_arpu(true, g, loops, orbits, num_graphs, num_nodes, const_cast<uint32_t*>(edges), edge_offsets, perm, in,
                     in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_ar_polya_pop_graphs(ans_gpu* g, int loops, int orbits, uint64_t num_graphs, const uint32_t* num_nodes,
                                const uint64_t* edge_offsets, const uint8_t* in, uint64_t in_len,
                                const uint64_t* in_offsets, const uint64_t* in_lens, uint32_t* out_edges,
                                uint32_t* out_num_edges, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                                uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total) return ANS_E_ARG;
    return host_arpu(false, g, loops, orbits, num_graphs, num_nodes, out_edges, edge_offsets, out_num_edges, in, in_len,
                     in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH

}  // extern "C"
