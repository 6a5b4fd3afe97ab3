// ans_polya.hip — the Pólya urn edge-index codec in bulk, one graph per message, one lane per
// graph: multiset_shuffle_codec(PolyaUrnEdgeIndicesCodec<Undirected>) (src/graph_codec.rs:210-375,
// src/recursive/multiset.rs:126-136) under the resume contract of include/ans_capi.h 4b.  Graph
// g's message is Message::unflatten(slot bytes) with the Empty tail; the codec is ans_polya.hpp's,
// the same functions the host codec runs, on the exact 64-bit message ops of ans_exact.hpp.
// A graph is a serial chain (64-bit divides, Fenwick walks, stack walks, each depending on the
// last); the parallelism is across graphs.  The per-lane state (ans_polya.hpp State) lives in the
// context's workspace, entry i of lane l at i * lanes + l, sized by the lanes resident.  The edge
// ranks by orbit id are a per-lane heapsort inside the coder (DESIGN.md §3.9 says why).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_hostio.hpp"
#include "ans_lane.hpp"
#include "ans_polya.hpp"

using namespace shuffle_coding::exact;
using namespace shuffle_coding::lane;
namespace pu = shuffle_coding::polya;

namespace {

#define HIP_TRY(expr) ANS_HIP_TRY(expr)

struct PolyaArgs {
    uint64_t num_graphs;
    const uint32_t* num_nodes;
    const uint64_t* edge_offsets;
    uint32_t max_nodes;
    uint64_t max_edges;
    uint8_t* slots;
    uint64_t slot_cap;
    uint32_t* lens;
    uint32_t* status;
    uint32_t* ws;
    int loops;
};

// graph g's shape, checked: false (ANS_E_ARG / ANS_E_LEN raised, lens[g] = 0) when it is not coded
__device__ bool graph_shape(const PolyaArgs& a, uint64_t g, uint32_t& n, uint64_t& e0, uint32_t& E) {
    n = a.num_nodes[g];
    e0 = a.edge_offsets[g];
    const uint64_t e1 = a.edge_offsets[g + 1];
    int code = ANS_OK;
    if (e1 < e0 || e1 - e0 > a.max_edges || n > a.max_nodes) code = ANS_E_ARG;
    else if (a.lens[g] > a.slot_cap) code = ANS_E_LEN;
    if (code) {
        raise(a.status, code);
        a.lens[g] = 0;
        return false;
    }
    E = static_cast<uint32_t>(e1 - e0);
    return true;
}

// ---- push: grid-stride over the graphs, lane = one graph at a time
template <bool kRedraws>
__global__ __launch_bounds__(kThreads) void k_polya_push(PolyaArgs a, const uint32_t* __restrict__ edges) {
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto st = pu::State<LaneAcc>::make(LaneWs{a.ws + lane, lanes}, a.max_nodes, a.max_edges);
    for (uint64_t g = lane; g < a.num_graphs; g += lanes) {
        uint32_t n = 0, E = 0;
        uint64_t e0 = 0;
        if (!graph_shape(a, g, n, e0, E)) continue;
        Sink sink(a.slots + g * a.slot_cap, a.slot_cap, a.lens[g]);
        SinkMsg m{0, &sink};  // Message::unflatten: head 0
        pu::Coder<SinkMsg> c{m, ANS_OK};
        int rc = pu::push_graph(c, st, n, a.loops != 0, kRedraws, edges + 2 * e0, E);
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

// ---- pop: graph g's pairs at edge_offsets[g] of edges
template <bool kRedraws>
__global__ __launch_bounds__(kThreads) void k_polya_pop(PolyaArgs a, uint32_t* __restrict__ edges) {
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    auto st = pu::State<LaneAcc>::make(LaneWs{a.ws + lane, lanes}, a.max_nodes, a.max_edges);
    for (uint64_t g = lane; g < a.num_graphs; g += lanes) {
        uint32_t n = 0, E = 0;
        uint64_t e0 = 0;
        if (!graph_shape(a, g, n, e0, E)) continue;
        RSource src{a.slots + g * a.slot_cap, a.slot_cap, a.lens[g], false, false};
        SourceMsg m{0, &src};  // Message::unflatten: head 0
        pu::Coder<SourceMsg> c{m, ANS_OK};
        int rc = pu::pop_graph(c, st, n, a.loops != 0, kRedraws, edges + 2 * e0, E);
        if (!rc) {
            flatten(m.head, [&](uint32_t byte) { src.unpop(byte & 0xFFu); });
            if (src.overflow || src.pos > 0xFFFFFFFFull) rc = ANS_E_LEN;
        }
        if (rc) {
            raise(a.status, rc);
            src.pos = 0;
        }
        a.lens[g] = static_cast<uint32_t>(src.pos);
    }
}

// ---- host side
int dev_polya(bool push, ans_gpu* g, int loops, int redraws, uint64_t num_graphs, const uint32_t* d_num_nodes,
              uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t max_nodes, uint64_t max_edges,
              uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, hipStream_t s) {
    unsigned grid = 0;
    uint32_t* ws = nullptr;
    if (max_edges > pu::kMaxEdges) return ANS_E_ARG;
    if (int rc = plan(g, num_graphs, pu::ws_entries(max_nodes, max_edges), grid, ws)) return rc;
    const PolyaArgs a{num_graphs, d_num_nodes, d_edge_offsets, max_nodes, max_edges, d_slots,
                      slot_cap,   d_lens,      d_status,       ws,        loops};
    g->last.clear();
    g->last.add(push ? kRecPolyaPush : kRecPolyaPop, 0, redraws != 0, rec_grid(grid));
    if (push) {
        if (redraws) k_polya_push<true><<<grid, kThreads, 0, s>>>(a, d_edges);
        else k_polya_push<false><<<grid, kThreads, 0, s>>>(a, d_edges);
    } else {
        if (redraws) k_polya_pop<true><<<grid, kThreads, 0, s>>>(a, d_edges);
        else k_polya_pop<false><<<grid, kThreads, 0, s>>>(a, d_edges);
    }
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}

// host buffers in and out (as ans_gpu_mset_*_var_chunks): the graphs' shapes checked on the host,
// the container expanded into slots with the slack of the largest graph, coded, packed
int host_polya(bool push, ans_gpu* g, int loops, int redraws, uint64_t num_graphs, const uint32_t* num_nodes,
               uint32_t* edges, const uint64_t* edge_offsets, const uint8_t* in, uint64_t in_len,
               const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
               uint64_t* lens, uint64_t* total) {
    *total = 0;
    if (num_graphs == 0) return ANS_OK;
    if (!num_nodes || !edge_offsets || !in_offsets || !in_lens || (in_len && !in)) return ANS_E_ARG;
    if (out && (!offsets || !lens)) return ANS_E_ARG;
    uint32_t max_nodes = 0;
    uint64_t max_edges = 0;
    for (uint64_t k = 0; k < num_graphs; ++k) {
        if (edge_offsets[k + 1] < edge_offsets[k]) return ANS_E_ARG;
        max_nodes = std::max(max_nodes, num_nodes[k]);
        max_edges = std::max(max_edges, edge_offsets[k + 1] - edge_offsets[k]);
    }
    const uint64_t num_edges = edge_offsets[num_graphs];
    if (max_edges > pu::kMaxEdges || (num_edges && !edges)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    Stage st;
    int rc = stage_in(g, edge_offsets, num_graphs, in, in_len, in_offsets, in_lens, pu::slack(max_nodes, max_edges), st);
    if (rc) return rc;
    DevBuf d_nodes, d_edges;
    HIP_TRY(d_nodes.alloc(4 * num_graphs));
    HIP_TRY(d_edges.alloc(8 * num_edges));
    HIP_TRY(hipMemcpyAsync(d_nodes.p, num_nodes, 4 * num_graphs, hipMemcpyHostToDevice, s));
    if (push && num_edges) HIP_TRY(hipMemcpyAsync(d_edges.p, edges, 8 * num_edges, hipMemcpyHostToDevice, s));
    uint32_t* d_status = st.d.status.as<uint32_t>();
    rc = dev_polya(push, g, loops, redraws, num_graphs, d_nodes.as<uint32_t>(), d_edges.as<uint32_t>(),
                   st.starts.as<uint64_t>(), max_nodes, max_edges, st.slots.as<uint8_t>(), st.cap,
                   st.d.lens.as<uint32_t>(), d_status, s);
    if (rc || (rc = read_status(g, d_status, s))) return rc;
    if (!push && num_edges) HIP_TRY(hipMemcpy(edges, d_edges.p, 8 * num_edges, hipMemcpyDeviceToHost));
    return download_container(g, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), num_graphs, s, out, out_cap,
                              offsets, lens, total);
}

bool dev_args_ok(const ans_gpu* g, uint64_t num_graphs, const uint32_t* d_num_nodes, const uint32_t* d_edges,
                 const uint64_t* d_edge_offsets, uint64_t max_edges, const uint8_t* d_slots, const uint32_t* d_lens,
                 const uint32_t* d_status) {
    return g && d_status && (!num_graphs || (d_num_nodes && d_edge_offsets && d_slots && d_lens && (d_edges || !max_edges)));
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

int ans_gpu_polya_slack(uint32_t max_nodes, uint64_t max_edges, uint64_t* bytes) try {
    if (!bytes || max_edges > pu::kMaxEdges) return ANS_E_ARG;
    *bytes = pu::slack(max_nodes, max_edges);
    return ANS_OK;
} ANS_CATCH

int ans_dev_polya_push(ans_gpu* g, int loops, int redraws, uint64_t num_graphs, const uint32_t* d_num_nodes,
                       const uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t max_nodes, uint64_t max_edges,
                       uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!dev_args_ok(g, num_graphs, d_num_nodes, d_edges, d_edge_offsets, max_edges, d_slots, d_lens, d_status))
        return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return dev_polya(true, g, loops, redraws, num_graphs, d_num_nodes, const_cast<uint32_t*>(d_edges), d_edge_offsets,
                     max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
} ANS_CATCH
int ans_dev_polya_pop(ans_gpu* g, int loops, int redraws, uint64_t num_graphs, const uint32_t* d_num_nodes,
                      uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t max_nodes, uint64_t max_edges,
                      uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!dev_args_ok(g, num_graphs, d_num_nodes, d_edges, d_edge_offsets, max_edges, d_slots, d_lens, d_status) ||
        slot_cap < 16)
        return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return dev_polya(false, g, loops, redraws, num_graphs, d_num_nodes, d_edges, d_edge_offsets, max_nodes, max_edges,
                     d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
} ANS_CATCH

int ans_gpu_polya_push_graphs(ans_gpu* g, int loops, int redraws, uint64_t num_graphs, const uint32_t* num_nodes,
                              const uint32_t* edges, const uint64_t* edge_offsets, const uint8_t* in, uint64_t in_len,
                              const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out, uint64_t out_cap,
                              uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !total) return ANS_E_ARG;
    return host_polya(true, g, loops, redraws, num_graphs, num_nodes, const_cast<uint32_t*>(edges), edge_offsets, in,
                      in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_polya_pop_graphs(ans_gpu* g, int loops, int redraws, uint64_t num_graphs, const uint32_t* num_nodes,
                             const uint64_t* edge_offsets, const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
                             const uint64_t* in_lens, uint32_t* out_edges, uint8_t* out, uint64_t out_cap,
                             uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !total) return ANS_E_ARG;
    return host_polya(false, g, loops, redraws, num_graphs, num_nodes, out_edges, edge_offsets, in, in_len, in_offsets,
                      in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH

}  // extern "C"
