// ans_arpu.hip — the autoregressive Pólya urn graph codecs in bulk, one graph per message, one lane
// per graph: Autoregressive(PolyaUrnSliceCodecs) and ShuffleCodec<PolyaUrnSliceCodecs,
// WLOrbitCodecs<GraphPrefix>> with wl_iter = 0 (src/recursive/mod.rs:117-216,
// src/recursive/graph/slice.rs:61-230, incomplete.rs:189-236) under the resume contract of
// include/ans_capi.h 4b. Graph g's message is Message::unflatten(slot bytes) with the Empty tail;
// the codec is ans_rgraph.hpp's recursion over ans_arpu.hpp's slices and ans_arer.hpp's counts, the
// same functions the host codec runs, on the exact 64-bit message ops of ans_exact.hpp; the
// per-lane loops and the host staging are ans_lane.hpp's.  A graph is a serial chain (two small
// uniform steps per node, an urn step and a permutation step per edge, an orbit step per node;
// Fenwick walks and a heapsort per large slice between them); the parallelism is across graphs.
// The per-lane state (ans_arpu.hpp PushState / PopState) lives in the context's workspace, entry i
// of lane l at i * lanes + l, sized by the lanes resident; the degrees' class ranks are the
// context's read-only table (as ans_arer.hip's).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ans_arpu.hpp"
#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_lane.hpp"

using namespace shuffle_coding::exact;
using namespace shuffle_coding::lane;
namespace ap = shuffle_coding::arpu;
namespace pu = shuffle_coding::polya;

namespace {

#define HIP_TRY(expr) ANS_HIP_TRY(expr)

// ---- grid-stride over the graphs, lane = one graph at a time (ans_lane.hpp's loops over the
// recursion of ans_rgraph.hpp)
template <int kOrbits>
__global__ __launch_bounds__(kThreads) void k_arpu_push(GraphArgs a, const uint32_t* __restrict__ edges,
                                                         uint32_t* __restrict__ perm) {
    const Lane l = Lane::mine();
    auto st = ap::PushState<LaneAcc, const uint32_t*>::make(l.ws(a.ws), a.max_nodes, a.max_edges, kOrbits, a.rank,
                                                            a.max_nodes + 1);
    push_loop(a, l, st, edges, perm);
}
template <int kOrbits>
__global__ __launch_bounds__(kThreads) void k_arpu_pop(GraphArgs a, uint32_t* __restrict__ edges,
                                                        uint32_t* __restrict__ num_edges) {
    const Lane l = Lane::mine();
    auto st = ap::PopState<LaneAcc, const uint32_t*>::make(l.ws(a.ws), a.max_nodes, a.max_edges, kOrbits, a.rank,
                                                           a.max_nodes + 1);
    pop_loop<false>(a, l, st, edges, num_edges);
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
    const GraphArgs a{num_graphs, d_num_nodes, d_edge_offsets, max_nodes, push ? max_edges : 0, d_slots, slot_cap, d_lens,
                      d_status, ws, loops, g->d_degree_rank, {}, 0, 0};
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

// host buffers in and out (ans_lane.hpp's staging).  max_edges: the largest graph's pairs on a push,
// its capacity on a pop (the slack's bound of what it can hold).
int host_arpu(bool push, ans_gpu* g, int loops, int orbits, uint64_t num_graphs, const uint32_t* num_nodes,
              uint32_t* edges, const uint64_t* edge_offsets, uint32_t* aux, const uint8_t* in, uint64_t in_len,
              const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
              uint64_t* lens, uint64_t* total) {
    *total = 0;
    if (!g || !orbits_ok(orbits)) return ANS_E_ARG;
    return host_graphs(
        push, g, PopEdges::kBounded, num_graphs, num_nodes, edges, edge_offsets, aux, in, in_len, in_offsets,
        in_lens, out, out_cap, offsets, lens, total,
        [&](uint32_t max_nodes, uint64_t max_edges) { return ap::slack(max_nodes, max_edges); },
        [&](auto... dev) { return dev_arpu(push, g, loops, orbits, num_graphs, dev...); });
}

bool dev_ok(const ans_gpu* g, int orbits, uint64_t num_graphs, const uint32_t* d_num_nodes,
            const uint64_t* d_edge_offsets, const uint8_t* d_slots, const uint32_t* d_lens, const uint32_t* d_status) {
    return dev_args_ok(g && orbits_ok(orbits), num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status);
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
    if (!dev_ok(g, orbits, num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status) ||
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
    if (!dev_ok(g, orbits, num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status) ||
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
