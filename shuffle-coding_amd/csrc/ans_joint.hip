// ans_joint.hip — joint shuffle coding of graphs with Weisfeiler-Lehman orbits in bulk, one graph per
// message, one lane per graph: ShuffleCodec<JointSliceCodecs<C>, WLOrbitCodecs<JointPrefix<Graph>>>
// (src/recursive/joint.rs, src/recursive/mod.rs:117-148, src/recursive/graph/incomplete.rs:154-187)
// with C the dense Erdős–Rényi indicator or the ordered Pólya urn, under the resume contract of
// include/ans_capi.h 4b, as ans_wl.hip has the recursive form.  The codec is ans_joint.hpp's over
// ans_wl.hpp's orbit stage and ans_polya.hpp's urn, the same functions the host codec runs, on the
// exact 64-bit message ops of ans_exact.hpp; the per-lane loops and the host staging are ans_lane.hpp's.
// The per-lane state (ans_joint.hpp ErPush / ErPop / PuPush / PuPop: the prefix graph or the decoded
// adjacency, the orbit stage, and over it the ordered urn's arrays) lives in the context's workspace,
// entry i of lane l at i * lanes + l, sized by the lanes resident; wl_iter, half_iter and redraws are
// runtime arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ans_joint.hpp"  // (before ans_lane.hpp: its loops find the joint states' push_graph / pop_graph)

#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_lane.hpp"

using namespace shuffle_coding::exact;
using namespace shuffle_coding::lane;
namespace ar = shuffle_coding::arer;
namespace jt = shuffle_coding::joint;
namespace pu = shuffle_coding::polya;
namespace wl = shuffle_coding::wl;

namespace {

#define HIP_TRY(expr) ANS_HIP_TRY(expr)

// ---- grid-stride over the graphs, lane = one graph at a time (ans_lane.hpp's loops over the codecs of
// ans_joint.hpp).  (edges is written by a pop and read back by its adjacency, so it is not
// __restrict__ there.)  A pop's range of edges is a capacity under the Erdős–Rényi codec and the
// graph's pair count under the urn; the state bounds either (ans_joint.hpp pop_joint).
__global__ __launch_bounds__(kThreads) void k_joint_er_push(GraphArgs a, const uint32_t* __restrict__ edges,
                                                             uint32_t* __restrict__ perm) {
    const Lane l = Lane::mine();
    auto st = jt::ErPush<LaneAcc>::make(l.ws(a.ws), a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    st.bern = a.bern;
    push_loop(a, l, st, edges, perm);
}
__global__ __launch_bounds__(kThreads) void k_joint_er_pop(GraphArgs a, uint32_t* edges, uint32_t* __restrict__ num_edges) {
    const Lane l = Lane::mine();
    auto st = jt::ErPop<LaneAcc>::make(l.ws(a.ws), a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    st.bern = a.bern;
    pop_loop<false>(a, l, st, edges, num_edges);
}
__global__ __launch_bounds__(kThreads) void k_joint_pu_push(GraphArgs a, int redraws, const uint32_t* __restrict__ edges,
                                                             uint32_t* __restrict__ perm) {
    const Lane l = Lane::mine();
    auto st = jt::PuPush<LaneAcc>::make(l.ws(a.ws), a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    st.redraws = redraws != 0;
    push_loop(a, l, st, edges, perm);
}
__global__ __launch_bounds__(kThreads) void k_joint_pu_pop(GraphArgs a, int redraws, uint32_t* edges,
                                                            uint32_t* __restrict__ num_edges) {
    const Lane l = Lane::mine();
    auto st = jt::PuPop<LaneAcc>::make(l.ws(a.ws), a.max_nodes, a.max_edges, a.wl_iter, a.half_iter != 0);
    st.redraws = redraws != 0;
    pop_loop<false>(a, l, st, edges, num_edges);
}

// ---- host side.  gt: the Bernoulli of the Erdős–Rényi codec, null for the urn (which reads redraws).
bool wl_ok(int wl_iter) { return wl_iter >= 0 && wl_iter <= static_cast<int>(wl::kMaxIter); }

int dev_joint(bool push, ans_gpu* g, const ans_gpu_table* gt, int loops, int redraws, int wl_iter, int half_iter,
              uint64_t num_graphs, const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets,
              uint32_t* d_aux, uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
              uint32_t* d_status, hipStream_t s) {
    const uint32_t w = static_cast<uint32_t>(wl_iter);
    if (!wl::nodes_ok(max_nodes, w) || max_edges > ar::kMaxEdges) return ANS_E_ARG;
    const uint64_t entries = gt ? (push ? jt::er_push_entries(max_nodes, max_edges, w) : jt::er_pop_entries(max_nodes, max_edges, w))
                                : (push ? jt::pu_push_entries(max_nodes, max_edges, w) : jt::pu_pop_entries(max_nodes, max_edges, w));
    unsigned grid = 0;
    uint32_t* ws = nullptr;
    if (int rc = plan(g, num_graphs, entries, grid, ws)) return rc;
    const GraphArgs a{num_graphs, d_num_nodes, d_edge_offsets, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, ws,
                      loops, nullptr, gt ? ar::bern_of(gt->mass2[0], gt->mass2[1]) : ar::Bern{}, w, half_iter != 0};
    g->last.clear();
    g->last.add(gt ? (push ? kRecJointErPush : kRecJointErPop) : (push ? kRecJointPuPush : kRecJointPuPop), 0, wl_iter,
                rec_grid(grid), half_iter != 0, redraws != 0);
    if (gt) {
        if (push) k_joint_er_push<<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
        else k_joint_er_pop<<<grid, kThreads, 0, s>>>(a, d_edges, d_aux);
    } else {
        if (push) k_joint_pu_push<<<grid, kThreads, 0, s>>>(a, redraws, d_edges, d_aux);
        else k_joint_pu_pop<<<grid, kThreads, 0, s>>>(a, redraws, d_edges, d_aux);
    }
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}

// host buffers in and out (ans_lane.hpp's staging) with the slack of ans_joint.hpp
int host_joint(bool push, ans_gpu* g, const ans_gpu_table* gt, int loops, int redraws, int wl_iter, int half_iter,
               uint64_t num_graphs, const uint32_t* num_nodes, uint32_t* edges, const uint64_t* edge_offsets, uint32_t* aux,
               const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out,
               uint64_t out_cap, uint64_t* offsets, uint64_t* lens, uint64_t* total) {
    *total = 0;
    if (!g || !wl_ok(wl_iter)) return ANS_E_ARG;
    return host_graphs(
        push, g, PopEdges::kBounded, num_graphs, num_nodes, edges, edge_offsets, aux, in, in_len, in_offsets, in_lens,
        out, out_cap, offsets, lens, total,
        [&](uint32_t max_nodes, uint64_t max_edges) {
            return gt ? jt::er_slack(ar::bern_of(gt->mass2[0], gt->mass2[1]), max_nodes, loops != 0)
                      : jt::pu_slack(max_nodes, max_edges);
        },
        [&](auto... dev) { return dev_joint(push, g, gt, loops, redraws, wl_iter, half_iter, num_graphs, dev...); });
}

bool dev_ok(const ans_gpu* g, int wl_iter, uint64_t num_graphs, const uint32_t* d_num_nodes,
            const uint64_t* d_edge_offsets, const uint8_t* d_slots, const uint32_t* d_lens, const uint32_t* d_status) {
    return dev_args_ok(g && wl_ok(wl_iter), num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status);
}

int dev_push(ans_gpu* g, const ans_gpu_table* gt, int loops, int redraws, int wl_iter, int half_iter, uint64_t num_graphs,
             const uint32_t* d_num_nodes, const uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t max_nodes,
             uint64_t max_edges, uint32_t* d_perm, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
             uint32_t* d_status, void* stream) {
    if (!dev_ok(g, wl_iter, num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status) ||
        (num_graphs && max_edges && !d_edges))
        return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return dev_joint(true, g, gt, loops, redraws, wl_iter, half_iter, num_graphs, d_num_nodes, const_cast<uint32_t*>(d_edges),
                     d_edge_offsets, d_perm, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
}
int dev_pop(ans_gpu* g, const ans_gpu_table* gt, int loops, int redraws, int wl_iter, int half_iter, uint64_t num_graphs,
            const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets, uint32_t* d_num_edges,
            uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
            uint32_t* d_status, void* stream) {
    if (!dev_ok(g, wl_iter, num_graphs, d_num_nodes, d_edge_offsets, d_slots, d_lens, d_status) ||
        (num_graphs && (!d_edges || !d_num_edges)) || slot_cap < 16)
        return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return dev_joint(false, g, gt, loops, redraws, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets,
                     d_num_edges, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

int ans_gpu_joint_er_slack(const ans_gpu_table* gt, uint32_t max_nodes, int loops, uint64_t* bytes) try {
    if (!bytes || !table_ok(gt)) return ANS_E_ARG;
    *bytes = jt::er_slack(ar::bern_of(gt->mass2[0], gt->mass2[1]), max_nodes, loops != 0);
    return ANS_OK;
} ANS_CATCH
int ans_gpu_joint_polya_slack(uint32_t max_nodes, uint64_t max_edges, uint64_t* bytes) try {
    if (!bytes || max_edges > pu::kMaxEdges) return ANS_E_ARG;
    *bytes = jt::pu_slack(max_nodes, max_edges);
    return ANS_OK;
} ANS_CATCH

int ans_dev_joint_er_wl_push(ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                             const uint32_t* d_num_nodes, const uint32_t* d_edges, const uint64_t* d_edge_offsets,
                             uint32_t max_nodes, uint64_t max_edges, uint32_t* d_perm, uint8_t* d_slots, uint64_t slot_cap,
                             uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!table_ok(gt)) return ANS_E_ARG;
    return dev_push(gt->g, gt, loops, 0, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets, max_nodes,
                    max_edges, d_perm, d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH
int ans_dev_joint_er_wl_pop(ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                            const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets,
                            uint32_t* d_num_edges, uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots,
                            uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!table_ok(gt)) return ANS_E_ARG;
    return dev_pop(gt->g, gt, loops, 0, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets, d_num_edges,
                   max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH
int ans_dev_joint_polya_wl_push(ans_gpu* g, int loops, int redraws, int wl_iter, int half_iter, uint64_t num_graphs,
                                const uint32_t* d_num_nodes, const uint32_t* d_edges, const uint64_t* d_edge_offsets,
                                uint32_t max_nodes, uint64_t max_edges, uint32_t* d_perm, uint8_t* d_slots,
                                uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    return dev_push(g, nullptr, loops, redraws, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets,
                    max_nodes, max_edges, d_perm, d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH
int ans_dev_joint_polya_wl_pop(ans_gpu* g, int loops, int redraws, int wl_iter, int half_iter, uint64_t num_graphs,
                               const uint32_t* d_num_nodes, uint32_t* d_edges, const uint64_t* d_edge_offsets,
                               uint32_t* d_num_edges, uint32_t max_nodes, uint64_t max_edges, uint8_t* d_slots,
                               uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    return dev_pop(g, nullptr, loops, redraws, wl_iter, half_iter, num_graphs, d_num_nodes, d_edges, d_edge_offsets,
                   d_num_edges, max_nodes, max_edges, d_slots, slot_cap, d_lens, d_status, stream);
} ANS_CATCH

int ans_gpu_joint_er_wl_push_graphs(ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                    const uint32_t* num_nodes, const uint32_t* edges, const uint64_t* edge_offsets,
                                    const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
                                    const uint64_t* in_lens, uint32_t* perm, uint8_t* out, uint64_t out_cap,
                                    uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total || !table_ok(gt)) return ANS_E_ARG;
    return host_joint(true, gt->g, gt, loops, 0, wl_iter, half_iter, num_graphs, num_nodes, const_cast<uint32_t*>(edges),
                      edge_offsets, perm, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_joint_er_wl_pop_graphs(ans_gpu_table* gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                   const uint32_t* num_nodes, const uint64_t* edge_offsets, const uint8_t* in,
                                   uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens,
                                   uint32_t* out_edges, uint32_t* out_num_edges, uint8_t* out, uint64_t out_cap,
                                   uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total || !table_ok(gt)) return ANS_E_ARG;
    return host_joint(false, gt->g, gt, loops, 0, wl_iter, half_iter, num_graphs, num_nodes, out_edges, edge_offsets,
                      out_num_edges, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_joint_polya_wl_push_graphs(ans_gpu* g, int loops, int redraws, int wl_iter, int half_iter, uint64_t num_graphs,
                                       const uint32_t* num_nodes, const uint32_t* edges, const uint64_t* edge_offsets,
                                       const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
                                       const uint64_t* in_lens, uint32_t* perm, uint8_t* out, uint64_t out_cap,
                                       uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total) return ANS_E_ARG;
    return host_joint(true, g, nullptr, loops, redraws, wl_iter, half_iter, num_graphs, num_nodes,
                      const_cast<uint32_t*>(edges), edge_offsets, perm, in, in_len, in_offsets, in_lens, out, out_cap, offsets,
                      lens, total);
} ANS_CATCH
int ans_gpu_joint_polya_wl_pop_graphs(ans_gpu* g, int loops, int redraws, int wl_iter, int half_iter, uint64_t num_graphs,
                                      const uint32_t* num_nodes, const uint64_t* edge_offsets, const uint8_t* in,
                                      uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens,
                                      uint32_t* out_edges, uint32_t* out_num_edges, uint8_t* out, uint64_t out_cap,
                                      uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!total) return ANS_E_ARG;
    return host_joint(false, g, nullptr, loops, redraws, wl_iter, half_iter, num_graphs, num_nodes, out_edges, edge_offsets,
                      out_num_edges, in, in_len, in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH

}  // extern "C"
