// ans_lane.hpp — what the one-lane-per-graph units share.  All five (ans_polya.hip, ans_arer.hip,
// ans_arpu.hip, ans_wl.hip, ans_wl_labelled.hip): the lane-interleaved accessor of a per-graph array
// in the context's workspace, the message of a push (head + Sink) and of a pop (head + RSource) as
// polya::Coder takes it, and the launch plan.  The four units of the recursion of ans_rgraph.hpp
// (ans_arer.hip, ans_arpu.hip, ans_wl.hip, ans_wl_labelled.hip) beside: the kernels' arguments, a
// graph's shape check, the per-lane push and pop loops, the host staging and the argument checks of
// the entry points, and the context's table of the degrees' class ranks.  Device code and its host
// launchers; included by those units only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ans_arer.hpp"
#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_hostio.hpp"

namespace shuffle_coding {
namespace lane {

constexpr size_t kWsMax = size_t(256) << 20;  // the workspace never passes this (as ans_mset.hip's)

// entry i of this lane's array: a wave on one entry reads 64 consecutive dwords
struct LaneAcc {
    uint32_t* p;
    uint64_t stride;
    __device__ uint32_t load(uint32_t i) const { return p[i * stride]; }
    __device__ void store(uint32_t i, uint32_t v) { p[i * stride] = v; }
};
// the arrays of a state, one after the other: at(offset, count) is `count` entries from `offset` on
// (the count is for accessors that check it; this one does not)
struct LaneWs {
    uint32_t* p;  // the workspace + the lane
    uint64_t lanes;
    __device__ LaneAcc at(uint64_t o, uint64_t = 0) const { return LaneAcc{p + o * lanes, lanes}; }
};

// the message of a push: head + the sink (the renorm of k_mset_push)
struct SinkMsg {
    uint64_t head;
    exact::Sink* sink;
    __device__ bool renorm(uint64_t min_head) {
        while (head < min_head) {
            uint32_t byte = 0;
            if (!sink->pop(byte)) return false;  // src/ans.rs:144
            head = (head << 8) | byte;
        }
        while ((head >> 8) >= min_head) {
            sink->put(static_cast<uint32_t>(head));
            head >>= 8;
        }
        return true;
    }
};
// ... and of a pop: head + the resumed source
struct SourceMsg {
    uint64_t head;
    exact::RSource* src;
    __device__ bool renorm(uint64_t min_head) {
        while (head < min_head && src->pull(head)) {}
        if (head < min_head) return false;
        while ((head >> 8) >= min_head) {
            src->unpop(static_cast<uint32_t>(head) & 0xFFu);
            head >>= 8;
        }
        return true;
    }
};

inline hipStream_t stream_of(const ans_gpu* g, void* stream) {
    return stream ? static_cast<hipStream_t>(stream) : g->stream;
}

// The launch: as many lanes as the device holds at two waves per SIMD, fewer while their state
// (`entries` dwords a lane) passes kWsMax; ANS_E_ARG when one wave's does.
inline int plan(ans_gpu* g, uint64_t num_graphs, uint64_t entries, unsigned& grid, uint32_t*& ws) {
    const size_t per_wave = size_t(4) * exact::kThreads * entries;
    if (per_wave > kWsMax) return ANS_E_ARG;
    const uint64_t blocks = (num_graphs + exact::kThreads - 1) / exact::kThreads;
    const uint64_t want = std::min<uint64_t>({blocks, static_cast<uint64_t>(g->ncu) * 8, kWsMax / per_wave});
    const size_t bytes = per_wave * want;
    if (g->cap_mset_ws < bytes) {  // the multiset kernels' workspace: one at a time uses it
        if (g->d_mset_ws) (void)hipFree(g->d_mset_ws);  // (waits for the kernels that use it)
        g->d_mset_ws = nullptr;
        g->cap_mset_ws = 0;
        ANS_HIP_TRY(hipMalloc(&g->d_mset_ws, bytes));
        g->cap_mset_ws = bytes;
    }
    ws = static_cast<uint32_t*>(g->d_mset_ws);
    grid = static_cast<unsigned>(want);
    return ANS_OK;
}

// The class ranks of the degrees 0 .. max_nodes on the device (arer::build_degree_ranks): kept by the
// context, rebuilt (sorted on the host, uploaded) when max_nodes changes.  The free waits for the
// kernels that read the old one.
inline int degree_ranks(ans_gpu* g, uint32_t max_nodes) {
    if (g->d_degree_rank && g->n_degree_rank == max_nodes + 1) return ANS_OK;
    std::vector<uint32_t> rank;
    if (!arer::build_degree_ranks(max_nodes, rank)) return ANS_E_ARG;
    if (g->d_degree_rank) (void)hipFree(g->d_degree_rank);
    g->d_degree_rank = nullptr;
    g->n_degree_rank = 0;
    ANS_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->d_degree_rank), 4 * rank.size()));
    ANS_HIP_TRY(hipMemcpy(g->d_degree_rank, rank.data(), 4 * rank.size(), hipMemcpyHostToDevice));
    g->n_degree_rank = max_nodes + 1;
    return ANS_OK;
}

inline bool orbits_ok(int orbits) {
    return orbits == ANS_ORBITS_NONE || orbits == ANS_ORBITS_ONE_CLASS || orbits == ANS_ORBITS_DEGREE;
}
inline bool table_ok(const ans_gpu_table* gt) { return gt && gt->g && gt->t.nsym == 2; }

// ---- the units of the recursion: one kernel argument block (a unit leaves what it does not read zero)
struct GraphArgs {
    uint64_t num_graphs;
    const uint32_t* num_nodes;
    const uint64_t* edge_offsets;
    uint32_t max_nodes;
    uint64_t max_edges;  // the bound of a graph's pairs in the state (nbr; next on a pop with WL orbits)
    uint8_t* slots;
    uint64_t slot_cap;
    uint32_t* lens;
    uint32_t* status;
    uint32_t* ws;
    int loops;
    const uint32_t* rank;  // class ranks of the degrees 0 .. max_nodes (the count stage under DEGREE)
    arer::Bern bern;       // (the Erdős–Rényi slices)
    uint32_t wl_iter;      // (the WL stage)
    int half_iter;
};

// this thread's lane among the launch's, and its entries of the workspace
struct Lane {
    uint64_t id, count;
    __device__ static Lane mine() {
        return Lane{static_cast<uint64_t>(blockIdx.x) * exact::kThreads + threadIdx.x,
                    static_cast<uint64_t>(gridDim.x) * exact::kThreads};
    }
    __device__ LaneWs ws(uint32_t* p) const { return LaneWs{p + id, count}; }
};

// graph g's shape, checked: false (ANS_E_ARG / ANS_E_LEN raised, lens[g] = 0) when it is not coded.
// A push holds the graph's pairs in its state, so they are bounded; a pop's range is a capacity, of
// which a state that keeps the decoded pairs (kPopRoomBounded) holds max_edges at the most.
template <bool kPush, bool kPopRoomBounded>
__device__ bool graph_shape(const GraphArgs& a, uint64_t g, uint32_t& n, uint64_t& e0, uint64_t& room) {
    n = a.num_nodes[g];
    e0 = a.edge_offsets[g];
    const uint64_t e1 = a.edge_offsets[g + 1];
    int code = ANS_OK;
    if (e1 < e0 || (kPush && e1 - e0 > a.max_edges) || n > a.max_nodes) code = ANS_E_ARG;
    else if (a.lens[g] > a.slot_cap) code = ANS_E_LEN;
    if (code) {
        exact::raise(a.status, code);
        a.lens[g] = 0;
        return false;
    }
    room = e1 - e0;
    if (kPopRoomBounded && room > a.max_edges) room = a.max_edges;
    return true;
}

// ---- push: grid-stride over the graphs, lane = one graph at a time.  st: an rgraph::PushState;
// begin(g, e0): what else the state needs of graph g, whose pairs start at e0 (its labels).
struct NoBegin {
    __device__ void operator()(uint64_t, uint64_t) const {}
};
template <class St, class Begin = NoBegin>
__device__ void push_loop(const GraphArgs& a, const Lane& l, St& st, const uint32_t* edges, uint32_t* perm,
                          Begin&& begin = Begin{}) {
    for (uint64_t g = l.id; g < a.num_graphs; g += l.count) {
        uint32_t n = 0;
        uint64_t e0 = 0, E = 0;
        if (!graph_shape<true, false>(a, g, n, e0, E)) continue;
        begin(g, e0);
        exact::Sink sink(a.slots + g * a.slot_cap, a.slot_cap, a.lens[g]);
        SinkMsg m{0, &sink};  // Message::unflatten: head 0
        polya::Coder<SinkMsg> c{m, ANS_OK};
        int rc = rgraph::push_graph(c, st, n, a.loops != 0, edges + 2 * e0, static_cast<uint32_t>(E),
                                    perm ? perm + g * a.max_nodes : nullptr);
        uint64_t len = 0;
        if (!rc) {
            exact::flatten(m.head, [&](uint32_t byte) { sink.put(byte); });
            len = sink.finish();
            if (sink.overflow || len > 0xFFFFFFFFull) rc = ANS_E_LEN;
        }
        if (rc) {
            exact::raise(a.status, rc);
            len = 0;
        }
        a.lens[g] = static_cast<uint32_t>(len);
    }
}

// ---- pop: graph g's pairs from edge_offsets[g] of edges on, their number in num_edges[g].  st: an
// rgraph::PopState; begin as a push's.
template <bool kRoomBounded, class St, class Begin = NoBegin>
__device__ void pop_loop(const GraphArgs& a, const Lane& l, St& st, uint32_t* edges, uint32_t* num_edges,
                         Begin&& begin = Begin{}) {
    for (uint64_t g = l.id; g < a.num_graphs; g += l.count) {
        uint32_t n = 0;
        uint64_t e0 = 0, cap = 0, count = 0;
        if (!graph_shape<false, kRoomBounded>(a, g, n, e0, cap)) {
            num_edges[g] = 0;
            continue;
        }
        begin(g, e0);
        exact::RSource src{a.slots + g * a.slot_cap, a.slot_cap, a.lens[g], false, false};
        SourceMsg m{0, &src};  // Message::unflatten: head 0
        polya::Coder<SourceMsg> c{m, ANS_OK};
        int rc = rgraph::pop_graph(c, st, n, a.loops != 0, edges + 2 * e0, cap, &count);
        if (!rc) {
            exact::flatten(m.head, [&](uint32_t byte) { src.unpop(byte & 0xFFu); });
            if (src.overflow || src.pos > 0xFFFFFFFFull) rc = ANS_E_LEN;
        }
        if (rc) {
            exact::raise(a.status, rc);
            src.pos = 0;
            count = 0;
        }
        a.lens[g] = static_cast<uint32_t>(src.pos);
        num_edges[g] = static_cast<uint32_t>(count);
    }
}

// ---- host side.  The device pointers every dev entry point of these units needs (`ok`: its own
// checks of the context and the setting).
inline bool dev_args_ok(bool ok, uint64_t num_graphs, const uint32_t* d_num_nodes, const uint64_t* d_edge_offsets,
                        const uint8_t* d_slots, const uint32_t* d_lens, const uint32_t* d_status) {
    return ok && d_status && (!num_graphs || (d_num_nodes && d_edge_offsets && d_slots && d_lens));
}

// Host buffers in and out: the graphs' shapes checked on the host, the container expanded into slots
// with the slack of the largest graph, coded, packed.  The caller has set *total = 0 and checked its
// context and setting.  pop_edges: whether a pop's capacities size its state (and so are bounded as
// a push's pairs are); slack(max_nodes, max_edges) the bytes a message can grow by;
// launch(d_num_nodes, d_edges, d_edge_offsets, d_aux, max_nodes, max_edges, d_slots, slot_cap,
// d_lens, d_status, stream) the unit's dev launcher.  aux: a push's perm (optional), a pop's
// num_edges.
enum class PopEdges { kUnbounded, kBounded };
template <class Slack, class Launch>
int host_graphs(bool push, ans_gpu* g, PopEdges pop_edges, uint64_t num_graphs, const uint32_t* num_nodes,
                uint32_t* edges, const uint64_t* edge_offsets, uint32_t* aux, const uint8_t* in, uint64_t in_len,
                const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                uint64_t* lens, uint64_t* total, Slack&& slack, Launch&& launch) {
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
    if (max_nodes > 0x7FFFFFFFu || ((push || pop_edges == PopEdges::kBounded) && max_edges > arer::kMaxEdges) || (num_edges && !edges))
        return ANS_E_ARG;
    ANS_HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    Stage st;
    int rc = stage_in(g, edge_offsets, num_graphs, in, in_len, in_offsets, in_lens, slack(max_nodes, max_edges), st);
    if (rc) return rc;
    const uint64_t aux_entries = push ? num_graphs * max_nodes : num_graphs;
    DevBuf d_nodes, d_edges, d_aux;
    ANS_HIP_TRY(d_nodes.alloc(4 * num_graphs));
    ANS_HIP_TRY(d_edges.alloc(8 * num_edges));
    if (aux) ANS_HIP_TRY(d_aux.alloc(4 * aux_entries));
    ANS_HIP_TRY(hipMemcpyAsync(d_nodes.p, num_nodes, 4 * num_graphs, hipMemcpyHostToDevice, s));
    if (push && num_edges) ANS_HIP_TRY(hipMemcpyAsync(d_edges.p, edges, 8 * num_edges, hipMemcpyHostToDevice, s));
    if (push && aux) ANS_HIP_TRY(hipMemsetAsync(d_aux.p, 0, 4 * aux_entries, s));  // (the entries past a graph's nodes)
    uint32_t* d_status = st.d.status.as<uint32_t>();
    rc = launch(d_nodes.as<uint32_t>(), d_edges.as<uint32_t>(), st.starts.as<uint64_t>(), aux ? d_aux.as<uint32_t>() : nullptr,
                max_nodes, max_edges, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), d_status, s);
    if (rc || (rc = read_status(g, d_status, s))) return rc;
    if (!push && num_edges) ANS_HIP_TRY(hipMemcpy(edges, d_edges.p, 8 * num_edges, hipMemcpyDeviceToHost));
    if (aux && aux_entries) ANS_HIP_TRY(hipMemcpy(aux, d_aux.p, 4 * aux_entries, hipMemcpyDeviceToHost));
    return download_container(g, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), num_graphs, s, out, out_cap,
                              offsets, lens, total);
}

}  // namespace lane
}  // namespace shuffle_coding
