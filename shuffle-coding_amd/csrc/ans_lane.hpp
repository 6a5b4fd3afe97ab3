// ans_lane.hpp — what the one-lane-per-graph units (ans_polya.hip, ans_arer.hip, ans_arpu.hip) share:
// the lane-interleaved accessor of a per-graph array in the context's workspace, the message of a
// push (head + Sink) and of a pop (head + RSource) as polya::Coder takes it, the launch plan, and the
// context's table of the degrees' class ranks.  Device code and its host launchers; included by those
// units only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ans_arer.hpp"
#include "ans_ctx.hpp"
#include "ans_exact.hpp"

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

}  // namespace lane
}  // namespace shuffle_coding
