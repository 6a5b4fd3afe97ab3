// ans_scan.hpp — the single-workgroup exclusive scan shared by the host-buffer pipeline
// (ans_pipe.hip) and the edge-list compaction (ans_graph.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// out[i] = v[0] + ... + v[i-1] for i < n, by one workgroup of 1024 threads (n <= a few 10^5 per
// call): each thread sums a contiguous segment, the segment sums are scanned in LDS
// (Hillis-Steele), then each thread writes its segment's offsets.  Returns the total to every
// thread.
__device__ __forceinline__ uint64_t block_excl_scan(const uint32_t* __restrict__ v, uint64_t n,
                                                    uint64_t* __restrict__ out) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n + 1023) / 1024, b = t * per, e = b + per < n ? b + per : n;
    uint64_t sum = 0;
    for (uint64_t i = b; i < e; ++i) sum += v[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t x = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    for (uint64_t i = b; i < e; ++i) {
        out[i] = run;
        run += v[i];
    }
    return part[1023];
}

// The scan alone, its total at *total (which may be out + n).
__global__ __launch_bounds__(1024) void k_excl_scan(const uint32_t* __restrict__ v, uint64_t n,
                                                    uint64_t* __restrict__ out, uint64_t* total) {
    const uint64_t sum = block_excl_scan(v, n, out);
    if (threadIdx.x == 1023) *total = sum;
}

}  // namespace
