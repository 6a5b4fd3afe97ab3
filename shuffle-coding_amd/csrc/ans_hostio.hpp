// ans_hostio.hpp — host-side staging shared by the synchronous host-buffer entries of
// ans_kernels.hip, ans_pipe.hip, ans_codecs.hip and ans_graph.hip (host code only; the pipeline
// takes its argument checks and status read from here, its copies are its own):
// argument checks, the RAII device buffer, the decode head (chunk table checked and uploaded
// with the container) and the encode tail (slots packed into the caller's container).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ans_ctx.hpp"

namespace {

// symbol widths: the table kernels take u8 / u16 / u32, the 64-bit codecs u64 as well
inline bool valid_width_u32(int w) { return w == 1 || w == 2 || w == 4; }
inline bool valid_width_u64(int w) { return valid_width_u32(w) || w == 8; }
inline bool valid_kind(int k) { return k == ANS_GEN_ZEROS || k == ANS_GEN_EMPTY || k == ANS_GEN_RANDOM; }

// f(Sym{}) for the symbol type of a valid_width_u32 width: a generic lambda takes the value as a
// tag, [&](auto t) { return launch<decltype(t)>(...); }
template <class F>
auto with_sym_type(int sym_bytes, F&& f) {
    switch (sym_bytes) {
    case 1: return f(uint8_t{});
    case 2: return f(uint16_t{});
    default: return f(uint32_t{});
    }
}
// ... and of a valid_width_u64 width (the 64-bit codecs)
template <class F>
auto with_sym_type_u64(int sym_bytes, F&& f) {
    return sym_bytes == 8 ? f(uint64_t{}) : with_sym_type(sym_bytes, f);
}

// the lowest error code raised in a status word (bit k = code k)
inline int lowest_status(uint32_t bits) {
    for (int k = 1; k < 32; ++k)
        if (bits & (1u << k)) return k;
    return ANS_OK;
}

// ans_dev_status as one code: the call's own failure, else the lowest status raised on the device
inline int read_status(ans_gpu* g, const uint32_t* d_status, hipStream_t s) {
    int st = ANS_OK;
    const int rc = ans_dev_status(g, d_status, s, &st);
    return rc ? rc : st;
}

// Device buffer that frees itself.
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// The caller's u64 stream lengths as the kernels' u32, every stream inside the input
// (ANS_E_LEN otherwise); *max_len receives the longest.
inline int narrow_lens(const uint64_t* offsets, const uint64_t* lens, uint64_t nchunks, uint64_t in_len,
                       std::vector<uint32_t>& l32, uint64_t* max_len = nullptr) {
    l32.resize(nchunks);
    uint64_t longest = 0;
    for (uint64_t c = 0; c < nchunks; ++c) {
        if (lens[c] > 0xffffffffull || offsets[c] > in_len || lens[c] > in_len - offsets[c]) return ANS_E_LEN;
        l32[c] = static_cast<uint32_t>(lens[c]);
        longest = std::max(longest, lens[c]);
    }
    if (max_len) *max_len = longest;
    return ANS_OK;
}

// The decode head: a container and its chunk table on the device, and a zeroed status block of
// 16 bytes (the status word; the graph decoders keep an edge total in its second half).
// kInPad: decoders that read the container in place may fetch whole aligned 128-B lines around
// each stream (k_decode_g and the staged variable-chunk decoders of ans_kernels.hip; the fast
// decoders of ans_codecs.hip had the same slack), so the last stream can touch the line past its
// end.  It is the largest padding the entries used (16, 128 or 256); those that expand into
// slots first (ans_gpu_dense_set_decode) or read byte by byte need none of it.
constexpr size_t kInPad = 256;
struct DevStreams {
    DevBuf in, offs, lens, status;
};
inline int upload_streams(const uint8_t* in, uint64_t in_len, const uint64_t* offsets, const std::vector<uint32_t>& l32,
                          hipStream_t s, DevStreams& d) {
    const size_t nchunks = l32.size();
    ANS_HIP_TRY(d.in.alloc(in_len + kInPad));
    ANS_HIP_TRY(d.offs.alloc(8 * nchunks));
    ANS_HIP_TRY(d.lens.alloc(4 * nchunks));
    ANS_HIP_TRY(d.status.alloc(16));
    if (in_len) ANS_HIP_TRY(hipMemcpyAsync(d.in.p, in, in_len, hipMemcpyHostToDevice, s));
    if (nchunks) {
        ANS_HIP_TRY(hipMemcpyAsync(d.offs.p, offsets, 8 * nchunks, hipMemcpyHostToDevice, s));
        ANS_HIP_TRY(hipMemcpyAsync(d.lens.p, l32.data(), 4 * nchunks, hipMemcpyHostToDevice, s));
    }
    ANS_HIP_TRY(hipMemsetAsync(d.status.p, 0, 16, s));
    return ANS_OK;
}

// The encode tail: the streams of nchunks slots (lengths d_lens, written on stream s) packed
// into the caller's container.  *total is the container's exact size whatever the outcome;
// out == NULL is the size query; out_cap < *total is ANS_E_LEN with nothing else written.
inline int download_container(ans_gpu* g, const uint8_t* d_slots, uint64_t slot_cap, const uint32_t* d_lens,
                              uint64_t nchunks, hipStream_t s, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                              uint64_t* lens, uint64_t* total) {
    std::vector<uint32_t> hl(nchunks);
    if (nchunks) ANS_HIP_TRY(hipMemcpyAsync(hl.data(), d_lens, 4 * nchunks, hipMemcpyDeviceToHost, s));
    ANS_HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint64_t> off(nchunks);
    uint64_t acc = 0;
    for (uint64_t c = 0; c < nchunks; ++c) {
        off[c] = acc;
        acc += hl[c];
    }
    *total = acc;
    if (!out) return ANS_OK;
    if (out_cap < acc) return ANS_E_LEN;
    for (uint64_t c = 0; c < nchunks; ++c) {
        offsets[c] = off[c];
        lens[c] = hl[c];
    }
    if (!acc) return ANS_OK;
    DevBuf d_offs, d_out;
    ANS_HIP_TRY(d_offs.alloc(8 * nchunks));
    ANS_HIP_TRY(d_out.alloc(acc));
    ANS_HIP_TRY(hipMemcpyAsync(d_offs.p, off.data(), 8 * nchunks, hipMemcpyHostToDevice, s));
    const int rc = ans_dev_compact(g, d_slots, slot_cap, d_lens, d_offs.as<uint64_t>(), nchunks, d_out.as<uint8_t>(), s);
    if (rc) return rc;
    ANS_HIP_TRY(hipMemcpyAsync(out, d_out.p, acc, hipMemcpyDeviceToHost, s));
    ANS_HIP_TRY(hipStreamSynchronize(s));
    return ANS_OK;
}

// The resume head of the host-buffer push / pop entries of ans_mset.hip and ans_polya.hip: the
// dense container in, expanded into slots of the longest stream + grow bytes (rounded to 128) on
// the context's stream, with the chunk table, a zeroed status block and, when given, the nchunks + 1
// chunk starts.
struct Stage {
    DevStreams d;
    DevBuf slots, starts;
    uint64_t cap = 0;
};
inline int stage_in(ans_gpu* g, const uint64_t* starts, uint64_t nchunks, const uint8_t* in, uint64_t in_len,
                    const uint64_t* in_offsets, const uint64_t* in_lens, uint64_t grow, Stage& st) {
    std::vector<uint32_t> l32;
    uint64_t lmax = 0;
    int rc = narrow_lens(in_offsets, in_lens, nchunks, in_len, l32, &lmax);
    if (rc) return rc;
    st.cap = (lmax + grow + 127) & ~uint64_t(127);
    const hipStream_t s = g->stream;
    if ((rc = upload_streams(in, in_len, in_offsets, l32, s, st.d))) return rc;
    ANS_HIP_TRY(st.slots.alloc(nchunks * st.cap));
    if (starts) {
        ANS_HIP_TRY(st.starts.alloc(8 * (nchunks + 1)));
        ANS_HIP_TRY(hipMemcpyAsync(st.starts.p, starts, 8 * (nchunks + 1), hipMemcpyHostToDevice, s));
    }
    return ans_dev_expand(g, st.d.in.as<uint8_t>(), st.d.offs.as<uint64_t>(), st.d.lens.as<uint32_t>(), nchunks,
                          st.slots.as<uint8_t>(), st.cap, s);
}
}  // namespace
