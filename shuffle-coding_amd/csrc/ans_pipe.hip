// ans_pipe.hip — the host-buffer pipeline: ans_gpu_encode_chunks / ans_gpu_decode_chunks take
// host symbols and a host dense container and run as batches of chunks whose copies and kernels
// overlap, through a workspace that persists in the context.  Host code and the
// batch length scan only: the coder kernels come from the launch units (ans_launch.hpp), the
// slot compaction from ans_kernels.hip through ans_dev_compact.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ans_hostio.hpp"
#include "ans_launch.hpp"
#include "ans_scan.hpp"

using namespace shuffle_coding::launch;

// Batches of chunks flow through kPipeDepth workspace slots, so that the H2D copy of batch b+1,
// the kernels of batch b and the D2H copy of batch b-1 overlap.  Kernels alternate between
// two compute streams (the context's and s_comp2): a batch's kernels occupy few CUs for about
// one chain latency (~1 ms for 4096-symbol chunks), so consecutive batches must overlap too.
// The three pipeline streams each get a hardware queue of their own (CU-masked queues are
// never shared; own_queue_stream).  The workspace persists in the context and grows on demand.
constexpr int kPipeDepthMax = 8;  // workspace slots: ANS_PIPE_DEPTH (default kPipeDepth) at creation
constexpr int kPipeDepth = 6;
struct PipeSlot {
    void* d_syms = nullptr;     // batch symbols
    uint8_t* d_slots = nullptr; // batch streams in the slot layout
    uint8_t* d_dense = nullptr; // batch streams, dense (encode output / decode input)
    uint32_t* d_lens = nullptr;
    uint64_t* d_offs = nullptr;  // batch offsets (+ total at [nchunks] after encode)
    uint32_t* h_lens = nullptr;  // pinned staging
    uint64_t* h_offs = nullptr;  // pinned staging
    hipEvent_t ev_in = nullptr, ev_comp = nullptr, ev_meta = nullptr, ev_out = nullptr;
    bool used = false;
};
struct HostPipe {
    hipStream_t s_in = nullptr, s_out = nullptr, s_comp2 = nullptr;
    PipeSlot slot[kPipeDepthMax];
    int depth = kPipeDepth;  // slots in use
    uint32_t* d_status = nullptr;
    size_t cap_syms = 0, cap_slots = 0, cap_dense = 0, cap_chunks = 0;  // per slot
};

namespace {

#define HIP_TRY ANS_HIP_TRY

constexpr int kPipeScattered = -1;

// the workspace slots in use
struct SlotRange {
    PipeSlot* a;
    PipeSlot* b;
    PipeSlot* begin() const { return a; }
    PipeSlot* end() const { return b; }
};
inline SlotRange slots_of(HostPipe* p) { return {p->slot, p->slot + p->depth}; }

void pipe_release(HostPipe* p) {
    for (PipeSlot& s : slots_of(p)) {
        (void)hipFree(s.d_syms);
        (void)hipFree(s.d_slots);
        (void)hipFree(s.d_dense);
        (void)hipFree(s.d_lens);
        (void)hipFree(s.d_offs);
        (void)hipHostFree(s.h_lens);
        (void)hipHostFree(s.h_offs);
        s.d_syms = nullptr;
        s.d_slots = s.d_dense = nullptr;
        s.d_lens = nullptr;
        s.d_offs = nullptr;
        s.h_lens = nullptr;
        s.h_offs = nullptr;
        s.used = false;
    }
    p->cap_syms = p->cap_slots = p->cap_dense = p->cap_chunks = 0;
}

// A stream on a hardware queue of its own, its kernels restricted to the CUs of `pattern`
// (repeated over the mask words): a CU-masked queue is never shared.  The runtime moves
// device-to-host bytes with blit kernels on the copy stream's queue; with GPU_MAX_HW_QUEUES = 4
// and five streams in the process that queue was shared with the second compute stream, whose
// decode kernels then waited for every blit (tools/host_timeline.py), and a blit spread over
// all CUs leaves none free for a decode workgroup (which fills a CU's VGPRs and LDS).
hipError_t own_queue_stream(hipStream_t* s, uint32_t pattern) {
    int dev = 0, ncu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess || ncu <= 0) return e != hipSuccess ? e : hipErrorInvalidDevice;
    std::vector<uint32_t> mask((ncu + 31) / 32, pattern);
    if (ncu % 32) mask.back() &= (1u << (ncu % 32)) - 1u;
    return hipExtStreamCreateWithCUMask(s, static_cast<uint32_t>(mask.size()), mask.data());
}

// The context's pipeline with per-slot room for `syms` symbol bytes, `slots` slot bytes,
// `dense` dense bytes and `chunks` chunks (reallocated, after draining, when it must grow),
// its slots unused and its status word cleared: a call's opening.
int pipe_get(ans_gpu* g, size_t syms, size_t slots, size_t dense, size_t chunks, HostPipe** out) {
    if (!g->pipe) {
        auto* p = new (std::nothrow) HostPipe{};
        if (!p) return ANS_E_ALLOC;
        g->pipe = p;
        if (const char* e = getenv("ANS_PIPE_DEPTH")) p->depth = std::min(kPipeDepthMax, std::max(2, atoi(e)));
        HIP_TRY(own_queue_stream(&p->s_in, ~0u));
        HIP_TRY(own_queue_stream(&p->s_out, 0x11111111u));  // device-to-host blits on a quarter of the CUs
        HIP_TRY(own_queue_stream(&p->s_comp2, ~0u));
        for (PipeSlot& s : slots_of(p)) {
            HIP_TRY(hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&s.ev_comp, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&s.ev_meta, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
        }
        HIP_TRY(hipMalloc(&p->d_status, sizeof(uint32_t)));
    }
    HostPipe* p = g->pipe;
    if (syms > p->cap_syms || slots > p->cap_slots || dense > p->cap_dense || chunks > p->cap_chunks) {
        HIP_TRY(hipDeviceSynchronize());
        syms = std::max(syms, p->cap_syms);
        slots = std::max(slots, p->cap_slots);
        dense = std::max(dense, p->cap_dense);
        chunks = std::max(chunks, p->cap_chunks);
        pipe_release(p);
        for (PipeSlot& s : slots_of(p)) {
            HIP_TRY(hipMalloc(&s.d_syms, syms + 16));
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.d_slots), slots + 16));
            // + 256: k_decode_g (the non-wide large-alphabet decoder, norm < 2^22) reads whole
            // aligned 128-B lines around each stream, so the last stream of a batch may touch the
            // line past its span (k_decode and k_decode_w read only the stream's own bytes)
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.d_dense), dense + 256));
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.d_lens), sizeof(uint32_t) * chunks + 16));
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.d_offs), sizeof(uint64_t) * (chunks + 1) + 16));
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s.h_lens), sizeof(uint32_t) * chunks + 16));
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s.h_offs), sizeof(uint64_t) * (chunks + 1) + 16));
        }
        p->cap_syms = syms;
        p->cap_slots = slots;
        p->cap_dense = dense;
        p->cap_chunks = chunks;
    }
    for (PipeSlot& s : slots_of(p)) s.used = false;
    HIP_TRY(hipMemsetAsync(p->d_status, 0, sizeof(uint32_t), g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    *out = p;
    return ANS_OK;
}

// Chunks per batch: about batch_bytes (default 128 MiB) of symbols.  A batch's kernels take
// about one chain latency (~1 ms) whatever its size until it fills the GPU, so batches must
// be large; 128 MiB batches through six workspace slots measured best for the round trip
// (tools/gpu_pipe_sweep.sh), with the workspace of three 256-MiB slots.
constexpr uint64_t kPipeBatchBytes = 128ull << 20;
uint64_t pipe_batch_chunks(const ans_gpu* g, uint64_t nchunks, uint64_t chunk_bytes) {
    const uint64_t target = g->batch_bytes ? g->batch_bytes : kPipeBatchBytes;
    uint64_t b = target / (chunk_bytes ? chunk_bytes : 1);
    if (b < 1) b = 1;
    return b < nchunks ? b : nchunks;
}

// Batch boundaries (chunk indices, first 0, last nchunks): batches of B chunks.  (Batches
// ramping up and down in size at the ends were measured too: with enough workspace slots
// they gained nothing over equal 128-MiB batches)
std::vector<uint64_t> pipe_cuts(uint64_t nchunks, uint64_t B) {
    std::vector<uint64_t> cuts{0};
    for (uint64_t c = B; c < nchunks; c += B) cuts.push_back(c);
    cuts.push_back(nchunks);
    return cuts;
}

// Batch b of a call over n symbols: its chunks [c0, c0 + nc) (their initial messages start at
// seed + c0), its symbols [n0, n0 + nb), its workspace slot and its compute stream.
struct Batch {
    PipeSlot& s;
    hipStream_t sc;
    uint64_t c0, nc, n0, nb;
};
Batch pipe_batch(const ans_gpu* g, HostPipe* p, const std::vector<uint64_t>& cuts, uint64_t b, uint64_t n,
                 uint64_t chunk_len) {
    const uint64_t c0 = cuts[b], nc = cuts[b + 1] - c0, n0 = c0 * chunk_len;
    return {p->slot[b % p->depth], (b & 1) ? p->s_comp2 : g->stream, c0, nc, n0, std::min(n - n0, nc * chunk_len)};
}

// Held from pipe_get to the call's return: whichever way the call leaves (a failed HIP call or
// a launcher's error code among them), the copies from and into the caller's buffers that
// earlier batches queued have finished before the caller may free those buffers, and before the
// next call's pipe_get marks the slots unused.
struct PipeDrain {
    ans_gpu* g;
    HostPipe* p;
    bool idle = false;
    // The closing of a call whose batches are all queued: every batch done (s_in's copies are
    // waited for by the compute streams), then the lowest status the kernels raised.
    int close() {
        HIP_TRY(hipStreamSynchronize(p->s_out));
        HIP_TRY(hipStreamSynchronize(p->s_comp2));
        int st = ANS_OK;
        const int rc = ans_dev_status(g, p->d_status, g->stream, &st);  // synchronises the context's stream
        idle = rc == ANS_OK;
        return rc ? rc : st;
    }
    ~PipeDrain() {
        if (idle) return;
        (void)hipStreamSynchronize(p->s_in);
        (void)hipStreamSynchronize(p->s_out);
        (void)hipStreamSynchronize(p->s_comp2);
        (void)hipStreamSynchronize(g->stream);
    }
};

// Encode from host symbols into a host dense container.  Batch b: H2D (s_in) -> encode,
// length scan, compaction, lengths D2H (compute stream b & 1); the host waits for batch
// b-1's lengths only after batch b is queued, then queues b-1's dense D2H (s_out) at its
// running offset.  With out == NULL (size query) nothing but the lengths comes back.
template <typename Sym>
int pipe_encode(ans_gpu_table* gt, const void* syms, uint64_t n, uint64_t chunk_len, uint8_t* out, uint64_t out_cap,
                uint64_t* offsets, uint64_t* lens, uint64_t* total, fast::ChunkInit ini) {
    constexpr uint64_t w = sizeof(Sym);
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    uint64_t slot_cap = 0;
    ans_gpu_slot_capacity(gt, chunk_len, &slot_cap);
    const uint64_t B = pipe_batch_chunks(gt->g, nchunks, chunk_len * w);
    HostPipe* p = nullptr;
    int rc = pipe_get(gt->g, B * chunk_len * w, B * slot_cap, out ? B * slot_cap : 0, B, &p);
    if (rc) return rc;
    PipeDrain drain{gt->g, p};
    const std::vector<uint64_t> cuts = pipe_cuts(nchunks, B);
    const uint64_t nbatch = cuts.size() - 1;
    const auto* src = static_cast<const uint8_t*>(syms);
    bool copy = out != nullptr;
    int len_err = ANS_OK;
    uint64_t acc = 0;
    auto enqueue = [&](uint64_t b) -> int {
        const auto [s, sc, c0, nc, n0, nb] = pipe_batch(gt->g, p, cuts, b, n, chunk_len);
        if (s.used) HIP_TRY(hipStreamWaitEvent(p->s_in, s.ev_comp, 0));  // symbols of batch b - depth consumed
        HIP_TRY(hipMemcpyAsync(s.d_syms, src + n0 * w, nb * w, hipMemcpyHostToDevice, p->s_in));
        HIP_TRY(hipEventRecord(s.ev_in, p->s_in));
        HIP_TRY(hipStreamWaitEvent(sc, s.ev_in, 0));
        if (s.used) HIP_TRY(hipStreamWaitEvent(sc, s.ev_out, 0));  // dense bytes of batch b - depth copied out
        int r = launch_encode<Sym>(gt, s.d_syms, nb, chunk_len, s.d_slots, slot_cap, s.d_lens, p->d_status, sc,
                                   fast::ChunkInit{ini.kind, ini.seed + c0});
        if (r) return r;
        // the batch's stream offsets: offs[j] = sum of lens[0..j), offs[nc] = total (ans_scan.hpp)
        k_excl_scan<<<1, 1024, 0, sc>>>(s.d_lens, nc, s.d_offs, s.d_offs + nc);
        HIP_TRY(hipGetLastError());
        if (copy && (r = ans_dev_compact(gt->g, s.d_slots, slot_cap, s.d_lens, s.d_offs, nc, s.d_dense, sc))) return r;
        HIP_TRY(hipEventRecord(s.ev_comp, sc));
        HIP_TRY(hipMemcpyAsync(s.h_lens, s.d_lens, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost, sc));
        HIP_TRY(hipMemcpyAsync(s.h_offs, s.d_offs + nc, sizeof(uint64_t), hipMemcpyDeviceToHost, sc));
        HIP_TRY(hipEventRecord(s.ev_meta, sc));
        s.used = true;
        return ANS_OK;
    };
    auto finish = [&](uint64_t b) -> int {
        const auto [s, sc, c0, nc, n0, nb] = pipe_batch(gt->g, p, cuts, b, n, chunk_len);
        HIP_TRY(hipEventSynchronize(s.ev_meta));
        const uint64_t bt = s.h_offs[0];
        if (copy && acc + bt > out_cap) {
            copy = false;  // keep coding to report the exact total
            len_err = ANS_E_LEN;
        }
        if (copy && bt) HIP_TRY(hipMemcpyAsync(out + acc, s.d_dense, bt, hipMemcpyDeviceToHost, p->s_out));
        HIP_TRY(hipEventRecord(s.ev_out, p->s_out));
        uint64_t o = acc;
        for (uint64_t j = 0; j < nc; ++j) {
            if (out) {
                offsets[c0 + j] = o;
                lens[c0 + j] = s.h_lens[j];
            }
            o += s.h_lens[j];
        }
        acc = o;
        return ANS_OK;
    };
    for (uint64_t b = 0; b < nbatch; ++b) {
        if ((rc = enqueue(b))) return rc;
        if (b > 0 && (rc = finish(b - 1))) return rc;
    }
    if (nbatch && (rc = finish(nbatch - 1))) return rc;
    if ((rc = drain.close())) return rc;
    *total = acc;
    return len_err;
}

// Decode a host dense container into host symbols.  Batch b: its byte span and rebased
// offsets/lengths H2D (s_in) -> decode of the span in place (compute stream b & 1; the
// decoders read a dense container at any alignment, fast::DecChain::start) -> symbols D2H
// (s_out).  No host synchronisation inside the loop beyond staging reuse.
// Returns kPipeScattered when some batch's streams spread over more than twice its slot bytes
// (a container that is not dense); the caller then takes the whole-buffer path.
template <typename Sym>
int pipe_decode(ans_gpu_table* gt, const uint8_t* in, const uint64_t* offsets, const uint32_t* l32, uint64_t slot_cap,
                uint64_t n, uint64_t chunk_len, int gen_kind, void* out, fast::ChunkInit ini) {
    constexpr uint64_t w = sizeof(Sym);
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    const uint64_t B = pipe_batch_chunks(gt->g, nchunks, chunk_len * w);
    const std::vector<uint64_t> cuts = pipe_cuts(nchunks, B);
    const uint64_t nbatch = cuts.size() - 1;
    std::vector<uint64_t> lo(nbatch), span(nbatch);
    uint64_t max_span = 0;
    for (uint64_t b = 0; b < nbatch; ++b) {
        const uint64_t c0 = cuts[b], c1 = cuts[b + 1];
        uint64_t l = ~0ull, h = 0;
        for (uint64_t j = c0; j < c1; ++j) {
            l = std::min(l, offsets[j]);
            h = std::max(h, offsets[j] + l32[j]);
        }
        lo[b] = l;
        span[b] = h - l;
        max_span = std::max(max_span, span[b]);
    }
    if (max_span > 2 * B * slot_cap) return kPipeScattered;
    HostPipe* p = nullptr;
    int rc = pipe_get(gt->g, B * chunk_len * w, B * slot_cap, max_span, B, &p);
    if (rc) return rc;
    PipeDrain drain{gt->g, p};
    auto* dst = static_cast<uint8_t*>(out);
    for (uint64_t b = 0; b < nbatch; ++b) {
        const auto [s, sc, c0, nc, n0, nb] = pipe_batch(gt->g, p, cuts, b, n, chunk_len);
        if (s.used) {
            HIP_TRY(hipEventSynchronize(s.ev_in));  // staging of batch b - depth uploaded
            HIP_TRY(hipStreamWaitEvent(p->s_in, s.ev_out, 0));  // its buffers drained
        }
        std::memcpy(s.h_lens, l32 + c0, sizeof(uint32_t) * nc);
        for (uint64_t j = 0; j < nc; ++j) s.h_offs[j] = offsets[c0 + j] - lo[b];  // into the batch's span
        if (span[b]) HIP_TRY(hipMemcpyAsync(s.d_dense, in + lo[b], span[b], hipMemcpyHostToDevice, p->s_in));
        HIP_TRY(hipMemcpyAsync(s.d_lens, s.h_lens, sizeof(uint32_t) * nc, hipMemcpyHostToDevice, p->s_in));
        HIP_TRY(hipMemcpyAsync(s.d_offs, s.h_offs, sizeof(uint64_t) * nc, hipMemcpyHostToDevice, p->s_in));
        HIP_TRY(hipEventRecord(s.ev_in, p->s_in));
        HIP_TRY(hipStreamWaitEvent(sc, s.ev_in, 0));
        if ((rc = launch_decode<Sym>(gt, s.d_dense, s.d_offs, slot_cap, s.d_lens, nb, chunk_len, gen_kind, s.d_syms,
                                     p->d_status, sc, fast::ChunkInit{ini.kind, ini.seed + c0})))
            return rc;
        HIP_TRY(hipEventRecord(s.ev_comp, sc));
        HIP_TRY(hipStreamWaitEvent(p->s_out, s.ev_comp, 0));
        HIP_TRY(hipMemcpyAsync(dst + n0 * w, s.d_syms, nb * w, hipMemcpyDeviceToHost, p->s_out));
        HIP_TRY(hipEventRecord(s.ev_out, p->s_out));
        s.used = true;
    }
    return drain.close();
}

}  // namespace

// Releases the context's pipeline workspace (ans_ctx.hpp; called by ans_gpu_free).
void ans_pipe_free(ans_gpu* g) {
    HostPipe* p = g->pipe;
    if (!p) return;
    (void)hipDeviceSynchronize();
    pipe_release(p);
    for (PipeSlot& s : slots_of(p)) {
        (void)hipEventDestroy(s.ev_in);
        (void)hipEventDestroy(s.ev_comp);
        (void)hipEventDestroy(s.ev_meta);
        (void)hipEventDestroy(s.ev_out);
    }
    (void)hipFree(p->d_status);
    (void)hipStreamDestroy(p->s_in);
    (void)hipStreamDestroy(p->s_out);
    (void)hipStreamDestroy(p->s_comp2);
    delete p;
    g->pipe = nullptr;
}

// ====================================================================== C ABI (host buffers)
extern "C" {

int ans_host_alloc(size_t bytes, void** out) try {
    if (!out) return ANS_E_ARG;
    *out = nullptr;
    if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        *out = nullptr;
        return ANS_E_ALLOC;
    }
    return ANS_OK;
} ANS_CATCH

void ans_host_free(void* p) try {
    if (p) (void)hipHostFree(p);
} ANS_CATCH_VOID

int ans_gpu_set_batch_bytes(ans_gpu* g, uint64_t batch_bytes) try {
    if (!g) return ANS_E_ARG;
    g->batch_bytes = batch_bytes;
    return ANS_OK;
} ANS_CATCH

int ans_gpu_pipe_depth(const ans_gpu* g, int* depth) try {
    if (!g || !depth) return ANS_E_ARG;
    *depth = g->pipe ? g->pipe->depth : 0;
    return ANS_OK;
} ANS_CATCH

int ans_gpu_encode_chunks_ex(ans_gpu_table* gt, const void* syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                             int gen_kind, uint64_t seed, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                             uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !valid_width_u32(sym_bytes) || chunk_len == 0 || !total || !valid_kind(gen_kind)) return ANS_E_ARG;
    const fast::ChunkInit ini{gen_kind, seed};
    if (n && !syms) return ANS_E_ARG;
    if (gt->ts64) {
        const uint64_t nc = (n + chunk_len - 1) / chunk_len;
        if (out && nc && (!offsets || !lens)) return ANS_E_ARG;
        return ans_tableset_host_encode(gt->ts64, syms, sym_bytes, n, chunk_len, nullptr, nc, gen_kind, seed, out,
                                        out_cap, offsets, lens, total);
    }
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    if (out && nchunks && (!offsets || !lens)) return ANS_E_ARG;
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(gt->g->device));
    return with_sym_type(sym_bytes, [&](auto t) {
        return pipe_encode<decltype(t)>(gt, syms, n, chunk_len, out, out_cap, offsets, lens, total, ini);
    });
} ANS_CATCH

int ans_gpu_encode_chunks(ans_gpu_table* gt, const void* syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                          uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    return ans_gpu_encode_chunks_ex(gt, syms, sym_bytes, n, chunk_len, ANS_GEN_ZEROS, 0, out, out_cap, offsets, lens,
                                    total);
} ANS_CATCH

int ans_gpu_decode_chunks_ex(ans_gpu_table* gt, const uint8_t* in, uint64_t in_len, const uint64_t* offsets,
                             const uint64_t* lens, uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed,
                             void* out, int sym_bytes) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !valid_width_u32(sym_bytes) || chunk_len == 0) return ANS_E_ARG;
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    if (nchunks && (!in || !offsets || !lens || !out)) return ANS_E_ARG;
    if (!valid_kind(gen_kind)) return ANS_E_ARG;
    if (gt->ts64)
        return ans_tableset_host_decode(gt->ts64, in, in_len, offsets, lens, n, chunk_len, nullptr, nchunks, gen_kind,
                                        seed, out, sym_bytes);
    const fast::ChunkInit ini{gen_kind, seed};
    if ((sym_bytes == 1 && gt->t.nsym > 256) || (sym_bytes == 2 && gt->t.nsym > 65536)) return ANS_E_ARG;
    std::vector<uint32_t> l32;
    uint64_t slot_cap = 0, max_len = 0;
    int rc = narrow_lens(offsets, lens, nchunks, in_len, l32, &max_len);
    if (rc) return rc;
    // The fast decoders read the container in place (any stream alignment); slot_cap (widened
    // if a possibly corrupt stream is longer than a valid one can be) sizes the pipeline's
    // batches and tells a dense container from a scattered one.
    ans_gpu_slot_capacity(gt, chunk_len, &slot_cap);
    slot_cap = std::max<uint64_t>(slot_cap, (max_len + 64 + 127) & ~uint64_t(127));
    HIP_TRY(hipSetDevice(gt->g->device));
    if (nchunks) {  // dense containers (the encoder's output) take the pipelined path
        rc = with_sym_type(sym_bytes, [&](auto t) {
            return pipe_decode<decltype(t)>(gt, in, offsets, l32.data(), slot_cap, n, chunk_len, gen_kind, out,
                                            ini);
        });
        if (rc != kPipeScattered) return rc;
    }
    // streams scattered over the buffer: one upload of the whole input, decoded in place
    const hipStream_t s = gt->g->stream;
    DevStreams d;
    DevBuf d_out;
    if ((rc = upload_streams(in, in_len, offsets, l32, s, d))) return rc;
    HIP_TRY(d_out.alloc(n * sym_bytes));
    rc = ans_dev_decode_chunks_ex(gt, d.in.as<uint8_t>(), d.offs.as<uint64_t>(), slot_cap, d.lens.as<uint32_t>(), n,
                                  chunk_len, gen_kind, seed, d_out.p, sym_bytes, d.status.as<uint32_t>(), s);
    if (rc || (rc = read_status(gt->g, d.status.as<uint32_t>(), s))) return rc;
    if (n) HIP_TRY(hipMemcpy(out, d_out.p, n * sym_bytes, hipMemcpyDeviceToHost));
    return ANS_OK;
} ANS_CATCH

int ans_gpu_decode_chunks(ans_gpu_table* gt, const uint8_t* in, uint64_t in_len, const uint64_t* offsets,
                          const uint64_t* lens, uint64_t n, uint64_t chunk_len, int gen_kind, void* out,
                          int sym_bytes) try {
    if (gen_kind != ANS_GEN_ZEROS && gen_kind != ANS_GEN_EMPTY) return ANS_E_ARG;  // RANDOM needs a seed: _ex
    return ans_gpu_decode_chunks_ex(gt, in, in_len, offsets, lens, n, chunk_len, gen_kind, 0, out, sym_bytes);
} ANS_CATCH

}  // extern "C"
