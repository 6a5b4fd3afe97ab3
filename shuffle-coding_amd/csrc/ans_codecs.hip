// ans_codecs.hip — the other static codecs of src/codec.rs on the GPU: exact 64-bit
// one-lane-per-chunk kernels for
//   * IID<Uniform(size)>, size <= MAX_SIZE = 2^46 (src/codec.rs:13-49, src/ans.rs:22);
//   * IID<LogUniform(excl_max_bits)> (src/codec.rs:561-611), the item of MaxBenfordIID
//     (src/param_codec.rs:91-129): per element a Uniform(2^(bits-1)) push of the low bits, then
//     a Uniform(excl_max_bits + 1) push of the bit count;
//   * Independent<Categorical> (src/codec.rs:366-403): a Categorical per position, from a table
//     set; one table with norm >= 2^32 (up to 2^56) is also how IID<Categorical> of such wide
//     norms runs (ans_gpu_table_create routes them here).
// Chunk c is one reference message, as in ans_kernels.hip: IID/Independent push in reverse
// (src/codec.rs:388-391, 415-420) through the blanket push (src/ans.rs:96-105) with the full
// renorm (src/ans.rs:233-253: up, then down — with codecs of different norms in one message,
// a push can pull back bytes it pushed earlier), flatten (src/ans.rs:255-260).  Decode is the
// mirror (src/ans.rs:107-116), whose renorm_down hands bytes back to the stream.
//
// These are the generic paths (byte-granular stream I/O, the compiler's 64-bit division): the
// bulk throughput path is the table kernels of ans_fast.hpp / ans_wide.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_hostio.hpp"
#include "ans_mfast_launch.hpp"

// the lane's stream I/O (Sink, Source, RSource), the blanket push / pop (PushT, PopT), the table
// set's model (TabHdr, CatSetModel), flatten and raise: ans_exact.hpp, shared with ans_mset.hip
using namespace shuffle_coding::exact;

namespace {

using shuffle_coding::fast::ChunkInit;
constexpr uint64_t kMaxSize = 1ull << 46;     // src/ans.rs:22

#define HIP_TRY(expr) ANS_HIP_TRY(expr)

// ---- the models
// Each model splits an element into what can be loaded ahead of the chain (Elem: the symbol and,
// for Independent, its table id; Pos: the table id of a position to decode) and the push / pop
// on the message.  The kernels load elements a block ahead (kPrefetch), so the HBM latency of the
// symbol and table-id reads stays off the serial per-chunk chain.
struct NoPos {};
struct UniformModel {  // IID<Uniform(size)>: pmf 1, cdf(x, 0) = x, icdf(cf) = (cf, 0)
    uint64_t size, K;
    struct Elem { uint64_t x; };
    using Pos = NoPos;
    __device__ void stage(unsigned char*) {}
    template <typename Sym>
    __device__ Elem load(const Sym* syms, uint64_t k) const { return Elem{static_cast<uint64_t>(syms[k])}; }
    __device__ Pos pos(uint64_t) const { return {}; }
    __device__ int push(Push& m, const Elem& e) const {
        if (e.x >= size) return ANS_E_SYMBOL;  // outside the alphabet (the reference would code garbage)
        m.push(1, size, K, e.x);
        return ANS_OK;
    }
    __device__ uint64_t pop(Pop& m, const Pos&) const {
        m.renorm(size, K);
        const uint64_t x = m.head % size;
        m.head /= size;
        return x;
    }
};

struct LogUniformModel {  // IID<LogUniform(E)>: bits = 64 - clz(x) by Uniform(E + 1), low bits by Uniform(2^(bits-1))
    uint64_t nbits, Kbits;  // nbits = E + 1 = the bits codec's size, Kbits = 2^56 / nbits
    struct Elem { uint64_t x; };
    using Pos = NoPos;
    __device__ void stage(unsigned char*) {}
    template <typename Sym>
    __device__ Elem load(const Sym* syms, uint64_t k) const { return Elem{static_cast<uint64_t>(syms[k])}; }
    __device__ Pos pos(uint64_t) const { return {}; }
    __device__ int push(Push& m, const Elem& e) const {
        const uint64_t x = e.x;
        const uint64_t bits = x ? 64u - static_cast<uint64_t>(__builtin_clzll(x)) : 0u;  // LogUniform::get_bits
        if (bits >= nbits) return ANS_E_SYMBOL;  // assert!(bits < self.bits.size)
        if (bits != 0) {
            if (bits - 1 > 46) return ANS_E_NORM_RANGE;  // Uniform::new asserts size <= MAX_SIZE
            const uint64_t size = 1ull << (bits - 1);
            m.push(1, size, kMaxMinHead >> (bits - 1), x & ~size);
        }
        m.push(1, nbits, Kbits, bits);
        return ANS_OK;
    }
    __device__ uint64_t pop(Pop& m, const Pos&) const {
        m.renorm(nbits, Kbits);
        const uint64_t bits = m.head % nbits;
        m.head /= nbits;
        if (bits == 0) return 0;
        const uint64_t size = 1ull << (bits - 1);
        m.renorm(size, kMaxMinHead >> (bits - 1));
        const uint64_t low = m.head & (size - 1);
        m.head >>= (bits - 1);
        return low | size;
    }
};

// ---- the kernels' shared steps
// Elements are loaded kPrefetch at a time, one block ahead of the block being coded (the loads
// of a block are independent of the chain: their HBM latency overlaps kPrefetch steps).
constexpr int kPrefetch = 8;

// The end of a decode, assert_eq!(initial, m) (src/ans.rs:56): the head pulled back up to the
// initial message's (chunk c's, worked out only once everything else holds), no byte left.  A pop
// that drew past the start of an EMPTY message is exhaustion (src/ans.rs:144).
__device__ __forceinline__ void check_initial(Pop& m, Source& src, int gen_kind, const ChunkInit& ini, uint64_t c,
                                              uint32_t* status) {
    for (int g = 0; m.head < kMaxMinHead && g < 8; ++g) m.head = (m.head << 8) | src.pop();
    if (src.generated && gen_kind == ANS_GEN_EMPTY) raise(status, ANS_E_EXHAUSTED);
    else if (src.bad || src.generated || src.pos != 0 || m.head != ini.head(c)) raise(status, ANS_E_MISMATCH);
}

// ---- the kernels: one lane per chunk
template <class Model, typename Sym>
__global__ __launch_bounds__(kThreads) void k_encode64(Model md, const Sym* __restrict__ syms, const uint64_t* starts,
                                                        uint64_t n, uint64_t chunk_len, uint64_t nchunks,
                                                        uint8_t* __restrict__ slots, uint64_t slot_cap,
                                                        uint32_t* __restrict__ lens, uint32_t* __restrict__ status,
                                                        ChunkInit ini) {
    extern __shared__ __align__(16) unsigned char lds[];
    md.stage(lds);
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const uint64_t a = starts ? starts[c] : c * chunk_len;
    const uint64_t b = starts ? starts[c + 1] : min(a + chunk_len, n);
    Sink sink(slots + c * slot_cap, slot_cap, 0);
    Push m{ini.head(c), &sink, 0};
    // (The chunk walks and failure tails of these kernels stay written in each.  As shared
    // functions they compiled to other code: the push walk cost the Uniform or the LogUniform
    // encoder 2-4%, the pop walk k_decode64 up to 5 VGPRs, the encode tail LogUniform encode 0.8%:
    // profiles/r09_ab_codecs_refactor.txt, r09_kernel_regs_codecs_refactor.txt.)
    using Elem = typename Model::Elem;
    Elem cur[kPrefetch], nxt[kPrefetch];
    auto load_block = [&](Elem* e, uint64_t top) {  // elements top-1, top-2, ... (those >= a)
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i)
            if (top >= a + 1 + i) e[i] = md.load(syms, top - 1 - i);
    };
    load_block(cur, b);
    for (uint64_t top = b; top > a; top = top >= a + kPrefetch ? top - kPrefetch : a) {  // last symbol first
        if (top >= a + kPrefetch + 1) load_block(nxt, top - kPrefetch);
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) {
            if (top < a + 1 + i) break;
            const int e = md.push(m, cur[i]);
            if (e) {
                raise(status, e);
                lens[c] = 0;
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) cur[i] = nxt[i];
    }
    flatten(m.head, [&](uint32_t byte) { sink.put(byte); });
    const uint64_t len = sink.finish();
    // a pull from the generator lives in the tail's num_generated, which a byte container does
    // not carry: that chunk would not decode back to its initial message
    if (sink.overflow || m.pulled) {
        raise(status, sink.overflow ? ANS_E_LEN : ANS_E_MISMATCH);
        lens[c] = 0;
        return;
    }
    lens[c] = static_cast<uint32_t>(len);
}

template <class Model, typename Sym>
__global__ __launch_bounds__(kThreads) void k_decode64(Model md, const uint8_t* __restrict__ in,
                                                        const uint64_t* __restrict__ offsets, uint64_t slot_cap,
                                                        const uint32_t* __restrict__ lens, const uint64_t* starts,
                                                        uint64_t n, uint64_t chunk_len, uint64_t nchunks, int gen_kind,
                                                        Sym* __restrict__ out, uint32_t* __restrict__ status,
                                                        ChunkInit ini) {
    extern __shared__ __align__(16) unsigned char lds[];
    md.stage(lds);
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const uint64_t a = starts ? starts[c] : c * chunk_len;
    const uint64_t b = starts ? starts[c + 1] : min(a + chunk_len, n);
    if (!offsets && lens[c] > slot_cap) {
        raise(status, ANS_E_LEN);
        return;
    }
    Source src{in + (offsets ? offsets[c] : c * slot_cap), lens[c], lens[c], 0, false};
    Pop m{0, &src};  // Message::unflatten: head 0
    using Pos = typename Model::Pos;
    Pos cur[kPrefetch], nxt[kPrefetch];
    auto load_block = [&](Pos* p, uint64_t k0) {  // positions k0, k0 + 1, ... (those < b)
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i)
            if (k0 + i < b) p[i] = md.pos(k0 + i);
    };
    load_block(cur, a);
    bool stop = false;
    for (uint64_t k0 = a; k0 < b && !stop; k0 += kPrefetch) {
        if (k0 + kPrefetch < b) load_block(nxt, k0 + kPrefetch);
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) {
            if (k0 + i >= b) break;
            out[k0 + i] = static_cast<Sym>(md.pop(m, cur[i]));
            if (src.generated && gen_kind == ANS_GEN_EMPTY) {  // src/ans.rs:144
                raise(status, ANS_E_EXHAUSTED);
                return;
            }
            if (src.bad) {
                stop = true;
                break;
            }
        }
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) cur[i] = nxt[i];
    }
    check_initial(m, src, gen_kind, ini, c, status);
}

// ---- resume: push onto / pop from the message already in chunk c's slot (include/ans_capi.h 4b)
// The message is Message::unflatten(slot bytes [0, lens[c])) with the Empty generator: head 0, so
// the first operation's renorm_up pulls from the top of the bytes (zero bytes on top included).
// Independent::push of the chunk's symbols, last first, then flatten: the head's bytes go back on
// at the final position (the single 0x00 of a zero head included) and lens[c] is the new length.
// A pull below the stream's start is ANS_E_EXHAUSTED, a result past slot_cap ANS_E_LEN; either
// leaves lens[c] = 0.
// flagged: only the chunks the fast encoder handed over (ans_mfast.hpp kResumeExact in lens[c]:
// messages too short for its prologue); every other chunk is already done.
template <typename Sym>
__global__ __launch_bounds__(kThreads) void k_push64(CatSetModel md, const Sym* __restrict__ syms, const uint64_t* starts,
                                                      uint64_t n, uint64_t chunk_len, uint64_t nchunks,
                                                      uint8_t* slots, uint64_t slot_cap, uint32_t* lens,
                                                      uint32_t* __restrict__ status, bool flagged) {
    extern __shared__ __align__(16) unsigned char lds[];
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    // (a flagged pass stages the tables only in a workgroup that holds a handed-over chunk)
    if (flagged && !__syncthreads_or(c < nchunks && (lens[c] & shuffle_coding::mfast::kResumeExact))) return;
    md.stage(lds);
    if (c >= nchunks) return;
    const uint64_t a = starts ? starts[c] : c * chunk_len;
    const uint64_t b = starts ? starts[c + 1] : min(a + chunk_len, n);
    auto fail = [&](int code) {
        raise(status, code);
        lens[c] = 0;
    };
    uint32_t len0 = lens[c];
    if (flagged) {
        if (!(len0 & shuffle_coding::mfast::kResumeExact)) return;
        len0 &= ~shuffle_coding::mfast::kResumeExact;
    }
    if (len0 > slot_cap) return fail(ANS_E_LEN);
    Sink sink(slots + c * slot_cap, slot_cap, len0);
    PushT<true> m{0, &sink, 0};  // Message::unflatten: head 0
    using Elem = CatSetModel::Elem;
    Elem cur[kPrefetch], nxt[kPrefetch];
    auto load_block = [&](Elem* e, uint64_t top) {  // elements top-1, top-2, ... (those >= a)
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i)
            if (top >= a + 1 + i) e[i] = md.load(syms, top - 1 - i);
    };
    load_block(cur, b);
    for (uint64_t top = b; top > a; top = top >= a + kPrefetch ? top - kPrefetch : a) {  // last symbol first
        if (top >= a + kPrefetch + 1) load_block(nxt, top - kPrefetch);
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) {
            if (top < a + 1 + i) break;
            const int e = md.push(m, cur[i]);
            if (e || m.pulled) return fail(e ? e : ANS_E_EXHAUSTED);
        }
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) cur[i] = nxt[i];
    }
    flatten(m.head, [&](uint32_t byte) { sink.put(byte); });
    const uint64_t len = sink.finish();
    if (sink.overflow || len > 0xFFFFFFFFull) return fail(ANS_E_LEN);
    lens[c] = static_cast<uint32_t>(len);
}

// chunk_len forward pops (Independent::pop, src/codec.rs:393-399), then flatten of what remains
// (flagged: only the chunks the fast decoder handed over, as k_push64)
template <typename Sym>
__global__ __launch_bounds__(kThreads) void k_pop64(CatSetModel md, uint8_t* slots, uint64_t slot_cap, uint32_t* lens,
                                                     const uint64_t* starts, uint64_t n, uint64_t chunk_len,
                                                     uint64_t nchunks, Sym* __restrict__ out,
                                                     uint32_t* __restrict__ status, bool flagged) {
    extern __shared__ __align__(16) unsigned char lds[];
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (flagged && !__syncthreads_or(c < nchunks && (lens[c] & shuffle_coding::mfast::kResumeExact))) return;
    md.stage(lds);
    if (c >= nchunks) return;
    const uint64_t a = starts ? starts[c] : c * chunk_len;
    const uint64_t b = starts ? starts[c + 1] : min(a + chunk_len, n);
    auto fail = [&](int code) {
        raise(status, code);
        lens[c] = 0;
    };
    uint32_t len0 = lens[c];
    if (flagged) {
        if (!(len0 & shuffle_coding::mfast::kResumeExact)) return;
        len0 &= ~shuffle_coding::mfast::kResumeExact;
    }
    if (len0 > slot_cap) return fail(ANS_E_LEN);
    RSource src{slots + c * slot_cap, slot_cap, len0, false, false};
    PopT<RSource> m{0, &src};  // Message::unflatten: head 0
    using Pos = CatSetModel::Pos;
    Pos cur[kPrefetch], nxt[kPrefetch];
    auto load_block = [&](Pos* p, uint64_t k0) {  // positions k0, k0 + 1, ... (those < b)
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i)
            if (k0 + i < b) p[i] = md.pos(k0 + i);
    };
    load_block(cur, a);
    for (uint64_t k0 = a; k0 < b; k0 += kPrefetch) {
        if (k0 + kPrefetch < b) load_block(nxt, k0 + kPrefetch);
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) {
            if (k0 + i >= b) break;
            const uint64_t x = md.pop(m, cur[i]);
            if (src.exhausted) return fail(ANS_E_EXHAUSTED);  // src/ans.rs:144
            out[k0 + i] = static_cast<Sym>(x);
        }
#pragma unroll
        for (int i = 0; i < kPrefetch; ++i) cur[i] = nxt[i];
    }
    flatten(m.head, [&](uint32_t byte) { src.unpop(byte & 0xFFu); });
    if (src.overflow || src.pos > 0xFFFFFFFFull) return fail(ANS_E_LEN);
    lens[c] = static_cast<uint32_t>(src.pos);
}

// ---- GraphIID<NodeC, EdgeC, ErdosRenyi> with Categorical labels, one graph per lane
// (src/graph_codec.rs:31-38 GraphIID, 61-71 EdgesIID, 111-120 DenseSetIID): graph g's message
// pops its node labels (IID<NodeC>), then the edge-indicator vector over AllEdgeIndices
// (IID<Bernoulli>), then as many edge labels (IID<EdgeC>) as the vector holds edges.  The
// encoder pushes the mirror: edge labels last-to-first, the indicator vector last-to-first, the
// node labels last-to-first.  The layout is data-dependent on the decode side (the edge-label
// count is known only once the indicator vector is decoded), so each lane walks its three
// segments itself instead of reading per-position table ids.
template <class Pusher>
__device__ __forceinline__ int push_segment(const CatSetModel& md, Pusher& m, uint32_t t, const uint32_t* x,
                                            uint64_t a, uint64_t b) {
    for (uint64_t k = b; k > a; --k) {  // IID::push: last element first (src/codec.rs:415-420)
        const int e = md.push(m, CatSetModel::Elem{x[k - 1], t});
        if (e) return e;
    }
    return ANS_OK;
}

__global__ __launch_bounds__(kThreads) void k_graph_encode64(CatSetModel md, GraphLayout gl, uint64_t num_graphs,
                                                              const uint32_t* __restrict__ node_labels,
                                                              const uint8_t* __restrict__ dense,
                                                              const uint32_t* __restrict__ edge_labels,
                                                              uint8_t* __restrict__ slots, uint64_t slot_cap,
                                                              uint32_t* __restrict__ lens, uint32_t* __restrict__ status,
                                                              ChunkInit ini) {
    extern __shared__ __align__(16) unsigned char lds[];
    md.stage(lds);
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= num_graphs) return;
    Sink sink(slots + g * slot_cap, slot_cap, 0);
    Push m{ini.head(g), &sink, 0};
    int e = ANS_OK;
    // EdgesIID::push: the labels (sorted by edge index), then the indices (src/graph_codec.rs:61-65)
    if (gl.t_edge != kNoTable) e = push_segment(md, m, gl.t_edge, edge_labels, gl.edge_off[g], gl.edge_off[g + 1]);
    for (uint64_t x = gl.slot_off[g + 1]; !e && x > gl.slot_off[g]; --x)
        e = md.push(m, CatSetModel::Elem{dense[x - 1], gl.t_bern});
    // then the node labels (src/graph_codec.rs:33)
    if (!e && gl.t_node != kNoTable) e = push_segment(md, m, gl.t_node, node_labels, gl.node_off[g], gl.node_off[g + 1]);
    if (e) {
        raise(status, e);
        lens[g] = 0;
        return;
    }
    flatten(m.head, [&](uint32_t byte) { sink.put(byte); });
    const uint64_t len = sink.finish();
    // a pull from the generator lives in the tail's num_generated, which a byte container does
    // not carry: that chunk would not decode back to its initial message
    if (sink.overflow || m.pulled) {
        raise(status, sink.overflow ? ANS_E_LEN : ANS_E_MISMATCH);
        lens[g] = 0;
        return;
    }
    lens[g] = static_cast<uint32_t>(len);
}

// Decode: node labels to node_labels[node_off[g] ..], the indicator vector to
// dense[slot_off[g] ..], and the edge labels in pop order to edge_scratch[slot_off[g] ..] (a
// graph holds at most as many edges as slots); edge_count[g] receives the number of edges.
__global__ __launch_bounds__(kThreads) void k_graph_decode64(CatSetModel md, GraphLayout gl, uint64_t num_graphs,
                                                              const uint8_t* __restrict__ in,
                                                              const uint64_t* __restrict__ offsets,
                                                              const uint32_t* __restrict__ lens, int gen_kind,
                                                              uint32_t* __restrict__ node_labels,
                                                              uint8_t* __restrict__ dense,
                                                              uint32_t* __restrict__ edge_scratch,
                                                              uint64_t* __restrict__ edge_count,
                                                              uint32_t* __restrict__ status, ChunkInit ini) {
    extern __shared__ __align__(16) unsigned char lds[];
    md.stage(lds);
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= num_graphs) return;
    Source src{in + offsets[g], lens[g], lens[g], 0, false};
    Pop m{0, &src};  // Message::unflatten
    uint64_t edges = 0;
    edge_count[g] = 0;
    // a pop that drew past the start of an EMPTY message is exhaustion (src/ans.rs:144)
    auto halted = [&]() { return (src.generated && gen_kind == ANS_GEN_EMPTY) || src.bad; };
    if (gl.t_node != kNoTable)
        for (uint64_t k = gl.node_off[g]; k < gl.node_off[g + 1] && !halted(); ++k)
            node_labels[k] = static_cast<uint32_t>(md.pop(m, CatSetModel::Pos{gl.t_node}));
    for (uint64_t x = gl.slot_off[g]; x < gl.slot_off[g + 1] && !halted(); ++x) {
        const uint64_t b = md.pop(m, CatSetModel::Pos{gl.t_bern});
        dense[x] = static_cast<uint8_t>(b);
        edges += b != 0;
    }
    if (gl.t_edge != kNoTable)
        for (uint64_t k = 0; k < edges && !halted(); ++k)
            edge_scratch[gl.slot_off[g] + k] = static_cast<uint32_t>(md.pop(m, CatSetModel::Pos{gl.t_edge}));
    edge_count[g] = edges;
    if (src.generated && gen_kind == ANS_GEN_EMPTY) {
        raise(status, ANS_E_EXHAUSTED);
        return;
    }
    check_initial(m, src, gen_kind, ini, g, status);
}

// ---- host side: the exact kernels' launchers
unsigned blocks(uint64_t lanes) { return static_cast<unsigned>((lanes + kThreads - 1) / kThreads); }
// an entry's stream argument: NULL is the context's own stream
hipStream_t stream_of(const ans_gpu* g, void* stream) { return stream ? static_cast<hipStream_t>(stream) : g->stream; }

// Worst-case stream bytes of one chunk of chunk_len symbols coding at most bits_per_symbol bits
// each (the virtual-bits bound of ans_gpu_slot_capacity), rounded up to 128 with margin.
uint64_t slot_bytes(uint64_t chunk_len, double bits_per_symbol) {
    const double b = (static_cast<double>(chunk_len) * (bits_per_symbol + 1e-6) + 2.0) / 8.0 + 16.0;
    const uint64_t cap = static_cast<uint64_t>(std::ceil(b)) + chunk_len / 64 + 64;
    return (cap + 127) & ~uint64_t(127);
}

template <class Model>
size_t lds_of(const Model&) { return 0; }
size_t lds_of(const CatSetModel& md) { return md.lds_bytes; }

// the exact model for the chunks from position k on (a call's ragged last chunk)
template <class Model>
Model at_offset(const Model& md, uint64_t) { return md; }
CatSetModel at_offset(const CatSetModel& md, uint64_t k) {
    CatSetModel m = md;
    if (m.tid) m.tid += k;
    if (m.tid8) m.tid8 += k;
    return m;
}

// the model's device table ids as bytes (Independent's exact model; none for the others)
template <class Model>
const uint8_t* tid8_of(const Model&) { return nullptr; }
const uint8_t* tid8_of(const CatSetModel& m) { return m.tid8; }

// the exact 64-bit kernels (any chunk layout; d_starts != NULL: variable chunks)
template <class Model>
int dev_encode(const Model& md, const void* d_syms, int w, const uint64_t* d_starts, uint64_t n, uint64_t chunk_len,
               uint64_t nchunks, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status,
               ChunkInit ini, hipStream_t s, LaunchLog* log = nullptr) {
    with_sym_type_u64(w, [&](auto t) {
        using Sym = decltype(t);
        if (log) log->add(kRecEncode64, sizeof(Sym));
        k_encode64<Model, Sym><<<blocks(nchunks), kThreads, lds_of(md), s>>>(
            md, static_cast<const Sym*>(d_syms), d_starts, n, chunk_len, nchunks, d_slots, slot_cap, d_lens, d_status, ini);
    });
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}
template <class Model>
int dev_decode(const Model& md, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t slot_cap,
               const uint32_t* d_lens, const uint64_t* d_starts, uint64_t n, uint64_t chunk_len, uint64_t nchunks,
               int gen_kind, void* d_syms, int w, uint32_t* d_status, ChunkInit ini, hipStream_t s,
               LaunchLog* log = nullptr) {
    with_sym_type_u64(w, [&](auto t) {
        using Sym = decltype(t);
        if (log) log->add(kRecDecode64, sizeof(Sym));
        k_decode64<Model, Sym><<<blocks(nchunks), kThreads, lds_of(md), s>>>(
            md, d_in, d_offsets, slot_cap, d_lens, d_starts, n, chunk_len, nchunks, gen_kind, static_cast<Sym*>(d_syms),
            d_status, ini);
    });
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}

// a launcher's entry: the context's launch record, cleared (NULL: a codec that keeps none)
inline LaunchLog* fresh(LaunchLog* log) {
    if (log) log->clear();
    return log;
}

// resume on the exact kernels (k_push64 / k_pop64): any set, any chunk layout
int dev_push(const CatSetModel& md, const void* d_syms, int w, const uint64_t* d_starts, uint64_t n, uint64_t chunk_len,
             uint64_t nchunks, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status,
             hipStream_t s, bool flagged = false, LaunchLog* log = nullptr) {
    with_sym_type_u64(w, [&](auto t) {
        using Sym = decltype(t);
        if (log) log->add(kRecPush64, sizeof(Sym));
        k_push64<Sym><<<blocks(nchunks), kThreads, lds_of(md), s>>>(
            md, static_cast<const Sym*>(d_syms), d_starts, n, chunk_len, nchunks, d_slots, slot_cap, d_lens, d_status, flagged);
    });
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}
int dev_pop(const CatSetModel& md, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, const uint64_t* d_starts,
            uint64_t n, uint64_t chunk_len, uint64_t nchunks, void* d_syms, int w, uint32_t* d_status, hipStream_t s,
            bool flagged = false, LaunchLog* log = nullptr) {
    with_sym_type_u64(w, [&](auto t) {
        using Sym = decltype(t);
        if (log) log->add(kRecPop64, sizeof(Sym));
        k_pop64<Sym><<<blocks(nchunks), kThreads, lds_of(md), s>>>(
            md, d_slots, slot_cap, d_lens, d_starts, n, chunk_len, nchunks, static_cast<Sym*>(d_syms), d_status, flagged);
    });
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}

// ---- the fast kernels (ans_mfast.hpp) for the full chunks of a fixed-chunk call
namespace mf = shuffle_coding::mfast;
namespace sc = shuffle_coding;

// Every chunk's symbols must be whole 128-B lines and its worst-case stream inside the decoder's
// 2^27-byte positions; the ragged last chunk, variable chunks and other layouts stay exact.
// ANS_CODECS_EXACT=1 keeps every chunk on the exact kernels (the A/B of tools/codecs_bench.py)
bool fast_layout(uint64_t chunk_len, int w, uint64_t slot_cap) {
    static const bool exact_only = [] {
        const char* e = getenv("ANS_CODECS_EXACT");
        return e && e[0] == '1';
    }();
    return !exact_only && chunk_len > 0 && (chunk_len * static_cast<uint64_t>(w)) % 128 == 0 && slot_cap % 128 == 0 &&
           slot_cap < (1ull << 27);
}
// the fast kernels move symbols, table ids and slot pages with 16-B vector loads and stores: a
// misaligned buffer (an offset torch view, say) sends the call to the exact kernels instead
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// IID codecs with at most 7 bytes per symbol: a point every min(U, 8) symbols (<= 56 bytes)
template <class M>
void menc_w(const M& md, const mf::EncArgs& a) {
    auto go = [&](auto sym, auto spp) { mf::menc_of(md, a, mf::kEncTab, sym, spp); };
    switch (a.w) {
    case 1: go(uint8_t{}, mf::Spp<8>{}); break;
    case 2: go(uint16_t{}, mf::Spp<8>{}); break;
    case 4: go(uint32_t{}, mf::Spp<4>{}); break;
    default: go(uint64_t{}, mf::Spp<2>{}); break;
    }
}
template <class M>
void mdec_w(const M& md, const mf::DecArgs& a) {
    auto go = [&](auto sym, auto spp) { mf::mdec_of(md, a, mf::kDecTab, sym, spp); };
    switch (a.w) {
    case 1: go(uint8_t{}, mf::Spp<8>{}); break;
    case 2: go(uint16_t{}, mf::Spp<8>{}); break;
    case 4: go(uint32_t{}, mf::Spp<4>{}); break;
    default: go(uint64_t{}, mf::Spp<2>{}); break;
    }
}

// ---- the codecs
// A codec: its exact model (any layout) and, for fixed chunks, its fast launchers.
struct UniformCodec {
    UniformModel ex;
    double bits;
    mf::UniformModel<true> f2;
    mf::UniformModel<false> fg;
    bool pow2;
    LaunchLog* log = nullptr;  // (the launch record covers the table codecs)
    bool fast_ok(int) const { return true; }
    void fast_encode(const mf::EncArgs& a) const {
        if (pow2) menc_w(f2, a);
        else menc_w(fg, a);
    }
    void fast_decode(const mf::DecArgs& a) const {
        if (pow2) mdec_w(f2, a);
        else mdec_w(fg, a);
    }
};
struct LogUniformCodec {
    LogUniformModel ex;
    double bits;
    mf::LogUniformModel f;
    LaunchLog* log = nullptr;
    bool fast_ok(int) const { return true; }
    void fast_encode(const mf::EncArgs& a) const { menc_w(f, a); }
    void fast_decode(const mf::DecArgs& a) const { mdec_w(f, a); }
};

// Independent<Categorical>: ex carries the call's table ids; on the fast kernels (ans_mfast.hpp
// IndepModel) when the set has their images (fast == NULL: the exact kernels alone, the wide-norm
// Categorical's one-table set) and the ids are bytes.  The launchers are their own translation
// units (ans_codecs_indep_{enc,push,dec,pop}.hip, ans_mfast_launch.hpp).
using mf::IndepFast;

struct IndepCodec {
    CatSetModel ex;
    double bits;
    const IndepFast* fast;
    LaunchLog* log = nullptr;  // the context's launch record (ans_launchlog.hpp)
    bool fast_ok(int w) const { return fast && fast->usable && ex.tid8 && w <= 4; }
    void fast_encode(const mf::EncArgs& a) const { mf::indep_fast_encode(*fast, a); }
    void fast_decode(const mf::DecArgs& a) const { mf::indep_fast_decode(*fast, a); }
};

uint64_t bitlen(uint64_t x) { return x ? 64u - static_cast<uint64_t>(__builtin_clzll(x)) : 0u; }

UniformCodec uniform_codec(uint64_t size) {
    UniformCodec c;
    c.ex = UniformModel{size, kMaxMinHead / size};
    c.bits = std::log2(static_cast<double>(size));
    const uint64_t K = kMaxMinHead / size, L = size * K;
    const uint64_t w = shuffle_coding::fast::enc_thr(K, L);
    const uint64_t magic = ~0ull / size;
    const uint32_t l2 = static_cast<uint32_t>(bitlen(size) - 1), hl8 = shuffle_coding::fast::renorm_screen(L);
    c.pow2 = (size & (size - 1)) == 0;
    c.f2 = mf::UniformModel<true>{size, K, L, w, magic, l2, hl8};
    c.fg = mf::UniformModel<false>{size, K, L, w, magic, l2, hl8};
    return c;
}
LogUniformCodec loguniform_codec(uint32_t excl_max_bits) {
    LogUniformCodec c;
    const uint64_t nb = static_cast<uint64_t>(excl_max_bits) + 1;
    c.ex = LogUniformModel{nb, kMaxMinHead / nb};
    c.bits = std::log2(static_cast<double>(nb)) + std::min<double>(excl_max_bits, 47);
    const uint64_t KE = kMaxMinHead / nb, LE = nb * KE;
    c.f = mf::LogUniformModel{nb, KE, LE, nb >= 2 ? 256 * KE - 1 : ~0ull, ~0ull / nb,
                              shuffle_coding::fast::renorm_screen(LE)};
    return c;
}
// Fixed chunks on the device: fast(nfull) runs the full chunks on the fast kernels where the
// codec, the layout and the buffers' alignment allow (fast_ok), exact(c, k, nchunks) the rest (the
// ragged last chunk, or every chunk) on the exact ones, from chunk c = position k on.
template <class Fast, class Exact>
int split_chunks(bool fast_ok, uint64_t n, uint64_t chunk_len, Fast&& fast, Exact&& exact) {
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    const uint64_t nfull = fast_ok ? n / chunk_len : 0;
    if (nfull) {
        if (int rc = fast(nfull)) return rc;
    }
    if (nfull == nchunks) return ANS_OK;
    return exact(nfull, nfull * chunk_len, nchunks - nfull);
}
inline const uint8_t* sym_at(const void* d_syms, uint64_t k, int w) { return static_cast<const uint8_t*>(d_syms) + k * w; }

template <class C>
int codec_dev_encode(const C& cd, const void* d_syms, int w, uint64_t n, uint64_t chunk_len, uint8_t* d_slots,
                     uint64_t cap, uint32_t* d_lens, uint32_t* d_status, ChunkInit ini, hipStream_t s) {
    const uint8_t* d_tid8 = tid8_of(cd.ex);
    LaunchLog* const log = fresh(cd.log);
    return split_chunks(
        cd.fast_ok(w) && fast_layout(chunk_len, w, cap) && aligned16(d_syms) && aligned16(d_tid8) && aligned16(d_slots), n,
        chunk_len,
        [&](uint64_t nfull) {
            cd.fast_encode(mf::EncArgs{d_syms, w, d_tid8, chunk_len, nfull, d_slots, cap, d_lens, d_status, ini, s, log});
            HIP_TRY(hipGetLastError());
            return ANS_OK;
        },
        [&](uint64_t c, uint64_t k, uint64_t nchunks) {
            return dev_encode(at_offset(cd.ex, k), sym_at(d_syms, k, w), w, nullptr, n - k, chunk_len, nchunks,
                              d_slots + c * cap, cap, d_lens + c, d_status, ChunkInit{ini.kind, ini.seed + c}, s, log);
        });
}
// (a container read through d_offsets needs no aligned d_in)
template <class C>
int codec_dev_decode(const C& cd, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t cap, const uint32_t* d_lens,
                     uint64_t n, uint64_t chunk_len, int gen_kind, void* d_syms, int w, uint32_t* d_status,
                     ChunkInit ini, hipStream_t s) {
    const uint8_t* d_tid8 = tid8_of(cd.ex);
    LaunchLog* const log = fresh(cd.log);
    return split_chunks(
        cd.fast_ok(w) && fast_layout(chunk_len, w, cap) && aligned16(d_syms) && aligned16(d_tid8) &&
            (d_offsets || aligned16(d_in)),
        n, chunk_len,
        [&](uint64_t nfull) {
            cd.fast_decode(mf::DecArgs{d_in, cap, d_offsets, d_lens, d_tid8, chunk_len, nfull, gen_kind, d_syms, w, d_status,
                                       ini, s, log});
            HIP_TRY(hipGetLastError());
            return ANS_OK;
        },
        [&](uint64_t c, uint64_t k, uint64_t nchunks) {
            return dev_decode(at_offset(cd.ex, k), d_offsets ? d_in : d_in + c * cap, d_offsets ? d_offsets + c : nullptr,
                              cap, d_lens + c, nullptr, n - k, chunk_len, nchunks, gen_kind,
                              const_cast<uint8_t*>(sym_at(d_syms, k, w)), w, d_status, ChunkInit{ini.kind, ini.seed + c}, s, log);
        });
}

// Resume over fixed chunks: the fast encoder / decoder (k_menc<kRes> / k_mdec<kRes>), then the
// exact kernel's flagged pass for the chunks it handed over (push: messages too short for its
// prologue; pop: zero bytes on top of a message, messages too short for the first pull).
int codec_dev_push(const IndepCodec& cd, const void* d_syms, int w, uint64_t n, uint64_t chunk_len, uint8_t* d_slots,
                   uint64_t cap, uint32_t* d_lens, uint32_t* d_status, hipStream_t s) {
    const uint8_t* d_tid8 = cd.ex.tid8;
    LaunchLog* const log = fresh(cd.log);
    return split_chunks(
        cd.fast_ok(w) && fast_layout(chunk_len, w, cap) && aligned16(d_syms) && aligned16(d_tid8) && aligned16(d_slots), n,
        chunk_len,
        [&](uint64_t nfull) {
            mf::indep_fast_push(*cd.fast,
                                mf::EncArgs{d_syms, w, d_tid8, chunk_len, nfull, d_slots, cap, d_lens, d_status, ChunkInit{}, s, log});
            HIP_TRY(hipGetLastError());
            return dev_push(cd.ex, d_syms, w, nullptr, nfull * chunk_len, chunk_len, nfull, d_slots, cap, d_lens, d_status, s,
                            true, log);
        },
        [&](uint64_t c, uint64_t k, uint64_t nchunks) {
            return dev_push(at_offset(cd.ex, k), sym_at(d_syms, k, w), w, nullptr, n - k, chunk_len, nchunks,
                            d_slots + c * cap, cap, d_lens + c, d_status, s, false, log);
        });
}
int codec_dev_pop(const IndepCodec& cd, uint8_t* d_slots, uint64_t cap, uint32_t* d_lens, uint64_t n, uint64_t chunk_len,
                  void* d_syms, int w, uint32_t* d_status, hipStream_t s) {
    const uint8_t* d_tid8 = cd.ex.tid8;
    LaunchLog* const log = fresh(cd.log);
    return split_chunks(
        cd.fast_ok(w) && fast_layout(chunk_len, w, cap) && aligned16(d_syms) && aligned16(d_tid8) && aligned16(d_slots), n,
        chunk_len,
        [&](uint64_t nfull) {
            mf::indep_fast_pop(*cd.fast, mf::DecArgs{d_slots, cap, nullptr, d_lens, d_tid8, chunk_len, nfull, ANS_GEN_EMPTY,
                                                     d_syms, w, d_status, ChunkInit{}, s, log});
            HIP_TRY(hipGetLastError());
            return dev_pop(cd.ex, d_slots, cap, d_lens, nullptr, nfull * chunk_len, chunk_len, nfull, d_syms, w, d_status, s,
                           true, log);
        },
        [&](uint64_t c, uint64_t k, uint64_t nchunks) {
            return dev_pop(at_offset(cd.ex, k), d_slots + c * cap, cap, d_lens + c, nullptr, n - k, chunk_len, nchunks,
                           const_cast<uint8_t*>(sym_at(d_syms, k, w)), w, d_status, s, false, log);
        });
}

}  // namespace

// ---- the table set
// A table set on the device (Independent<Categorical>, or one wide-norm Categorical).
struct ans_gpu_tableset {
    ans_gpu* g;
    void* d_mem;
    int device;       // g->device, kept here: freeing the set never touches its context
    CatSetModel md;   // device pointers (tid set per call)
    double max_bits;  // largest log2(norm / pmin) over the tables: sizes the slots
    IndepFast fast;   // ans_mfast.hpp images when every table is in the fast range
    std::vector<uint32_t> nsym;  // symbols per table (host copy: argument checks)
    MsetState* mset = nullptr;   // rank tables of the multiset calls (ans_mset.hip), built on first use
    std::vector<ans_tab_info> info = {};  // norm, smallest non-zero mass and first mass per table (host copy)
};

namespace {

// 1/d rounded up (kNormSmall's exact high division step, ans_fast.hpp div_hi)
double rcp_up(uint64_t d) {
    double r = 1.0 / static_cast<double>(d);
    while (std::fma(r, static_cast<double>(d), -1.0) < 0.0) r = std::nextafter(r, 2.0);
    return r;
}

// the norm range of one table (ans_fast.hpp kNormStd / kNormSmall / kNormBig), -1 for norm >= 2^32
int norm_range(uint64_t norm) {
    if (norm >= (1ull << 16) && norm <= (1ull << 31)) return sc::fast::kNormStd;
    if (norm < (1ull << 16)) return sc::fast::kNormSmall;
    return norm < (1ull << 32) ? sc::fast::kNormBig : -1;
}

// The IndepModel LDS images (ans_mfast.hpp) of a set whose tables all have <= 256 symbols and
// norms in one range (ans_fast.hpp kNormStd / kNormSmall / kNormBig); false (exact kernels only)
// otherwise or when the images do not fit.
bool build_indep_fast(ans_gpu* g, const Categorical* const* cats, uint32_t T, IndepFast* f) {
    using u128 = unsigned __int128;
    if (T == 0 || T > mf::kIndMaxTables) return false;
    uint64_t Hmin = kMaxMinHead;  // the lowest head a push starts from (the initial heads are >= 2^56)
    const int nr = norm_range(cats[0]->norm());
    for (uint32_t t = 0; t < T; ++t) {
        const uint64_t nsym = cats[t]->masses.size(), norm = cats[t]->norm();
        if (nsym == 0 || nsym > 256 || nr < 0 || norm_range(norm) != nr) return false;
        Hmin = std::min(Hmin, norm * (kMaxMinHead / norm));
    }
    const bool small = nr == sc::fast::kNormSmall;
    // ---- encoder image (ans_mfast.hpp IndepModel): T x 257 rows {p, cdf, w} of 16 B, the rcp
    // array (8 B per row), {norm_t, its exponent term}, K_t, and (sets with screened rows) a
    // screen per row
    const uint32_t nrow = 257 * T;
    const uint32_t ro = 16 * nrow, no = ro + 8 * nrow, k_off = no + 8 * T, so = k_off + 8 * T;
    std::vector<uint8_t> enc(so + 4 * nrow, 0);
    std::vector<uint32_t> nsyms(T);
    bool rare = false;
    uint32_t kmax = 0;
    for (uint32_t t = 0; t < T; ++t) {
        const Categorical& cat = *cats[t];
        const uint64_t nsym = cat.masses.size(), norm = cat.norm(), K = kMaxMinHead / norm;
        nsyms[t] = static_cast<uint32_t>(nsym);
        // {norm, -0x43300000 norm mod 2^32}: the push's high word takes the raw estimate's
        // exponent off with the product (ans_mfast.hpp IndepModel::push)
        const uint32_t n32[2] = {static_cast<uint32_t>(norm), 0u - 0x43300000u * static_cast<uint32_t>(norm)};
        std::memcpy(&enc[no + 8 * t], n32, 8);
        std::memcpy(&enc[k_off + 8 * t], &K, 8);
        for (uint32_t sy = 0; sy < 257; ++sy) {
            const uint64_t p = sy < nsym ? cat.masses[sy] : 0, cum = sy < nsym ? cat.cummasses[sy] : norm;
            double rcp = 0;
            uint64_t w = 0xFFFFFFFFFFFFFF00ull;  // zero mass: the voted remainder branch records it
            uint32_t screen = 0;
            if (p) {
                rcp = small ? rcp_up(p) : 1.0 / static_cast<double>(p);
                const uint64_t pK = p * K;
                uint32_t j0 = 1;
                while (static_cast<u128>(pK) << (8 * j0) <= Hmin) ++j0;
                const u128 T0 = static_cast<u128>(pK) << (8 * j0);  // the first bound above Hmin
                if (T0 < (static_cast<u128>(1) << 56) || T0 >= (static_cast<u128>(1) << 64)) screen = ~0u;
                else if (pK > Hmin) screen = static_cast<uint32_t>(pK >> 32);
                if (T0 < (static_cast<u128>(1) << 64)) w = static_cast<uint64_t>(T0) + 8 * (j0 - 1);
                if (screen) rare = true;
                uint32_t km = 0;  // most bytes out of any head < 2^64
                while (km < 7 && (~0ull >> (8 * (km + 1))) >= pK) ++km;
                kmax = std::max(kmax, km);
            }
            const uint32_t i = 257 * t + sy, m32 = static_cast<uint32_t>(p), c32 = static_cast<uint32_t>(cum);
            std::memcpy(&enc[16 * i], &m32, 4);
            std::memcpy(&enc[16 * i + 4], &c32, 4);
            std::memcpy(&enc[16 * i + 8], &w, 8);
            std::memcpy(&enc[ro + 8 * i], &rcp, 8);
            std::memcpy(&enc[so + 4 * i], &screen, 4);
        }
    }
    if (!rare) enc.resize(so);  // (no screen array)
    enc.resize((enc.size() + 15) & ~size_t(15), 0);
    const uint32_t enc_bytes = static_cast<uint32_t>(enc.size());
    if (mf::kEncTab + enc_bytes > mf::kLdsMax) return false;
    // ---- decoder images: headers, rows, buckets; bucket widths per table chosen so the image
    // fits `budget` bytes (the headers hold bucket offsets / 8 relative to the image; IndepModel::pop
    // adds the layout's image base, DecLayout::kTab):
    // the 256-lane layout's (room for two workgroups per CU, else one) and, where it fits the
    // 1,024-lane layout's 28 KiB, that one too (ans_mfast.hpp DecLayout)
    const uint32_t rows_bytes = 8 * 257 * T;
    const uint32_t fixed = mf::kIndRowOff + rows_bytes;
    // kLean (ans_mfast.hpp IndepModel): masses and hi32(q) below 2^24, every row's p K >= 2^32
    // (kmax <= 3), and standard-range norms at least 2^20 (the nearest-rounded quotient)
    bool p24 = kmax <= 3;
    for (uint32_t t = 0; t < T; ++t) {
        p24 = p24 && cats[t]->norm() > 256 && (nr != sc::fast::kNormStd || cats[t]->norm() >= (1ull << 20));
        for (uint64_t m : cats[t]->masses) p24 = p24 && m < (1ull << 24);
    }
    auto build_dec = [&](std::initializer_list<uint32_t> budgets, std::vector<uint8_t>& dec) {
        std::vector<uint32_t> us(T);
        auto image_bytes = [&]() {
            uint64_t b = fixed;
            for (uint32_t t = 0; t < T; ++t) b += 8 * (((cats[t]->norm() - 1) >> us[t]) + 1);
            return (b + 15) & ~uint64_t(15);
        };
        bool fits = false;
        for (uint32_t budget : budgets) {
            for (uint32_t t = 0; t < T; ++t) us[t] = static_cast<uint32_t>(std::max<int>(3, static_cast<int>(bitlen(cats[t]->norm())) - 12));
            while (image_bytes() > budget) {  // widen the buckets of the table with the most
                uint32_t best = 0;
                uint64_t most = 0;
                for (uint32_t t = 0; t < T; ++t) {
                    const uint64_t nb = ((cats[t]->norm() - 1) >> us[t]) + 1;
                    if (nb > most) most = nb, best = t;
                }
                if (most <= 1) break;
                ++us[best];
            }
            bool ok = image_bytes() <= budget;
            for (uint32_t t = 0; t < T; ++t) ok = ok && us[t] <= mf::kIndMaxShift;  // rshift >= 10: the 9-bit symbol fits
            if (ok) {
                fits = true;
                break;
            }
        }
        if (!fits) return false;
        if (image_bytes() / 8 >= (1u << (mf::kIndRowShift - mf::kIndBktShift))) return false;  // bucket offsets / 8 in 14 bits
        dec.assign(image_bytes(), 0);
        uint32_t bkt_off = fixed;
        for (uint32_t t = 0; t < T; ++t) {
            const Categorical& cat = *cats[t];
            const uint64_t nsym = cat.masses.size(), norm = cat.norm(), K = kMaxMinHead / norm, L = norm * K;
            auto cdf = [&](uint64_t sy) { return sy < nsym ? cat.cummasses[sy] : norm; };
            for (uint32_t sy = 0; sy < 257; ++sy) {
                const uint32_t row[2] = {static_cast<uint32_t>(cdf(sy)), static_cast<uint32_t>(sy < nsym ? cat.masses[sy] : 0)};
                std::memcpy(&dec[mf::kIndRowOff + 8 * (257 * t + sy)], row, 8);
            }
            // (kLean kNormStd: 1/(8 norm), the 2^49-binade estimate of IndepModel::pop; an exact scaling)
            const double rn = small ? rcp_up(norm) : (nr == sc::fast::kNormStd && p24) ? 0.125 / static_cast<double>(norm)
                                                                                    : 1.0 / static_cast<double>(norm);
            // the 16-B header (ans_mfast.hpp IndepModel: one ds_read_b128 per pop) and L apart
            const uint32_t hdr_w[2] = {static_cast<uint32_t>(norm),
                                       us[t] | ((bkt_off / 8u) << mf::kIndBktShift) | ((257u * t) << mf::kIndRowShift)};
            std::memcpy(&dec[mf::kIndHdrBytes * t], &rn, 8);
            std::memcpy(&dec[mf::kIndHdrBytes * t + 8], hdr_w, 8);
            std::memcpy(&dec[mf::kIndLOff + 8 * t], &L, 8);
            const uint32_t u = us[t];
            const uint64_t nb = ((norm - 1) >> u) + 1;
            uint64_t s0 = 0;
            for (uint64_t j = 0; j < nb; ++j) {
                const uint64_t a = j << u;
                while (s0 + 1 < nsym && cdf(s0 + 1) <= a) ++s0;  // icdf(a): the last s with cdf(s) <= a
                const uint64_t c1 = cdf(s0 + 1), c2 = cdf(s0 + 2);
                const uint32_t w1 = sc::fast::dec_u_word(a, c1, static_cast<uint32_t>(s0), u);
                const uint32_t w2 = sc::fast::dec_u_word(a, c2, 0, u);
                std::memcpy(&dec[bkt_off + 8 * j], &w1, 4);
                std::memcpy(&dec[bkt_off + 8 * j + 4], &w2, 4);
            }
            bkt_off += static_cast<uint32_t>(8 * nb);
        }
        return true;
    };
    std::vector<uint8_t> dec, decw;
    if (!build_dec({mf::kLdsMax / 2 - mf::kDecTab, mf::kLdsMax - mf::kDecTab}, dec)) return false;
    f->lean = p24;
    if (!build_dec({mf::kDecTabW}, decw)) decw.clear();
    f->lean_w = p24;
    const uint32_t dec_bytes = static_cast<uint32_t>(dec.size()), decw_bytes = static_cast<uint32_t>(decw.size());
    // ---- upload: encoder image | decoder image | nsym | 1,024-lane decoder image
    const size_t o_dec = (enc_bytes + 255) & ~size_t(255), o_ns = o_dec + ((dec_bytes + 255) & ~size_t(255));
    const size_t o_decw = o_ns + ((4 * T + 255) & ~size_t(255));
    void* mem = nullptr;
    if (hipSetDevice(g->device) != hipSuccess || hipMalloc(&mem, o_decw + decw_bytes + 16) != hipSuccess) return false;
    char* base = static_cast<char*>(mem);
    if (hipMemcpy(base, enc.data(), enc_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + o_dec, dec.data(), dec_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + o_ns, nsyms.data(), 4 * T, hipMemcpyHostToDevice) != hipSuccess ||
        (decw_bytes && hipMemcpy(base + o_decw, decw.data(), decw_bytes, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipFree(mem);
        return false;
    }
    f->dec_img_w = decw_bytes ? reinterpret_cast<const uint4*>(base + o_decw) : nullptr;
    f->dec_bytes_w = decw_bytes;
    f->ncu = g->ncu;
    f->usable = true;
    f->nr = nr;
    f->rare = rare;
    f->kmax = kmax;
    f->d_mem = mem;
    f->md = mf::IndepModel<false>{reinterpret_cast<const uint4*>(base), reinterpret_cast<const uint4*>(base + o_dec),
                                  reinterpret_cast<const uint32_t*>(base + o_ns), enc_bytes, dec_bytes, k_off, ro, no, so};
    f->enc_wide = enc_bytes <= mf::kEncTabW;
    return true;
}

}  // namespace

// Builds the device tables (also used by ans_gpu_table_create for norms >= 2^32).
int ans_tableset_build(ans_gpu* g, const Categorical* const* cats, uint32_t ntables, ans_gpu_tableset** out) {
    *out = nullptr;
    if (ntables == 0) return ANS_E_ARG;
    std::vector<uint64_t> cum;
    std::vector<uint32_t> bkt;
    std::vector<TabHdr> hdr(ntables);
    std::vector<ans_tab_info> info;
    double max_bits = 0;
    for (uint32_t t = 0; t < ntables; ++t) {
        const Categorical& cat = *cats[t];
        const uint64_t nsym = cat.masses.size(), norm = cat.norm();
        if (nsym == 0 || nsym > 0xFFFFFFFFull || norm == 0 || norm > kMaxMinHead) return ANS_E_NORM_RANGE;
        TabHdr& h = hdr[t];
        h.cum_off = cum.size();
        h.nsym = static_cast<uint32_t>(nsym);
        h.norm = norm;
        h.K = kMaxMinHead / norm;
        uint64_t pmin = ~0ull;
        for (uint64_t s = 0; s < nsym; ++s) {
            cum.push_back(cat.cummasses[s]);
            if (cat.masses[s]) pmin = std::min(pmin, cat.masses[s]);
        }
        cum.push_back(norm);
        cum.push_back(norm);  // one past the sentinel: the icdf walk reads c[s + 1] for s <= nsym
        if (pmin != ~0ull) max_bits = std::max(max_bits, std::log2(static_cast<double>(norm) / static_cast<double>(pmin)));
        info.push_back(ans_tab_info{norm, pmin != ~0ull ? pmin : 0, cat.masses[0]});
        uint32_t bits = 0;
        while (bits < 63 && (1ull << bits) < norm) ++bits;
        h.shift = bits > 12 ? bits - 12 : 0;  // <= 4096 icdf buckets per table
        h.bkt_off = bkt.size();
        const uint64_t nb = ((norm - 1) >> h.shift) + 1;
        for (uint64_t j = 0; j < nb; ++j) bkt.push_back(static_cast<uint32_t>(cat.icdf(j << h.shift).first));
        bkt.push_back(static_cast<uint32_t>(nsym - 1));  // the last bucket's upper bound (cf < norm)
    }
    const size_t o_bkt = (8 * cum.size() + 255) & ~size_t(255);
    const size_t o_hdr = o_bkt + ((4 * bkt.size() + 255) & ~size_t(255));
    const size_t bytes = o_hdr + sizeof(TabHdr) * hdr.size();
    const size_t staged = (bytes + 15) & ~size_t(15);
    HIP_TRY(hipSetDevice(g->device));
    void* mem = nullptr;
    HIP_TRY(hipMalloc(&mem, staged + 16));
    char* base = static_cast<char*>(mem);
    if (hipMemcpy(base, cum.data(), 8 * cum.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + o_bkt, bkt.data(), 4 * bkt.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + o_hdr, hdr.data(), sizeof(TabHdr) * hdr.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(mem);
        return ANS_E_DEVICE;
    }
    auto* ts = new (std::nothrow) ans_gpu_tableset{g, mem, g->device, CatSetModel{reinterpret_cast<const uint64_t*>(base),
                                                                       reinterpret_cast<const uint32_t*>(base + o_bkt),
                                                                       reinterpret_cast<const TabHdr*>(base + o_hdr),
                                                                       nullptr, nullptr, ntables,
                                                                       staged <= kCatLdsMax ? static_cast<uint32_t>(staged) : 0u},
                                                   max_bits, IndepFast{}, {}};
    if (!ts) {
        (void)hipFree(mem);
        return ANS_E_ALLOC;
    }
    ts->nsym.resize(ntables);
    for (uint32_t t = 0; t < ntables; ++t) ts->nsym[t] = hdr[t].nsym;
    ts->info = std::move(info);
    build_indep_fast(g, cats, ntables, &ts->fast);  // (exact kernels only when it declines)
    *out = ts;
    return ANS_OK;
}

// GraphIID per graph (k_graph_encode64 / k_graph_decode64); argument checks are the caller's
// (ans_graph.hip), the table ids are validated here.
static bool graph_tables_ok(const ans_gpu_tableset* ts, const GraphLayout& gl) {
    const uint32_t T = ts->md.ntables;
    if (gl.t_bern >= T || ts->nsym[gl.t_bern] != 2) return false;  // a Bernoulli table
    return (gl.t_node == kNoTable || gl.t_node < T) && (gl.t_edge == kNoTable || gl.t_edge < T);
}
int ans_tableset_graph_encode(ans_gpu_tableset* ts, const GraphLayout& gl, uint64_t num_graphs,
                              const uint32_t* d_node_labels, const uint8_t* d_dense, const uint32_t* d_edge_labels,
                              int gen_kind, uint64_t seed, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                              uint32_t* d_status, hipStream_t s) {
    if (!graph_tables_ok(ts, gl)) return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    k_graph_encode64<<<blocks(num_graphs), kThreads, ts->md.lds_bytes, s>>>(
        ts->md, gl, num_graphs, d_node_labels, d_dense, d_edge_labels, d_slots, slot_cap, d_lens, d_status,
        ChunkInit{gen_kind, seed});
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}
int ans_tableset_graph_decode(ans_gpu_tableset* ts, const GraphLayout& gl, uint64_t num_graphs, const uint8_t* d_in,
                              const uint64_t* d_offsets, const uint32_t* d_lens, int gen_kind, uint64_t seed,
                              uint32_t* d_node_labels, uint8_t* d_dense, uint32_t* d_edge_scratch,
                              uint64_t* d_edge_count, uint32_t* d_status, hipStream_t s) {
    if (!graph_tables_ok(ts, gl)) return ANS_E_ARG;
    if (num_graphs == 0) return ANS_OK;
    k_graph_decode64<<<blocks(num_graphs), kThreads, ts->md.lds_bytes, s>>>(
        ts->md, gl, num_graphs, d_in, d_offsets, d_lens, gen_kind, d_node_labels, d_dense, d_edge_scratch,
        d_edge_count, d_status, ChunkInit{gen_kind, seed});
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}
ans_gpu* ans_tableset_gpu(const ans_gpu_tableset* ts) { return ts->g; }
uint64_t ans_tableset_slot_bytes(const ans_gpu_tableset* ts, uint64_t chunk_len) {
    return slot_bytes(chunk_len, ts->max_bits);
}
void ans_tableset_destroy(ans_gpu_tableset* ts) {
    if (!ts) return;
    (void)hipSetDevice(ts->device);
    (void)hipFree(ts->d_mem);
    if (ts->fast.d_mem) (void)hipFree(ts->fast.d_mem);
    ans_mset_state_free(ts->mset);
    delete ts;
}
const CatSetModel& ans_tableset_model(const ans_gpu_tableset* ts) { return ts->md; }
const std::vector<uint32_t>& ans_tableset_nsyms(const ans_gpu_tableset* ts) { return ts->nsym; }
const std::vector<ans_tab_info>& ans_tableset_info(const ans_gpu_tableset* ts) { return ts->info; }
MsetState*& ans_tableset_mset(ans_gpu_tableset* ts) { return ts->mset; }

// ---- staging: host buffers in and out
namespace {
// table ids as one byte each (sets of at most 256 tables) for the device; ANS_E_ARG when one
// is outside the set
int narrow_tids(const uint32_t* tids, uint64_t n, uint32_t ntables, std::vector<uint8_t>& t8) {
    if (ntables > 256) return ANS_E_ARG;
    t8.resize(n);
    for (uint64_t k = 0; k < n; ++k) {
        if (tids[k] >= ntables) return ANS_E_ARG;
        t8[k] = static_cast<uint8_t>(tids[k]);
    }
    return ANS_OK;
}

// The set's exact model with the host table ids of n positions uploaded: one byte each for sets
// of at most 256 tables, else u32 (ANS_E_ARG for an id outside the set).
int model_with_tids(const ans_gpu_tableset* ts, const uint32_t* tids, uint64_t n, DevBuf& d_tid, CatSetModel& md) {
    md = ts->md;
    if (ts->md.ntables <= 256) {
        std::vector<uint8_t> t8;
        if (int rc = narrow_tids(tids, n, ts->md.ntables, t8)) return rc;
        HIP_TRY(d_tid.alloc(n + 16));
        if (n) HIP_TRY(hipMemcpy(d_tid.p, t8.data(), n, hipMemcpyHostToDevice));
        md.tid8 = d_tid.as<uint8_t>();
        return ANS_OK;
    }
    for (uint64_t k = 0; k < n; ++k)
        if (tids[k] >= ts->md.ntables) return ANS_E_ARG;
    HIP_TRY(d_tid.alloc(4 * n));
    if (n) HIP_TRY(hipMemcpy(d_tid.p, tids, 4 * n, hipMemcpyHostToDevice));
    md.tid = d_tid.as<uint32_t>();
    return ANS_OK;
}

// ... and with ids already on the device, one byte per position (the device-resident entries)
CatSetModel model_with_tid8(const ans_gpu_tableset* ts, const uint8_t* d_tids) {
    CatSetModel md = ts->md;
    md.tid8 = d_tids;
    return md;
}
// the set's codec on a model that carries a call's table ids
IndepCodec indep_codec(const ans_gpu_tableset* ts, const CatSetModel& md) { return IndepCodec{md, ts->max_bits, &ts->fast, &ts->g->last}; }

// Host buffers in and out, synchronous: fixed chunks (starts == NULL: the codec's kernels as
// codec_dev_*) or variable ones (the exact kernels).  Independent's cd.ex carries table ids
// already on the device (model_with_tids).
template <class C>
int host_encode(ans_gpu* g, const C& cd, const void* syms, int w, uint64_t n, uint64_t chunk_len,
                const uint64_t* starts, uint64_t nchunks, ChunkInit ini, uint8_t* out, uint64_t out_cap,
                uint64_t* offsets, uint64_t* lens, uint64_t* total) {
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    uint64_t longest = chunk_len;
    if (starts)
        for (uint64_t c = 0; c < nchunks; ++c) longest = std::max(longest, starts[c + 1] - starts[c]);
    const uint64_t cap = slot_bytes(longest, cd.bits);
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    DevBuf d_syms, d_starts, d_slots, d_lens, d_status;
    HIP_TRY(d_syms.alloc(n * w));
    HIP_TRY(d_slots.alloc(nchunks * cap));
    HIP_TRY(d_lens.alloc(4 * nchunks));
    HIP_TRY(d_status.alloc(4));
    if (n) HIP_TRY(hipMemcpyAsync(d_syms.p, syms, n * w, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_status.p, 0, 4, s));
    int rc;
    if (starts) {
        HIP_TRY(d_starts.alloc(8 * (nchunks + 1)));
        HIP_TRY(hipMemcpyAsync(d_starts.p, starts, 8 * (nchunks + 1), hipMemcpyHostToDevice, s));
        rc = dev_encode(cd.ex, d_syms.p, w, d_starts.as<uint64_t>(), n, chunk_len, nchunks, d_slots.as<uint8_t>(), cap,
                        d_lens.as<uint32_t>(), d_status.as<uint32_t>(), ini, s, fresh(cd.log));
    } else {
        rc = codec_dev_encode(cd, d_syms.p, w, n, chunk_len, d_slots.as<uint8_t>(), cap, d_lens.as<uint32_t>(),
                              d_status.as<uint32_t>(), ini, s);
    }
    if (rc || (rc = read_status(g, d_status.as<uint32_t>(), s))) return rc;
    return download_container(g, d_slots.as<uint8_t>(), cap, d_lens.as<uint32_t>(), nchunks, s, out, out_cap, offsets,
                              lens, total);
}

template <class C>
int host_decode(ans_gpu* g, const C& cd, const uint8_t* in, uint64_t in_len, const uint64_t* offsets,
                const uint64_t* lens, uint64_t n, uint64_t chunk_len, const uint64_t* starts, uint64_t nchunks,
                int gen_kind, ChunkInit ini, void* out, int w) {
    if (nchunks == 0) return ANS_OK;
    if (!in || !offsets || !lens) return ANS_E_ARG;
    std::vector<uint32_t> l32;
    uint64_t lmax = 0;
    int rc = narrow_lens(offsets, lens, nchunks, in_len, l32, &lmax);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    DevStreams d;
    DevBuf d_starts, d_out;
    if ((rc = upload_streams(in, in_len, offsets, l32, s, d))) return rc;
    HIP_TRY(d_out.alloc(n * w));
    if (starts) {
        HIP_TRY(d_starts.alloc(8 * (nchunks + 1)));
        HIP_TRY(hipMemcpyAsync(d_starts.p, starts, 8 * (nchunks + 1), hipMemcpyHostToDevice, s));
        rc = dev_decode(cd.ex, d.in.as<uint8_t>(), d.offs.as<uint64_t>(), 0, d.lens.as<uint32_t>(),
                        d_starts.as<uint64_t>(), n, chunk_len, nchunks, gen_kind, d_out.p, w, d.status.as<uint32_t>(),
                        ini, s, fresh(cd.log));
    } else {
        // the dense container through offsets: the fast decoders read it in place (no slot
        // bound applies, 0 is not a multiple the fast layout accepts: pass the largest stream)
        const uint64_t cap = (lmax + 128) & ~uint64_t(127);
        rc = codec_dev_decode(cd, d.in.as<uint8_t>(), d.offs.as<uint64_t>(), cap, d.lens.as<uint32_t>(), n, chunk_len,
                              gen_kind, d_out.p, w, d.status.as<uint32_t>(), ini, s);
    }
    if (rc || (rc = read_status(g, d.status.as<uint32_t>(), s))) return rc;
    if (n) HIP_TRY(hipMemcpy(out, d_out.p, n * w, hipMemcpyDeviceToHost));
    return ANS_OK;
}

// Resume on host buffers, synchronous: the dense container in is expanded into slots wide enough
// for each result (grow bytes past the longest input message), the chunks are pushed or popped
// in place, and the slots are packed into the container out.  starts == NULL: fixed chunks.
struct ResumeStage {
    DevStreams d;
    DevBuf slots, starts, tid;
    CatSetModel md;
    uint64_t cap = 0;
};
int resume_stage(ans_gpu_tableset* ts, const uint32_t* table_ids, uint64_t n, const uint64_t* starts, uint64_t nchunks,
                 const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens, uint64_t grow,
                 ResumeStage& st) {
    std::vector<uint32_t> l32;
    uint64_t lmax = 0;
    int rc = narrow_lens(in_offsets, in_lens, nchunks, in_len, l32, &lmax);
    if (rc) return rc;
    st.cap = (lmax + grow + 127) & ~uint64_t(127);
    ans_gpu* g = ts->g;
    const hipStream_t s = g->stream;
    if ((rc = model_with_tids(ts, table_ids, n, st.tid, st.md))) return rc;
    if ((rc = upload_streams(in, in_len, in_offsets, l32, s, st.d))) return rc;
    HIP_TRY(st.slots.alloc(nchunks * st.cap));
    if (starts) {
        HIP_TRY(st.starts.alloc(8 * (nchunks + 1)));
        HIP_TRY(hipMemcpyAsync(st.starts.p, starts, 8 * (nchunks + 1), hipMemcpyHostToDevice, s));
    }
    return ans_dev_expand(g, st.d.in.as<uint8_t>(), st.d.offs.as<uint64_t>(), st.d.lens.as<uint32_t>(), nchunks,
                          st.slots.as<uint8_t>(), st.cap, s);
}

int host_push(ans_gpu_tableset* ts, const uint32_t* table_ids, const void* syms, int w, uint64_t n, uint64_t chunk_len,
              const uint64_t* starts, uint64_t nchunks, const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
              const uint64_t* in_lens, uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens,
              uint64_t* total) {
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (!in_offsets || !in_lens || (in_len && !in) || (n && (!syms || !table_ids))) return ANS_E_ARG;
    if (out && (!offsets || !lens)) return ANS_E_ARG;
    uint64_t longest = chunk_len;
    if (starts)
        for (uint64_t c = 0; c < nchunks; ++c) longest = std::max(longest, starts[c + 1] - starts[c]);
    ans_gpu* g = ts->g;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    ResumeStage st;
    int rc = resume_stage(ts, table_ids, n, starts, nchunks, in, in_len, in_offsets, in_lens,
                          slot_bytes(std::max<uint64_t>(longest, 1), ts->max_bits), st);
    if (rc) return rc;
    DevBuf d_syms;
    HIP_TRY(d_syms.alloc(n * w));
    if (n) HIP_TRY(hipMemcpyAsync(d_syms.p, syms, n * w, hipMemcpyHostToDevice, s));
    uint32_t* d_status = st.d.status.as<uint32_t>();
    if (starts)
        rc = dev_push(st.md, d_syms.p, w, st.starts.as<uint64_t>(), n, chunk_len, nchunks, st.slots.as<uint8_t>(), st.cap,
                      st.d.lens.as<uint32_t>(), d_status, s, false, fresh(&g->last));
    else
        rc = codec_dev_push(indep_codec(ts, st.md), d_syms.p, w, n, chunk_len, st.slots.as<uint8_t>(), st.cap,
                            st.d.lens.as<uint32_t>(), d_status, s);
    if (rc || (rc = read_status(g, d_status, s))) return rc;
    return download_container(g, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), nchunks, s, out, out_cap,
                              offsets, lens, total);
}

int host_pop(ans_gpu_tableset* ts, const uint32_t* table_ids, const uint8_t* in, uint64_t in_len,
             const uint64_t* in_offsets, const uint64_t* in_lens, uint64_t n, uint64_t chunk_len, const uint64_t* starts,
             uint64_t nchunks, void* out_syms, int w, uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens,
             uint64_t* total) {
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (!in_offsets || !in_lens || (in_len && !in) || (n && (!out_syms || !table_ids))) return ANS_E_ARG;
    if (out && (!offsets || !lens)) return ANS_E_ARG;
    ans_gpu* g = ts->g;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    ResumeStage st;
    int rc = resume_stage(ts, table_ids, n, starts, nchunks, in, in_len, in_offsets, in_lens, 16, st);
    if (rc) return rc;
    DevBuf d_syms;
    HIP_TRY(d_syms.alloc(n * w));
    uint32_t* d_status = st.d.status.as<uint32_t>();
    if (starts)
        rc = dev_pop(st.md, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), st.starts.as<uint64_t>(), n,
                     chunk_len, nchunks, d_syms.p, w, d_status, s, false, fresh(&g->last));
    else
        rc = codec_dev_pop(indep_codec(ts, st.md), st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), n, chunk_len,
                           d_syms.p, w, d_status, s);
    if (rc || (rc = read_status(g, d_status, s))) return rc;
    if (n) HIP_TRY(hipMemcpy(out_syms, d_syms.p, n * w, hipMemcpyDeviceToHost));
    return download_container(g, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), nchunks, s, out, out_cap,
                              offsets, lens, total);
}
}  // namespace

// IID<Categorical> with a wide norm through a one-table set (ans_kernels.hip's launchers): the
// exact kernels alone
int ans_tableset_dev_encode(ans_gpu_tableset* ts, const void* d_syms, int w, const uint64_t* d_starts, uint64_t n,
                            uint64_t chunk_len, uint64_t nchunks, uint8_t* d_slots, uint64_t slot_cap,
                            uint32_t* d_lens, uint32_t* d_status, int gen_kind, uint64_t seed, void* stream) {
    return dev_encode(ts->md, d_syms, w, d_starts, n, chunk_len, nchunks, d_slots, slot_cap, d_lens, d_status,
                      ChunkInit{gen_kind, seed}, static_cast<hipStream_t>(stream), fresh(&ts->g->last));
}
int ans_tableset_dev_decode(ans_gpu_tableset* ts, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t slot_cap,
                            const uint32_t* d_lens, const uint64_t* d_starts, uint64_t n, uint64_t chunk_len,
                            uint64_t nchunks, int gen_kind, uint64_t seed, void* d_syms, int w, uint32_t* d_status,
                            void* stream) {
    return dev_decode(ts->md, d_in, d_offsets, slot_cap, d_lens, d_starts, n, chunk_len, nchunks, gen_kind, d_syms, w,
                      d_status, ChunkInit{gen_kind, seed}, static_cast<hipStream_t>(stream), fresh(&ts->g->last));
}
int ans_tableset_host_encode(ans_gpu_tableset* ts, const void* syms, int w, uint64_t n, uint64_t chunk_len,
                             const uint64_t* starts, uint64_t nchunks, int gen_kind, uint64_t seed, uint8_t* out,
                             uint64_t out_cap, uint64_t* offsets, uint64_t* lens, uint64_t* total) {
    return host_encode(ts->g, IndepCodec{ts->md, ts->max_bits, nullptr, &ts->g->last}, syms, w, n, chunk_len, starts, nchunks,
                       ChunkInit{gen_kind, seed}, out, out_cap, offsets, lens, total);
}
int ans_tableset_host_decode(ans_gpu_tableset* ts, const uint8_t* in, uint64_t in_len, const uint64_t* offsets,
                             const uint64_t* lens, uint64_t n, uint64_t chunk_len, const uint64_t* starts,
                             uint64_t nchunks, int gen_kind, uint64_t seed, void* out, int w) {
    return host_decode(ts->g, IndepCodec{ts->md, ts->max_bits, nullptr, &ts->g->last}, in, in_len, offsets, lens, n, chunk_len, starts,
                       nchunks, gen_kind, ChunkInit{gen_kind, seed}, out, w);
}

// ====================================================================== C ABI
extern "C" {

int ans_gpu_uniform_encode_chunks(ans_gpu* g, uint64_t size, const void* syms, int sym_bytes, uint64_t n,
                                  uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t* out, uint64_t out_cap,
                                  uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !total || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || (n && !syms))
        return ANS_E_ARG;
    if (size == 0 || size > kMaxSize) return ANS_E_NORM_RANGE;  // Uniform::new asserts size <= MAX_SIZE
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    if (out && nchunks && (!offsets || !lens)) return ANS_E_ARG;
    return host_encode(g, uniform_codec(size), syms, sym_bytes, n, chunk_len, nullptr, nchunks,
                       ChunkInit{gen_kind, seed}, out, out_cap, offsets, lens, total);
} ANS_CATCH

int ans_gpu_uniform_decode_chunks(ans_gpu* g, uint64_t size, const uint8_t* in, uint64_t in_len,
                                  const uint64_t* offsets, const uint64_t* lens, uint64_t n, uint64_t chunk_len,
                                  int gen_kind, uint64_t seed, void* out, int sym_bytes) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || (n && !out)) return ANS_E_ARG;
    if (size == 0 || size > kMaxSize) return ANS_E_NORM_RANGE;
    return host_decode(g, uniform_codec(size), in, in_len, offsets, lens, n, chunk_len, nullptr,
                       (n + chunk_len - 1) / chunk_len, gen_kind, ChunkInit{gen_kind, seed}, out, sym_bytes);
} ANS_CATCH

int ans_gpu_loguniform_encode_chunks(ans_gpu* g, uint32_t excl_max_bits, const void* syms, int sym_bytes, uint64_t n,
                                     uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t* out, uint64_t out_cap,
                                     uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !total || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || (n && !syms))
        return ANS_E_ARG;
    if (excl_max_bits > 64) return ANS_E_NORM_RANGE;  // LogUniform::new asserts excl_max_bits <= 64
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    if (out && nchunks && (!offsets || !lens)) return ANS_E_ARG;
    return host_encode(g, loguniform_codec(excl_max_bits), syms, sym_bytes, n, chunk_len, nullptr, nchunks,
                       ChunkInit{gen_kind, seed}, out, out_cap, offsets, lens, total);
} ANS_CATCH

int ans_gpu_loguniform_decode_chunks(ans_gpu* g, uint32_t excl_max_bits, const uint8_t* in, uint64_t in_len,
                                     const uint64_t* offsets, const uint64_t* lens, uint64_t n, uint64_t chunk_len,
                                     int gen_kind, uint64_t seed, void* out, int sym_bytes) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || (n && !out)) return ANS_E_ARG;
    if (excl_max_bits > 64) return ANS_E_NORM_RANGE;
    return host_decode(g, loguniform_codec(excl_max_bits), in, in_len, offsets, lens, n, chunk_len, nullptr,
                       (n + chunk_len - 1) / chunk_len, gen_kind, ChunkInit{gen_kind, seed}, out, sym_bytes);
} ANS_CATCH

int ans_gpu_tableset_create(ans_gpu* g, const ans_table* const* tables, uint32_t ntables, ans_gpu_tableset** out) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !tables || !out || ntables == 0) return ANS_E_ARG;
    std::vector<const Categorical*> cats(ntables);
    for (uint32_t t = 0; t < ntables; ++t) {
        if (!tables[t]) return ANS_E_ARG;
        cats[t] = &tables[t]->cat;
    }
    return ans_tableset_build(g, cats.data(), ntables, out);
} ANS_CATCH

void ans_gpu_tableset_free(ans_gpu_tableset* ts) { ans_tableset_destroy(ts); }

int ans_gpu_independent_encode_chunks(ans_gpu_tableset* ts, const uint32_t* table_ids, const void* syms, int sym_bytes,
                                      uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t* out,
                                      uint64_t out_cap, uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind)) return ANS_E_ARG;
    if (n && (!syms || !table_ids)) return ANS_E_ARG;
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    if (out && nchunks && (!offsets || !lens)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(ts->g->device));
    DevBuf d_tid;
    CatSetModel md;
    if (int rc = model_with_tids(ts, table_ids, n, d_tid, md)) return rc;
    return host_encode(ts->g, indep_codec(ts, md), syms, sym_bytes, n, chunk_len, nullptr, nchunks,
                       ChunkInit{gen_kind, seed}, out, out_cap, offsets, lens, total);
} ANS_CATCH

int ans_gpu_independent_decode_chunks(ans_gpu_tableset* ts, const uint32_t* table_ids, const uint8_t* in,
                                      uint64_t in_len, const uint64_t* offsets, const uint64_t* lens, uint64_t n,
                                      uint64_t chunk_len, int gen_kind, uint64_t seed, void* out, int sym_bytes) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind)) return ANS_E_ARG;
    if (n && (!out || !table_ids)) return ANS_E_ARG;
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    HIP_TRY(hipSetDevice(ts->g->device));
    DevBuf d_tid;
    CatSetModel md;
    if (int rc = model_with_tids(ts, table_ids, n, d_tid, md)) return rc;
    return host_decode(ts->g, indep_codec(ts, md), in, in_len, offsets, lens, n, chunk_len, nullptr, nchunks, gen_kind,
                       ChunkInit{gen_kind, seed}, out, sym_bytes);
} ANS_CATCH

// Independent<Categorical> over variable-length chunks: chunk c is positions [starts[c], starts[c+1])
// (the exact kernels, one lane per chunk)
static int var_starts_ok(uint64_t nchunks, const uint64_t* starts) {
    for (uint64_t c = 0; c < nchunks; ++c)
        if (starts[c + 1] < starts[c]) return ANS_E_ARG;
    return ANS_OK;
}
int ans_gpu_independent_encode_var_chunks(ans_gpu_tableset* ts, const uint32_t* table_ids, const void* syms,
                                          int sym_bytes, uint64_t nchunks, const uint64_t* starts, int gen_kind,
                                          uint64_t seed, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                                          uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u64(sym_bytes) || !valid_kind(gen_kind) || (nchunks && !starts)) return ANS_E_ARG;
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (int rc = var_starts_ok(nchunks, starts)) return rc;
    if (out && (!offsets || !lens)) return ANS_E_ARG;
    const uint64_t n = starts[nchunks];
    if (n && (!syms || !table_ids)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(ts->g->device));
    DevBuf d_tid;
    CatSetModel md;
    if (int rc = model_with_tids(ts, table_ids, n, d_tid, md)) return rc;
    return host_encode(ts->g, indep_codec(ts, md), syms, sym_bytes, n, 0, starts, nchunks, ChunkInit{gen_kind, seed}, out,
                       out_cap, offsets, lens, total);
} ANS_CATCH

int ans_gpu_independent_decode_var_chunks(ans_gpu_tableset* ts, const uint32_t* table_ids, const uint8_t* in,
                                          uint64_t in_len, const uint64_t* offsets, const uint64_t* lens,
                                          uint64_t nchunks, const uint64_t* starts, int gen_kind, uint64_t seed,
                                          void* out, int sym_bytes) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || !valid_kind(gen_kind) || (nchunks && !starts)) return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    if (int rc = var_starts_ok(nchunks, starts)) return rc;
    const uint64_t n = starts[nchunks];
    if (n && (!out || !table_ids)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(ts->g->device));
    DevBuf d_tid;
    CatSetModel md;
    if (int rc = model_with_tids(ts, table_ids, n, d_tid, md)) return rc;
    return host_decode(ts->g, indep_codec(ts, md), in, in_len, offsets, lens, n, 0, starts, nchunks, gen_kind,
                       ChunkInit{gen_kind, seed}, out, sym_bytes);
} ANS_CATCH

// device-resident: d_tids one byte per position, d_starts nchunks + 1 entries (device)
int ans_dev_independent_encode_var(ans_gpu_tableset* ts, const uint8_t* d_tids, const void* d_syms, int sym_bytes,
                                   uint64_t nchunks, const uint64_t* d_starts, int gen_kind, uint64_t seed,
                                   uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status,
                                   void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || !valid_kind(gen_kind) || ts->md.ntables > 256 || !d_status ||
        (nchunks && (!d_starts || !d_syms || !d_tids || !d_slots || !d_lens)))
        return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(ts->g->device));
    return dev_encode(model_with_tid8(ts, d_tids), d_syms, sym_bytes, d_starts, 0, 0, nchunks, d_slots, slot_cap, d_lens, d_status,
                      ChunkInit{gen_kind, seed}, stream_of(ts->g, stream), fresh(&ts->g->last));
} ANS_CATCH
int ans_dev_independent_decode_var(ans_gpu_tableset* ts, const uint8_t* d_tids, const uint8_t* d_in,
                                   const uint64_t* d_offsets, uint64_t slot_cap, const uint32_t* d_lens,
                                   uint64_t nchunks, const uint64_t* d_starts, int gen_kind, uint64_t seed,
                                   void* d_syms, int sym_bytes, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || !valid_kind(gen_kind) || ts->md.ntables > 256 || !d_status ||
        (nchunks && (!d_starts || !d_syms || !d_tids || !d_in || !d_lens)))
        return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(ts->g->device));
    return dev_decode(model_with_tid8(ts, d_tids), d_in, d_offsets, slot_cap, d_lens, d_starts, 0, 0, nchunks, gen_kind, d_syms, sym_bytes,
                      d_status, ChunkInit{gen_kind, seed}, stream_of(ts->g, stream), fresh(&ts->g->last));
} ANS_CATCH

// ---- device-resident entries (include/ans_capi.h section 4b): fixed chunks in slots
int ans_gpu_uniform_slot_capacity(uint64_t size, uint64_t chunk_len, uint64_t* slot_cap) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!slot_cap || chunk_len == 0) return ANS_E_ARG;
    if (size == 0 || size > kMaxSize) return ANS_E_NORM_RANGE;
    *slot_cap = slot_bytes(chunk_len, std::log2(static_cast<double>(size)));
    return ANS_OK;
} ANS_CATCH
int ans_gpu_loguniform_slot_capacity(uint32_t excl_max_bits, uint64_t chunk_len, uint64_t* slot_cap) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!slot_cap || chunk_len == 0) return ANS_E_ARG;
    if (excl_max_bits > 64) return ANS_E_NORM_RANGE;
    *slot_cap = slot_bytes(chunk_len, loguniform_codec(excl_max_bits).bits);
    return ANS_OK;
} ANS_CATCH
int ans_gpu_tableset_slot_capacity(const ans_gpu_tableset* ts, uint64_t chunk_len, uint64_t* slot_cap) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !slot_cap || chunk_len == 0) return ANS_E_ARG;
    *slot_cap = slot_bytes(chunk_len, ts->max_bits);
    return ANS_OK;
} ANS_CATCH
int ans_gpu_tableset_lanes(ans_gpu_tableset* ts, int lanes) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || (lanes != 0 && lanes != mf::kLanes && lanes != mf::kLanesW)) return ANS_E_ARG;
    if (lanes == mf::kLanesW && !ts->fast.dec_img_w && !ts->fast.enc_wide) return ANS_E_ARG;
    ts->fast.lanes = lanes;
    return ANS_OK;
} ANS_CATCH

int ans_gpu_tableset_fast(const ans_gpu_tableset* ts, int* fast) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !fast) return ANS_E_ARG;
    *fast = ts->fast.usable ? (ts->fast.rare ? 2 : 1) : 0;
    return ANS_OK;
} ANS_CATCH

int ans_dev_uniform_encode(ans_gpu* g, uint64_t size, const void* d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                           int gen_kind, uint64_t seed, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                           uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || (n && (!d_syms || !d_slots || !d_lens)) ||
        !d_status)
        return ANS_E_ARG;
    if (size == 0 || size > kMaxSize) return ANS_E_NORM_RANGE;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return codec_dev_encode(uniform_codec(size), d_syms, sym_bytes, n, chunk_len, d_slots, slot_cap, d_lens,
                            d_status, ChunkInit{gen_kind, seed}, stream_of(g, stream));
} ANS_CATCH
int ans_dev_uniform_decode(ans_gpu* g, uint64_t size, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t slot_cap,
                           const uint32_t* d_lens, uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed,
                           void* d_syms, int sym_bytes, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || (n && (!d_in || !d_lens || !d_syms)) ||
        !d_status)
        return ANS_E_ARG;
    if (size == 0 || size > kMaxSize) return ANS_E_NORM_RANGE;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return codec_dev_decode(uniform_codec(size), d_in, d_offsets, slot_cap, d_lens, n, chunk_len, gen_kind,
                            d_syms, sym_bytes, d_status, ChunkInit{gen_kind, seed},
                            stream_of(g, stream));
} ANS_CATCH
int ans_dev_loguniform_encode(ans_gpu* g, uint32_t excl_max_bits, const void* d_syms, int sym_bytes, uint64_t n,
                              uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t* d_slots, uint64_t slot_cap,
                              uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || (n && (!d_syms || !d_slots || !d_lens)) ||
        !d_status)
        return ANS_E_ARG;
    if (excl_max_bits > 64) return ANS_E_NORM_RANGE;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return codec_dev_encode(loguniform_codec(excl_max_bits), d_syms, sym_bytes, n, chunk_len, d_slots,
                            slot_cap, d_lens, d_status, ChunkInit{gen_kind, seed},
                            stream_of(g, stream));
} ANS_CATCH
int ans_dev_loguniform_decode(ans_gpu* g, uint32_t excl_max_bits, const uint8_t* d_in, const uint64_t* d_offsets,
                              uint64_t slot_cap, const uint32_t* d_lens, uint64_t n, uint64_t chunk_len, int gen_kind,
                              uint64_t seed, void* d_syms, int sym_bytes, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || (n && (!d_in || !d_lens || !d_syms)) ||
        !d_status)
        return ANS_E_ARG;
    if (excl_max_bits > 64) return ANS_E_NORM_RANGE;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    return codec_dev_decode(loguniform_codec(excl_max_bits), d_in, d_offsets, slot_cap, d_lens, n, chunk_len,
                            gen_kind, d_syms, sym_bytes, d_status, ChunkInit{gen_kind, seed},
                            stream_of(g, stream));
} ANS_CATCH
// d_tids: one byte per position (sets of at most 256 tables); table ids are not range-checked
// on the device: an id outside the set is undefined behaviour, as an index past the reference's
// codec vector would panic (src/codec.rs:388-391)
int ans_dev_independent_encode(ans_gpu_tableset* ts, const uint8_t* d_tids, const void* d_syms, int sym_bytes,
                               uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t* d_slots,
                               uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || ts->md.ntables > 256 ||
        (n && (!d_syms || !d_tids || !d_slots || !d_lens)) || !d_status)
        return ANS_E_ARG;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(ts->g->device));
    return codec_dev_encode(indep_codec(ts, model_with_tid8(ts, d_tids)), d_syms, sym_bytes, n, chunk_len, d_slots, slot_cap, d_lens, d_status,
                            ChunkInit{gen_kind, seed}, stream_of(ts->g, stream));
} ANS_CATCH
int ans_dev_independent_decode(ans_gpu_tableset* ts, const uint8_t* d_tids, const uint8_t* d_in,
                               const uint64_t* d_offsets, uint64_t slot_cap, const uint32_t* d_lens, uint64_t n,
                               uint64_t chunk_len, int gen_kind, uint64_t seed, void* d_syms, int sym_bytes,
                               uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind) || ts->md.ntables > 256 ||
        (n && (!d_in || !d_tids || !d_lens || !d_syms)) || !d_status)
        return ANS_E_ARG;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(ts->g->device));
    return codec_dev_decode(indep_codec(ts, model_with_tid8(ts, d_tids)), d_in, d_offsets, slot_cap, d_lens, n, chunk_len, gen_kind, d_syms, sym_bytes,
                            d_status, ChunkInit{gen_kind, seed}, stream_of(ts->g, stream));
} ANS_CATCH

// ---- resume (include/ans_capi.h section 4b): push onto / pop from the messages in the slots
int ans_dev_independent_push(ans_gpu_tableset* ts, const uint8_t* d_tids, const void* d_syms, int sym_bytes, uint64_t n,
                             uint64_t chunk_len, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                             uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || chunk_len == 0 || ts->md.ntables > 256 ||
        (n && (!d_syms || !d_tids || !d_slots || !d_lens)) || !d_status)
        return ANS_E_ARG;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(ts->g->device));
    return codec_dev_push(indep_codec(ts, model_with_tid8(ts, d_tids)), d_syms, sym_bytes, n, chunk_len, d_slots, slot_cap, d_lens, d_status,
                          stream_of(ts->g, stream));
} ANS_CATCH
int ans_dev_independent_pop(ans_gpu_tableset* ts, const uint8_t* d_tids, uint8_t* d_slots, uint64_t slot_cap,
                            uint32_t* d_lens, uint64_t n, uint64_t chunk_len, void* d_syms, int sym_bytes,
                            uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || chunk_len == 0 || ts->md.ntables > 256 || slot_cap < 16 ||
        (n && (!d_syms || !d_tids || !d_slots || !d_lens)) || !d_status)
        return ANS_E_ARG;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(ts->g->device));
    return codec_dev_pop(indep_codec(ts, model_with_tid8(ts, d_tids)), d_slots, slot_cap, d_lens, n, chunk_len, d_syms, sym_bytes, d_status,
                         stream_of(ts->g, stream));
} ANS_CATCH
int ans_dev_independent_push_var(ans_gpu_tableset* ts, const uint8_t* d_tids, const void* d_syms, int sym_bytes,
                                 uint64_t nchunks, const uint64_t* d_starts, uint8_t* d_slots, uint64_t slot_cap,
                                 uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || ts->md.ntables > 256 || !d_status ||
        (nchunks && (!d_starts || !d_syms || !d_tids || !d_slots || !d_lens)))
        return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(ts->g->device));
    return dev_push(model_with_tid8(ts, d_tids), d_syms, sym_bytes, d_starts, 0, 0, nchunks, d_slots, slot_cap, d_lens, d_status,
                    stream_of(ts->g, stream), false, fresh(&ts->g->last));
} ANS_CATCH
int ans_dev_independent_pop_var(ans_gpu_tableset* ts, const uint8_t* d_tids, uint8_t* d_slots, uint64_t slot_cap,
                                uint32_t* d_lens, uint64_t nchunks, const uint64_t* d_starts, void* d_syms,
                                int sym_bytes, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u64(sym_bytes) || ts->md.ntables > 256 || !d_status || slot_cap < 16 ||
        (nchunks && (!d_starts || !d_syms || !d_tids || !d_slots || !d_lens)))
        return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(ts->g->device));
    return dev_pop(model_with_tid8(ts, d_tids), d_slots, slot_cap, d_lens, d_starts, 0, 0, nchunks, d_syms, sym_bytes, d_status,
                   stream_of(ts->g, stream), false, fresh(&ts->g->last));
} ANS_CATCH

int ans_gpu_independent_push_chunks(ans_gpu_tableset* ts, const uint32_t* table_ids, const void* syms, int sym_bytes,
                                    uint64_t n, uint64_t chunk_len, const uint8_t* in, uint64_t in_len,
                                    const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out, uint64_t out_cap,
                                    uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u64(sym_bytes) || chunk_len == 0) return ANS_E_ARG;
    return host_push(ts, table_ids, syms, sym_bytes, n, chunk_len, nullptr, (n + chunk_len - 1) / chunk_len, in, in_len,
                     in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_independent_pop_chunks(ans_gpu_tableset* ts, const uint32_t* table_ids, const uint8_t* in, uint64_t in_len,
                                   const uint64_t* in_offsets, const uint64_t* in_lens, uint64_t n, uint64_t chunk_len,
                                   void* out_syms, int sym_bytes, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                                   uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u64(sym_bytes) || chunk_len == 0) return ANS_E_ARG;
    return host_pop(ts, table_ids, in, in_len, in_offsets, in_lens, n, chunk_len, nullptr,
                    (n + chunk_len - 1) / chunk_len, out_syms, sym_bytes, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_independent_push_var_chunks(ans_gpu_tableset* ts, const uint32_t* table_ids, const void* syms, int sym_bytes,
                                        uint64_t nchunks, const uint64_t* starts, const uint8_t* in, uint64_t in_len,
                                        const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out,
                                        uint64_t out_cap, uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u64(sym_bytes) || (nchunks && !starts)) return ANS_E_ARG;
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (int rc = var_starts_ok(nchunks, starts)) return rc;
    return host_push(ts, table_ids, syms, sym_bytes, starts[nchunks], 0, starts, nchunks, in, in_len, in_offsets,
                     in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_independent_pop_var_chunks(ans_gpu_tableset* ts, const uint32_t* table_ids, const uint8_t* in,
                                       uint64_t in_len, const uint64_t* in_offsets, const uint64_t* in_lens,
                                       uint64_t nchunks, const uint64_t* starts, void* out_syms, int sym_bytes,
                                       uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens,
                                       uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u64(sym_bytes) || (nchunks && !starts)) return ANS_E_ARG;
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (int rc = var_starts_ok(nchunks, starts)) return rc;
    return host_pop(ts, table_ids, in, in_len, in_offsets, in_lens, starts[nchunks], 0, starts, nchunks, out_syms,
                    sym_bytes, out, out_cap, offsets, lens, total);
} ANS_CATCH

}  // extern "C"
