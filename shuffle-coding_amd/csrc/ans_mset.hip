// ans_mset.hip — recursive multiset shuffle coding in bulk, one multiset per chunk, one lane per
// chunk: ShuffleCodec<IIDVecSliceCodecs<Categorical>, VecOrbitCodecs> (src/recursive/mod.rs:117-148,
// src/recursive/multiset.rs:13-91,139-141) under the resume contract of include/ans_capi.h 4b.
// Chunk c's message is Message::unflatten(slot bytes) with the Empty tail.
//   push: the chunk's values are counted per rank (ans_mset.hpp); then for L = n .. 1 a rank is
//         POPPED from the message under the orbit distribution of the L values left (norm L,
//         pmf = the rank's count), its count drops by one, and the rank's symbol is pushed under
//         the table; flatten.
//   pop:  for k = 0 .. n-1 a symbol is popped under the table, its rank's count rises by one, and
//         the rank is PUSHED under the orbit distribution of the k + 1 values so far; flatten.
// The table side is ans_exact.hpp's (CatSetModel::push / pop on PushT<true> / PopT<RSource>); what
// is new here is the orbit pop on the sink-side message, the orbit push on the source-side one and
// the per-lane counts: lane-interleaved u16 in LDS (alphabets up to 1,024 symbols, chunks up to
// 65,535 values), or u32 in a workspace the context owns, sized by the lanes resident.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ans_ctx.hpp"
#include "ans_exact.hpp"
#include "ans_hostio.hpp"
#include "ans_mset.hpp"

using namespace shuffle_coding::exact;
namespace ms = shuffle_coding::mset;

// a set's rank tables, one pair per table coded as a multiset so far (device memory of the set's)
struct MsetState {
    struct Tab {
        uint32_t* d_rank = nullptr;  // rank[s] | sym_of_rank[r], nsym entries each
        int state = 0;               // 0: not built; 1: built; -1: two symbols share an orbit id
    };
    std::vector<Tab> tabs;
};
void ans_mset_state_free(MsetState* st) {
    if (!st) return;
    for (auto& t : st->tabs)
        if (t.d_rank) (void)hipFree(t.d_rank);
    delete st;
}

namespace {

#define HIP_TRY(expr) ANS_HIP_TRY(expr)

constexpr uint32_t kLdsAll = 160 * 1024;     // one CU's LDS
constexpr uint32_t kLdsCounts = 128 * 1024;  // the most the counts take of it: 1,024 symbols x 64 lanes x u16
constexpr uint32_t kLdsMaxLen = 65535;       // the longest chunk a u16 count holds
constexpr size_t kWsMax = size_t(256) << 20; // the global counts' workspace never passes this
constexpr int kPrefetch = 8;

// The counts' nodes of one lane.  LDS: node i of lane l is the u16 at index i * 64 + l, so the
// lanes of a wave reading one node (the top of every walk) read 32 consecutive dwords, one bank
// each, and lanes on different nodes spread over the banks by lane.  Global: node i of lane l at
// i * lanes + l, so a wave on one node reads one 256-B line.
struct LdsCnt {
    uint16_t* p;
    __device__ uint32_t load(uint32_t i) const { return p[i * kThreads]; }
    __device__ void store(uint32_t i, uint32_t v) { p[i * kThreads] = static_cast<uint16_t>(v); }
    __device__ static LdsCnt make(unsigned char* lds, uint32_t off, uint32_t*, uint64_t, uint64_t) {
        return LdsCnt{reinterpret_cast<uint16_t*>(lds + off) + threadIdx.x};
    }
};
struct GlobalCnt {
    uint32_t* p;
    uint64_t stride;
    __device__ uint32_t load(uint32_t i) const { return p[i * stride]; }
    __device__ void store(uint32_t i, uint32_t v) { p[i * stride] = v; }
    __device__ static GlobalCnt make(unsigned char*, uint32_t, uint32_t* ws, uint64_t lane, uint64_t lanes) {
        return GlobalCnt{ws + lane, lanes};
    }
};

struct MsetTab {
    const uint32_t* rank;         // rank[s]
    const uint32_t* sym_of_rank;  // its inverse
    uint32_t table, nsym;
    uint32_t cnt_off;  // the counts' offset in dynamic LDS (after the staged table set)
    uint32_t max_len;  // the longest chunk the counts hold
};

// ---- push: grid-stride over the chunks, lane = one chunk at a time
template <typename Sym, class Cnt>
__global__ __launch_bounds__(kThreads) void k_mset_push(CatSetModel md, MsetTab mt, const Sym* __restrict__ syms,
                                                         const uint64_t* starts, uint64_t n, uint64_t chunk_len,
                                                         uint64_t nchunks, uint8_t* slots, uint64_t slot_cap,
                                                         uint32_t* lens, uint32_t* __restrict__ status, uint32_t* ws) {
    extern __shared__ __align__(16) unsigned char lds[];
    md.stage(lds);
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    ms::Counts<Cnt> cnt{Cnt::make(lds, mt.cnt_off, ws, lane, lanes), mt.nsym};
    for (uint64_t c = lane; c < nchunks; c += lanes) {
        const uint64_t a = starts ? starts[c] : c * chunk_len;
        const uint64_t b = starts ? starts[c + 1] : min(a + chunk_len, n);
        auto fail = [&](int code) {
            raise(status, code);
            lens[c] = 0;
        };
        const uint32_t len0 = lens[c];
        if (len0 > slot_cap || b - a > mt.max_len) {
            fail(ANS_E_LEN);
            continue;
        }
        // the histogram per rank; the symbols and their ranks are loaded a block ahead
        cnt.clear();
        uint32_t cur[kPrefetch], nxt[kPrefetch];
        auto load_block = [&](uint32_t* r, uint64_t k0) {  // ranks of positions k0, k0 + 1, ... (those < b)
#pragma unroll
            for (int i = 0; i < kPrefetch; ++i)
                if (k0 + i < b) {
                    const uint64_t x = syms[k0 + i];
                    r[i] = x < mt.nsym ? mt.rank[x] : 0xFFFFFFFFu;
                }
        };
        load_block(cur, a);
        bool bad = false;
        for (uint64_t k0 = a; k0 < b && !bad; k0 += kPrefetch) {
            if (k0 + kPrefetch < b) load_block(nxt, k0 + kPrefetch);
#pragma unroll
            for (int i = 0; i < kPrefetch; ++i) {
                if (k0 + i >= b) break;
                if (cur[i] >= mt.nsym) {
                    bad = true;  // src/codec.rs:63
                    break;
                }
                cnt.tally(cur[i]);
            }
#pragma unroll
            for (int i = 0; i < kPrefetch; ++i) cur[i] = nxt[i];
        }
        if (bad) {
            fail(ANS_E_SYMBOL);
            continue;
        }
        cnt.build();
        Sink sink(slots + c * slot_cap, slot_cap, len0);
        PushT<true> m{0, &sink, 0};  // Message::unflatten: head 0
        int err = ANS_OK;
        for (uint64_t L = b - a; L > 0; --L) {
            // the blanket pop (src/ans.rs:107-116) under the orbit distribution, norm L, on the
            // message whose tail is the sink: renorm(L K), up then down (src/ans.rs:233-253)
            const uint64_t bound = L * (kMaxMinHead / L);
            while (m.head < bound) {
                uint32_t byte = 0;
                if (!sink.pop(byte)) {
                    err = ANS_E_EXHAUSTED;  // src/ans.rs:144
                    break;
                }
                m.head = (m.head << 8) | byte;
            }
            if (err) break;
            while ((m.head >> 8) >= bound) {
                sink.put(static_cast<uint32_t>(m.head));
                m.head >>= 8;
            }
            const uint64_t q = m.head / L, cf = m.head - q * L;
            const ms::Found f = cnt.find(cf);
            if (f.rank >= mt.nsym) {  // (cannot happen while the counts add up to L)
                err = ANS_E_MISMATCH;
                break;
            }
            m.head = f.count * q + (cf - f.cum);
            cnt.add(f.rank, -1);
            // ... and the rank's symbol under the table (src/ans.rs:96-105; this push can pull)
            err = md.push(m, CatSetModel::Elem{mt.sym_of_rank[f.rank], mt.table});
            if (!err && m.pulled) err = ANS_E_EXHAUSTED;
            if (err) break;
        }
        if (err) {
            fail(err);
            continue;
        }
        flatten(m.head, [&](uint32_t byte) { sink.put(byte); });
        const uint64_t len = sink.finish();
        if (sink.overflow || len > 0xFFFFFFFFull) {
            fail(ANS_E_LEN);
            continue;
        }
        lens[c] = static_cast<uint32_t>(len);
    }
}

// ---- pop: the values in pop order into out
template <typename Sym, class Cnt>
__global__ __launch_bounds__(kThreads) void k_mset_pop(CatSetModel md, MsetTab mt, uint8_t* slots, uint64_t slot_cap,
                                                        uint32_t* lens, const uint64_t* starts, uint64_t n,
                                                        uint64_t chunk_len, uint64_t nchunks, Sym* __restrict__ out,
                                                        uint32_t* __restrict__ status, uint32_t* ws) {
    extern __shared__ __align__(16) unsigned char lds[];
    md.stage(lds);
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t lanes = static_cast<uint64_t>(gridDim.x) * kThreads;
    ms::Counts<Cnt> cnt{Cnt::make(lds, mt.cnt_off, ws, lane, lanes), mt.nsym};
    for (uint64_t c = lane; c < nchunks; c += lanes) {
        const uint64_t a = starts ? starts[c] : c * chunk_len;
        const uint64_t b = starts ? starts[c + 1] : min(a + chunk_len, n);
        auto fail = [&](int code) {
            raise(status, code);
            lens[c] = 0;
        };
        const uint32_t len0 = lens[c];
        if (len0 > slot_cap || b - a > mt.max_len) {
            fail(ANS_E_LEN);
            continue;
        }
        cnt.clear();
        RSource src{slots + c * slot_cap, slot_cap, len0, false, false};
        PopT<RSource> m{0, &src};  // Message::unflatten: head 0
        for (uint64_t k = a; k < b; ++k) {
            const uint64_t x = md.pop(m, CatSetModel::Pos{mt.table});
            if (src.exhausted) break;  // src/ans.rs:144
            out[k] = static_cast<Sym>(x);
            const uint32_t r = mt.rank[x];
            cnt.add(r, 1);
            // the blanket push (src/ans.rs:96-105) of the rank under the orbit distribution of the
            // k - a + 1 values so far, on the message whose tail is the source
            const uint64_t p = cnt.count(r), cum = cnt.prefix(r), norm = k - a + 1;
            m.renorm(p, kMaxMinHead / norm);
            if (src.exhausted) break;
            m.head = norm * (m.head / p) + cum + m.head % p;
        }
        if (src.exhausted) {
            fail(ANS_E_EXHAUSTED);
            continue;
        }
        flatten(m.head, [&](uint32_t byte) { src.unpop(byte & 0xFFu); });
        if (src.overflow || src.pos > 0xFFFFFFFFull) {
            fail(ANS_E_LEN);
            continue;
        }
        lens[c] = static_cast<uint32_t>(src.pos);
    }
}

// ---- host side
hipStream_t stream_of(const ans_gpu* g, void* stream) { return stream ? static_cast<hipStream_t>(stream) : g->stream; }

// table `table` of the set as a multiset alphabet: its rank tables, built and uploaded on first use
int rank_tables(ans_gpu_tableset* ts, uint32_t table, MsetTab& mt) {
    const std::vector<uint32_t>& nsyms = ans_tableset_nsyms(ts);
    if (table >= nsyms.size()) return ANS_E_ARG;
    const uint32_t nsym = nsyms[table];
    if (nsym == 0 || nsym > ms::kMaxSymbols) return ANS_E_ARG;
    MsetState*& st = ans_tableset_mset(ts);
    if (!st) {
        st = new MsetState;
        st->tabs.resize(nsyms.size());
    }
    MsetState::Tab& t = st->tabs[table];
    if (t.state == 0) {
        std::vector<uint32_t> rank, sym_of_rank;
        if (!ms::build_ranks(nsym, rank, sym_of_rank)) {
            t.state = -1;
        } else {
            void* mem = nullptr;
            HIP_TRY(hipMalloc(&mem, size_t(8) * nsym));
            if (hipMemcpy(mem, rank.data(), size_t(4) * nsym, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(static_cast<uint32_t*>(mem) + nsym, sym_of_rank.data(), size_t(4) * nsym,
                          hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipFree(mem);
                return ANS_E_DEVICE;
            }
            t.d_rank = static_cast<uint32_t*>(mem);
            t.state = 1;
        }
    }
    if (t.state < 0) return ANS_E_ARG;  // two symbols of the alphabet share an orbit id
    mt = MsetTab{t.d_rank, t.d_rank + nsym, table, nsym, 0, 0xFFFFFFFFu};
    return ANS_OK;
}

// The launch: counts in LDS when the alphabet's u16 counts fit (longest: the longest chunk when
// the host knows it, else 0 = unknown: device-resident variable chunks take the global form),
// else in the context's workspace, with as many lanes as it and the device hold at once.
struct Plan {
    CatSetModel md;
    MsetTab mt;
    bool lds;
    unsigned grid;
    uint32_t lds_bytes;
    uint32_t* ws;
};
int plan(ans_gpu_tableset* ts, uint32_t table, uint64_t nchunks, uint64_t longest, Plan& pl) {
    if (int rc = rank_tables(ts, table, pl.mt)) return rc;
    ans_gpu* g = ans_tableset_gpu(ts);
    pl.md = ans_tableset_model(ts);
    pl.ws = nullptr;
    const uint64_t blocks = (nchunks + kThreads - 1) / kThreads;
    const uint32_t cnt_bytes = pl.mt.nsym * kThreads * 2;
    pl.lds = longest != 0 && longest <= kLdsMaxLen && cnt_bytes <= kLdsCounts;
    if (pl.lds) {
        // the table set's own LDS staging yields when both do not fit
        uint32_t tab = (pl.md.lds_bytes + 15u) & ~15u;
        if (tab + cnt_bytes > kLdsAll) pl.md.lds_bytes = tab = 0;
        pl.mt.cnt_off = tab;
        pl.mt.max_len = kLdsMaxLen;
        pl.lds_bytes = tab + cnt_bytes;
        pl.grid = static_cast<unsigned>(std::min<uint64_t>(blocks, 0x7FFFFFFFull));
        return ANS_OK;
    }
    // two waves per SIMD resident, fewer when the alphabet is large
    const size_t per_lane = size_t(4) * pl.mt.nsym;
    uint64_t want = std::min<uint64_t>(blocks, static_cast<uint64_t>(g->ncu) * 8);
    want = std::max<uint64_t>(1, std::min<uint64_t>(want, kWsMax / (per_lane * kThreads)));
    const size_t bytes = per_lane * kThreads * want;
    if (g->cap_mset_ws < bytes) {
        if (g->d_mset_ws) (void)hipFree(g->d_mset_ws);  // (waits for the kernels that use it)
        g->d_mset_ws = nullptr;
        g->cap_mset_ws = 0;
        HIP_TRY(hipMalloc(&g->d_mset_ws, bytes));
        g->cap_mset_ws = bytes;
    }
    pl.ws = static_cast<uint32_t*>(g->d_mset_ws);
    pl.lds_bytes = pl.md.lds_bytes;
    pl.grid = static_cast<unsigned>(want);
    return ANS_OK;
}

int dev_mset_push(ans_gpu_tableset* ts, uint32_t table, const void* d_syms, int w, const uint64_t* d_starts, uint64_t n,
                  uint64_t chunk_len, uint64_t nchunks, uint64_t longest, uint8_t* d_slots, uint64_t slot_cap,
                  uint32_t* d_lens, uint32_t* d_status, hipStream_t s) {
    Plan pl;
    if (int rc = plan(ts, table, nchunks, longest, pl)) return rc;
    LaunchLog& log = ans_tableset_gpu(ts)->last;
    log.clear();
    with_sym_type(w, [&](auto t) {
        using Sym = decltype(t);
        log.add(kRecMsetPush, sizeof(Sym), pl.lds, rec_grid(pl.grid));
        if (pl.lds)
            k_mset_push<Sym, LdsCnt><<<pl.grid, kThreads, pl.lds_bytes, s>>>(
                pl.md, pl.mt, static_cast<const Sym*>(d_syms), d_starts, n, chunk_len, nchunks, d_slots, slot_cap, d_lens,
                d_status, pl.ws);
        else
            k_mset_push<Sym, GlobalCnt><<<pl.grid, kThreads, pl.lds_bytes, s>>>(
                pl.md, pl.mt, static_cast<const Sym*>(d_syms), d_starts, n, chunk_len, nchunks, d_slots, slot_cap, d_lens,
                d_status, pl.ws);
    });
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}
int dev_mset_pop(ans_gpu_tableset* ts, uint32_t table, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                 const uint64_t* d_starts, uint64_t n, uint64_t chunk_len, uint64_t nchunks, uint64_t longest,
                 void* d_syms, int w, uint32_t* d_status, hipStream_t s) {
    Plan pl;
    if (int rc = plan(ts, table, nchunks, longest, pl)) return rc;
    LaunchLog& log = ans_tableset_gpu(ts)->last;
    log.clear();
    with_sym_type(w, [&](auto t) {
        using Sym = decltype(t);
        log.add(kRecMsetPop, sizeof(Sym), pl.lds, rec_grid(pl.grid));
        if (pl.lds)
            k_mset_pop<Sym, LdsCnt><<<pl.grid, kThreads, pl.lds_bytes, s>>>(
                pl.md, pl.mt, d_slots, slot_cap, d_lens, d_starts, n, chunk_len, nchunks, static_cast<Sym*>(d_syms),
                d_status, pl.ws);
        else
            k_mset_pop<Sym, GlobalCnt><<<pl.grid, kThreads, pl.lds_bytes, s>>>(
                pl.md, pl.mt, d_slots, slot_cap, d_lens, d_starts, n, chunk_len, nchunks, static_cast<Sym*>(d_syms),
                d_status, pl.ws);
    });
    HIP_TRY(hipGetLastError());
    return ANS_OK;
}

// ---- host buffers in and out, synchronous (as ans_gpu_independent_push_chunks / _pop_chunks): the
// dense container in is expanded into slots with room for each result, the chunks are coded in
// place and the slots are packed into the container out (Stage, stage_in: ans_hostio.hpp).
// starts == NULL: fixed chunks.
uint64_t longest_of(const uint64_t* starts, uint64_t nchunks, uint64_t chunk_len) {
    uint64_t longest = chunk_len;
    if (starts)
        for (uint64_t c = 0; c < nchunks; ++c) longest = std::max(longest, starts[c + 1] - starts[c]);
    return longest;
}

int host_mset_push(ans_gpu_tableset* ts, uint32_t table, const void* syms, int w, uint64_t n, uint64_t chunk_len,
                   const uint64_t* starts, uint64_t nchunks, const uint8_t* in, uint64_t in_len,
                   const uint64_t* in_offsets, const uint64_t* in_lens, uint8_t* out, uint64_t out_cap,
                   uint64_t* offsets, uint64_t* lens, uint64_t* total) {
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (!in_offsets || !in_lens || (in_len && !in) || (n && !syms)) return ANS_E_ARG;
    if (out && (!offsets || !lens)) return ANS_E_ARG;
    const uint64_t longest = longest_of(starts, nchunks, chunk_len);
    if (longest > 0xFFFFFFFFull) return ANS_E_ARG;
    ans_gpu* g = ans_tableset_gpu(ts);
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    Stage st;
    int rc = stage_in(g, starts, nchunks, in, in_len, in_offsets, in_lens,
                      ans_tableset_slot_bytes(ts, std::max<uint64_t>(longest, 1)), st);
    if (rc) return rc;
    DevBuf d_syms;
    HIP_TRY(d_syms.alloc(n * w));
    if (n) HIP_TRY(hipMemcpyAsync(d_syms.p, syms, n * w, hipMemcpyHostToDevice, s));
    uint32_t* d_status = st.d.status.as<uint32_t>();
    rc = dev_mset_push(ts, table, d_syms.p, w, st.starts.as<uint64_t>(), n, chunk_len, nchunks, std::max<uint64_t>(longest, 1),
                       st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), d_status, s);
    if (rc || (rc = read_status(g, d_status, s))) return rc;
    return download_container(g, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), nchunks, s, out, out_cap,
                              offsets, lens, total);
}

int host_mset_pop(ans_gpu_tableset* ts, uint32_t table, const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
                  const uint64_t* in_lens, uint64_t n, uint64_t chunk_len, const uint64_t* starts, uint64_t nchunks,
                  void* out_syms, int w, uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens,
                  uint64_t* total) {
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (!in_offsets || !in_lens || (in_len && !in) || (n && !out_syms)) return ANS_E_ARG;
    if (out && (!offsets || !lens)) return ANS_E_ARG;
    const uint64_t longest = longest_of(starts, nchunks, chunk_len);
    if (longest > 0xFFFFFFFFull) return ANS_E_ARG;
    ans_gpu* g = ans_tableset_gpu(ts);
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = g->stream;
    Stage st;
    int rc = stage_in(g, starts, nchunks, in, in_len, in_offsets, in_lens, ms::pop_slack(longest), st);
    if (rc) return rc;
    DevBuf d_syms;
    HIP_TRY(d_syms.alloc(n * w));
    uint32_t* d_status = st.d.status.as<uint32_t>();
    rc = dev_mset_pop(ts, table, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), st.starts.as<uint64_t>(), n,
                      chunk_len, nchunks, std::max<uint64_t>(longest, 1), d_syms.p, w, d_status, s);
    if (rc || (rc = read_status(g, d_status, s))) return rc;
    if (n) HIP_TRY(hipMemcpy(out_syms, d_syms.p, n * w, hipMemcpyDeviceToHost));
    return download_container(g, st.slots.as<uint8_t>(), st.cap, st.d.lens.as<uint32_t>(), nchunks, s, out, out_cap,
                              offsets, lens, total);
}

int var_starts_ok(uint64_t nchunks, const uint64_t* starts) {
    for (uint64_t c = 0; c < nchunks; ++c)
        if (starts[c + 1] < starts[c]) return ANS_E_ARG;
    return ANS_OK;
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

int ans_gpu_mset_pop_slack(uint64_t chunk_len, uint64_t* bytes) try {
    if (!bytes || chunk_len > 0xFFFFFFFFull) return ANS_E_ARG;
    *bytes = ms::pop_slack(chunk_len);
    return ANS_OK;
} ANS_CATCH

int ans_dev_mset_push(ans_gpu_tableset* ts, uint32_t table, const void* d_syms, int sym_bytes, uint64_t n,
                      uint64_t chunk_len, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status,
                      void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u32(sym_bytes) || chunk_len == 0 || chunk_len > 0xFFFFFFFFull ||
        (n && (!d_syms || !d_slots || !d_lens)) || !d_status)
        return ANS_E_ARG;
    if (n == 0) return ANS_OK;
    ans_gpu* g = ans_tableset_gpu(ts);
    HIP_TRY(hipSetDevice(g->device));
    return dev_mset_push(ts, table, d_syms, sym_bytes, nullptr, n, chunk_len, (n + chunk_len - 1) / chunk_len, chunk_len,
                         d_slots, slot_cap, d_lens, d_status, stream_of(g, stream));
} ANS_CATCH
int ans_dev_mset_pop(ans_gpu_tableset* ts, uint32_t table, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                     uint64_t n, uint64_t chunk_len, void* d_syms, int sym_bytes, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u32(sym_bytes) || chunk_len == 0 || chunk_len > 0xFFFFFFFFull || slot_cap < 16 ||
        (n && (!d_syms || !d_slots || !d_lens)) || !d_status)
        return ANS_E_ARG;
    if (n == 0) return ANS_OK;
    ans_gpu* g = ans_tableset_gpu(ts);
    HIP_TRY(hipSetDevice(g->device));
    return dev_mset_pop(ts, table, d_slots, slot_cap, d_lens, nullptr, n, chunk_len, (n + chunk_len - 1) / chunk_len,
                        chunk_len, d_syms, sym_bytes, d_status, stream_of(g, stream));
} ANS_CATCH
// (the chunk lengths are on the device: the longest is unknown here, so the counts are global)
int ans_dev_mset_push_var(ans_gpu_tableset* ts, uint32_t table, const void* d_syms, int sym_bytes, uint64_t nchunks,
                          const uint64_t* d_starts, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                          uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u32(sym_bytes) || !d_status || (nchunks && (!d_starts || !d_syms || !d_slots || !d_lens)))
        return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    ans_gpu* g = ans_tableset_gpu(ts);
    HIP_TRY(hipSetDevice(g->device));
    return dev_mset_push(ts, table, d_syms, sym_bytes, d_starts, 0, 0, nchunks, 0, d_slots, slot_cap, d_lens, d_status,
                         stream_of(g, stream));
} ANS_CATCH
int ans_dev_mset_pop_var(ans_gpu_tableset* ts, uint32_t table, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                         uint64_t nchunks, const uint64_t* d_starts, void* d_syms, int sym_bytes, uint32_t* d_status,
                         void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !valid_width_u32(sym_bytes) || !d_status || slot_cap < 16 ||
        (nchunks && (!d_starts || !d_syms || !d_slots || !d_lens)))
        return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    ans_gpu* g = ans_tableset_gpu(ts);
    HIP_TRY(hipSetDevice(g->device));
    return dev_mset_pop(ts, table, d_slots, slot_cap, d_lens, d_starts, 0, 0, nchunks, 0, d_syms, sym_bytes, d_status,
                        stream_of(g, stream));
} ANS_CATCH

int ans_gpu_mset_push_chunks(ans_gpu_tableset* ts, uint32_t table, const void* syms, int sym_bytes, uint64_t n,
                             uint64_t chunk_len, const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
                             const uint64_t* in_lens, uint8_t* out, uint64_t out_cap, uint64_t* offsets, uint64_t* lens,
                             uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u32(sym_bytes) || chunk_len == 0) return ANS_E_ARG;
    return host_mset_push(ts, table, syms, sym_bytes, n, chunk_len, nullptr, (n + chunk_len - 1) / chunk_len, in, in_len,
                          in_offsets, in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_mset_pop_chunks(ans_gpu_tableset* ts, uint32_t table, const uint8_t* in, uint64_t in_len,
                            const uint64_t* in_offsets, const uint64_t* in_lens, uint64_t n, uint64_t chunk_len,
                            void* out_syms, int sym_bytes, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                            uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u32(sym_bytes) || chunk_len == 0) return ANS_E_ARG;
    return host_mset_pop(ts, table, in, in_len, in_offsets, in_lens, n, chunk_len, nullptr,
                         (n + chunk_len - 1) / chunk_len, out_syms, sym_bytes, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_mset_push_var_chunks(ans_gpu_tableset* ts, uint32_t table, const void* syms, int sym_bytes, uint64_t nchunks,
                                 const uint64_t* starts, const uint8_t* in, uint64_t in_len, const uint64_t* in_offsets,
                                 const uint64_t* in_lens, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                                 uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u32(sym_bytes) || (nchunks && !starts)) return ANS_E_ARG;
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (int rc = var_starts_ok(nchunks, starts)) return rc;
    return host_mset_push(ts, table, syms, sym_bytes, starts[nchunks], 0, starts, nchunks, in, in_len, in_offsets,
                          in_lens, out, out_cap, offsets, lens, total);
} ANS_CATCH
int ans_gpu_mset_pop_var_chunks(ans_gpu_tableset* ts, uint32_t table, const uint8_t* in, uint64_t in_len,
                                const uint64_t* in_offsets, const uint64_t* in_lens, uint64_t nchunks,
                                const uint64_t* starts, void* out_syms, int sym_bytes, uint8_t* out, uint64_t out_cap,
                                uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!ts || !total || !valid_width_u32(sym_bytes) || (nchunks && !starts)) return ANS_E_ARG;
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    if (int rc = var_starts_ok(nchunks, starts)) return rc;
    return host_mset_pop(ts, table, in, in_len, in_offsets, in_lens, starts[nchunks], 0, starts, nchunks, out_syms,
                         sym_bytes, out, out_cap, offsets, lens, total);
} ANS_CATCH

}  // extern "C"
