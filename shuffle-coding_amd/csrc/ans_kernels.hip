// ans_kernels.hip — what surrounds the coder kernels of the Categorical tables (the coders
// themselves are in the launch units, ans_launch.hpp; the host-buffer pipeline in ans_pipe.hip):
//   * the copy and pack kernels between the slot layout and a dense container (k_compact,
//     k_expand), the tiled length scan of the device-resident dense container
//     (§3.4c), k_span_stats and the renorm self-check k_check_renorm;
//   * build_fast_table: the fast kernels' tables derived from a Categorical (ans_table.hpp);
//   * the C ABI's context and table entries (ans_gpu_create, ans_gpu_table_create, ...), its
//     device-resident entries (ans_dev_*) and the variable-chunk host entries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ans_hostio.hpp"
#include "ans_kcommon.hpp"
#include "ans_launch.hpp"

using namespace shuffle_coding::launch;

namespace {

// Self-check of the decoders' renorm step (fast::renorm_up) on caller-chosen (head, window)
// pairs, for tests: its rare exact path (X >> 8 landing in [L, 2^56)) is too rare in coded
// data to be reached reliably (~norm / 2^56 per symbol).
__global__ __launch_bounds__(256) void k_check_renorm(const uint64_t* __restrict__ heads,
                                                      const uint32_t* __restrict__ windows, uint64_t L, uint64_t n,
                                                      uint64_t* __restrict__ out_heads, uint32_t* __restrict__ out_k) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t h = heads[i];
    out_k[i] = fast::renorm_up(h, windows[i], L, fast::renorm_screen(L));
    out_heads[i] = h;
}

// One wave copies one stream: byte head until dst is dword-aligned, then aligned dword
// stores funnelled from two source dwords (v_alignbyte), then the byte tail.  Source reads
// are aligned dwords that each hold at least one byte of the stream (no over-read past the
// dword holding its last byte).
__device__ __forceinline__ void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                          uint32_t lane) {
    const uint32_t head = min(len, (4u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 3)) & 3u);
    if (lane < head) dst[lane] = src[lane];
    dst += head;
    src += head;
    len -= head;
    const uint32_t nd = len / 4, sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(src) & 3);
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(src) & ~uintptr_t(3));
    uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
    for (uint32_t i = lane; i < nd; i += 64) {
        const uint32_t lo = s4[i], hi = sh ? s4[i + 1] : 0u;  // sh is wave-uniform
        d4[i] = __builtin_amdgcn_alignbyte(hi, lo, sh);
    }
    if (lane < len - 4 * nd) dst[4 * nd + lane] = src[4 * nd + lane];
}

// One wave packs one stream from a 16-B-aligned source (a slot) to any destination in whole
// aligned 16-B stores: destination block j (of the 16-B-aligned line holding dst, dsh = dst & 15)
// takes stream bytes [16j - dsh, 16j - dsh + 16), i.e. source blocks j-1 and j funnelled by
// v_alignbyte at a wave-uniform dword step and byte shift.  The first and last blocks may hold
// a neighbouring stream's bytes: those are written byte by byte (no store touches a byte
// outside the stream, so neighbouring waves never race).  Only source blocks holding stream
// bytes are read, each once: block j-1 comes from the lane below (DPP wave_shr:1), and for lane
// 0 from lane 63 of the previous pass (v_readlane), where a second load per lane read every
// block twice through the L1 (the pack ran at 5.2 TB/s, profiles/r03b_kernel_stats_c3.csv).
__device__ __forceinline__ uint32_t from_lane_below(uint32_t v, uint32_t carry) {
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(carry), static_cast<int>(v), 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ void wave_pack(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                          uint32_t lane) {
    if (len == 0) return;
    const uint32_t dsh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 15);
    uint8_t* dbase = dst - dsh;
    const uint4* s16 = reinterpret_cast<const uint4*>(src);
    const uint32_t nblk = (dsh + len + 15) / 16;
    const uint32_t bs = (16u - dsh) & 3u;         // byte shift inside the 32-B window
    const uint32_t i0 = (16u - dsh) >> 2;         // first window dword of an output block
    uint4 carry = make_uint4(0, 0, 0, 0);         // block j0 - 1 (none before the stream)
    // passes of up to four 64-block rounds whose loads are all issued first (four 16-B loads in
    // flight per lane: one at a time left the copy latency-bound at ~5.6 TB/s)
    constexpr int kR = 4;
    for (uint32_t j0 = 0; j0 < nblk; j0 += 64 * kR) {  // (wave-uniform: every lane takes part in the DPP moves)
        uint4 bb[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const uint32_t j = j0 + 64 * r + lane;
            bb[r] = (j < nblk && 16 * j < len) ? s16[j] : make_uint4(0, 0, 0, 0);  // only blocks holding stream bytes
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const uint32_t j = j0 + 64 * r + lane;
            if (j0 + 64 * r >= nblk) break;  // (uniform)
            const uint4 b = bb[r];
            const uint4 a = make_uint4(from_lane_below(b.x, carry.x), from_lane_below(b.y, carry.y),
                                       from_lane_below(b.z, carry.z), from_lane_below(b.w, carry.w));
            carry = make_uint4(__builtin_amdgcn_readlane(b.x, 63), __builtin_amdgcn_readlane(b.y, 63),
                               __builtin_amdgcn_readlane(b.z, 63), __builtin_amdgcn_readlane(b.w, 63));
            if (j >= nblk) continue;
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t o[4];
            // i0 is wave-uniform: a scalar branch picks constant register indices
            switch (i0) {
#define PACK_CASE(I)                                                                 \
    case I:                                                                          \
        for (int k = 0; k < 4; ++k)                                                  \
            o[k] = (I + k + 1 < 8) ? __builtin_amdgcn_alignbyte(w[(I + k + 1) & 7], w[I + k], bs) : w[I + k]; \
        break;
                PACK_CASE(0)
                PACK_CASE(1)
                PACK_CASE(2)
                PACK_CASE(3)
                default:
                    for (int k = 0; k < 4; ++k) o[k] = w[4 + k];  // dsh = 0: block j itself
#undef PACK_CASE
            }
            const uint32_t lo = j == 0 ? dsh : 0u;                           // first byte of the stream here
            const uint32_t hi = min(16u, dsh + len - 16u * j);               // one past its last
            if (lo == 0 && hi == 16) {
                *reinterpret_cast<uint4*>(dbase + 16ull * j) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (uint32_t t = 0; t < 16; ++t)
                    if (t >= lo && t < hi) dbase[16ull * j + t] = static_cast<uint8_t>(o[t >> 2] >> (8 * (t & 3)));
            }
        }
    }
}

// One wave per chunk copies its slot into the dense container.
__global__ __launch_bounds__(kBlock) void k_compact(const uint8_t* __restrict__ slots, uint64_t slot_cap,
                                                    const uint32_t* __restrict__ lens,
                                                    const uint64_t* __restrict__ offsets, uint64_t nchunks,
                                                    uint8_t* __restrict__ out) {
    const uint64_t c = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / 64;
    const uint32_t lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    const uint8_t* s = slots + c * slot_cap;
    uint8_t* d = out + offsets[c];
    const uint32_t len = static_cast<uint32_t>(min<uint64_t>(lens[c], slot_cap));  // never past the slot
    if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) wave_pack(d, s, len, lane);
    else wave_copy(d, s, len, lane);
}

// One wave per chunk copies a dense-container stream into its slot (the inverse of k_compact).
__global__ __launch_bounds__(kBlock) void k_expand(const uint8_t* __restrict__ in, const uint64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ lens, uint64_t nchunks,
                                                   uint8_t* __restrict__ slots, uint64_t slot_cap) {
    const uint64_t c = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / 64;
    const uint32_t lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    const uint8_t* s = in + offsets[c];
    uint8_t* d = slots + c * slot_cap;
    wave_copy(d, s, lens[c], lane);
}

// ---- device-resident dense container (include/ans_capi.h ans_dev_encode_dense_ex)
// Exclusive scan of the stream lengths in tiles of 4,096 chunks (1,024 threads x 4, a
// 64-lane shuffle scan per wave, the 16 wave totals through LDS): each tile leaves its local
// offsets and its total; k_scan_tile_sums scans the totals in place (one workgroup); then
// k_compact_dense adds its tile's prefix, publishes the final offset and packs the stream.
// Lengths are clamped to the slot like k_compact's copies, so offsets and bytes agree.
constexpr uint32_t kScanTile = 4096;

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, uint32_t lane) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(v, d, 64);
        if (lane >= d) v += y;
    }
    return v;
}

__global__ __launch_bounds__(1024) void k_scan_tiles(const uint32_t* __restrict__ lens, uint64_t n, uint64_t slot_cap,
                                                     uint64_t* __restrict__ offs, uint64_t* __restrict__ tile_sum) {
    __shared__ uint64_t wsum[16];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kScanTile + 4 * threadIdx.x;
    uint64_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? min<uint64_t>(lens[i0 + k], slot_cap) : 0;
    const uint64_t t = v[0] + v[1] + v[2] + v[3];
    const uint64_t incl = wave_incl_scan(t, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t run = incl - t;
    for (uint32_t w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < n) offs[i0 + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 1023) tile_sum[blockIdx.x] = run;  // the tile's total
}

__global__ __launch_bounds__(1024) void k_scan_tile_sums(uint64_t* __restrict__ tile_sum, uint64_t ntiles,
                                                         uint64_t* __restrict__ total) {
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t carry;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    for (uint64_t b = 0; b < ntiles; b += 1024) {
        __syncthreads();  // carry written, last round's wsum reads done
        const uint64_t i = b + threadIdx.x;
        const uint64_t t = i < ntiles ? tile_sum[i] : 0;
        const uint64_t incl = wave_incl_scan(t, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint64_t pre = carry + incl - t;
        for (uint32_t w = 0; w < wave; ++w) pre += wsum[w];
        if (i < ntiles) tile_sum[i] = pre;
        __syncthreads();  // every carry read done
        if (threadIdx.x == 1023) carry = pre + t;
    }
    __syncthreads();
    if (threadIdx.x == 0) *total = carry;
}

// One wave per chunk: offset = local + tile prefix; the stream is packed unless it would end
// past out_cap (ANS_E_LEN).
__global__ __launch_bounds__(kBlock) void k_compact_dense(const uint8_t* __restrict__ slots, uint64_t slot_cap,
                                                          const uint32_t* __restrict__ lens, uint64_t* __restrict__ offs,
                                                          const uint64_t* __restrict__ tile_pre, uint64_t nchunks,
                                                          uint8_t* __restrict__ out, uint64_t out_cap,
                                                          uint32_t* __restrict__ status) {
    const uint64_t c = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / 64;
    const uint32_t lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    const uint32_t len = static_cast<uint32_t>(min<uint64_t>(lens[c], slot_cap));
    const uint64_t off = offs[c] + tile_pre[c / kScanTile];
    if (lane == 0) offs[c] = off;  // (every lane has read offs[c]: one load instruction)
    if (off + len > out_cap) {
        if (lane == 0) atomicOr(status, 1u << ANS_E_LEN);
        return;
    }
    const uint8_t* src = slots + c * slot_cap;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) wave_pack(out + off, src, len, lane);
    else wave_copy(out + off, src, len, lane);
}

// 1/d rounded UP (fma(r, d, -1) is the exact sign of r d - 1): kNormSmall's exact high division
// step (ans_fast.hpp div_hi) needs r >= 1/d, and r - 1/d < 2^-52 / d keeps its estimates as
// tight as fl(1/d)'s
static double rcp_up(uint32_t d) {
    double r = 1.0 / static_cast<double>(d);
    while (std::fma(r, static_cast<double>(d), -1.0) < 0.0) r = std::nextafter(r, 2.0);
    return r;
}

// Derives the fast-path tables (ans_table.hpp FastTable) when the table qualifies: nsym <= 65536
// and norm < 2^32, in one of the three norm ranges (2^16 <= norm <= 2^31: one f64 quotient
// estimate; below 2^16 or above 2^31: the kNormSmall / kNormBig division of
// DESIGN.md §4b, in the LDS kernels and the large-alphabet ones alike).  Up to 256 symbols the
// rows and decode buckets are staged in LDS; above, the encoder reads its rows from global memory
// (k_encode with global rows, or k_encode_w from 2^22 on) and decodes take k_decode_w / k_decode_g.
int build_fast_table(ans_gpu_table* gt, const Categorical& cat) {
    const DevTable& t = gt->t;
    FastTable ft{};
    const uint32_t nr = t.fast ? fast::kNormStd : (t.norm < (1u << 16) ? fast::kNormSmall : fast::kNormBig);
    if (t.nsym > 65536u) {
        gt->ft = ft;
        return ANS_OK;
    }
    using u128 = unsigned __int128;
    const uint32_t nsym = t.nsym;
    std::vector<EncRow> enc(nsym + 1);
    uint32_t kmax = 1;
    std::vector<uint32_t> kmax_row(nsym + 1, 0);
    for (uint32_t s = 0; s <= nsym; ++s) {
        const uint64_t m = s < nsym ? cat.masses[s] : 0;
        const double rcp = nr == fast::kNormSmall ? rcp_up(static_cast<uint32_t>(m)) : 1.0 / static_cast<double>(m);
        enc[s] = EncRow{m ? rcp : 0.0, static_cast<uint32_t>(m),
                        s < nsym ? static_cast<uint32_t>(cat.cummasses[s]) : t.norm};
        if (!m) continue;
        const u128 pK = static_cast<u128>(m) * t.K;
        for (uint32_t j = 1; j <= 4; ++j)  // can a push emit j bytes? (head < 2^64 <= p*K*2^8j otherwise)
            if ((pK << (8 * j)) < (static_cast<u128>(1) << 64)) kmax_row[s] = j;
        kmax = std::max(kmax, kmax_row[s]);
    }
    // a symbol holding all of a power-of-two norm (L = 2^56) is the one row fast::enc_thr cannot
    // express (its renorm test must never hold, and every head up to 2^64 - 1 is possible)
    for (uint32_t s = 0; s < nsym; ++s)
        if (cat.masses[s] == t.norm && t.L == (1ull << 56)) {
            gt->ft = ft;
            return ANS_OK;
        }
    ft.enc_global = nsym > 256;
    ft.dec_usable = nsym <= 256;
    // decode buckets: the finest power-of-two width whose table fits fast::kDecTableBytes in
    // LDS (with the cdf table); for large alphabets, at most 2^16 buckets in global memory
    uint32_t shift = 0;
    const size_t cum_bytes = sizeof(uint32_t) * (nsym + 5);
    const uint64_t max_buckets = ft.dec_usable ? fast::kDecNbMax : (1ull << 16);
    while (((static_cast<uint64_t>(t.norm) - 1) >> shift) + 1 > max_buckets) ++shift;
    const uint32_t nb = static_cast<uint32_t>(((static_cast<uint64_t>(t.norm) - 1) >> shift) + 1);
    std::vector<uint32_t> cum(nsym + 6, t.norm);
    for (uint32_t s = 0; s < nsym; ++s) cum[s] = static_cast<uint32_t>(cat.cummasses[s]);
    std::vector<DecBucket> dec(ft.dec_usable ? nb : 0);
    std::vector<uint8_t> dec_s0(ft.dec_usable ? nb : 0);  // nsym <= 256: one byte each
    std::vector<DecBucketG> decg(ft.dec_usable ? 0 : nb);
    for (uint32_t j = 0; j < nb; ++j) {
        const uint32_t s0 = static_cast<uint32_t>(cat.icdf(static_cast<uint64_t>(j) << shift).first);
        if (ft.dec_usable) {
            DecBucket& d = dec[j];
            for (int i = 0; i < 4; ++i) d.c[i] = cum[s0 + i];
            dec_s0[j] = static_cast<uint8_t>(s0);
            // every cf of the bucket below cdf(s0 + 3)?  (the last bucket ends at norm)
            const uint64_t end = std::min<uint64_t>(t.norm, (static_cast<uint64_t>(j) + 1) << shift);
            if (d.c[3] < end) ft.dec_far = 1;
        } else {
            DecBucketG& d = decg[j];
            for (int i = 0; i < 6; ++i) d.c[i] = cum[s0 + i];
            d.s0 = s0;
            d.pad = 0;
        }
    }
    // the fix-up-free decoder's tables (ans_fast.hpp kModeU): the virtual alphabet over
    // u in [0, 2 norm) (v < 256: symbol v at cdf(v); v >= 256: symbol v - 256 at norm + cdf),
    // at the finest bucket width that fits; kept only if every bucket resolves among three
    // candidates (a table with fewer than 256 symbols can leave a bucket straddling u = norm
    // with the zero-mass gap between the halves: those keep the kModeRows tables)
    std::vector<uint8_t> uimg;
    if (ft.dec_usable && !ft.dec_far && t.norm < (1u << 31)) {
        const uint64_t n2 = 2ull * t.norm;
        auto cdfv = [&](uint32_t v) -> uint64_t {
            if (v >= 512) return n2;
            const uint32_t sv = v & 255u;
            const uint64_t c = cum[std::min(sv, nsym)];
            return v < 256 ? c : t.norm + c;
        };
        auto icdfv = [&](uint64_t x) {  // the last v in [0, 512) with cdfv(v) <= x
            uint32_t lo = 0, hi = 511;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) / 2;
                if (cdfv(mid) <= x) lo = mid;
                else hi = mid - 1;
            }
            return lo;
        };
        uint32_t us = 1;
        while (((n2 - 1) >> us) + 1 > fast::kDecUNbMax) ++us;
        const uint32_t nbu = static_cast<uint32_t>(((n2 - 1) >> us) + 1);
        uimg.assign(fast::kDecTableBytes, 0);
        bool ok = us <= fast::kDecUShiftMax;  // (norm <= 3072 * 2^17: u + k1 stays in 32 bits)
        // the bucket's two additive words (ans_dec_u.hpp): s0 rides in the first, and the kernel
        // picks v = s0 + [u >= c1] + [u >= c2] with fast::dec_u_pick
        for (uint32_t j = 0; j < nbu && ok; ++j) {
            const uint64_t a = static_cast<uint64_t>(j) << us, end = std::min<uint64_t>(n2, a + (1ull << us));
            const uint32_t s0 = icdfv(a);
            if (cdfv(s0 + 3) < end) ok = false;
            const uint32_t w12[2] = {fast::dec_u_word(a, cdfv(s0 + 1), s0, us), fast::dec_u_word(a, cdfv(s0 + 2), 0, us)};
            std::memcpy(uimg.data() + 8 * j, w12, 8);
        }
        for (uint32_t v = 0; v < 512 && ok; ++v) {
            const uint32_t sv = v & 255u;
            const uint32_t m = sv < nsym ? static_cast<uint32_t>(cat.masses[sv]) : 0u;
            const uint32_t c = cum[std::min(sv, nsym)];
            // head = p * q_m + (u - cum_row): lower half q = q_m, cf = u; upper q = q_m + 1, cf = u - norm
            const uint32_t row[2] = {v < 256 ? c : t.norm + c - m, m};
            std::memcpy(uimg.data() + fast::kDecURowOff + 8 * v, row, 8);
        }
        if (ok) {
            ft.dec_u = 1;
            ft.dec_u_shift = us;
        } else {
            uimg.clear();
        }
    }
    ft.dec_global = !ft.dec_usable;
    // compact 16-B buckets for k_decode_w: the finest width with at most 2^17 buckets (2 MiB),
    // if every bucket's five candidate offsets fit u16
    std::vector<DecBucketC> decc, decl;
    if (ft.dec_global) {
        uint32_t cs = 0;
        while (((static_cast<uint64_t>(t.norm) - 1) >> cs) + 1 > (1ull << 17)) ++cs;
        const uint32_t ncb = static_cast<uint32_t>(((static_cast<uint64_t>(t.norm) - 1) >> cs) + 1);
        decc.resize(ncb);
        bool fits = true;
        for (uint32_t j = 0; j < ncb && fits; ++j) {
            const uint32_t s0 = static_cast<uint32_t>(cat.icdf(static_cast<uint64_t>(j) << cs).first);
            DecBucketC& d = decc[j];
            d.c0 = cum[s0];
            d.s0 = static_cast<uint16_t>(s0);
            for (int k = 0; k < 5; ++k) {
                const uint32_t off = cum[s0 + 1 + k] - cum[s0];
                if (off > 0xFFFFu) fits = false;
                d.d[k] = static_cast<uint16_t>(off);
            }
        }
        if (fits) {
            ft.dec_c = 1;
            ft.dec_c_shift = cs;
            ft.dec_cl_shift = cs;
        } else {
            decc.clear();
        }
        // the LDS beside k_decode_w's ring holds kWideDecBktLds buckets; a table with more stages
        // its first ones at twice the width, which doubles the share of lookups the LDS serves
        // (C4: 9.2% -> 18.3%), if they resolve among their five candidates for all but 1/256 of
        // the cf they cover (C4: 0.23%; the rest re-fetch their global bucket, ans_wide.hpp)
        if (ft.dec_c && ncb > fast::kWideDecBktLds) {
            const uint32_t ls = cs + 1;
            const uint32_t nl = static_cast<uint32_t>(std::min<uint64_t>(((static_cast<uint64_t>(t.norm) - 1) >> ls) + 1,
                                                                         fast::kWideDecBktLds));
            decl.resize(nl);
            bool lfits = true;
            uint64_t far = 0, covered = 0;
            for (uint32_t j = 0; j < nl && lfits; ++j) {
                const uint64_t b0 = static_cast<uint64_t>(j) << ls;
                const uint64_t b1 = std::min<uint64_t>(b0 + (1ull << ls), t.norm);
                const uint32_t s0 = static_cast<uint32_t>(cat.icdf(b0).first);
                DecBucketC& d = decl[j];
                d.c0 = cum[s0];
                d.s0 = static_cast<uint16_t>(s0);
                for (int k = 0; k < 5; ++k) {
                    const uint32_t off = cum[s0 + 1 + k] - cum[s0];
                    if (off > 0xFFFFu) lfits = false;
                    d.d[k] = static_cast<uint16_t>(off);
                }
                const uint64_t c5 = std::max<uint64_t>(cum[s0 + 5], b0);
                far += b1 > c5 ? b1 - c5 : 0;
                covered += b1 - b0;
            }
            if (lfits && far * 256 <= covered) ft.dec_cl_shift = ls;
            else decl.clear();
        }
    }
    ft.enc_wide = ft.enc_global && t.norm >= fast::kWideNormMin;
    ft.enc_nl = std::min<uint32_t>(nsym, fast::kWideEncCumMax - 1);
    // the packed prefix (ans_table.hpp enc_pack): the longest multiple of 16 symbols whose image
    // fits the same LDS and whose in-block offsets fit u16; used when it is longer
    std::vector<uint32_t> pack_img;
    uint32_t pmax = 0;
    for (uint32_t s = 0; s < nsym; ++s) pmax = std::max<uint32_t>(pmax, static_cast<uint32_t>(cat.masses[s]));
    // k_encode_w<kSa> (ans_wide.hpp): a renorm shift byte per mass 0..pmax at LDS offset 0, when
    // every mass has one (ans_renorm.hpp enc_sa); it takes kWideSaBytes from the prefix
    std::vector<uint8_t> sa_img;
    if (ft.enc_wide && pmax <= fast::kWideSaMax) {
        sa_img.assign(fast::kWideSaBytes, 8);
        for (uint32_t p = 0; p <= pmax && !sa_img.empty(); ++p) {
            const uint32_t sa = fast::enc_sa(static_cast<uint64_t>(p) * t.K, t.L);
            if (sa == 0) sa_img.clear();
            else sa_img[p] = static_cast<uint8_t>(sa);
        }
    }
    if (ft.enc_wide && pmax <= 0xFFFFu) {  // (pmf from two low halves: every mass below 2^16)
        const uint32_t nl_max = fast::wide_pack_nl_max(!sa_img.empty());  // (the LDS regions, ans_wide.hpp)
        auto img_bytes = [](uint32_t nl) {
            const uint32_t ooff = 4 * ((nl >> 4) + 2);
            return (ooff + 2 * (nl + 2) + 3) & ~3u;
        };
        uint32_t nlp = 0;
        while (nlp + 16 <= nsym && nlp + 16 <= nl_max) {
            bool fits = true;
            for (uint32_t k = nlp; k < nlp + 16 && fits; ++k) fits = cum[k + 1] - cum[nlp] <= 0xFFFFu || ((k + 1) & 15) == 0;
            if (!fits) break;
            nlp += 16;
        }
        if (nlp > ft.enc_nl) {
            const uint32_t ooff = 4 * ((nlp >> 4) + 2);
            pack_img.assign(img_bytes(nlp) / 4, 0);
            for (uint32_t k = 0; k < (nlp >> 4) + 2; ++k) pack_img[k] = cum[std::min<uint32_t>(16 * k, nsym + 5)];
            auto* o16 = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(pack_img.data()) + ooff);
            for (uint32_t k = 0; k < nlp + 2; ++k) o16[k] = static_cast<uint16_t>(cum[std::min<uint32_t>(k, nsym + 5)]);
            ft.enc_pack = 1;
            ft.enc_nl = nlp;
            ft.enc_pack_ooff = ooff;
            ft.enc_pack_bytes = img_bytes(nlp);
            ft.enc_sa = sa_img.empty() ? 0 : 1;
        }
    }
    if (!ft.enc_sa) sa_img.clear();
    // the packed encoder's global rows (ans_table.hpp enc_grow): (cdf(s), O(s) | O(s+1) << 16)
    // k_encode_w reads the global row of every symbol, the prefix's lanes at row nl - 1 (zero), and
    // every symbol's LDS row at min(s, nl), which for s >= nl is row C = (cdf(nl), O(nl) | O(nl+1)
    // << 16); it XORs the two, so the global rows from nl on are stored XORed with C
    std::vector<uint32_t> grow;
    if (ft.enc_pack) {
        const uint32_t nl = ft.enc_nl;
        grow.resize(2 * (static_cast<size_t>(nsym) + 1));
        const uint32_t c0 = cum[nl], c1 = (cum[nl] & 0xFFFFu) | (cum[nl + 1] << 16);
        for (uint32_t k = 0; k <= nsym; ++k) {
            grow[2 * k] = k >= nl ? cum[k] ^ c0 : 0u;
            grow[2 * k + 1] = k >= nl ? ((cum[k] & 0xFFFFu) | (cum[k + 1] << 16)) ^ c1 : 0u;
        }
    }
    // k_decode_w's LDS prefix: for each bucket width 2^shp, the longest prefix of symbols whose
    // bucket starts (u16) and cdf fit beside the ring; keep the width whose prefix covers the most
    // probability among those whose cf needs a fifth candidate at most 0.1% of the time
    std::vector<uint16_t> wide_s0;
    if (ft.dec_global && nsym <= 65536) {
        const uint32_t budget = fast::kWideDecTabBytes;
        uint32_t best_shp = 0, best_nlp = 0;
        uint64_t best_cov = 0;
        double best_far = 2.0;
        for (uint32_t shp = 0; shp <= 24; ++shp) {
            auto bytes = [&](uint32_t nlp) {
                const uint64_t nbp = nlp ? ((static_cast<uint64_t>(cum[nlp]) + (1ull << shp) - 1) >> shp) : 0;
                return ((2 * nbp + 15) & ~uint64_t(15)) + 4ull * (nlp + 6);
            };
            uint32_t lo = 0, hi = nsym;  // largest nlp with bytes(nlp) <= budget (bytes grows with nlp)
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) / 2;
                if (bytes(mid) <= budget) lo = mid;
                else hi = mid - 1;
            }
            const uint32_t nlp = lo;
            if (nlp == 0 || cum[nlp] == 0) continue;
            const uint64_t cpre = cum[nlp], nbp = (cpre + (1ull << shp) - 1) >> shp;
            uint64_t far = 0;  // cf values of the prefix past their bucket's fifth candidate
            for (uint64_t b = 0; b < nbp; ++b) {
                const uint64_t a = b << shp, e = std::min<uint64_t>(cpre, (b + 1) << shp);
                const uint64_t s0 = cat.icdf(a).first;
                const uint64_t c4 = s0 + 4 <= nsym ? cum[s0 + 4] : t.norm;
                if (c4 < e) far += e - std::max<uint64_t>(a, c4);
            }
            const double far_frac = static_cast<double>(far) / static_cast<double>(cpre);
            const bool ok = far_frac <= 1e-3, best_ok = best_far <= 1e-3;
            if ((ok && (!best_ok || cpre > best_cov)) || (!ok && !best_ok && far_frac < best_far)) {
                best_shp = shp;
                best_nlp = nlp;
                best_cov = cpre;
                best_far = far_frac;
            }
        }
        if (best_nlp > 0) {
            ft.dec_wide = 1;
            ft.dec_w_shp = best_shp;
            ft.dec_w_nlp = best_nlp;
            ft.dec_w_cpre = cum[best_nlp];
            ft.dec_w_nbp = static_cast<uint32_t>((static_cast<uint64_t>(ft.dec_w_cpre) + (1ull << best_shp) - 1) >> best_shp);
            ft.dec_w_cum_off = (2 * ft.dec_w_nbp + 15) & ~15u;
            wide_s0.resize(ft.dec_w_nbp + 2, 0);
            for (uint32_t b = 0; b < ft.dec_w_nbp; ++b)
                wide_s0[b] = static_cast<uint16_t>(cat.icdf(static_cast<uint64_t>(b) << best_shp).first);
        }
    }
    ft.nsym = nsym;
    ft.enc_rows = nsym + 1;
    ft.dec_buckets = nb;
    ft.dec_shift = shift;
    ft.norm = t.norm;
    ft.enc_lds_bytes = fast::kEncLdsBytes;  // nsym + 1 <= 257 rows, split (ans_fast.hpp)
    ft.dec_s0_off = fast::kDecS0Off;  // fixed layout (ans_fast.hpp)
    ft.dec_cum_off = fast::kDecCumOff;
    ft.dec_lds_bytes = static_cast<uint32_t>((ft.dec_cum_off + cum_bytes + 15) & ~size_t(15));
    ft.kmax = kmax;
    ft.pmax = pmax;
    ft.nr = nr;
    // k_decode's 24-bit high-word product needs hi32(q) < 2^24 too: q < 2^64 / norm
    ft.p24 = pmax < (1u << 24) && t.norm > 256 ? 1u : 0u;
    ft.K = t.K;
    ft.L = t.L;
    ft.rcp_norm = nr == fast::kNormSmall ? rcp_up(t.norm) : t.rcp_norm;
    const size_t enc_b = sizeof(EncRow) * enc.size(), dec_b = ft.dec_cum_off;  // buckets + s0 array
    const size_t decg_b = sizeof(DecBucketG) * decg.size();
    const size_t o_dec = (enc_b + 255) & ~size_t(255), o_cum = o_dec + ((dec_b + 255) & ~size_t(255));
    const size_t o_decg = o_cum + ((sizeof(uint32_t) * cum.size() + 255) & ~size_t(255));
    const size_t o_ws0 = o_decg + ((decg_b + 255) & ~size_t(255));
    const size_t ws0_b = sizeof(uint16_t) * wide_s0.size();
    const size_t o_decc = o_ws0 + ((ws0_b + 255) & ~size_t(255));
    const size_t decc_b = sizeof(DecBucketC) * decc.size();
    const size_t o_decl = o_decc + ((decc_b + 255) & ~size_t(255));
    const size_t decl_b = sizeof(DecBucketC) * decl.size();
    const size_t o_pack = o_decl + ((decl_b + 255) & ~size_t(255));
    const size_t pack_b = sizeof(uint32_t) * pack_img.size();
    const size_t o_sa = o_pack + ((pack_b + 255) & ~size_t(255));
    const size_t o_grow = o_sa + ((sa_img.size() + 255) & ~size_t(255));
    const size_t o_uimg = o_grow + ((4 * grow.size() + 255) & ~size_t(255));
    HIP_TRY(hipSetDevice(gt->g->device));
    void* mem = nullptr;
    HIP_TRY(hipMalloc(&mem, o_uimg + uimg.size() + 16));
    gt->d_fast = mem;
    char* base = static_cast<char*>(mem);
    HIP_TRY(hipMemcpy(base, enc.data(), enc_b, hipMemcpyHostToDevice));
    if (!dec.empty()) {  // buckets at 0, s0 bytes at kDecS0Off (staged into LDS as one block)
        std::vector<uint8_t> img(ft.dec_cum_off, 0);
        for (size_t j = 0; j < dec.size(); ++j) {  // halves (c0,c1) at 8j, (c2,c3) at 8 (kDecNbMax + j)
            std::memcpy(img.data() + 8 * j, &dec[j].c[0], 8);
            std::memcpy(img.data() + 8 * (fast::kDecNbMax + j), &dec[j].c[2], 8);
        }
        std::memcpy(img.data() + ft.dec_s0_off, dec_s0.data(), dec_s0.size());
        HIP_TRY(hipMemcpy(base + o_dec, img.data(), img.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(base + o_cum, cum.data(), sizeof(uint32_t) * cum.size(), hipMemcpyHostToDevice));
    if (decg_b) HIP_TRY(hipMemcpy(base + o_decg, decg.data(), decg_b, hipMemcpyHostToDevice));
    if (ws0_b) HIP_TRY(hipMemcpy(base + o_ws0, wide_s0.data(), ws0_b, hipMemcpyHostToDevice));
    if (decc_b) HIP_TRY(hipMemcpy(base + o_decc, decc.data(), decc_b, hipMemcpyHostToDevice));
    ft.dbkt_c = reinterpret_cast<const DecBucketC*>(base + o_decc);
    if (decl_b) HIP_TRY(hipMemcpy(base + o_decl, decl.data(), decl_b, hipMemcpyHostToDevice));
    ft.dbkt_cl = decl_b ? reinterpret_cast<const DecBucketC*>(base + o_decl) : ft.dbkt_c;
    if (pack_b) HIP_TRY(hipMemcpy(base + o_pack, pack_img.data(), pack_b, hipMemcpyHostToDevice));
    ft.enc_pack_img = reinterpret_cast<const uint32_t*>(base + o_pack);
    if (!sa_img.empty()) HIP_TRY(hipMemcpy(base + o_sa, sa_img.data(), sa_img.size(), hipMemcpyHostToDevice));
    ft.enc_sa_img = reinterpret_cast<const uint32_t*>(base + o_sa);
    if (!grow.empty()) HIP_TRY(hipMemcpy(base + o_grow, grow.data(), 4 * grow.size(), hipMemcpyHostToDevice));
    ft.enc_grow = reinterpret_cast<const uint32_t*>(base + o_grow);
    if (!uimg.empty()) HIP_TRY(hipMemcpy(base + o_uimg, uimg.data(), uimg.size(), hipMemcpyHostToDevice));
    ft.dec_u_img = reinterpret_cast<const uint32_t*>(base + o_uimg);
    ft.dec_w_s0 = reinterpret_cast<const uint16_t*>(base + o_ws0);
    ft.dbkt_g = reinterpret_cast<const DecBucketG*>(base + o_decg);
    ft.enc = reinterpret_cast<const EncRow*>(base);
    ft.dbkt = reinterpret_cast<const DecBucket*>(base + o_dec);
    ft.cum = reinterpret_cast<const uint32_t*>(base + o_cum);
    ft.usable = 1;
    gt->ft = ft;
    return ANS_OK;
}

}  // namespace

// Variable-chunk encode of symbols already on the device (ans_ctx.hpp): the body of
// ans_gpu_encode_var_chunks, also used by the graph dataset coder (ans_graph.hip).
int ans_encode_var_from_device(ans_gpu_table* gt, const void* d_syms, int sym_bytes, uint64_t nchunks,
                               const uint64_t* starts, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                               uint64_t* lens, uint64_t* total, int gen_kind, uint64_t seed) {
    if (out && nchunks && (!offsets || !lens)) return ANS_E_ARG;
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    uint64_t maxlen = 0;
    for (uint64_t c = 0; c < nchunks; ++c) maxlen = std::max(maxlen, starts[c + 1] - starts[c]);
    uint64_t slot_cap = 0;
    ans_gpu_slot_capacity(gt, maxlen, &slot_cap);
    HIP_TRY(hipSetDevice(gt->g->device));
    const hipStream_t s = gt->g->stream;
    DevBuf d_starts, d_slots, d_lens, d_status;
    HIP_TRY(d_starts.alloc(8 * (nchunks + 1)));
    HIP_TRY(d_slots.alloc(nchunks * slot_cap));
    HIP_TRY(d_lens.alloc(4 * nchunks));
    HIP_TRY(d_status.alloc(4));
    HIP_TRY(hipMemcpyAsync(d_starts.p, starts, 8 * (nchunks + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_status.p, 0, 4, s));
    int rc = dev_encode_var(gt, d_syms, sym_bytes, nchunks, d_starts.as<uint64_t>(), gen_kind, seed,
                            d_slots.as<uint8_t>(), slot_cap, d_lens.as<uint32_t>(), d_status.as<uint32_t>(), s,
                            staged_lmax(nchunks, maxlen, starts[nchunks] - starts[0], sym_bytes));
    if (rc || (rc = read_status(gt->g, d_status.as<uint32_t>(), s))) return rc;
    return download_container(gt->g, d_slots.as<uint8_t>(), slot_cap, d_lens.as<uint32_t>(), nchunks, s, out, out_cap,
                              offsets, lens, total);
}

// ====================================================================== C ABI (GPU part)
extern "C" {

int ans_gpu_device_count(int* count) try {
    if (!count) return ANS_E_ARG;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
    return ANS_OK;
} ANS_CATCH

int ans_gpu_create(int device, ans_gpu** out) try {
    if (!out) return ANS_E_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return ANS_E_DEVICE;
    HIP_TRY(hipSetDevice(device));
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
    auto* g = new (std::nothrow) ans_gpu{device, ncu, nullptr, nullptr, 0, nullptr, 0, LaunchLog{}};
    if (!g) return ANS_E_ALLOC;
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
        delete g;
        return ANS_E_DEVICE;
    }
    *out = g;
    return ANS_OK;
} ANS_CATCH

// The launch record as text (include/ans_capi.h).  Formatting happens here, never on a launch path.
int ans_gpu_last_launch(const ans_gpu* g, char* buf, size_t cap, size_t* len) try {
    if (!g || !len) return ANS_E_ARG;
    static const char* const kSym[9] = {"?", "u8", "u16", "?", "u32", "?", "?", "?", "u64"};
    static const char* const kNr[3] = {"std", "small", "big"};    // fast::kNormStd / kNormSmall / kNormBig
    static const char* const kMode[3] = {"far", "rows", "u"};     // fast::kModeFar / kModeRows / kModeU
    static_assert(fast::kNormStd == 0 && fast::kNormSmall == 1 && fast::kNormBig == 2, "kNr's order");
    static_assert(fast::kModeFar == 0 && fast::kModeRows == 1 && fast::kModeU == 2, "kMode's order");
    const LaunchLog& log = g->last;
    char text[LaunchLog::kCap * 96 + 8];
    size_t at = 0;
    const uint32_t n = std::min(log.n, LaunchLog::kCap);
    for (uint32_t i = 0; i < n; ++i) {
        const LaunchRec& r = log.r[i];
        const char* sym = kSym[r.sym_bytes <= 8 ? r.sym_bytes : 0];
        const int16_t* a = r.a;
        auto nr = [&](int v) { return kNr[v >= 0 && v < 3 ? v : 0]; };
        char* o = text + at;
        const size_t room = sizeof(text) - at;
        int w = 0;
        if (i) { *o++ = ';'; ++at; }
        switch (r.kind) {
        case kRecEncode: w = std::snprintf(o, room - 1, "k_encode<%s,kmax=%d,k32=%d,grows=%d,var=%d,nr=%s,m24=%d>", sym, a[0], a[1], a[2], a[3], nr(a[4]), a[5]); break;
        case kRecEncodeW: w = std::snprintf(o, room - 1, "k_encode_w<%s,k32=%d,pack=%d,sa=%d,var=%d,nr=%s>", sym, a[0], a[1], a[2], a[3], nr(a[4])); break;
        case kRecDecode: w = std::snprintf(o, room - 1, "k_decode<%s,spp=%d,mode=%s,p24=%d,j4=%d,var=%d,nr=%s>", sym, a[0], kMode[a[1] >= 0 && a[1] < 3 ? a[1] : 0], a[2], a[3], a[4], nr(a[5])); break;
        case kRecDecodeW: w = std::snprintf(o, room - 1, "k_decode_w<%s,compact=%d,prefix=%d,var=%d,p24=%d,nr=%s>", sym, a[0], a[1], a[2], a[3], nr(a[4])); break;
        case kRecDecodeG: w = std::snprintf(o, room - 1, "k_decode_g<%s,nr=%s>", sym, nr(a[0])); break;
        case kRecEncodeGeneric: w = std::snprintf(o, room - 1, "k_encode_generic<%s,lds=%d,fast=%d>", sym, a[0], a[1]); break;
        case kRecDecodeGeneric: w = std::snprintf(o, room - 1, "k_decode_generic<%s,lds=%d,fast=%d>", sym, a[0], a[1]); break;
        case kRecMenc: w = std::snprintf(o, room - 1, "k_menc<indep,%s,spp=%d,lanes=%d,res=%d,rare=%d,nr=%s>", sym, a[0], a[1], a[2], a[3], nr(a[4])); break;
        case kRecMdec: w = std::snprintf(o, room - 1, "k_mdec<indep,%s,spp=%d,lanes=%d,res=%d,lean=%d,nr=%s>", sym, a[0], a[1], a[2], a[3], nr(a[4])); break;
        case kRecEncode64: w = std::snprintf(o, room - 1, "k_encode64<catset,%s>", sym); break;
        case kRecDecode64: w = std::snprintf(o, room - 1, "k_decode64<catset,%s>", sym); break;
        case kRecPush64: w = std::snprintf(o, room - 1, "k_push64<%s>", sym); break;
        case kRecPop64: w = std::snprintf(o, room - 1, "k_pop64<%s>", sym); break;
        case kRecMsetPush: w = std::snprintf(o, room - 1, "k_mset_push<%s,cnt=%s>", sym, a[0] ? "lds" : "global"); break;
        case kRecMsetPop: w = std::snprintf(o, room - 1, "k_mset_pop<%s,cnt=%s>", sym, a[0] ? "lds" : "global"); break;
        case kRecPolyaPush: w = std::snprintf(o, room - 1, "k_polya_push<redraws=%d>", a[0]); break;
        case kRecPolyaPop: w = std::snprintf(o, room - 1, "k_polya_pop<redraws=%d>", a[0]); break;
        case kRecArerPush: w = std::snprintf(o, room - 1, "k_arer_push<orbits=%d>", a[0]); break;
        case kRecArerPop: w = std::snprintf(o, room - 1, "k_arer_pop<orbits=%d>", a[0]); break;
        case kRecArpuPush: w = std::snprintf(o, room - 1, "k_arpu_push<orbits=%d>", a[0]); break;
        case kRecArpuPop: w = std::snprintf(o, room - 1, "k_arpu_pop<orbits=%d>", a[0]); break;
        case kRecArerWlPush: w = std::snprintf(o, room - 1, "k_arer_wl_push(wl_iter=%d,half_iter=%d)", a[0], a[2]); break;
        case kRecArerWlPop: w = std::snprintf(o, room - 1, "k_arer_wl_pop(wl_iter=%d,half_iter=%d)", a[0], a[2]); break;
        case kRecArpuWlPush: w = std::snprintf(o, room - 1, "k_arpu_wl_push(wl_iter=%d,half_iter=%d)", a[0], a[2]); break;
        case kRecArpuWlPop: w = std::snprintf(o, room - 1, "k_arpu_wl_pop(wl_iter=%d,half_iter=%d)", a[0], a[2]); break;
        case kRecArerWllPush: w = std::snprintf(o, room - 1, "k_arer_wll_push(wl_iter=%d,half_iter=%d,node=%d,edge=%d)", a[0], a[2], a[3], a[4]); break;
        case kRecArerWllPop: w = std::snprintf(o, room - 1, "k_arer_wll_pop(wl_iter=%d,half_iter=%d,node=%d,edge=%d)", a[0], a[2], a[3], a[4]); break;
        case kRecArpuWllPush: w = std::snprintf(o, room - 1, "k_arpu_wll_push(wl_iter=%d,half_iter=%d,node=%d,edge=%d)", a[0], a[2], a[3], a[4]); break;
        case kRecArpuWllPop: w = std::snprintf(o, room - 1, "k_arpu_wll_pop(wl_iter=%d,half_iter=%d,node=%d,edge=%d)", a[0], a[2], a[3], a[4]); break;
        case kRecJointErPush: w = std::snprintf(o, room - 1, "k_joint_er_push(wl_iter=%d,half_iter=%d)", a[0], a[2]); break;
        case kRecJointErPop: w = std::snprintf(o, room - 1, "k_joint_er_pop(wl_iter=%d,half_iter=%d)", a[0], a[2]); break;
        case kRecJointPuPush: w = std::snprintf(o, room - 1, "k_joint_pu_push(wl_iter=%d,half_iter=%d,redraws=%d)", a[0], a[2], a[3]); break;
        case kRecJointPuPop: w = std::snprintf(o, room - 1, "k_joint_pu_pop(wl_iter=%d,half_iter=%d,redraws=%d)", a[0], a[2], a[3]); break;
        default: w = std::snprintf(o, room - 1, "?"); break;
        }
        at += static_cast<size_t>(w);
    }
    if (log.n > LaunchLog::kCap) at += static_cast<size_t>(std::snprintf(text + at, sizeof(text) - at, ";+%u", log.n - LaunchLog::kCap));
    *len = at;
    if (!buf || cap <= at) return ANS_E_LEN;
    std::memcpy(buf, text, at);
    buf[at] = 0;
    return ANS_OK;
} ANS_CATCH

// The workgroup count of a recorded launch (include/ans_capi.h): kept by the kinds whose launch
// bounds the lanes by a workspace, 0 for the others.
int ans_gpu_last_launch_grid(const ans_gpu* g, uint32_t index, uint32_t* workgroups) try {
    if (!g || !workgroups) return ANS_E_ARG;
    const LaunchLog& log = g->last;
    if (index >= std::min(log.n, LaunchLog::kCap)) return ANS_E_ARG;
    const LaunchRec& r = log.r[index];
    const int slot = rec_grid_slot(r.kind);
    *workgroups = slot < 0 ? 0u : static_cast<uint32_t>(r.a[slot]);
    return ANS_OK;
} ANS_CATCH

void ans_gpu_free(ans_gpu* g) try {
    if (!g) return;
    (void)hipSetDevice(g->device);
    ans_pipe_free(g);
    if (g->d_scratch) (void)hipFree(g->d_scratch);
    if (g->d_mset_ws) (void)hipFree(g->d_mset_ws);
    if (g->d_degree_rank) (void)hipFree(g->d_degree_rank);
    (void)hipStreamDestroy(g->stream);
    delete g;
} ANS_CATCH_VOID

int ans_gpu_table_create(ans_gpu* g, const ans_table* tab, ans_gpu_table** out) try {
    if (!g || !tab || !out) return ANS_E_ARG;
    *out = nullptr;
    const Categorical& cat = tab->cat;
    const uint64_t nsym = cat.masses.size();
    if (nsym == 0 || cat.norm() == 0 || cat.norm() > kMaxMinHead) return ANS_E_NORM_RANGE;
    if (nsym > 65536 || cat.norm() >= (1ull << 32)) {  // the exact 64-bit kernels (ans_codecs.hip)
        const Categorical* one = &cat;
        ans_gpu_tableset* ts = nullptr;
        const int rc = ans_tableset_build(g, &one, 1, &ts);
        if (rc) return rc;
        DevTable t{};
        t.nsym = nsym > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(nsym);
        auto* gt = new (std::nothrow) ans_gpu_table{g, g->device, t, nullptr, 0, FastTable{}, nullptr, ts};
        if (!gt) {
            ans_tableset_destroy(ts);
            return ANS_E_ALLOC;
        }
        if (nsym == 2) std::copy_n(cat.masses.begin(), 2, gt->mass2);
        *out = gt;
        return ANS_OK;
    }
    DevTable t{};
    t.nsym = static_cast<uint32_t>(nsym);
    t.norm = static_cast<uint32_t>(cat.norm());
    t.K = kMaxMinHead / t.norm;
    t.L = static_cast<uint64_t>(t.norm) * t.K;
    t.rcp_norm = 1.0 / static_cast<double>(t.norm);
    t.fast = (t.norm >= (1u << 16) && t.norm <= (1u << 31)) ? 1u : 0u;
    std::vector<DevSym> rows(nsym + 1);
    uint32_t pmin = 0xffffffffu;
    for (uint64_t s = 0; s < nsym; ++s) {
        const uint32_t m = static_cast<uint32_t>(cat.masses[s]);
        rows[s] = DevSym{m, static_cast<uint32_t>(cat.cummasses[s]), m ? 1.0 / static_cast<double>(m) : 0.0};
        if (m && m < pmin) pmin = m;
    }
    rows[nsym] = DevSym{0, t.norm, 0.0};
    t.pmin = pmin;
    // icdf buckets: width 2^shift so that ceil(norm / 2^shift) <= 2^kBucketBits.
    uint32_t bits = 0;
    while (bits < 32 && (1ull << bits) < t.norm) ++bits;  // 2^bits >= norm
    t.shift = bits > kBucketBits ? bits - kBucketBits : 0;
    t.nbucket = static_cast<uint32_t>((static_cast<uint64_t>(t.norm) + (1ull << t.shift) - 1) >> t.shift);
    std::vector<uint16_t> buckets(t.nbucket);
    for (uint32_t j = 0; j < t.nbucket; ++j)
        buckets[j] = static_cast<uint16_t>(cat.icdf(static_cast<uint64_t>(j) << t.shift).first);
    const size_t rows_bytes = sizeof(DevSym) * rows.size();
    const size_t bucket_bytes = sizeof(uint16_t) * buckets.size();
    HIP_TRY(hipSetDevice(g->device));
    void* mem = nullptr;
    HIP_TRY(hipMalloc(&mem, rows_bytes + bucket_bytes + 16));
    HIP_TRY(hipMemcpy(mem, rows.data(), rows_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(static_cast<char*>(mem) + rows_bytes, buckets.data(), bucket_bytes, hipMemcpyHostToDevice));
    t.sym = static_cast<const DevSym*>(mem);
    t.bucket = reinterpret_cast<const uint16_t*>(static_cast<char*>(mem) + rows_bytes);
    auto* gt = new (std::nothrow) ans_gpu_table{g, g->device, t, mem, 0, FastTable{}, nullptr, nullptr};
    if (!gt) { (void)hipFree(mem); return ANS_E_ALLOC; }
    if (nsym == 2) std::copy_n(cat.masses.begin(), 2, gt->mass2);
    if (rows_bytes + bucket_bytes <= kLdsTableLimit) gt->lds_bytes = static_cast<uint32_t>(rows_bytes + bucket_bytes);
    const int rc = build_fast_table(gt, cat);
    if (rc) {
        ans_gpu_table_free(gt);
        return rc;
    }
    *out = gt;
    return ANS_OK;
} ANS_CATCH

void ans_gpu_table_free(ans_gpu_table* gt) try {
    if (!gt) return;
    (void)hipSetDevice(gt->device);  // (not gt->g: a table may be freed after its context)
    if (gt->ts64) ans_tableset_destroy(gt->ts64);
    if (gt->d_mem) (void)hipFree(gt->d_mem);
    if (gt->d_fast) (void)hipFree(gt->d_fast);
    delete gt;
} ANS_CATCH_VOID

int ans_gpu_table_paths(const ans_gpu_table* gt, uint32_t* paths) try {
    if (!gt || !paths) return ANS_E_ARG;
    const FastTable& ft = gt->ft;
    uint32_t p = 0;
    if (ft.usable) p |= ft.enc_global ? ANS_PATH_ENC_GLOBAL : ANS_PATH_ENC_LDS;
    if (ft.usable && ft.dec_usable) p |= ANS_PATH_DEC_LDS;
    if (ft.usable && ft.dec_global) p |= ANS_PATH_DEC_GLOBAL;
    if (ft.usable && ft.enc_wide) p |= ANS_PATH_ENC_WIDE;
    if (ft.usable && ft.dec_wide) p |= ANS_PATH_DEC_WIDE;
    if (ft.usable && ft.dec_wide && ft.dec_c) p |= ANS_PATH_DEC_COMPACT;
    if (ft.usable && ft.enc_wide && ft.enc_pack) p |= ANS_PATH_ENC_PACKED;
    if (ft.usable && ft.enc_wide && ft.enc_sa) p |= ANS_PATH_ENC_SHIFT;
    if (ft.usable && ft.dec_usable && !ft.dec_far && ft.dec_u) p |= ANS_PATH_DEC_U;
    *paths = p;
    return ANS_OK;
} ANS_CATCH

int ans_gpu_slot_capacity(const ans_gpu_table* gt, uint64_t chunk_len, uint64_t* slot_cap) try {
    if (!gt || !slot_cap) return ANS_E_ARG;
    if (gt->ts64) {
        *slot_cap = ans_tableset_slot_bytes(gt->ts64, chunk_len);
        return ANS_OK;
    }
    // Bytes of one flattened chunk <= (sum_i log2(norm/p_i) + 1 + L*log2(1+1/K)) / 8 + 8
    // (virtual-bits argument); take every p_i = pmin, plus margin.
    const double per_sym = std::log2(static_cast<double>(gt->t.norm) / static_cast<double>(gt->t.pmin)) +
                           2.0 / static_cast<double>(gt->t.K) + 1e-6;
    const double bytes = (static_cast<double>(chunk_len) * per_sym + 2.0) / 8.0 + 9.0;
    // + one page of slack: the fast encoder writes whole 64-byte pages (ans_fast.hpp)
    const uint64_t cap = static_cast<uint64_t>(std::ceil(bytes)) + 8 + 64;
    *slot_cap = (cap + 127) & ~uint64_t(127);
    return ANS_OK;
} ANS_CATCH

int ans_dev_encode_chunks_ex(ans_gpu_table* gt, const void* d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                             int gen_kind, uint64_t seed, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                             uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !d_status || !valid_width_u32(sym_bytes) || chunk_len == 0 || (slot_cap & 15) || !valid_kind(gen_kind))
        return ANS_E_ARG;
    if (n && (!d_syms || !d_slots || !d_lens)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    const hipStream_t s = pick(gt, stream);
    if (gt->ts64)
        return ans_tableset_dev_encode(gt->ts64, d_syms, sym_bytes, nullptr, n, chunk_len, (n + chunk_len - 1) / chunk_len,
                                       d_slots, slot_cap, d_lens, d_status, gen_kind, seed, s);
    const fast::ChunkInit ini{gen_kind, seed};
    return with_sym_type(sym_bytes, [&](auto t) {
        return launch_encode<decltype(t)>(gt, d_syms, n, chunk_len, d_slots, slot_cap, d_lens, d_status, s, ini);
    });
} ANS_CATCH

int ans_dev_encode_chunks(ans_gpu_table* gt, const void* d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                          uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    return ans_dev_encode_chunks_ex(gt, d_syms, sym_bytes, n, chunk_len, ANS_GEN_ZEROS, 0, d_slots, slot_cap, d_lens,
                                    d_status, stream);
} ANS_CATCH

int ans_dev_decode_chunks_ex(ans_gpu_table* gt, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t slot_cap,
                             const uint32_t* d_lens, uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed,
                             void* d_syms, int sym_bytes, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !d_status || !valid_width_u32(sym_bytes) || chunk_len == 0 || !valid_kind(gen_kind)) return ANS_E_ARG;
    if (n && (!d_in || !d_lens || !d_syms)) return ANS_E_ARG;
    if (sym_bytes == 1 && gt->t.nsym > 256) return ANS_E_ARG;
    if (sym_bytes == 2 && gt->t.nsym > 65536) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    const hipStream_t s = pick(gt, stream);
    if (gt->ts64)
        return ans_tableset_dev_decode(gt->ts64, d_in, d_offsets, slot_cap, d_lens, nullptr, n, chunk_len,
                                       (n + chunk_len - 1) / chunk_len, gen_kind, seed, d_syms, sym_bytes, d_status, s);
    const fast::ChunkInit ini{gen_kind, seed};
    return with_sym_type(sym_bytes, [&](auto t) {
        return launch_decode<decltype(t)>(gt, d_in, d_offsets, slot_cap, d_lens, n, chunk_len, gen_kind, d_syms, d_status,
                                          s, ini);
    });
} ANS_CATCH

int ans_dev_decode_chunks(ans_gpu_table* gt, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t slot_cap,
                          const uint32_t* d_lens, uint64_t n, uint64_t chunk_len, int gen_kind, void* d_syms,
                          int sym_bytes, uint32_t* d_status, void* stream) try {
    if (gen_kind != ANS_GEN_ZEROS && gen_kind != ANS_GEN_EMPTY) return ANS_E_ARG;  // RANDOM needs a seed: _ex
    return ans_dev_decode_chunks_ex(gt, d_in, d_offsets, slot_cap, d_lens, n, chunk_len, gen_kind, 0, d_syms, sym_bytes,
                                    d_status, stream);
} ANS_CATCH

int ans_dev_gen_iid(ans_gpu_table* gt, uint64_t seed, uint64_t start, uint64_t n, void* d_syms, int sym_bytes,
                    void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !valid_width_u32(sym_bytes) || (n && !d_syms)) return ANS_E_ARG;
    if (gt->ts64) return ANS_E_NORM_RANGE;  // the synthetic generator reads u32 tables
    if (sym_bytes == 1 && gt->t.nsym > 256) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    const hipStream_t s = pick(gt, stream);
    return with_sym_type(sym_bytes, [&](auto t) {
        return launch_gen<decltype(t)>(gt, seed, start, n, d_syms, s);
    });
} ANS_CATCH

int ans_dev_check_renorm(ans_gpu* g, const uint64_t* d_heads, const uint32_t* d_windows, uint64_t L, uint64_t n,
                         uint64_t* d_out_heads, uint32_t* d_out_k, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g || (n && (!d_heads || !d_windows || !d_out_heads || !d_out_k))) return ANS_E_ARG;
    if (n == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = stream ? static_cast<hipStream_t>(stream) : g->stream;
    k_check_renorm<<<static_cast<unsigned>((n + 255) / 256), 256, 0, s>>>(d_heads, d_windows, L, n, d_out_heads, d_out_k);
    HIP_TRY(hipGetLastError());
    return ANS_OK;
} ANS_CATCH

int ans_dev_sample_iid(ans_gpu_table* gt, uint64_t seed, uint64_t n, uint64_t chunk_len, void* d_syms, int sym_bytes,
                       void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !valid_width_u32(sym_bytes) || chunk_len == 0 || (n && !d_syms)) return ANS_E_ARG;
    if (gt->ts64) return ANS_E_NORM_RANGE;  // the sampler reads u32 tables
    if (sym_bytes == 1 && gt->t.nsym > 256) return ANS_E_ARG;
    if (sym_bytes == 2 && gt->t.nsym > 65536) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    const hipStream_t s = pick(gt, stream);
    return with_sym_type(sym_bytes, [&](auto t) {
        return launch_sample<decltype(t)>(gt, seed, n, chunk_len, d_syms, s);
    });
} ANS_CATCH

int ans_gpu_sample_iid(ans_gpu_table* gt, uint64_t seed, uint64_t n, uint64_t chunk_len, void* out, int sym_bytes) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !valid_width_u32(sym_bytes) || chunk_len == 0 || (n && !out)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    DevBuf d;
    HIP_TRY(d.alloc(n * sym_bytes));
    const int rc = ans_dev_sample_iid(gt, seed, n, chunk_len, d.p, sym_bytes, nullptr);
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(out, d.p, n * sym_bytes, hipMemcpyDeviceToHost, gt->g->stream));
    HIP_TRY(hipStreamSynchronize(gt->g->stream));
    return ANS_OK;
} ANS_CATCH

// The longest variable chunk and the total of device-resident starts (one workgroup: a strided
// max per lane, a wave shfl_xor reduction, the 16 wave maxima through LDS) -> out[0], out[1].
__global__ __launch_bounds__(1024) void k_span_stats(const uint64_t* __restrict__ starts, uint64_t nchunks,
                                                    uint64_t* __restrict__ out) {
    __shared__ uint64_t part[16];
    uint64_t m = 0;
    for (uint64_t c = threadIdx.x; c < nchunks; c += 1024) {
        const uint64_t a = starts[c], b = starts[c + 1];
        m = max(m, b >= a ? b - a : ~0ull);  // decreasing starts: no staging (the kernels report them)
    }
    for (int d = 32; d >= 1; d >>= 1) m = max(m, static_cast<uint64_t>(__shfl_xor(m, d)));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = max(m, part[w]);
        out[0] = m;
        out[1] = starts[nchunks] - starts[0];
    }
}

// staged_lmax for device-resident starts: k_span_stats, one 16-B copy back and a stream
// synchronisation (the device API's variable chunks then take the staged fast kernels, as the
// host API's do); 0 (the generic kernels) when the staged layout would exceed the budget
static int device_lmax(const uint64_t* d_starts, uint64_t nchunks, int sym_bytes, hipStream_t s, uint64_t* lmax) {
    *lmax = 0;
    if (nchunks == 0) return ANS_OK;
    void* mem = nullptr;
    if (hipMallocAsync(&mem, 16, s) != hipSuccess) {
        (void)hipGetLastError();
        return ANS_OK;  // the generic kernels
    }
    uint64_t h[2] = {0, 0};
    k_span_stats<<<1, 1024, 0, s>>>(d_starts, nchunks, static_cast<uint64_t*>(mem));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, mem, 16, hipMemcpyDeviceToHost, s);
    const hipError_t f = hipFreeAsync(mem, s);
    if (e == hipSuccess) e = f;
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    HIP_TRY(e);
    *lmax = (h[0] >> 32) ? 0 : staged_lmax(nchunks, h[0], h[1], sym_bytes);
    return ANS_OK;
}

// lmax > 0 (the longest chunk): the staged fast kernels where the table has them
// (launch_staged_encode); the device API finds it with device_lmax
int dev_encode_var(ans_gpu_table* gt, const void* d_syms, int sym_bytes, uint64_t nchunks,
                          const uint64_t* d_starts, int gen_kind, uint64_t seed, uint8_t* d_slots, uint64_t slot_cap,
                          uint32_t* d_lens, uint32_t* d_status, void* stream, uint64_t lmax) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !d_status || !valid_width_u32(sym_bytes) || (slot_cap & 15) || !valid_kind(gen_kind)) return ANS_E_ARG;
    if (nchunks && (!d_syms || !d_starts || !d_slots || !d_lens)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    const hipStream_t s = pick(gt, stream);
    if (gt->ts64)
        return ans_tableset_dev_encode(gt->ts64, d_syms, sym_bytes, d_starts, 0, 0, nchunks, d_slots, slot_cap, d_lens,
                                       d_status, gen_kind, seed, s);
    const fast::ChunkInit ini{gen_kind, seed};
    return with_sym_type(sym_bytes, [&](auto t) {
        return launch_encode_var<decltype(t)>(gt, d_syms, nchunks, d_starts, d_slots, slot_cap, d_lens, d_status, s, ini,
                                              lmax);
    });
} ANS_CATCH

int ans_dev_encode_var_chunks_ex(ans_gpu_table* gt, const void* d_syms, int sym_bytes, uint64_t nchunks,
                                 const uint64_t* d_starts, int gen_kind, uint64_t seed, uint8_t* d_slots,
                                 uint64_t slot_cap, uint32_t* d_lens, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();
    if (!gt || !valid_width_u32(sym_bytes)) return ANS_E_ARG;
    if (nchunks && !d_starts) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    uint64_t lmax = 0;
    if (!gt->ts64) {
        const int rc = device_lmax(d_starts, nchunks, sym_bytes, pick(gt, stream), &lmax);
        if (rc) return rc;
    }
    return dev_encode_var(gt, d_syms, sym_bytes, nchunks, d_starts, gen_kind, seed, d_slots, slot_cap, d_lens, d_status,
                          stream, lmax);
} ANS_CATCH

int ans_dev_encode_var_chunks(ans_gpu_table* gt, const void* d_syms, int sym_bytes, uint64_t nchunks,
                              const uint64_t* d_starts, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                              uint32_t* d_status, void* stream) try {
    return ans_dev_encode_var_chunks_ex(gt, d_syms, sym_bytes, nchunks, d_starts, ANS_GEN_ZEROS, 0, d_slots, slot_cap,
                                        d_lens, d_status, stream);
} ANS_CATCH

int dev_decode_var(ans_gpu_table* gt, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t slot_cap,
                          const uint32_t* d_lens, uint64_t nchunks, const uint64_t* d_starts, int gen_kind,
                          uint64_t seed, void* d_syms, int sym_bytes, uint32_t* d_status, void* stream, uint64_t lmax) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !d_status || !valid_width_u32(sym_bytes) || !valid_kind(gen_kind)) return ANS_E_ARG;
    if (nchunks && (!d_in || !d_lens || !d_starts || !d_syms)) return ANS_E_ARG;
    if ((sym_bytes == 1 && gt->t.nsym > 256) || (sym_bytes == 2 && gt->t.nsym > 65536)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    const hipStream_t s = pick(gt, stream);
    if (gt->ts64)
        return ans_tableset_dev_decode(gt->ts64, d_in, d_offsets, slot_cap, d_lens, d_starts, 0, 0, nchunks, gen_kind,
                                       seed, d_syms, sym_bytes, d_status, s);
    const fast::ChunkInit ini{gen_kind, seed};
    return with_sym_type(sym_bytes, [&](auto t) {
        return launch_decode_var<decltype(t)>(gt, d_in, d_offsets, slot_cap, d_lens, nchunks, d_starts, gen_kind, d_syms,
                                              d_status, s, ini, lmax);
    });
} ANS_CATCH

int ans_dev_decode_var_chunks_ex(ans_gpu_table* gt, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t slot_cap,
                                 const uint32_t* d_lens, uint64_t nchunks, const uint64_t* d_starts, int gen_kind,
                                 uint64_t seed, void* d_syms, int sym_bytes, uint32_t* d_status, void* stream) try {
    (void)hipGetLastError();
    if (!gt || !valid_width_u32(sym_bytes)) return ANS_E_ARG;
    if (nchunks && !d_starts) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    uint64_t lmax = 0;
    if (!gt->ts64) {
        const int rc = device_lmax(d_starts, nchunks, sym_bytes, pick(gt, stream), &lmax);
        if (rc) return rc;
    }
    return dev_decode_var(gt, d_in, d_offsets, slot_cap, d_lens, nchunks, d_starts, gen_kind, seed, d_syms, sym_bytes,
                          d_status, stream, lmax);
} ANS_CATCH

int ans_dev_decode_var_chunks(ans_gpu_table* gt, const uint8_t* d_in, const uint64_t* d_offsets, uint64_t slot_cap,
                              const uint32_t* d_lens, uint64_t nchunks, const uint64_t* d_starts, int gen_kind,
                              void* d_syms, int sym_bytes, uint32_t* d_status, void* stream) try {
    if (gen_kind != ANS_GEN_ZEROS && gen_kind != ANS_GEN_EMPTY) return ANS_E_ARG;  // RANDOM needs a seed: _ex
    return ans_dev_decode_var_chunks_ex(gt, d_in, d_offsets, slot_cap, d_lens, nchunks, d_starts, gen_kind, 0, d_syms,
                                        sym_bytes, d_status, stream);
} ANS_CATCH

int ans_gpu_encode_var_chunks_ex(ans_gpu_table* gt, const void* syms, int sym_bytes, uint64_t nchunks,
                                 const uint64_t* starts, int gen_kind, uint64_t seed, uint8_t* out, uint64_t out_cap,
                                 uint64_t* offsets, uint64_t* lens, uint64_t* total) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !valid_width_u32(sym_bytes) || !total || (nchunks && !starts) || !valid_kind(gen_kind)) return ANS_E_ARG;
    *total = 0;
    if (nchunks == 0) return ANS_OK;
    for (uint64_t c = 0; c < nchunks; ++c)
        if (starts[c + 1] < starts[c]) return ANS_E_ARG;
    const uint64_t n = starts[nchunks];
    if (n && !syms) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    DevBuf d_syms;
    HIP_TRY(d_syms.alloc(n * sym_bytes));
    if (n) HIP_TRY(hipMemcpyAsync(d_syms.p, syms, n * sym_bytes, hipMemcpyHostToDevice, gt->g->stream));
    return ans_encode_var_from_device(gt, d_syms.p, sym_bytes, nchunks, starts, out, out_cap, offsets, lens, total,
                                      gen_kind, seed);
} ANS_CATCH

int ans_gpu_encode_var_chunks(ans_gpu_table* gt, const void* syms, int sym_bytes, uint64_t nchunks,
                              const uint64_t* starts, uint8_t* out, uint64_t out_cap, uint64_t* offsets,
                              uint64_t* lens, uint64_t* total) try {
    return ans_gpu_encode_var_chunks_ex(gt, syms, sym_bytes, nchunks, starts, ANS_GEN_ZEROS, 0, out, out_cap, offsets,
                                        lens, total);
} ANS_CATCH

int ans_gpu_decode_var_chunks_ex(ans_gpu_table* gt, const uint8_t* in, uint64_t in_len, const uint64_t* offsets,
                                 const uint64_t* lens, uint64_t nchunks, const uint64_t* starts, int gen_kind,
                                 uint64_t seed, void* out, int sym_bytes) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!gt || !valid_width_u32(sym_bytes) || (nchunks && (!starts || !offsets || !lens)) || !valid_kind(gen_kind))
        return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    uint64_t maxlen = 0;
    for (uint64_t c = 0; c < nchunks; ++c) {
        if (starts[c + 1] < starts[c]) return ANS_E_ARG;
        maxlen = std::max(maxlen, starts[c + 1] - starts[c]);
    }
    std::vector<uint32_t> l32;
    int rc = narrow_lens(offsets, lens, nchunks, in_len, l32);
    if (rc) return rc;
    const uint64_t n = starts[nchunks];
    if ((n && !out) || (in_len && !in)) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(gt->g->device));
    const hipStream_t s = gt->g->stream;
    DevStreams d;
    DevBuf d_starts, d_out;
    if ((rc = upload_streams(in, in_len, offsets, l32, s, d))) return rc;
    HIP_TRY(d_starts.alloc(8 * (nchunks + 1)));
    HIP_TRY(d_out.alloc(n * sym_bytes));
    HIP_TRY(hipMemcpyAsync(d_starts.p, starts, 8 * (nchunks + 1), hipMemcpyHostToDevice, s));
    rc = dev_decode_var(gt, d.in.as<uint8_t>(), d.offs.as<uint64_t>(), 0, d.lens.as<uint32_t>(), nchunks,
                        d_starts.as<uint64_t>(), gen_kind, seed, d_out.p, sym_bytes, d.status.as<uint32_t>(), s,
                        staged_lmax(nchunks, maxlen, n, sym_bytes));
    if (rc || (rc = read_status(gt->g, d.status.as<uint32_t>(), s))) return rc;
    if (n) HIP_TRY(hipMemcpy(out, d_out.p, n * sym_bytes, hipMemcpyDeviceToHost));
    return ANS_OK;
} ANS_CATCH

int ans_gpu_decode_var_chunks(ans_gpu_table* gt, const uint8_t* in, uint64_t in_len, const uint64_t* offsets,
                              const uint64_t* lens, uint64_t nchunks, const uint64_t* starts, int gen_kind, void* out,
                              int sym_bytes) try {
    if (gen_kind != ANS_GEN_ZEROS && gen_kind != ANS_GEN_EMPTY) return ANS_E_ARG;  // RANDOM needs a seed: _ex
    return ans_gpu_decode_var_chunks_ex(gt, in, in_len, offsets, lens, nchunks, starts, gen_kind, 0, out, sym_bytes);
} ANS_CATCH

int ans_dev_compact(ans_gpu* g, const uint8_t* d_slots, uint64_t slot_cap, const uint32_t* d_lens,
                    const uint64_t* d_offsets, uint64_t nchunks, uint8_t* d_out, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g) return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = stream ? static_cast<hipStream_t>(stream) : g->stream;
    k_compact<<<grid_for(nchunks * 64), kBlock, 0, s>>>(d_slots, slot_cap, d_lens, d_offsets, nchunks, d_out);
    HIP_TRY(hipGetLastError());
    return ANS_OK;
} ANS_CATCH

int ans_dev_expand(ans_gpu* g, const uint8_t* d_in, const uint64_t* d_offsets, const uint32_t* d_lens,
                   uint64_t nchunks, uint8_t* d_slots, uint64_t slot_cap, void* stream) try {
    (void)hipGetLastError();  // drop a stale error another caller left on this thread
    if (!g) return ANS_E_ARG;
    if (nchunks == 0) return ANS_OK;
    if (!d_in || !d_offsets || !d_lens || !d_slots) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = stream ? static_cast<hipStream_t>(stream) : g->stream;
    k_expand<<<grid_for(nchunks * 64), kBlock, 0, s>>>(d_in, d_offsets, d_lens, nchunks, d_slots, slot_cap);
    HIP_TRY(hipGetLastError());
    return ANS_OK;
} ANS_CATCH

uint64_t ans_dense_offsets_entries(uint64_t nchunks) { return nchunks + 1 + (nchunks + kScanTile - 1) / kScanTile; }

int ans_dev_encode_dense_ex(ans_gpu_table* gt, const void* d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                            int gen_kind, uint64_t seed, uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens,
                            uint64_t* d_offsets, uint8_t* d_out, uint64_t out_cap, uint32_t* d_status, void* stream) try {
    if (n && (!d_offsets || !d_out)) return ANS_E_ARG;
    int rc = ans_dev_encode_chunks_ex(gt, d_syms, sym_bytes, n, chunk_len, gen_kind, seed, d_slots, slot_cap, d_lens,
                                      d_status, stream);
    if (rc) return rc;
    const uint64_t nchunks = (n + chunk_len - 1) / chunk_len;
    const hipStream_t s = pick(gt, stream);
    if (nchunks == 0) {
        if (d_offsets) HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), s));
        return ANS_OK;
    }
    const uint64_t ntiles = (nchunks + kScanTile - 1) / kScanTile;
    uint64_t* tile = d_offsets + nchunks + 1;
    k_scan_tiles<<<static_cast<unsigned>(ntiles), 1024, 0, s>>>(d_lens, nchunks, slot_cap, d_offsets, tile);
    k_scan_tile_sums<<<1, 1024, 0, s>>>(tile, ntiles, d_offsets + nchunks);
    k_compact_dense<<<grid_for(nchunks * 64), kBlock, 0, s>>>(d_slots, slot_cap, d_lens, d_offsets, tile, nchunks,
                                                              d_out, out_cap, d_status);
    HIP_TRY(hipGetLastError());
    return ANS_OK;
} ANS_CATCH

int ans_dev_encode_dense(ans_gpu_table* gt, const void* d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                         uint8_t* d_slots, uint64_t slot_cap, uint32_t* d_lens, uint64_t* d_offsets, uint8_t* d_out,
                         uint64_t out_cap, uint32_t* d_status, void* stream) try {
    return ans_dev_encode_dense_ex(gt, d_syms, sym_bytes, n, chunk_len, ANS_GEN_ZEROS, 0, d_slots, slot_cap, d_lens,
                                   d_offsets, d_out, out_cap, d_status, stream);
} ANS_CATCH

int ans_dev_status(ans_gpu* g, const uint32_t* d_status, void* stream, int* status) try {
    if (!g || !d_status || !status) return ANS_E_ARG;
    HIP_TRY(hipSetDevice(g->device));
    const hipStream_t s = stream ? static_cast<hipStream_t>(stream) : g->stream;
    uint32_t bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, d_status, sizeof(bits), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *status = lowest_status(bits);
    return ANS_OK;
} ANS_CATCH

}  // extern "C"
