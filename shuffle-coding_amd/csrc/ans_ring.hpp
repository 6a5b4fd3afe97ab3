// ans_ring.hpp — the one stream ring of the fast coders (included by ans_fast.hpp).
//
// Every fast coder keeps its chunk's byte stream in a lane-private LDS ring of 32 dwords (two
// 64-B pages) in a [dword][lane] image, so any lane-varying index is bank-conflict free and a
// page is 16 accesses at immediate offsets from one address.  This header holds everything about
// moving a stream between global memory and that ring, on a layout policy (RingLayout): the ring
// and the byte funnel of the encoders (RingT, FunnelT, PageOut) and the page-landing ring of the
// decoders (DecRingT).  It holds nothing about coding: the chains of ans_fast.hpp, ans_wide.hpp
// and ans_mfast.hpp are one of these rings plus their own renorm, lookup and update.
// (k_decode_g's DecChainG is a different ring, four 64-B pages, and stays in ans_fast.hpp.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace shuffle_coding {
namespace fast {

// Non-temporal 16-byte global load / store (streamed data that must not evict cached tables).
typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 nt_load(const uint4* p) {
    const v4u32 v = __builtin_nontemporal_load(reinterpret_cast<const v4u32*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_store(uint4* p, const uint4& v) {
    __builtin_nontemporal_store(v4u32{v.x, v.y, v.z, v.w}, reinterpret_cast<v4u32*>(p));
}

// s_waitcnt vmcnt(0) (gfx9 encoding; expcnt/lgkmcnt left at their maxima).
__device__ __forceinline__ void wait_vm() { __builtin_amdgcn_s_waitcnt(0x0F70); }
// s_waitcnt vmcnt(N): all but the N youngest vector-memory operations done (in issue order)
template <int N>
__device__ __forceinline__ void wait_vm_n() {
    static_assert(N >= 0 && N < 64, "vmcnt field");
    __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
}

// x << S in 16 bits (the upper half of the result is zero on gfx950): v_lshlrev_b16 issues in
// ~2.5 cycles per wave64 instruction where v_lshlrev_b32 and its SDWA forms take ~4.4
// (tools/b16_probe.hip), so LDS addresses below 2^16 are formed with it
template <int S>
__device__ __forceinline__ uint32_t shl16(uint32_t x) {
    static_assert(S >= 0 && S < 16, "16-bit shift");
    uint32_t r;
    asm("v_lshlrev_b16 %0, %1, %2" : "=v"(r) : "I"(S), "v"(x));
    return r;
}

__device__ __forceinline__ uint32_t ab(uint32_t hi, uint32_t lo, uint32_t s) {
    return __builtin_amdgcn_alignbyte(hi, lo, s);
}

// LDS accesses by byte offset (address space 3): keeps the address arithmetic in 32 bits
// where the compiler otherwise adds the (zero) LDS base or splits constants out of offsets.
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint64_t lds_u64;
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
__device__ __forceinline__ uint32_t lds_ld32(uint32_t off) { return *reinterpret_cast<const lds_u32*>(static_cast<uintptr_t>(off)); }
__device__ __forceinline__ uint64_t lds_ld64(uint32_t off) { return *reinterpret_cast<const lds_u64*>(static_cast<uintptr_t>(off)); }
typedef __attribute__((address_space(3))) v4u32 lds_v4u32;
__device__ __forceinline__ uint4 lds_ld128(uint32_t off) {
    const v4u32 v = *reinterpret_cast<const lds_v4u32*>(static_cast<uintptr_t>(off));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// ====================================================================== layout
// Where one ring lives and how its addresses are formed: static members only, one instance per
// ring.  Stream dword i lives in ring row i & 31 of the lane's column col = 4 * lane, at
// kRing + ((i & 31) << kRowShift) + col.  Each kernel keeps the row-address form it was tuned
// with (RowForm); the forms compute the same address.
//  kL     lanes per workgroup (a row is 4 kL bytes)
//  kBase  the ring's LDS base (row 0); added in the instructions' offset fields
//  kUnit  what a stream position counts: 1 = bytes, 8 = bits (renorm_up8 returns bit counts, and
//         v_alignbit_b32 takes the window's bit offset 8 (P & 3) = P8 & 31 as it is)
//  kFold  a decoder's page landing folds the ring base and the page's first row into the
//         ds_write2st64 offset fields and stores from col itself (rows 4 kL bytes apart are
//         kL / 64 st64 units: 32 rows fit the 8-bit fields up to 512 lanes); otherwise both go
//         into the base register
//  kMirrorPtr  the mirror row (DecRingT) is written through a generic pointer to the ring that
//         the kernel sets (k_decode's form: from col the compiler forms the address with fewer
//         instructions and allocates registers differently); otherwise at its LDS address from col
enum RowForm {
    kRowLshlOr,  // the mask first, then one v_lshl_or (a left shift by a constant issues at the
                 // slow rate, profiles/r02_valu_microbench.txt, and v_and_or would need it); bits
    kRowLshlOr7, // the same instruction for 1,024 lanes with its shift written in the asm text
                 // where kRowLshlOr passes it as an operand: the compiler schedules around an asm
                 // statement by its operand list, so each kernel keeps the statement it was tuned with
    kRowShl16,   // v_lshlrev_b16 (shl16), the mask, v_or: the address fits 16 bits; bits
    kRowPlain    // plain C++ shift and mask; bytes
};
template <int kL, uint32_t kBase, int kUnit, RowForm kForm, bool kFold = false, bool kMirrorPtr = false>
struct RingLayout {
    static_assert(kL == 256 || kL == 512 || kL == 1024, "lanes per workgroup");
    static_assert(kUnit == (kForm == kRowPlain ? 1 : 8), "the asm forms take bit positions");
    static_assert(kForm != kRowLshlOr7 || kL == 1024, "the shift in the text is 1,024 lanes'");
    static constexpr int kLanes = kL;
    static constexpr uint32_t kRing = kBase;
    static constexpr uint32_t kRowShift = kL == 256 ? 10u : kL == 512 ? 11u : 12u;  // log2 of a row's bytes
    static constexpr uint32_t kRowMask = 31u << kRowShift;
    static constexpr int kPosUnit = kUnit;
    static constexpr bool kFoldLanding = kFold;
    static constexpr bool kMirrorGeneric = kMirrorPtr;
    static_assert(!kFold || (kBase % 256 == 0 && kBase / 256 + 31 * (kL / 64) <= 255), "32 rows in the st64 offsets");
    // the row address of stream position pos (dword pos / (4 kUnit)), without the ring base
    static __device__ __forceinline__ uint32_t row_of(uint32_t pos, uint32_t col) {
        if constexpr (kForm == kRowLshlOr) {
            uint32_t a;
            asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(a) : "v"(pos & 0x3E0u), "i"(kRowShift - 5), "v"(col));
            return a;
        } else if constexpr (kForm == kRowLshlOr7) {
            uint32_t a;
            asm("v_lshl_or_b32 %0, %1, 7, %2" : "=v"(a) : "v"(pos & 0x3E0u), "v"(col));
            return a;
        } else if constexpr (kForm == kRowShl16) {
            static_assert(kRowShift <= 11, "16-bit addresses");
            return (shl16<kRowShift - 5>(pos) & kRowMask) | col;
        } else {
            return ((pos << (kRowShift - 2)) & kRowMask) | col;
        }
    }
};

// ====================================================================== encode side
// the ring by dword index: a row address is one v_and_or of the row bits and the lane's column
template <class Lay>
struct RingT {
    uint32_t col;  // 4 * lane
    __device__ __forceinline__ lds_u32& at(int32_t i) const {
        const uint32_t a = ((static_cast<uint32_t>(i) << Lay::kRowShift) & Lay::kRowMask) | col;
        return *reinterpret_cast<lds_u32*>(static_cast<uintptr_t>(a + Lay::kRing));
    }
};

// Byte funnel.  pos8 = 8 * (stream bytes so far), neg8 = -pos8; the stream's dword w = pos/4
// lives in ring row w & 31, and X holds its contents with the b = pos & 3 written bytes at the
// bottom (garbage above).  A push of the head's low k bytes (lo, little-endian = stream order,
// src/ans.rs:246-253) forms both dwords it can touch, whatever k is:
//   dword w   = X's b bytes | lo << 8b           (v_bfe_u32 + v_lshl_or_b32)
//   dword w+1 = lo >> (32 - 8b)                  (v_lshrrev_b32; for b = 0 all of lo: unused bytes)
// and stores only dword w (one ds_write_b32).  Dword w+1, when the push reached it, becomes X:
// the next push (or finish) stores it with its own bytes, before any page holding it completes.
// Bytes past the new end are garbage that the next push overwrites.
// Nine VALU per push, any k up to four bytes: the funnel of k_encode's KMAX = 4 instantiations,
// of ans_wide.hpp and of ans_mfast.hpp.  The instantiations whose pushes stay at three bytes or
// fewer take the sliding window of ans_funnel.hpp, six VALU (ans_fast.hpp EncFunnel).
template <class Lay>
struct FunnelT {
    uint32_t X, pos8, neg8, addr, col;  // addr = ring address (less the ring base) of dword pos/4

    __device__ __forceinline__ static FunnelT start(uint32_t col) { return FunnelT{0, 0, 0, col, col}; }
    __device__ __forceinline__ uint32_t end8() const { return pos8; }
    // the low nb = 7 or 8 bytes of a head (the flatten, src/ans.rs:255-260)
    __device__ __forceinline__ void push_head(uint64_t head, uint32_t nb) {
        push(static_cast<uint32_t>(head), 32);
        push(static_cast<uint32_t>(head >> 32), 8 * (nb - 4));
    }
    __device__ __forceinline__ void push(uint32_t lo, uint32_t k8) {
        uint32_t xv, d0, d1;
        asm("v_bfe_u32 %0, %1, 0, %2" : "=v"(xv) : "v"(X), "v"(pos8));
        asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(d0) : "v"(lo), "v"(pos8), "v"(xv));
        asm("v_lshrrev_b32 %0, %1, %2" : "=v"(d1) : "v"(neg8), "v"(lo));
        *reinterpret_cast<lds_u32*>(static_cast<uintptr_t>(addr + Lay::kRing)) = d0;
        pos8 += k8;
        neg8 -= k8;
        const uint32_t a = Lay::row_of(pos8, col);
        X = a != addr ? d1 : d0;
        addr = a;
    }
    // the last byte back (renorm_up during a push, src/ans.rs:239-243); pos8 > 0.  Only k_menc's
    // bidirectional renorm calls this (ans_mfast.hpp)
    __device__ __forceinline__ uint32_t take_back() {
        pos8 -= 8;
        neg8 += 8;
        const uint32_t a = Lay::row_of(pos8, col);
        if (a != addr) {  // the byte lies in the dword below, which is in the ring
            X = *reinterpret_cast<const lds_u32*>(static_cast<uintptr_t>(a + Lay::kRing));
            addr = a;
        }
        return (X >> (pos8 & 31u)) & 0xFFu;
    }
    __device__ __forceinline__ uint32_t len() const { return pos8 >> 3; }
    // the partial last dword, zero-padded, into its ring row (nothing is pushed after this)
    __device__ __forceinline__ void finish() {
        uint32_t xv;
        asm("v_bfe_u32 %0, %1, 0, %2" : "=v"(xv) : "v"(X), "v"(pos8));
        *reinterpret_cast<lds_u32*>(static_cast<uintptr_t>(addr + Lay::kRing)) = xv;
    }
};

// Completed ring pages leave in aligned pairs, one whole 128-B line per lane: the even page
// waits in registers for its odd partner.  A lone 64-B store leaves its line half-written in L2
// until the next page, and the streaming traffic around it evicts such lines in pieces (1.2x
// the stream's bytes written, profiles/r02c_pmc_c3_summary.txt; the 128-B symbol stores of
// k_decode write exactly theirs, profiles/r02d_pmc_c3_summary.txt).
struct PageOut {
    uint4 h0, h1, h2, h3;  // page 2m, until 2m+1 completes
    template <class Ring>
    __device__ __forceinline__ void page(const Ring& ring, uint32_t p, uint8_t* dst) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = ring.at(static_cast<int32_t>(16 * p + i));
        const uint4 v0 = make_uint4(w[0], w[1], w[2], w[3]), v1 = make_uint4(w[4], w[5], w[6], w[7]);
        const uint4 v2 = make_uint4(w[8], w[9], w[10], w[11]), v3 = make_uint4(w[12], w[13], w[14], w[15]);
        if (p & 1) {
            uint4* d = reinterpret_cast<uint4*>(dst + 64ull * (p - 1));
            d[0] = h0;
            d[1] = h1;
            d[2] = h2;
            d[3] = h3;
            d[4] = v0;
            d[5] = v1;
            d[6] = v2;
            d[7] = v3;
        }
        // held unconditionally (an odd page's copy is dead): as an else branch the compiler
        // merged these writes with the stores above into stores through a selected pointer,
        // which put the held page in scratch
        h0 = v0;
        h1 = v1;
        h2 = v2;
        h3 = v3;
    }
    // after the last page: np pages completed in all (an odd count leaves the last one held)
    __device__ __forceinline__ void finish(uint32_t np, uint8_t* dst) {
        if (np & 1) {
            uint4* d = reinterpret_cast<uint4*>(dst + 64ull * (np - 1));
            d[0] = h0;
            d[1] = h1;
            d[2] = h2;
            d[3] = h3;
        }
    }
};

// ====================================================================== decode side
// One decode chain = one chunk, read from the end.  pos is the stream position P minus 4, in
// Lay::kPosUnit units: the window W = stream bytes [P, P+4) (byte P+3 on top) comes from ring
// dwords y = P>>2 and y+1 with one v_alignbit / v_alignbyte.  The ring is [row][lane] with 33
// rows: row 32 mirrors row 0, so y and y+1 are one ds_read2st64_b32 even across the wrap.  Pages
// (16 rows) land at points: page low+1 is free once dword y+1 lies in page low, and the page
// below `low` is always in flight in registers (Q); pages below 0 are zeros (the Zeros
// generator, src/ans.rs:160-170).  A point covers at most 60 stream bytes, so no read between
// points can reach an unlanded page.
constexpr int kDecRingRows = 33;
__device__ const uint4 kZeroPair[8] = {};  // 128 zero bytes: the Zeros tail generator's pages

template <class Lay>
struct DecRingT {
    static constexpr int kU = Lay::kPosUnit;
    // (the members' order is k_decode_w's: the compiler's register allocation follows it, and
    // with this order every kernel of the three chains keeps its instruction stream)
    uint32_t col;  // 4 * lane: the lane's byte column in the ring
    const uint8_t* src;
    uint4 Q[8];  // the aligned page pair (2m, 2m+1) not yet landed: one 128-B L2 line per fetch
    int32_t low, pos;
    uint32_t wx, wy, W;
    uint64_t head;
    int32_t lim;     // kU (64 low + 60), see point()
    uint32_t* ring;  // Lay::kMirrorGeneric only: &ring[0][lane] as a generic pointer, set by the kernel

    // pages are fetched as aligned 128-B pairs (2m, 2m+1): a 64-B read leaves the other half of
    // its 128-B line to be fetched again later (profiles/r02_hbm_calib.txt: 2x the bytes).
    // Pairs below 0 come from a zero pair in global memory: the same loads, where a register
    // zero-fill cost a point's worth of v_mov on every wave with one lane at its stream start
    // (global address space: a flat load would also count in lgkmcnt and stall the LDS waits)
    // Positions count from the stream's first byte (src), at any alignment: a pair below the
    // top one lies wholly inside the stream, so its 16-B loads (unaligned in a dense container;
    // the hardware runs in unaligned mode) touch only the stream's own bytes.
    __device__ __forceinline__ void fetch_pair(int32_t m) {
        typedef __attribute__((address_space(1), aligned(1))) const v4u32 gv4;
        const uint4* g = m >= 0 ? reinterpret_cast<const uint4*>(src + 128ll * m) : kZeroPair;
        const gv4* gg = reinterpret_cast<const gv4*>(reinterpret_cast<uintptr_t>(g));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const v4u32 v = gg[k];
            Q[k] = make_uint4(v.x, v.y, v.z, v.w);
        }
    }
    // the top pair m (once per stream) may reach past the stream's end, where a wide load could
    // cross into an unmapped page: it is read as the aligned dwords holding stream bytes (each
    // inside its 128-B line) and funnelled to the stream's byte alignment by v_alignbyte
    __device__ __forceinline__ void fetch_top(int32_t m, int32_t len) {
        typedef __attribute__((address_space(1))) const uint32_t gu32;
        const uintptr_t a = reinterpret_cast<uintptr_t>(src) + 128ll * m;
        const gu32* d0 = reinterpret_cast<const gu32*>(a & ~uintptr_t(3));
        const uint32_t b = static_cast<uint32_t>(a & 3u);
        const int32_t last = static_cast<int32_t>(((reinterpret_cast<uintptr_t>(src) + len - 1) >> 2) - (a >> 2));
        uint32_t d[33];
#pragma unroll
        for (int q = 0; q < 33; ++q) d[q] = q <= last ? d0[q] : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            Q[k] = make_uint4(ab(d[4 * k + 1], d[4 * k], b), ab(d[4 * k + 2], d[4 * k + 1], b),
                              ab(d[4 * k + 3], d[4 * k + 2], b), ab(d[4 * k + 4], d[4 * k + 3], b));
    }
    // page p (its half of Q) into ring slot p & 1, rows R0..R0+15
    // (positions count from the stream's start, so no landed page holds another stream's
    // bytes: pages below the start are the zero page; nothing to clear)
    // The sixteen rows go out as eight ds_write2st64_b32 from one base address: rows 4 kL bytes
    // apart are kL / 64 st64 units, so sixteen rows fit the 8-bit offset fields (Lay::kFoldLanding:
    // all 32, and the ring base, from col itself).  As C++ stores the compiler formed each row's
    // address with its own v_add (the rows lie beyond the 16-bit byte offsets) and stored them one
    // dword at a time.
    template <int R0>
    __device__ __forceinline__ uint32_t put_half(uint4 a0, uint4 a1, uint4 a2, uint4 a3) {
        constexpr int st = Lay::kLanes / 64;
        constexpr int o = Lay::kFoldLanding ? static_cast<int>(Lay::kRing / 256) + st * R0 : 0;
        const uint32_t base = Lay::kFoldLanding ? col : col + Lay::kRing + R0 * Lay::kLanes * 4;
        asm volatile(
            "ds_write2st64_b32 %0, %1, %2 offset0:%17 offset1:%18\n\t"
            "ds_write2st64_b32 %0, %3, %4 offset0:%19 offset1:%20\n\t"
            "ds_write2st64_b32 %0, %5, %6 offset0:%21 offset1:%22\n\t"
            "ds_write2st64_b32 %0, %7, %8 offset0:%23 offset1:%24\n\t"
            "ds_write2st64_b32 %0, %9, %10 offset0:%25 offset1:%26\n\t"
            "ds_write2st64_b32 %0, %11, %12 offset0:%27 offset1:%28\n\t"
            "ds_write2st64_b32 %0, %13, %14 offset0:%29 offset1:%30\n\t"
            "ds_write2st64_b32 %0, %15, %16 offset0:%31 offset1:%32"
            :
            : "v"(base), "v"(a0.x), "v"(a0.y), "v"(a0.z), "v"(a0.w), "v"(a1.x), "v"(a1.y), "v"(a1.z), "v"(a1.w),
              "v"(a2.x), "v"(a2.y), "v"(a2.z), "v"(a2.w), "v"(a3.x), "v"(a3.y), "v"(a3.z), "v"(a3.w),
              "i"(o), "i"(o + st), "i"(o + 2 * st), "i"(o + 3 * st), "i"(o + 4 * st), "i"(o + 5 * st), "i"(o + 6 * st),
              "i"(o + 7 * st), "i"(o + 8 * st), "i"(o + 9 * st), "i"(o + 10 * st), "i"(o + 11 * st), "i"(o + 12 * st),
              "i"(o + 13 * st), "i"(o + 14 * st), "i"(o + 15 * st)
            : "memory");
        return a0.x;
    }
    // the LDS address of the mirror row (row 32) of the lane's column
    __device__ __forceinline__ uint32_t mirror_addr() const { return col + Lay::kRing + 32u * Lay::kLanes * 4; }
    // two exec-masked store sets, one per parity: as one store set from selected registers the
    // compiler spent 16 v_cndmask per landing (the barrier keeps it from merging them again)
    __device__ __forceinline__ void put_page(int32_t p) {
        if (p & 1) {
            put_half<16>(Q[4], Q[5], Q[6], Q[7]);
        } else {
            const uint32_t r0 = put_half<0>(Q[0], Q[1], Q[2], Q[3]);
            // row 32 mirrors row 0
            if constexpr (Lay::kMirrorGeneric) ring[32 * Lay::kLanes] = r0;
            else *reinterpret_cast<lds_u32*>(static_cast<uintptr_t>(mirror_addr())) = r0;
        }
    }
    // ring row (P >> 2) & 31 of the lane's column (the ring base added by the caller / offsets)
    __device__ __forceinline__ uint32_t row_addr(int32_t p) const { return Lay::row_of(static_cast<uint32_t>(p), col); }
    // W = bytes [P, P+4): ring rows (P>>2)&31 and the next (row 32 mirrors row 0), the ring base
    // in the ds offsets
    __device__ __forceinline__ void read_window() {
        const uint32_t a = row_addr(pos);
        wy = lds_ld32(a + Lay::kRing);
        wx = lds_ld32(a + Lay::kRing + 4 * Lay::kLanes);
    }
    // (v_alignbit_b32 reads only the low five bits of its shift operand, v_alignbyte_b32 the low
    // two: pos needs no mask)
    __device__ __forceinline__ void form_window() {
        if constexpr (kU == 8) W = __builtin_amdgcn_alignbit(wx, wy, static_cast<uint32_t>(pos));
        else W = ab(wx, wy, static_cast<uint32_t>(pos));
    }
    // the byte just below the position (stream byte P + 3, the window's top), as the ring holds it
    __device__ __forceinline__ uint32_t top_byte() const {
        static_assert(kU == 8, "bit positions");
        const int32_t p8 = pos + 24;
        return (lds_ld32(row_addr(p8) + Lay::kRing) >> (static_cast<uint32_t>(p8) & 24u)) & 0xFFu;
    }
    // the stream bytes not yet consumed; < 0: bytes below the stream's start (generated) were read
    __device__ __forceinline__ int32_t bytes_left() const {
        if constexpr (kU == 8) return (pos >> 3) + 4;
        else return pos + 4;
    }
    // the top two pages land before decoding starts; the pair below them is requested.
    // s: the stream's first byte, at any alignment (a dense container).  Positions count from s
    // itself, so every lane's pages start at its own stream's start: streams of similar
    // length then cross page boundaries at nearly the same symbols, in a dense container as in
    // slots, and a wave runs the landing code about once per page rather than at every point
    // (with pages at absolute 64-B boundaries the packed streams' random phases put some lane's
    // landing at nearly every point: +2.2 VALU per symbol, profiles/r03_pmc_dense_vs_slot.txt).
    __device__ __forceinline__ void start(const uint8_t* s, int32_t len) {
        src = s;
        const int32_t top = len > 0 ? (len - 1) >> 6 : 0;
        if (len > 0) fetch_top(top >> 1, len);
        else fetch_pair(-1);
        wait_vm();
        put_page(top);
        if (top & 1) {
            put_page(top - 1);
            fetch_pair((top >> 1) - 1);  // holds top-3, top-2
        } else {
            fetch_pair((top >> 1) - 1);  // holds top-2, top-1
            wait_vm();
            put_page(top - 1);  // top-2 stays in the low half
        }
        low = top - 1;
        lim = kU * (64 * low + 60);
        pos = kU * (len - 4);
        read_window();
        head = 0;
    }
    // renorm_up one byte at a time (unflatten and the final equality check only)
    __device__ __forceinline__ void pull_until(uint64_t bound) {
        for (int g = 0; g < 9 && head < bound; ++g) {
            form_window();
            head = (head << 8) | (W >> 24);
            pos -= kU;
            read_window();
        }
    }
    // at a point (after s_waitcnt vmcnt(0)): page low+1 is no longer read once
    // ((P >> 2) + 1) >> 4 <= low, i.e. P < 64 low + 60 (floor division throughout, negative
    // positions included): one compare per point, in the position's unit
    __device__ __forceinline__ void point() {
        if (pos < lim) {  // land the page below
            put_page(low - 1);
            --low;
            lim -= 64 * kU;
            if (!(low & 1)) fetch_pair((low >> 1) - 1);  // the next page (low-1, odd) opens a new pair
        }
    }
};

}  // namespace fast
}  // namespace shuffle_coding
