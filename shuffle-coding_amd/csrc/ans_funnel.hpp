// ans_funnel.hpp — the sliding-window byte funnel of the bulk encoder (ans_fast.hpp k_encode,
// pushes of at most three bytes).  The same text is device code under hipcc and plain C++ under
// g++, so the CPU test suite drives it against a byte-append model (tests/test_window_funnel.py):
// alignbit and the ring's row address are the gfx950 instructions on the device and their
// definitions on the host, and the ring store is the Store policy (an LDS write in the kernels,
// an array in the test).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ANS_FUNNEL_FN __device__ __forceinline__
#else
#define ANS_FUNNEL_FN inline
#endif

namespace shuffle_coding {
namespace fast {

// v_alignbit_b32: the low dword of {hi:lo} >> (s & 31)
ANS_FUNNEL_FN uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIPCC__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (s & 31u));
#endif
}

// the row bits of a ring address, (x << 6) & 0xF800 for x = 8 * (a stream position): dword
// x >> 5 lives in ring row (x >> 5) & 31, and a row is 2^11 bytes of the [dword][lane] image.
// On the device the shift is v_lshlrev_b16 (the five row bits come from x's bits 5..9; ans_ring.hpp
// shl16 has its cost)
ANS_FUNNEL_FN uint32_t funnel_row(uint32_t x) {
#if defined(__HIPCC__)
    uint32_t r;
    asm("v_lshlrev_b16 %0, 6, %1" : "=v"(r) : "v"(x));
    return r & 0xF800u;
#else
    return (x << 6) & 0xF800u;
#endif
}

// Sliding-window byte funnel.  Z holds the stream's LAST FOUR bytes, [end - 4, end) in
// little-endian order, wherever end falls; the "current" dword is the one holding byte end - 1
// and b = ((end - 1) & 3) + 1 in 1..4 of its bytes are written.  m8 = 8 end - 8 (addr is the
// ring address of dword m8 >> 5, the current one), neg8 = -8 end, so neg8 & 31 = 8 (4 - b).
// A push of the low k <= 3 bytes of lo (k8 = 8 k; little-endian = stream order,
// src/ans.rs:246-253):
//   d0 = {lo:Z} >> 8 (4 - b)   the current dword: its b bytes from the top of Z, then the new ones
//   ring[addr] = d0            one aligned store
//   Z  = {lo:Z} >> 8 k         the window slides by k bytes
// Every count is 0, 8, 16 or 24, exact in v_alignbit's five bits: b = 4 gives d0 = Z (the
// complete dword rewritten with itself) and k = 0 leaves Z alone.  A count of 32 would wrap:
// pushes of four bytes (KMAX = 4 tables) keep FunnelT (ans_ring.hpp).
//
// Why the ring holds the stream: b >= 1 and k <= 3, so a push crosses at most one dword
// boundary, and the dword it completes is the old current one, which d0 stores complete and
// final.  Bytes that spilled into the next dword live only in Z until the next push, which
// stores them as part of its current dword; finish() does so at the end.  So after every push
// each dword wholly below end is in the ring (a page that end has reached, exactly or beyond, is
// complete: its last dword went out with a d0 store), and the bytes above the new end inside a
// stored dword are garbage that the next store to that dword overwrites.
//
// Stream start: end = 0 makes dword -1 the "current" one, ring row 31, with b = 4: the first
// push rewrites row 31 with the initial Z and otherwise runs the one code path.  Row 31 belongs
// to page 1, which leaves the ring only after the stream itself has stored row 31 (stream dword
// 31), so the early store is never read.  (Starting addr at row 0 with a partial first store
// would need b = 0, the one count, 32, that v_alignbit cannot do.)
template <typename Store>
struct WindowFunnelT {
    uint32_t Z, m8, neg8, addr, col;  // col: the lane's column, 4 * lane

    ANS_FUNNEL_FN static WindowFunnelT start(uint32_t col) {
        return WindowFunnelT{0u, 0u - 8u, 0u, funnel_row(0u - 8u) | col, col};
    }
    ANS_FUNNEL_FN void push(uint32_t lo, uint32_t k8) {
        Store::st(addr, alignbit(lo, Z, neg8));
        Z = alignbit(lo, Z, k8);
        m8 += k8;
        neg8 -= k8;
        addr = funnel_row(m8) | col;
    }
    // 8 * (stream bytes so far): the page test of the kernels' points reads bits 9 and up
    ANS_FUNNEL_FN uint32_t end8() const { return m8 + 8u; }
    ANS_FUNNEL_FN uint32_t len() const { return (m8 + 8u) >> 3; }
    // the low nb = 7 or 8 bytes of a head (the flatten, src/ans.rs:255-260) in pushes of <= 3
    ANS_FUNNEL_FN void push_head(uint64_t head, uint32_t nb) {
        push(static_cast<uint32_t>(head), 24);
        push(static_cast<uint32_t>(head >> 24), 24);
        push(static_cast<uint32_t>(head >> 48), 8 * (nb - 6));
    }
    // the current dword, zero-padded, into its ring row (nothing is pushed after this); for an
    // empty stream that is row 31 again
    ANS_FUNNEL_FN void finish() { Store::st(addr, alignbit(0u, Z, neg8)); }
};

}  // namespace fast
}  // namespace shuffle_coding
