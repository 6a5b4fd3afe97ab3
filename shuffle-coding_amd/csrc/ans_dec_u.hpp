// ans_dec_u.hpp — the fix-up-free decoder's bucket words and its symbol pick (ans_fast.hpp
// k_decode kMode = kModeU; built in ans_kernels.hip build_fast_table).  Plain C++ (a constexpr
// function is host and device code alike under hipcc), so the CPU test suite checks the rule
// against a search over the virtual alphabet with g++ (tests/test_dec_u_words.py).
#pragma once
#include <cstdint>

namespace shuffle_coding {
namespace fast {

// The word of boundary c in the bucket at a = j << us (width 2^us), to be ADDED to u: with
// rel = min(c - a, 2^us) (>= 1: c > a) and off = u - a in [0, 2^us),
//   u + dec_u_word(a, c, e, us) = (e << us) + (2^us + off - rel)   (mod 2^32)
// whose second term lies in [0, 2^(us+1)) and has bit us set exactly when off >= rel, that is
// when u >= c (never for a boundary at or past the bucket's end, where rel = 2^us).  So
// (u + word) >> us = e + [u >= c].  A bucket holds k1 = word(a, cdfv(s0 + 1), s0) and
// k2 = word(a, cdfv(s0 + 2), 0) for s0 = the virtual symbol at a.  No overflow while
// (e + 2) << us <= 2^32: e <= 511 and us <= 18 (kDecUShiftMax) give at most 513 * 2^18.
constexpr uint32_t dec_u_word(uint64_t a, uint64_t c, uint32_t e, uint32_t us) {
    const uint64_t w = 1ull << us, rel = c - a < w ? c - a : w;
    return static_cast<uint32_t>(((static_cast<uint64_t>(e) + 1) << us) - a - rel);
}

// The virtual symbol of u from its bucket's words: s0 + [u >= c1] + [u >= c2].  u + k2 is below
// 2^(us+1), so its bit us alone is [u >= c2] << us and adds into u + k1 above that sum's own
// offset bits before ONE shift: v_add, v_and (the mask 1 << us in an SGPR), v_add3, v_lshrrev,
// and the result is the clean 9-bit v (no bits above it: its low byte is the symbol, v << 3 the
// row address).  The sum stays below (s0 + 3) << us <= 514 * 2^18.
constexpr uint32_t dec_u_pick(uint32_t u, uint32_t k1, uint32_t k2, uint32_t us) {
    return (u + k1 + ((u + k2) & (1u << us))) >> us;
}

// The same pick as two shifts ((u + k1) >> us) + ((u + k2) >> us): the form a kernel takes when
// it folds the sum into a shift-add of the row address (v_add_lshl).
constexpr uint32_t dec_u_pick2(uint32_t u, uint32_t k1, uint32_t k2, uint32_t us) {
    return ((u + k1) >> us) + ((u + k2) >> us);
}

}  // namespace fast
}  // namespace shuffle_coding
