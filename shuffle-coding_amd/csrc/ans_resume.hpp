// ans_resume.hpp — the arithmetic of resuming a flattened message on the fast encoder
// (ans_mfast.hpp k_menc<kRes>): where the coder's state starts when chunk c's message is
// Message::unflatten(bytes) (src/ans.rs:262-264: head 0, the bytes as the tail).  Plain C++ (a
// constexpr function is host and device code alike under hipcc), so the CPU test suite checks it
// against the oracle's unflatten + push with g++ (tests/test_resume_host.py).
#pragma once
#include <cstdint>

namespace shuffle_coding {
namespace resume {

constexpr uint64_t kFull = 1ull << 56;  // MAX_MIN_HEAD (src/ans.rs:19): every bound p K is at most this

// The prologue: head = head << 8 | bytes[--pos] (renorm_up, src/ans.rs:239-243) until head >= 2^56
// or the stream's start.  The reference's first push renorms to its own bound pK <= 2^56 instead:
// up while head < pK, then down while head >> 8 >= pK.  Pulling to 2^56 first changes nothing: the
// heads along the message's byte prefixes grow monotonically, exactly one of them lies in
// [pK, 2^8 pK), and the push's renorm_down walks back to it, re-emitting the bytes pulled beyond it
// unchanged.  A head still below 2^56 at pos = 0 (a message of fewer than eight significant
// bytes) may or may not reach pK: only the exact coder decides that (exhaustion, src/ans.rs:144).
constexpr uint64_t pull_to_full(const uint8_t* bytes, uint32_t& pos) {
    uint64_t head = 0;
    while (head < kFull && pos > 0) head = (head << 8) | bytes[--pos];
    return head;
}

// The first 64-B page the resumed encoder still owns.  It flushes page fp once the position is a
// byte past it (pos >= 64 fp + 65), because a push may take back the one byte below the position;
// so at position pos the pages below (pos - 1) / 64 count as flushed and stay as they are in the
// slot, and page (pos - 1) / 64 (the one holding byte pos - 1) is loaded into the ring.
constexpr uint32_t first_open_page(uint32_t pos) { return pos ? (pos - 1) >> 6 : 0u; }

}  // namespace resume
}  // namespace shuffle_coding
