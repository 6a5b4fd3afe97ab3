"""The bulk encoder's sliding-window byte funnel (shuffle-coding_amd/csrc/ans_funnel.hpp
WindowFunnelT) against a byte-append model, on the CPU.

The funnel keeps the stream's last four bytes in one register and stores, per push of k <= 3
bytes, the one ring dword that holds the stream's last byte.  This test compiles the product
header with g++ (alignbit and the row address take their host definitions, the ring store is an
array) and drives it beside a plain byte vector:

  * after EVERY push, each dword wholly below the stream's end that the 32-row ring still holds
    (the last 31 of them: the remaining row is the one the funnel stores next) equals the
    model's, so a page is complete in the ring as soon as the end reaches its boundary, exactly
    or beyond; each push makes exactly one store;
  * after finish(), the partial last dword is in its row zero-padded, and the whole ring image
    equals the model's last 32 dwords (row 31 of an image that never reached dword 31 holds the
    start's zero);
  * exhaustively: every sequence of six pushes with k in {0, 1, 2, 3} from each of the four
    start residues (a prefix of 0..3 single-byte pushes, then the start at 60..63 bytes too, so
    that page boundaries are reached exactly and crossed by every k);
  * random sequences of 400 to 1,000 bytes (three to eight ring laps), pushed words random in all
    32 bits (the bytes above k are garbage the funnel must not keep);
  * the head's flatten (push_head, 7 and 8 bytes) at every residue, and the empty stream.

The ring is checked as the kernel reads it: row (dword index & 31), column 0 of a one-lane image
with the kernel's row pitch of 2^11 bytes.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shuffle-coding_amd", "csrc")

CHECKER = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "ans_funnel.hpp"

static uint32_t g_ring[32];
static long g_stores = 0;
struct Store {
    static void st(uint32_t addr, uint32_t v) {
        // addr = row << 11 | col, col = 4 * lane; this image has the one lane 5
        if ((addr & 0x7FFu) != 20u || (addr >> 11) > 31u) { printf("bad address %x\n", addr); g_ring[0] = ~0u; return; }
        g_ring[addr >> 11] = v;
        ++g_stores;
    }
};
using F = shuffle_coding::fast::WindowFunnelT<Store>;

static long bad = 0, checks = 0;
static std::vector<uint8_t> model;

static uint32_t model_dword(size_t w) {  // zero-padded past the end
    uint32_t v = 0;
    for (int i = 0; i < 4; ++i)
        if (4 * w + i < model.size()) v |= (uint32_t)model[4 * w + i] << (8 * i);
    return v;
}
static void fail(const char* what, size_t w) {
    if (bad < 10) printf("%s: dword %zu of a stream of %zu bytes\n", what, w, model.size());
    ++bad;
}
// every dword wholly below the end that the ring must still hold
static void check_complete(const F& f) {
    if (f.len() != model.size() || f.end8() != 8 * model.size()) fail("length", 0);
    const size_t full = model.size() / 4;  // dwords wholly below the end
    const size_t first = full > 31 ? full - 31 : 0;
    for (size_t w = first; w < full; ++w) {
        ++checks;
        if (g_ring[w & 31] != model_dword(w)) fail("complete dword", w);
    }
}
static void check_finished() {
    const size_t nd = (model.size() + 3) / 4;  // dwords the stream touches
    const size_t first = nd > 32 ? nd - 32 : 0;
    for (size_t w = first; w < nd; ++w) {
        ++checks;
        if (g_ring[w & 31] != model_dword(w)) fail("finished dword", w);
    }
}
static void push(F& f, uint32_t word, uint32_t k) {
    const long s0 = g_stores;
    f.push(word, 8 * k);
    if (g_stores != s0 + 1) fail("one store per push", 0);
    for (uint32_t i = 0; i < k; ++i) model.push_back((uint8_t)(word >> (8 * i)));
    check_complete(f);
}
static F fresh() {
    model.clear();
    for (int i = 0; i < 32; ++i) g_ring[i] = 0xDEADBEEFu;  // stale rows
    return F::start(20);
}

int main() {
    std::mt19937_64 R(2024);
    // exhaustive: six pushes of k in 0..3 after `pre` single bytes
    const int pres[] = {0, 1, 2, 3, 58, 59, 60, 61, 62, 63, 64, 65, 124, 125, 126, 127, 128};
    for (int pre : pres)
        for (int seq = 0; seq < 4096; ++seq) {
            F f = fresh();
            for (int i = 0; i < pre; ++i) push(f, (uint32_t)R(), 1);
            for (int i = 0; i < 6; ++i) push(f, (uint32_t)R(), (seq >> (2 * i)) & 3);
            f.finish();
            check_finished();
        }
    // random streams of 400..1000 bytes
    for (int it = 0; it < 3000; ++it) {
        F f = fresh();
        const size_t want = 400 + R() % 601;
        while (model.size() < want) push(f, (uint32_t)R(), (uint32_t)(R() % 4));
        f.finish();
        check_finished();
    }
    // the flatten at every residue, 7 and 8 bytes; then nothing but the flatten
    for (int pre = 0; pre < 140; ++pre)
        for (uint32_t nb = 7; nb <= 8; ++nb) {
            F f = fresh();
            for (int i = 0; i < pre; ++i) push(f, (uint32_t)R(), 1 + (uint32_t)(R() % 3));
            const uint64_t head = nb == 8 ? (R() | (1ull << 63)) : ((R() >> 8) | (1ull << 55));
            const long s0 = g_stores;
            f.push_head(head, nb);
            if (g_stores != s0 + 3) fail("three stores per flatten", 0);
            for (uint32_t i = 0; i < nb; ++i) model.push_back((uint8_t)(head >> (8 * i)));
            check_complete(f);
            f.finish();
            check_finished();
        }
    // the empty stream: length 0, and finish leaves rows 0..30 alone
    {
        F f = fresh();
        if (f.len() != 0 || f.end8() != 0) fail("empty length", 0);
        f.push(0x12345678u, 0);
        check_complete(f);
        f.finish();
        for (int i = 0; i < 31; ++i) {
            ++checks;
            if (g_ring[i] != 0xDEADBEEFu) fail("empty stream wrote a row", i);
        }
        if (f.len() != 0) fail("empty length", 0);
    }
    printf("checked %ld bad %ld\n", checks, bad);
    return bad != 0;
}
"""


def test_window_funnel_matches_byte_append_model(tmp_path):
    src = tmp_path / "funnel_check.cpp"
    exe = tmp_path / "funnel_check"
    src.write_text(CHECKER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    line = out.stdout.strip().splitlines()[-1]
    assert line.startswith("checked") and line.endswith("bad 0"), out.stdout
    assert int(line.split()[1]) > 10_000_000
