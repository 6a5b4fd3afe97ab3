"""The fix-up-free decoder's additive bucket words and its symbol pick (shuffle-coding_amd/csrc/
ans_dec_u.hpp: fast::dec_u_word, fast::dec_u_pick) against a partition-point
search over the 512 virtual boundaries, on the CPU.

k_decode's kModeU lookup reads the two words of u's bucket and takes the virtual symbol as
(u + k1 + ((u + k2) & 2^us)) >> us.  This test compiles a checker with g++ against the product
header, builds the words of every bucket as build_fast_table does (ans_kernels.hip: us is the
finest width with at most kDecUNbMax buckets over [0, 2 norm), s0 the virtual symbol at the
bucket's start, a table whose bucket holds a fourth candidate is rejected), and compares the pick
with the search at every bucket's start and end - 1, at each inner boundary - 1, + 0 and + 1
where those fall inside the bucket, and at a few random points.  It also checks that neither
u + k1 nor the picked sum reaches 2^32 before the reduction mod 2^32, and that the two-shift form
of the pick agrees.

Tables: C3's masses (1 + splitmix64(0x5EED ^ s) mod 2^20); the same shape at other scales from
norms near 2^16 to just under 3,072 * 2^17 (us = 18, the widest the kernel takes) and at exactly
that norm; milder masses (a floor of a quarter of the range) at the same scales; tables with fewer
than 256 symbols (254 or 255, and shorter ones whose norm is a multiple of the bucket width: any
other leaves a bucket straddling u = norm across the zero-mass gap, which the builder rejects);
tables with isolated zero-mass and mass-1 symbols.  The checker fails if fewer than half of its
tables yield an image.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shuffle-coding_amd", "csrc")

CHECKER = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "ans_dec_u.hpp"
using shuffle_coding::fast::dec_u_pick;
using shuffle_coding::fast::dec_u_pick2;
using shuffle_coding::fast::dec_u_word;

// ans_fast.hpp: (kDecTableBytes - 8 * 512) / 8 buckets at most, bucket widths up to 2^18
static const uint32_t kDecUNbMax = (28672 - 8 * 512) / 8, kDecUShiftMax = 18;

static uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Table {
    std::vector<uint64_t> m;
    uint64_t norm() const { uint64_t n = 0; for (uint64_t x : m) n += x; return n; }
};

static uint32_t shift_of(uint64_t norm) {  // build_fast_table's us
    uint32_t us = 1;
    while (((2 * norm - 1) >> us) + 1 > kDecUNbMax) ++us;
    return us;
}

static long n_cases = 0, n_bad = 0, n_tables = 0, n_images = 0, n_us18 = 0, n_zero = 0, n_short = 0;

// the builder's loop over the buckets, then the pick at the test points of every bucket
static bool check(const Table& t, std::mt19937_64& R) {
    ++n_tables;
    const uint32_t nsym = (uint32_t)t.m.size();
    const uint64_t norm = t.norm(), n2 = 2 * norm;
    if (norm < (1ull << 16) || norm >= (1ull << 31)) return false;
    std::vector<uint64_t> cum(nsym + 1, 0);
    for (uint32_t s = 0; s < nsym; ++s) cum[s + 1] = cum[s] + t.m[s];
    auto cdfv = [&](uint32_t v) -> uint64_t {
        if (v >= 512) return n2;
        const uint64_t c = cum[std::min(v & 255u, nsym)];
        return v < 256 ? c : norm + c;
    };
    uint64_t bound[513];  // the 512 virtual boundaries and the end, non-decreasing
    for (uint32_t v = 0; v <= 512; ++v) bound[v] = cdfv(v);
    auto search = [&](uint64_t u) {  // the last v in [0, 512) with cdfv(v) <= u
        return (uint32_t)(std::upper_bound(bound, bound + 512, u) - bound) - 1;
    };
    const uint32_t us = shift_of(norm);
    if (us > kDecUShiftMax) return false;
    const uint32_t nbu = (uint32_t)(((n2 - 1) >> us) + 1);
    std::vector<uint32_t> k1(nbu), k2(nbu), s0s(nbu);
    for (uint32_t j = 0; j < nbu; ++j) {
        const uint64_t a = (uint64_t)j << us, end = std::min<uint64_t>(n2, a + (1ull << us));
        const uint32_t s0 = search(a);
        if (cdfv(s0 + 3) < end) return false;  // a fourth candidate: no image
        s0s[j] = s0;
        k1[j] = dec_u_word(a, cdfv(s0 + 1), s0, us);
        k2[j] = dec_u_word(a, cdfv(s0 + 2), 0, us);
    }
    ++n_images;
    if (us == 18) ++n_us18;
    if (nsym < 256) ++n_short;
    for (uint32_t s = 0; s < nsym; ++s)
        if (!t.m[s]) { ++n_zero; break; }
    for (uint32_t j = 0; j < nbu; ++j) {
        const uint64_t a = (uint64_t)j << us, end = std::min<uint64_t>(n2, a + (1ull << us));
        uint64_t pts[16];
        int np = 0;
        pts[np++] = a;
        pts[np++] = end - 1;
        for (int i = 1; i <= 2; ++i) {
            const uint64_t c = cdfv(s0s[j] + i);
            for (int d = -1; d <= 1; ++d)
                if (c + d >= a && c + d < end) pts[np++] = c + d;
        }
        for (int r = 0; r < 3; ++r) pts[np++] = a + R() % (end - a);
        for (int i = 0; i < np; ++i) {
            const uint32_t u = (uint32_t)pts[i];
            const uint32_t want = search(pts[i]), got = dec_u_pick(u, k1[j], k2[j], us);
            // before the reduction mod 2^32: (s0 << us) + (2^us + off - rel_1), then + [u >= c2] << us
            const uint64_t rel1 = std::min<uint64_t>(cdfv(s0s[j] + 1) - a, 1ull << us);
            const uint64_t d1 = ((uint64_t)s0s[j] << us) + ((1ull << us) + (pts[i] - a) - rel1);
            const uint64_t sum = d1 + ((uint64_t)((u + k2[j]) >> us) << us);
            ++n_cases;
            if (got != want || dec_u_pick2(u, k1[j], k2[j], us) != want || d1 >> 32 || sum >> 32 ||
                (uint32_t)d1 != u + k1[j] || (u + k2[j]) >> (us + 1)) {
                if (n_bad < 5)
                    printf("bad norm=%llu nsym=%u us=%u bucket=%u u=%u want=%u got=%u d1=%llx\n",
                           (unsigned long long)norm, nsym, us, j, u, want, got, (unsigned long long)d1);
                ++n_bad;
            }
        }
    }
    return true;
}

// the last mass takes up the difference to `target` (left alone where that would not be positive)
static void set_norm(Table& t, uint64_t target) {
    const uint64_t rest = t.norm() - t.m.back();
    if (target > rest) t.m.back() = target - rest;
}

int main(int argc, char** argv) {
    std::mt19937_64 R(0xDECu);
    const int rounds = argc > 1 ? atoi(argv[1]) : 40;
    const uint64_t top = 3072ull << 17;  // the largest norm with us = 18
    {   // C3 itself: it must yield an image (the benchmark decodes through it)
        Table t;
        for (uint64_t s = 0; s < 256; ++s) t.m.push_back(1 + (splitmix64(0x5EEDull ^ s) & ((1u << 20) - 1)));
        if (t.norm() != 139224331ull || !check(t, R)) { printf("C3 has no image\n"); return 1; }
    }
    for (int it = 0; it < rounds; ++it) {
        for (int kind = 0; kind < 6; ++kind) {
            // scales: 256 masses below 2^b sum to about 2^(b+7), so b = 9 .. 21 spans 2^16 .. 2^28
            const uint32_t b = 9 + (uint32_t)(R() % 13);
            const uint64_t seed = R();
            const uint32_t nsym = kind == 3 ? 254 + (uint32_t)(R() % 2) : kind == 4 ? 2 + (uint32_t)(R() % 252) : 256;
            Table t;
            for (uint64_t s = 0; s < nsym; ++s) {
                const uint64_t r = splitmix64(seed ^ s);
                // kind 0: C3's shape; others: a floor of a quarter of the range under the same draw
                t.m.push_back(kind == 0 ? 1 + (r & ((1ull << b) - 1)) : (1ull << (b - 2)) + (r & ((1ull << b) - 1)));
            }
            if (t.norm() < (1ull << 16)) set_norm(t, (1ull << 16) + 1 + R() % 64);
            if (kind == 1) {  // the ends of the range: 2^16 + 1, just under the top, the top itself
                const int e = it % 4;
                if (e == 0) { for (auto& x : t.m) x = 200 + (x & 63); set_norm(t, (1ull << 16) + 1); }
                if (e == 1) { for (auto& x : t.m) x = (1ull << 20) + (x & ((1ull << 19) - 1)); set_norm(t, top - 1 - R() % 1000); }
                if (e == 2) { for (auto& x : t.m) x = (1ull << 20) + (x & ((1ull << 19) - 1)); set_norm(t, top); }
            }
            if (kind == 2 || kind == 5) {  // isolated zero-mass and mass-1 symbols
                for (int z = 0; z < 4; ++z) {
                    const uint32_t s = 2 + (uint32_t)(R() % (nsym - 4));
                    if (t.m[s - 1] > 1 && t.m[s + 1] > 1 && t.m[s - 2] > 1 && t.m[s + 2] > 1) t.m[s] = z % 2;
                }
                if (kind == 5) t.m[0] = 0;  // a zero-mass first symbol: cdfv(0) = cdfv(1) = 0
            }
            if (kind == 4) {  // a short table: the norm a multiple of the bucket width
                for (int pass = 0; pass < 3; ++pass) {
                    const uint64_t w = 1ull << shift_of(t.norm());
                    set_norm(t, (t.norm() + w - 1) / w * w);
                }
            }
            check(t, R);
        }
    }
    printf("tables %ld images %ld us18 %ld zero-mass %ld short %ld\n", n_tables, n_images, n_us18, n_zero, n_short);
    printf("checked %ld bad %ld\n", n_cases, n_bad);
    if (2 * n_images < n_tables) { printf("fewer than half of the tables yield an image\n"); return 1; }
    return n_bad != 0;
}
"""


def test_dec_u_pick_matches_partition_point_search(tmp_path):
    src = tmp_path / "dec_u_check.cpp"
    exe = tmp_path / "dec_u_check"
    src.write_text(CHECKER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), "40"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1].startswith("checked") and lines[-1].endswith("bad 0"), out.stdout
    assert int(lines[-1].split()[1]) > 1_000_000, out.stdout
    counts = dict(zip(lines[-2].split()[0::2], map(int, lines[-2].split()[1::2])))
    assert 2 * counts["images"] >= counts["tables"], out.stdout
    # every kind of table reached the pick, not only the rejection
    assert counts["us18"] >= 5 and counts["zero-mass"] >= 20 and counts["short"] >= 20, out.stdout
