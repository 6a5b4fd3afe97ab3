"""Recursive multiset shuffle coding on the host (include/ans_capi.h section 3: ans_orbit_id,
ans_mset_push, ans_mset_pop; ans_amd.MultisetShuffle) against the expected-bytes mirror of
tests/mset_mirror.py, and the count structure of csrc/ans_mset.hpp (compiled with g++) against a
brute-force cumulative sum."""
import math
import os
import subprocess

import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

import mset_mirror as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shuffle-coding_amd", "csrc")

# a second restatement's values (a cross-check between restatements, not reference output)
KNOWN_IDS = {0: 0xbd60acb658c79e45, 1: 0x1e9f734161d62dd9, 1023: 0x6cb8c108e104a440}


def test_orbit_id_is_siphash13_of_the_usize():
    for x in (0, 1, 1023, 1 << 32, (1 << 64) - 1):
        assert A.orbit_id(x) == MM.siphash13_usize(x), hex(x)
    for x, want in KNOWN_IDS.items():
        assert A.orbit_id(x) == want and MM.siphash13_usize(x) == want, x


def _uniform(values):
    """The reference's own vectors code with IID<Uniform(max + 1)>: a Categorical of equal masses."""
    return np.ones(max(values) + 1, np.uint64)


def _cases(multiset_masses, multiset_vectors):
    yield "[1,1]", _uniform([1, 1]), [1, 1]
    v = [1, 0, 4, 2, 2, 1, 1]  # src/multiset.rs:114
    yield "[1,0,4,2,2,1,1]", _uniform(v), v
    yield "multiset_1000", multiset_masses, [int(x) for x in multiset_vectors[1000]]
    yield "n=0", multiset_masses, []
    yield "n=1", multiset_masses, [int(multiset_vectors[1000][0])]


def _seed():
    return MM.seeds(np.random.default_rng(11), 1)[0]


def _initials(seed):
    """(name, the library's initial message, the oracle's)."""
    yield "unflatten(seed, EMPTY)", A.Message.unflatten(seed, A.GEN_EMPTY), orc.Message.unflatten(seed, orc.EMPTY)
    yield "zeros", A.Message.zeros(), orc.Message.zeros()


def test_push_pop_bytes_equal_the_mirror(multiset_masses, multiset_vectors):
    seed = _seed()
    for name, masses, values in _cases(multiset_masses, multiset_vectors):
        mirror = MM.Mirror(masses)
        codec = A.MultisetShuffle(A.Categorical(masses), len(values))
        for iname, m, om in _initials(seed):
            where = f"{name} from {iname}"
            m0, om0 = m.clone(), om.clone()
            assert mirror.push(om, values), f"{where}: the mirror reports exhaustion"
            codec.push(m, values)
            assert m.flatten() == om.flatten(), f"{where}: push"
            want = mirror.pop(om, len(values))
            assert want is not None, f"{where}: the mirror reports exhaustion"
            got = codec.pop(m)
            assert list(got) == want, f"{where}: pop order"
            assert m.flatten() == om.flatten(), f"{where}: what remains"
            assert m == m0 and om == om0, f"{where}: back at the initial message"


def test_order_of_the_input_does_not_matter(multiset_masses, multiset_vectors):
    values = np.array(multiset_vectors[1000])
    codec = A.MultisetShuffle(A.Categorical(multiset_masses), len(values))
    m = A.Message.unflatten(_seed(), A.GEN_EMPTY)
    codec.push(m, values)
    want = m.flatten()
    rng = np.random.default_rng(5)
    for perm in (values[::-1], np.sort(values), rng.permutation(values)):
        m = A.Message.unflatten(_seed(), A.GEN_EMPTY)
        codec.push(m, perm)
        assert m.flatten() == want


def test_invertibility_and_bits(multiset_masses, multiset_vectors):
    """Codec.test_invertibility (src/ans.rs:47-59): the pop returns the same multiset and the message
    is back at the initial one; the amortized bits are bits(x) = IID.bits - log2(n!/prod mult!)."""
    for name, masses, values in _cases(multiset_masses, multiset_vectors):
        codec = A.MultisetShuffle(A.Categorical(masses), len(values))
        for initial in (A.Message.random(3), A.Message.zeros(), A.Message.unflatten(_seed(), A.GEN_EMPTY)):
            codec.test(values, initial)  # test_invertibility, then assert_bits_eq(bits(x), amortized bits)
        decoded = codec.pop(_pushed(codec, values))
        assert decoded == values and sorted(decoded) == sorted(values)
        if len(set(values)) > 1:
            assert decoded != [values[0]] * len(values)


def _pushed(codec, values):
    m = A.Message.random(9)
    codec.push(m, values)
    return m


def test_saving_is_the_orders_bits(multiset_masses, multiset_vectors):
    """len(ordered IID push) - len(multiset push) is within 2 bytes of log2(n!/prod mult!)/8: each
    length is floor(virtual bits / 8) + 1, so the floors cost at most a byte each way."""
    cat = A.Categorical(multiset_masses)
    for n in (1000, 10000):
        values = multiset_vectors[10000][:n]
        _, mult = np.unique(values, return_counts=True)
        order_bytes = (math.lgamma(n + 1) - sum(math.lgamma(int(c) + 1) for c in mult)) / math.log(2) / 8
        seed = _seed()
        a, b = A.Message.unflatten(seed, A.GEN_EMPTY), A.Message.unflatten(seed, A.GEN_EMPTY)
        A.IID(cat, n).push(a, values)
        A.MultisetShuffle(cat, n).push(b, values)
        saved = len(a.flatten()) - len(b.flatten())
        print(f"n={n}: ordered {len(a.flatten())} B, multiset {len(b.flatten())} B, saved {saved} B, "
              f"log2(n!/prod mult!)/8 = {order_bytes:.2f} B")
        assert abs(saved - order_bytes) <= 2.0


def test_exhaustion_and_argument_errors():
    rng = np.random.default_rng(2)
    masses = rng.integers(1, 1 << 16, 256).astype(np.uint64)
    values = rng.integers(0, 256, 256)
    assert MM.Mirror(masses).push_bytes(b"\x07", values) is None  # as the mirror reports
    codec = A.MultisetShuffle(A.Categorical(masses), 256)
    with pytest.raises(A.AnsError) as e:
        codec.push(A.Message.unflatten(b"\x07", A.GEN_EMPTY), values)
    assert e.value.code == A.ANS_E_EXHAUSTED
    with pytest.raises(A.AnsError) as e:
        A.MultisetShuffle(A.Categorical(masses), 300).pop(A.Message.unflatten(b"\x07" * 8, A.GEN_EMPTY))
    assert e.value.code == A.ANS_E_EXHAUSTED
    with pytest.raises(A.AnsError) as e:
        A.MultisetShuffle(A.Categorical(masses), 2).push(A.Message.zeros(), [3, 256])
    assert e.value.code == A.ANS_E_SYMBOL
    with pytest.raises(A.AnsError) as e:
        A.MultisetShuffle(A.Categorical([5, 0, 7]), 2).push(A.Message.zeros(), [0, 1])
    assert e.value.code == A.ANS_E_ZERO_MASS
    with pytest.raises(A.AnsError) as e:
        A.MultisetShuffle(A.Categorical(np.ones(65537, np.uint64)), 1).push(A.Message.zeros(), [0])
    assert e.value.code == A.ANS_E_ARG
    A.MultisetShuffle(A.Categorical(np.ones(65536, np.uint64)), 2).test_invertibility([65535, 0], A.Message.zeros())


# ---- the count structure of csrc/ans_mset.hpp with g++ (no HIP) against a brute-force sum
CHECKER = r"""
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "ans_mset.hpp"
using namespace shuffle_coding::mset;
struct Vec {
    uint32_t* p;
    uint32_t load(uint32_t i) const { return p[i]; }
    void store(uint32_t i, uint32_t v) { p[i] = v; }
};
struct Vec16 {  // 16-bit nodes, as the kernels' LDS counts
    uint16_t* p;
    uint32_t load(uint32_t i) const { return p[i]; }
    void store(uint32_t i, uint32_t v) { p[i] = (uint16_t)v; }
};
template <class Acc, class Node>
long run(uint32_t nsym, uint32_t cap, std::mt19937_64& R, long& ops) {
    long bad = 0;
    std::vector<Node> nodes(nsym, 0);
    std::vector<uint32_t> raw(nsym, 0);
    Counts<Acc> c{Acc{nodes.data()}, nsym};
    // build from a histogram
    c.clear();
    uint64_t total = 0;
    const uint32_t n0 = (uint32_t)(R() % (cap / 2 + 1));
    for (uint32_t k = 0; k < n0; ++k) {
        const uint32_t r = (R() % 4 == 0) ? (uint32_t)(R() % nsym) : (uint32_t)((R() % nsym) * (R() % nsym) / nsym);
        c.tally(r);
        ++raw[r];
        ++total;
    }
    c.build();
    auto brute_prefix = [&](uint32_t r) { uint64_t s = 0; for (uint32_t i = 0; i < r; ++i) s += raw[i]; return s; };
    for (int it = 0; it < 4000; ++it, ++ops) {
        const int op = (int)(R() % 4);
        const uint32_t r = (uint32_t)(R() % nsym);
        if (op == 0 && total < cap) { c.add(r, 1); ++raw[r]; ++total; }
        else if (op == 1 && raw[r]) { c.add(r, -1); --raw[r]; --total; }
        else if (op == 2) {
            if (c.prefix(r) != brute_prefix(r) || c.count(r) != raw[r]) { ++bad; if (bad < 5) printf("prefix/count nsym %u rank %u\n", nsym, r); }
        } else if (total) {
            const uint64_t cf = R() % total;
            uint32_t want = 0; uint64_t cum = 0;
            while (cum + raw[want] <= cf) cum += raw[want++];
            const Found f = c.find(cf);
            if (f.rank != want || f.cum != cum || f.count != raw[want]) { ++bad; if (bad < 5) printf("find nsym %u cf %llu: rank %u want %u\n", nsym, (unsigned long long)cf, f.rank, want); }
        }
    }
    // the ends of the cumulative range
    if (total) {
        const Found lo = c.find(0), hi = c.find(total - 1);
        uint32_t first = 0, last = nsym - 1;
        while (!raw[first]) ++first;
        while (!raw[last]) --last;
        if (lo.rank != first || lo.cum != 0 || hi.rank != last || hi.cum + hi.count != total) { ++bad; printf("ends nsym %u\n", nsym); }
    }
    return bad;
}
int main() {
    std::mt19937_64 R(7);
    long bad = 0, ops = 0;
    const uint32_t sizes[] = {1, 2, 3, 255, 256, 257, 1024};
    for (uint32_t nsym : sizes)
        for (int rep = 0; rep < 6; ++rep) {
            bad += run<Vec, uint32_t>(nsym, rep % 2 ? 70000u : 300u, R, ops);
            bad += run<Vec16, uint16_t>(nsym, rep % 2 ? 65535u : 300u, R, ops);
        }
    // orbit ids and rank tables
    if (orbit_id(0) != 0xbd60acb658c79e45ull || orbit_id(1023) != 0x6cb8c108e104a440ull) { ++bad; printf("orbit_id\n"); }
    std::vector<uint32_t> rank, sym;
    if (!build_ranks(1024, rank, sym)) { ++bad; printf("build_ranks\n"); }
    for (uint32_t r = 0; r + 1 < 1024; ++r)
        if (orbit_id(sym[r]) >= orbit_id(sym[r + 1]) || rank[sym[r]] != r) ++bad;
    printf("ops %ld bad %ld\n", ops, bad);
    return bad != 0;
}
"""


def test_count_structure_matches_brute_force(tmp_path):
    """ans_mset.hpp's Counts (build from a histogram, find, prefix, count, add) with 32- and 16-bit
    nodes over nsym in {1, 2, 3, 255, 256, 257, 1024}, random operations, against a plain array."""
    src, exe = tmp_path / "mset_counts.cpp", tmp_path / "mset_counts"
    src.write_text(CHECKER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    line = out.stdout.strip().splitlines()[-1].split()
    assert line[0] == "ops" and int(line[1]) == 7 * 6 * 2 * 4000 and line[-1] == "0", out.stdout
