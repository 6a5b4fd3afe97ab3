"""The Pólya urn edge-index codec on the host (include/ans_capi.h section 3: ans_polya_push,
ans_polya_pop; ans_amd.PolyaUrn) against the expected-bytes mirror of
tests/polya_mirror.py, and the adjacency stacks, the edge ranking and the rank select of
csrc/ans_polya.hpp (compiled with g++) against brute force."""
import math
import os
import subprocess

import numpy as np
import pytest

import ans_amd as A

import mset_mirror as MM
import polya_mirror as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shuffle-coding_amd", "csrc")

SETTINGS = [(True, True), (False, False), (True, False)]  # (loops, redraws): the harness's, with and without loops

# a second restatement's values (a cross-check between restatements, not reference output)
KNOWN_IDS = {(0, 0): 0x76be999e3e25b2a0, (0, 1): 0x7359aa1156ce877a, (3, 7): 0x3e0e9daa0f6f333d,
             (299, 4294967295): 0xcfaf4889c241cf9b}


def test_mirrors_edge_id_is_siphash13_of_the_pair():
    """The mirror's hash against a scratch restatement's values; the library's edge_id meets the
    same values in the g++ program below, and the bytes of every E >= 12 case depend on both."""
    for (i, j), want in KNOWN_IDS.items():
        assert PM.siphash13_pair(i, j) == want, (i, j)
    assert PM.siphash13_pair(1, 0) != PM.siphash13_pair(0, 1)  # the tuple as given


def _graphs(loops):
    """(name, n, edges): both sides of the plain / joint switch, loops where the setting has them."""
    rng = np.random.default_rng(17)
    yield "empty", 4, []
    yield "one edge", 2, [(0, 1)]
    yield "E=11", 6, PM.random_graph(rng, 6, 11)
    yield "E=12", 6, PM.random_graph(rng, 6, 12)
    yield "K6", 6, PM.complete(6)
    yield "n=40 E=90", 40, PM.random_graph(rng, 40, 90)
    if loops:
        yield "the one loop", 1, [(0, 0)]
        yield "n=2 with loops", 2, [(0, 0), (0, 1), (1, 1)]
        yield "n=9 E=20 with loops", 9, PM.random_graph(rng, 9, 20, loops=True)


def _seeds():
    """Random seed messages, and the same with zero bytes on top (the pull runs through them)."""
    seed = MM.seeds(np.random.default_rng(11), 1, 96)[0]
    return [("seed", seed), ("seed + zeros", seed + b"\x00\x00\x00")]


@pytest.mark.parametrize("loops,redraws", SETTINGS)
def test_push_pop_bytes_equal_the_mirror(loops, redraws):
    for name, n, edges in _graphs(loops):
        mirror = PM.Mirror(n, loops, redraws)
        codec = A.PolyaUrn(n, len(edges), loops, redraws)
        for sname, seed in _seeds():
            where = f"{name} from {sname}"
            want = mirror.push_bytes(seed, edges)
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            codec.push(m, edges)
            assert m.flatten() == want, f"{where}: push"
            want_edges, want_rest = mirror.pop_bytes(want, len(edges))
            m = A.Message.unflatten(want, A.GEN_EMPTY)
            got = codec.pop(m)
            assert list(got) == want_edges, f"{where}: the edges as the codec returns them"
            assert m.flatten() == want_rest, f"{where}: what remains"
            assert sorted(got) == sorted(edges), where
            if len(edges) <= 11:
                assert list(got) == sorted(edges), f"{where}: the plain codec returns the edges sorted"


@pytest.mark.parametrize("loops,redraws", SETTINGS)
def test_order_of_the_edge_list_does_not_matter(loops, redraws):
    rng = np.random.default_rng(5)
    seed = _seeds()[0][1]
    for name, n, edges in _graphs(loops):
        codec = A.PolyaUrn(n, len(edges), loops, redraws)
        want = None
        for order in (edges, edges[::-1], sorted(edges), [edges[k] for k in rng.permutation(len(edges))]):
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            codec.push(m, order)
            want = want or m.flatten()
            assert m.flatten() == want, name


@pytest.mark.parametrize("loops,redraws", SETTINGS)
def test_pop_of_push_restores_the_message_and_the_multiset(loops, redraws):
    """Codec.test_invertibility (src/ans.rs:47-59) from a random, a zeros and a resumed message."""
    for name, n, edges in _graphs(loops):
        codec = A.PolyaUrn(n, len(edges), loops, redraws)
        for initial in (A.Message.random(3), A.Message.zeros(), A.Message.unflatten(_seeds()[0][1], A.GEN_EMPTY)):
            codec.test_invertibility(edges, initial)
        m = A.Message.random(9)
        codec.push(m, edges)
        decoded = codec.pop(m)
        assert decoded == edges and sorted(decoded) == sorted(edges), name
        if len(edges) > 1:
            assert decoded != [edges[0]] * len(edges)


def test_growth_is_the_urns_bits_less_the_orders():
    """Loop-free graphs under (loops, redraws) = (true, true): no mass is ever excluded, so the
    urn's probability of an edge sequence is prod_v deg_v! / prod_{k<E} (n + 2k)^2 whatever its
    order, each edge gives its orientation bit back and the multiset its log2(E!): the message grows
    by [sum_k 2 log2(n + 2k) - sum_v log2(deg_v!) - log2(E!) - E] / 8 bytes, within 2 (each length
    is floor(virtual bits / 8) + 1, as in test_mset_host.py)."""
    rng = np.random.default_rng(23)
    for n, num_edges in ((6, 11), (6, 12), (40, 90), (300, 1000)):
        edges = PM.random_graph(rng, n, num_edges)
        deg = np.bincount(np.asarray(edges).ravel(), minlength=n)
        bits = sum(2 * math.log2(n + 2 * k) for k in range(num_edges))
        bits -= sum(math.lgamma(int(d) + 1) for d in deg) / math.log(2)
        bits -= math.lgamma(num_edges + 1) / math.log(2) + num_edges
        seed = MM.seeds(rng, 1, 2048)[0]  # the orbit pops take log2(E!) + E bits out before any push
        m = A.Message.unflatten(seed, A.GEN_EMPTY)
        before = len(m.flatten())
        A.PolyaUrn(n, num_edges, True, True).push(m, edges)
        grown = len(m.flatten()) - before
        print(f"n={n} E={num_edges}: grew {grown} B, closed form {bits / 8:.2f} B")
        assert abs(grown - bits / 8) <= 2.0


def _code_of(fn):
    with pytest.raises(A.AnsError) as e:
        fn()
    return e.value.code


def test_every_error_is_a_status():
    zeros, seed = A.Message.zeros, _seeds()[0][1]
    # the alphabet (src/graph_codec.rs:137, 222, 257)
    assert _code_of(lambda: A.PolyaUrn(4, 1, True, True).push(zeros(), [(2, 1)])) == A.ANS_E_SYMBOL
    assert _code_of(lambda: A.PolyaUrn(4, 1, True, True).push(zeros(), [(1, 4)])) == A.ANS_E_SYMBOL
    assert _code_of(lambda: A.PolyaUrn(4, 1, False, True).push(zeros(), [(1, 1)])) == A.ANS_E_SYMBOL
    assert _code_of(lambda: A.PolyaUrn(4, 2, True, True).push(zeros(), [(0, 1), (0, 1)])) == A.ANS_E_SYMBOL
    many = PM.complete(6) + [(2, 3)]  # a pair given twice, past the plain / joint switch
    assert _code_of(lambda: A.PolyaUrn(6, len(many), True, True).push(zeros(), many)) == A.ANS_E_SYMBOL
    assert _code_of(lambda: A.PolyaUrn(4, 1, True, True, directed=True)) == A.ANS_E_ARG
    # a pull past the start of a short seed, push (the orientation pop) and pop
    assert _code_of(lambda: A.PolyaUrn(4, 1, True, True).push(A.Message.unflatten(b"\x07", A.GEN_EMPTY),
                                                             [(0, 1)])) == A.ANS_E_EXHAUSTED
    with pytest.raises(PM.Fail) as f:
        PM.Mirror(4, True, True).push_bytes(b"\x07", [(0, 1)])
    assert f.value.code == PM.E_EXHAUSTED  # as the mirror reports
    assert _code_of(lambda: A.PolyaUrn(50, 40, True, True).pop(A.Message.unflatten(b"\x07" * 9, A.GEN_EMPTY))) \
        == A.ANS_E_EXHAUSTED
    # pops of bytes no push wrote: a norm of 0 after the exclusions (the one node of n = 1 excluded;
    # no node at all), and an edge decoded twice (n = 1 with loops decodes (0, 0) both times)
    assert _code_of(lambda: A.PolyaUrn(1, 1, False, True).pop(A.Message.unflatten(seed, A.GEN_EMPTY))) \
        == A.ANS_E_ZERO_MASS
    assert _code_of(lambda: A.PolyaUrn(0, 1, True, True).pop(A.Message.unflatten(seed, A.GEN_EMPTY))) \
        == A.ANS_E_ZERO_MASS
    assert _code_of(lambda: A.PolyaUrn(1, 2, True, True).pop(A.Message.unflatten(seed, A.GEN_EMPTY))) \
        == A.ANS_E_SYMBOL
    for n, num_edges, loops, code in ((1, 1, False, PM.E_ZERO_MASS), (1, 2, True, PM.E_SYMBOL)):
        with pytest.raises(PM.Fail) as f:
            PM.Mirror(n, loops, True).pop_bytes(seed, num_edges)
        assert f.value.code == code
    # K2 without redraws: after (0, 1) node 0 excludes itself and its neighbour, nothing is left
    assert _code_of(lambda: A.PolyaUrn(2, 2, False, False).pop(A.Message.unflatten(seed, A.GEN_EMPTY))) \
        == A.ANS_E_ZERO_MASS


def test_random_bytes_decode_to_a_status_or_a_graph():
    """Pops of arbitrary bytes under every setting end in a graph of the alphabet or in one of the
    statuses, the mirror's where it has one."""
    rng = np.random.default_rng(31)
    for trial in range(60):
        loops, redraws = SETTINGS[trial % 3]
        n, num_edges = int(rng.integers(1, 7)), int(rng.integers(0, 16))
        data = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        try:
            want = PM.Mirror(n, loops, redraws).pop_bytes(data, num_edges)
        except PM.Fail as f:
            want = f.code
        m = A.Message.unflatten(data, A.GEN_EMPTY)
        try:
            got = (list(A.PolyaUrn(n, num_edges, loops, redraws).pop(m)), m.flatten())
        except A.AnsError as e:
            got = e.code
        if isinstance(want, tuple) or want != PM.E_SYMBOL:
            assert got == want, (trial, n, num_edges, loops, redraws)
        else:  # the library finds the repeated edge after the last pop, which can fail first
            assert got in (A.ANS_E_SYMBOL, A.ANS_E_EXHAUSTED, A.ANS_E_ZERO_MASS), trial


# ---- csrc/ans_polya.hpp with g++ (no HIP): the adjacency stacks, the exclusion, the edge
# ranking and the rank select against brute force
CHECKER = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>
#include "ans_polya.hpp"
using namespace shuffle_coding;
struct Vec {
    uint32_t* p;
    uint32_t load(uint32_t i) const { return p[i]; }
    void store(uint32_t i, uint32_t v) { p[i] = v; }
};
struct Ws {
    uint32_t* p;
    Vec at(uint64_t o) const { return Vec{p + o}; }
};
static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++bad < 8) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

// a random graph of n nodes and E distinct pairs (loops allowed), in random order
static std::vector<uint32_t> graph(uint32_t n, uint32_t E, std::mt19937_64& R) {
    std::set<std::pair<uint32_t, uint32_t>> seen;
    std::vector<uint32_t> e;
    while (seen.size() < E) {
        uint32_t i = (uint32_t)(R() % n), j = (uint32_t)(R() % n);
        if (i > j) std::swap(i, j);
        if (seen.insert({i, j}).second) { e.push_back(i); e.push_back(j); }
    }
    return e;
}

static void stacks(uint32_t n, uint32_t E, bool loops, std::mt19937_64& R, long& walks) {
    const std::vector<uint32_t> e = graph(n, E, R);
    std::vector<uint32_t> ws(polya::ws_entries(n, E));
    auto st = polya::State<Vec>::make(Ws{ws.data()}, n, E);
    auto edge_at = [&](uint32_t p, uint32_t& i, uint32_t& j) { i = e[2 * p]; j = e[2 * p + 1]; };
    std::vector<std::multiset<uint32_t>> adj(n);
    std::vector<uint32_t> mass(n, 1);
    polya::graph_empty(st, n, false);
    st.urn.build();
    auto check = [&](uint32_t v) {
        // the stack names v's neighbours, newest first; the urn holds degree + 1
        std::multiset<uint32_t> got;
        for (uint32_t s = st.head.load(v); s != polya::kNil; s = st.next.load(s)) {
            uint32_t i, j;
            edge_at(s >> 1, i, j);
            got.insert((s & 1) ? i : j);
        }
        CHECK(got == adj[v], "stack of node %u (n %u E %u)", v, n, E);
        CHECK(st.urn.count(v) == mass[v], "mass of node %u", v);
        // use_codec_without(v): what leaves, what is left, and everything back afterwards
        uint64_t want = loops ? 0 : mass[v];
        std::set<uint32_t> out(adj[v].begin(), adj[v].end());
        for (uint32_t u : out) if (loops || u != v) want += mass[u];
        const uint64_t gone = polya::exclude(st, v, loops, false, edge_at);
        CHECK(gone == want, "exclude(%u) took %llu, want %llu", v, (unsigned long long)gone, (unsigned long long)want);
        for (uint32_t u = 0; u < n; ++u) {
            const bool excluded = (!loops && u == v) || out.count(u);
            CHECK(st.urn.count(u) == (excluded ? 0 : mass[u]), "mass of %u while %u is excluded", u, v);
        }
        uint64_t total = 0;
        for (uint32_t u = 0; u < n; ++u) total += mass[u];
        CHECK(st.urn.prefix(n) == total - gone && st.total == total, "norm while %u is excluded", v);
        polya::include(st, v, loops, false, edge_at);
        for (uint32_t u = 0; u < n; ++u) CHECK(st.urn.count(u) == mass[u], "mass of %u after include", u);
        ++walks;
    };
    auto touch = [&](uint32_t p, int d) {
        const uint32_t i = e[2 * p], j = e[2 * p + 1];
        if (d > 0) { adj[i].insert(j); if (i != j) adj[j].insert(i); }
        else { adj[i].erase(adj[i].find(j)); if (i != j) adj[j].erase(adj[j].find(i)); }
        mass[i] += d; if (i != j) mass[j] += d;
    };
    for (uint32_t p = 0; p < E; ++p) {
        polya::link_edge(st, p, e[2 * p], e[2 * p + 1]);
        polya::urn_edge(st, e[2 * p], e[2 * p + 1], 1);
        touch(p, 1);
        check(e[2 * p]); check(e[2 * p + 1]); check((uint32_t)(R() % n));
    }
    for (uint32_t p = E; p-- > 0;) {  // ... and out again, last to first
        polya::unlink_edge(st, p, e[2 * p], e[2 * p + 1]);
        polya::urn_edge(st, e[2 * p], e[2 * p + 1], -1);
        touch(p, -1);
        check(e[2 * p]); check(e[2 * p + 1]); check((uint32_t)(R() % n));
    }
    for (uint32_t v = 0; v < n; ++v) CHECK(st.head.load(v) == polya::kNil, "node %u not empty at the end", v);
}

static void ranks(uint32_t n, uint32_t E, std::mt19937_64& R) {
    const std::vector<uint32_t> e = graph(n, E, R);
    std::vector<uint32_t> ws(polya::ws_entries(n, E));
    auto st = polya::State<Vec>::make(Ws{ws.data()}, n, E);
    for (int joint = 0; joint < 2; ++joint) {
        CHECK(polya::rank_edges(st, e.data(), E, joint != 0) == ANS_OK, "rank_edges status");
        std::vector<uint32_t> want(E);
        for (uint32_t k = 0; k < E; ++k) want[k] = k;
        std::sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) {
            if (joint) return polya::edge_id(e[2 * a], e[2 * a + 1]) < polya::edge_id(e[2 * b], e[2 * b + 1]);
            return std::make_pair(e[2 * a], e[2 * a + 1]) < std::make_pair(e[2 * b], e[2 * b + 1]);
        });
        for (uint32_t r = 0; r < E; ++r) CHECK(st.ord.load(r) == want[r], "ord[%u] (E %u joint %d)", r, E, joint);
    }
    if (E >= 2) {  // a pair given twice
        std::vector<uint32_t> twice = e;
        const uint32_t a = (uint32_t)(R() % E), b = (a + 1 + (uint32_t)(R() % (E - 1))) % E;
        twice[2 * a] = twice[2 * b];
        twice[2 * a + 1] = twice[2 * b + 1];
        for (int joint = 0; joint < 2; ++joint)
            CHECK(polya::rank_edges(st, twice.data(), E, joint != 0) == ANS_E_SYMBOL, "a pair twice (E %u joint %d)", E, joint);
    }
    // the select of the joint push: ranks leave one by one, find(cf) is the cf-th left
    st.orb.nsym = E;
    for (uint32_t r = 0; r < E; ++r) st.orb.a.store(r, 1);
    st.orb.build();
    std::vector<uint32_t> left(E);
    for (uint32_t r = 0; r < E; ++r) left[r] = r;
    for (uint32_t L = E; L > 0; --L) {
        const uint32_t cf = (uint32_t)(R() % L);
        const mset::Found f = st.orb.find(cf);
        CHECK(f.rank == left[cf] && f.count == 1 && f.cum == cf, "select %u of %u", cf, L);
        CHECK(st.orb.prefix(f.rank) == cf, "prefix of rank %u", f.rank);
        st.orb.add(f.rank, -1);
        left.erase(left.begin() + cf);
    }
}

int main() {
    std::mt19937_64 R(7);
    long walks = 0;
    const uint32_t shapes[][2] = {{1, 1}, {2, 3}, {3, 2}, {5, 15}, {7, 12}, {33, 32}, {40, 39}, {50, 200}, {64, 300}};
    for (auto& s : shapes)
        for (int loops = 0; loops < 2; ++loops) stacks(s[0], s[1], loops != 0, R, walks);
    const uint32_t sizes[][2] = {{2, 1}, {3, 2}, {6, 11}, {6, 12}, {6, 13}, {40, 255}, {40, 256}, {40, 257}, {300, 1000}};
    for (auto& s : sizes) ranks(s[0], s[1], R);
    if (polya::edge_id(3, 7) != 0x3e0e9daa0f6f333dull || polya::edge_id(0, 0) != 0x76be999e3e25b2a0ull ||
        polya::edge_id(0, 1) != 0x7359aa1156ce877aull || polya::edge_id(299, 4294967295u) != 0xcfaf4889c241cf9bull) { ++bad; printf("edge_id\n"); }
    printf("walks %ld bad %ld\n", walks, bad);
    return bad != 0;
}
"""


def test_stacks_ranks_and_select_match_brute_force(tmp_path):
    """ans_polya.hpp's adjacency stacks (link / unlink in reverse order, the neighbour walk),
    exclude / include on the urn, rank_edges (both orders, a repeated pair) and the 0/1 rank
    select, over sizes on both sides of powers of two and of the plain / joint switch."""
    src, exe = tmp_path / "polya_check.cpp", tmp_path / "polya_check"
    src.write_text(CHECKER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    line = out.stdout.strip().splitlines()[-1].split()
    shapes = [1, 3, 2, 15, 12, 32, 39, 200, 300]
    assert line[0] == "walks" and int(line[1]) == 2 * 2 * 3 * sum(shapes) and line[-1] == "0", out.stdout
