"""The autoregressive Erdős–Rényi graph codecs on the host (include/ans_capi.h section 3:
ans_ar_er_push, ans_ar_er_pop; ans_amd.AutoregressiveER) against the expected-bytes mirror of
tests/arer_mirror.py, against the oracle's IID pushes where no mirror is needed, and the class ids
of csrc/ans_arer.hpp (compiled with g++) against the mirror's."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

import arer_mirror as AM
import mset_mirror as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shuffle-coding_amd", "csrc")

MASS, NORM = 100, 1000
ORBITS = [A.ORBITS_NONE, A.ORBITS_ONE_CLASS, A.ORBITS_DEGREE]

# a second restatement's values (cross-checks between restatements, not reference output)
H0 = 0xbd60acb658c79e45
KNOWN_IDS = [0x3de3a71ddb1c510b, 0x0f082841e50df5b4, 0x35e71bc5b90dcd54, 0xbdbead4301d2200c]
DEGREES_BY_ID = [1, 2, 0, 7, 3, 5, 4, 6]


def _seeds():
    """A random seed message, and the same with zero bytes on top (the pull runs through them)."""
    seed = MM.seeds(np.random.default_rng(11), 1, 96)[0]
    return [("seed", seed), ("seed + zeros", seed + b"\x00\x00\x00")]


@functools.lru_cache(maxsize=None)
def _expected(orbits):
    """{(shape, seed name): (bytes after push, perm, pairs as pop returns them, bytes after pop)}."""
    out = {}
    for name, n, edges, loops in AM.shapes():
        mirror = AM.Mirror(MASS, NORM, n, loops, orbits)
        for sname, seed in _seeds():
            pushed, perm = mirror.push_bytes(seed, edges)
            popped, rest = mirror.pop_bytes(pushed)
            out[name, sname] = (pushed, perm, popped, rest)
    return out


def test_mirrors_ids_are_the_known_values():
    assert AM.H0 == H0 == MM.siphash13_usize(0) == A.lib().ans_orbit_id(0)
    assert [AM.degree_id(d) for d in range(4)] == KNOWN_IDS
    assert sorted(range(8), key=AM.degree_id) == DEGREES_BY_ID


@pytest.mark.parametrize("orbits", ORBITS)
def test_push_pop_bytes_equal_the_mirror(orbits):
    bern = A.Bernoulli(MASS, NORM)
    want = _expected(orbits)
    for name, n, edges, loops in AM.shapes():
        codec = A.AutoregressiveER(bern, n, loops, orbits)
        for sname, seed in _seeds():
            where = f"{name} from {sname}"
            pushed, perm, popped, rest = want[name, sname]
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            got_perm = codec.push(m, edges)
            assert m.flatten() == pushed, f"{where}: push"
            assert list(got_perm) == perm, f"{where}: perm"
            m = A.Message.unflatten(pushed, A.GEN_EMPTY)
            got = codec.pop(m)
            assert got == popped, f"{where}: the pairs as the codec returns them"
            assert m.flatten() == rest, f"{where}: what remains"
            # the decoded graph is the input pushed through perm; pop order is v ascending, then
            # the slice's alphabet, the loop last
            assert sorted(got) == AM.relabelled(edges, perm), where
            assert got == sorted(got, key=lambda e: (e[0], e[1] == e[0], e[1])), f"{where}: pop order"
            if orbits == A.ORBITS_NONE:
                assert perm == list(range(n)) and sorted(got) == sorted(edges), where


def test_none_is_a_chain_of_the_oracles_iid_pushes():
    """Autoregressive: IID<Bernoulli>::push of slice v for v = n-1 .. 0, the oracle's own
    Categorical([norm - mass, mass]).push_iid; no mirror between."""
    bern = A.Bernoulli(MASS, NORM)
    cat = orc.Categorical(np.array([NORM - MASS, MASS], np.uint64))
    for name, n, edges, loops in AM.shapes():
        have = set(edges)
        for sname, seed in _seeds():
            m = orc.Message.unflatten(seed, orc.EMPTY)
            for v in reversed(range(n)):
                alphabet = [(v, j) for j in range(v + 1, n)] + ([(v, v)] if loops else [])
                if alphabet:
                    assert cat.push_iid(m, [int(e in have) for e in alphabet]) == 0 and not m.err
            got = A.Message.unflatten(seed, A.GEN_EMPTY)
            A.AutoregressiveER(bern, n, loops, A.ORBITS_NONE).push(got, edges)
            assert got.flatten() == m.flatten(), f"{name} from {sname}"


@pytest.mark.parametrize("orbits", ORBITS)
def test_order_of_the_pairs_does_not_matter(orbits):
    rng = np.random.default_rng(5)
    bern = A.Bernoulli(MASS, NORM)
    seed = _seeds()[0][1]
    for name, n, edges, loops in AM.shapes():
        codec = A.AutoregressiveER(bern, n, loops, orbits)
        want = _expected(orbits)[name, "seed"]
        for order in (edges[::-1], sorted(edges), [edges[k] for k in rng.permutation(len(edges))]):
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            perm = codec.push(m, order)
            assert m.flatten() == want[0] and list(perm) == want[1], name


def test_degree_orbits_save_the_order_of_the_nodes():
    """len(NONE) - len(DEGREE) = log2(n! / prod c_k!) / 8 bytes within 2 (each length is
    floor(virtual bits / 8) + 1, the margin test_mset_host.py gives its closed form); c_k = the nodes
    of the k-th distinct degree.  ONE_CLASS saves nothing.  Lengths are compared from the seed whose
    top byte is not zero: zero bytes on top are no content, the first renorm of any step drops them
    and a call without a step (NONE at n <= 1) keeps them, so they would count as savings."""
    for name, n, edges, loops in AM.shapes():
        deg = np.zeros(n, np.int64)
        for i, j in edges:
            deg[i] += 1
            deg[j] += i != j
        saved = math.lgamma(n + 1) - sum(math.lgamma(int(c) + 1) for c in np.unique(deg, return_counts=True)[1])
        saved /= 8 * math.log(2)
        for sname in ("seed",):
            none, one, degree = (len(_expected(o)[name, sname][0]) for o in ORBITS)
            print(f"{name} from {sname}: NONE {none} B, ONE_CLASS {one} B, DEGREE {degree} B, closed form {saved:.2f} B")
            assert abs((none - degree) - saved) <= 2.0, name
            if n >= 2:
                assert none == one, name


def _code_of(fn):
    with pytest.raises(A.AnsError) as e:
        fn()
    return e.value.code


def test_every_error_is_a_status():
    bern, zeros = A.Bernoulli(MASS, NORM), A.Message.zeros
    seed = _seeds()[0][1]
    for orbits in ORBITS:
        def push(n, loops, edges, b=bern, o=orbits):
            return lambda: A.AutoregressiveER(b, n, loops, o).push(zeros(), edges)
        # the alphabet: i > j, a node >= n, a loop without loops, a pair given twice (also a loop)
        assert _code_of(push(4, True, [(2, 1)])) == A.ANS_E_SYMBOL
        assert _code_of(push(4, True, [(1, 4)])) == A.ANS_E_SYMBOL
        assert _code_of(push(4, False, [(1, 1)])) == A.ANS_E_SYMBOL
        assert _code_of(push(4, True, [(0, 1), (2, 3), (0, 1)])) == A.ANS_E_SYMBOL
        assert _code_of(push(4, True, [(1, 1), (0, 1), (1, 1)])) == A.ANS_E_SYMBOL
        # a needed symbol of mass 0: an edge under mass 0, a non-edge under mass = norm; the symbol that
        # is not needed may have mass 0
        assert _code_of(push(3, False, [(0, 1)], A.Bernoulli(0, NORM))) == A.ANS_E_ZERO_MASS
        assert _code_of(push(3, False, [(0, 1)], A.Bernoulli(NORM, NORM))) == A.ANS_E_ZERO_MASS
        A.AutoregressiveER(A.Bernoulli(0, NORM), 3, False, orbits).push(A.Message.unflatten(seed, A.GEN_EMPTY), [])
        # a table of three symbols
        three = A.Categorical([1, 2, 3])
        assert _code_of(push(3, False, [(0, 1)], three)) == A.ANS_E_ARG
        assert _code_of(lambda: A.AutoregressiveER(three, 3, False, orbits).pop(zeros())) == A.ANS_E_ARG
        # a pop of a message cut to 2 bytes; a pop with cap one short
        m = A.Message.unflatten(seed, A.GEN_EMPTY)
        edges = [(0, 1), (0, 3), (2, 3), (4, 5), (1, 5)]
        A.AutoregressiveER(bern, 6, False, orbits).push(m, edges)
        data = m.flatten()
        assert _code_of(lambda: A.AutoregressiveER(bern, 6, False, orbits).pop(A.Message.unflatten(data[:2], A.GEN_EMPTY))) \
            == A.ANS_E_EXHAUSTED
        assert _code_of(lambda: A.AutoregressiveER(bern, 6, False, orbits).pop(A.Message.unflatten(data, A.GEN_EMPTY),
                                                                          cap=len(edges) - 1)) == A.ANS_E_LEN
        assert len(A.AutoregressiveER(bern, 6, False, orbits).pop(A.Message.unflatten(data, A.GEN_EMPTY),
                                                                  cap=len(edges))) == len(edges)
    with pytest.raises(AM.Fail) as f:
        AM.Mirror(0, NORM, 3, False, AM.DEGREE).push_bytes(seed, [(0, 1)])
    assert f.value.code == AM.E_ZERO_MASS  # as the mirror reports
    # an orbits value outside the three
    assert _code_of(lambda: A.AutoregressiveER(bern, 3, False, 3).push(zeros(), [(0, 1)])) == A.ANS_E_ARG
    assert _code_of(lambda: A.AutoregressiveER(bern, 3, False, 3).pop(zeros())) == A.ANS_E_ARG
    assert _code_of(lambda: A.AutoregressiveER(bern, 3, False, -1).pop(zeros())) == A.ANS_E_ARG


# ---- csrc/ans_arer.hpp with g++ (no HIP): the class ids and the degree rank table
CHECKER = r"""
#include <cstdio>
#include "ans_arer.hpp"
using namespace shuffle_coding;
int main() {
    printf("%016llx\n", (unsigned long long)arer::kH0);
    for (unsigned d = 0; d < 4; ++d) printf("%016llx\n", (unsigned long long)arer::class_id(d));
    std::vector<uint32_t> rank;
    if (!arer::build_degree_ranks(7, rank)) return 1;
    for (unsigned d = 0; d < 8; ++d) printf("%u\n", rank[d]);
    // no two degrees below 70,000 share an id
    printf("%d\n", arer::build_degree_ranks(69999, rank) ? 1 : 0);
    return 0;
}
"""


def test_the_librarys_ids_are_the_known_values(tmp_path):
    src, exe = tmp_path / "arer_ids.cpp", tmp_path / "arer_ids"
    src.write_text(CHECKER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split()
    assert [int(v, 16) for v in lines[:5]] == [H0] + KNOWN_IDS
    rank = [int(v) for v in lines[5:13]]
    assert sorted(range(8), key=rank.__getitem__) == DEGREES_BY_ID
    assert lines[13] == "1"
