"""The autoregressive Pólya urn graph codecs on the host (include/ans_capi.h section 3:
ans_ar_polya_push, ans_ar_polya_pop; ans_amd.AutoregressivePolya) against the expected-bytes mirror
of tests/arpu_mirror.py, and, where every slice holds at most one pair, against a chain of the
oracle's own Categorical and Uniform steps written out here, with no mirror between."""
import functools

import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

import arpu_mirror as PM2
import mset_mirror as MM
from polya_mirror import random_graph

ORBITS = [A.ORBITS_NONE, A.ORBITS_ONE_CLASS, A.ORBITS_DEGREE]


def _seeds():
    """Two random seed messages; the second with zero bytes on top (the pull runs through them)."""
    a, b = MM.seeds(np.random.default_rng(13), 2, 96)
    return [("seed", a), ("seed + zeros", b + b"\x00\x00\x00")]


@functools.lru_cache(maxsize=None)
def _expected(orbits):
    """{(shape, seed name): (bytes after push, perm, pairs as pop returns them, bytes after pop)}."""
    out = {}
    for name, n, edges, loops in PM2.shapes():
        mirror = PM2.Mirror(n, loops, orbits)
        for sname, seed in _seeds():
            m = orc.Message.unflatten(seed, orc.EMPTY)
            perm = mirror.push(m, edges)
            pushed = m.flatten()
            m = orc.Message.unflatten(pushed, orc.EMPTY)
            popped = mirror.pop(m)
            out[name, sname] = (pushed, perm, popped, m.flatten())
    return out


def _check_roundtrip(where, n, edges, loops, orbits, seed, want):
    pushed, perm, popped, rest = want
    codec = A.AutoregressivePolya(n, loops, orbits)
    m = A.Message.unflatten(seed, A.GEN_EMPTY)
    got_perm = codec.push(m, edges)
    assert m.flatten() == pushed, f"{where}: push"
    assert list(got_perm) == perm, f"{where}: perm"
    m = A.Message.unflatten(pushed, A.GEN_EMPTY)
    got = codec.pop(m)
    assert got == popped, f"{where}: the pairs as the codec returns them"
    assert m.flatten() == rest, f"{where}: what remains"
    # the decoded graph is the input pushed through perm; the pairs come v ascending, within v by w
    # ascending, the loop first: sorted as tuples
    assert got == PM2.relabelled(edges, perm), f"{where}: the relabelled input, in the documented order"
    if orbits == A.ORBITS_NONE:
        assert perm == list(range(n)) and got == sorted(edges), where
    return rest


@pytest.mark.parametrize("orbits", ORBITS)
def test_push_pop_bytes_equal_the_mirror(orbits):
    want = _expected(orbits)
    for name, n, edges, loops in PM2.shapes():
        for sname, seed in _seeds():
            rest = _check_roundtrip(f"{name} from {sname}", n, edges, loops, orbits, seed, want[name, sname])
            if sname == "seed":  # what remains is the seed (no node: two flattens, a zero byte each)
                assert rest == (seed if n else seed + bytes(2)), name


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("orbits", ORBITS)
def test_random_graphs_equal_the_mirror(orbits, loops):
    """200 random graphs over the settings (a third of them here), each from its own random seed."""
    rng = np.random.default_rng(100 + 2 * orbits + loops)
    seeds = MM.seeds(rng, 34, 64)
    for k, seed in enumerate(seeds):
        n = int(rng.integers(0, 41))
        alphabet = n * (n - 1) // 2 + (n if loops else 0)
        # sparse and dense in turn: dense graphs of 14 nodes or more have joint slices
        most = min(alphabet, 3 * n) if k % 2 else alphabet
        edges = random_graph(rng, n, int(rng.integers(0, most + 1)), loops)
        mirror = PM2.Mirror(n, loops, orbits)
        m = orc.Message.unflatten(seed, orc.EMPTY)
        perm = mirror.push(m, edges)
        pushed = m.flatten()
        m = orc.Message.unflatten(pushed, orc.EMPTY)
        popped = mirror.pop(m)
        rest = _check_roundtrip(f"graph {k}: n={n} E={len(edges)}", n, edges, loops, orbits, seed,
                                (pushed, perm, popped, m.flatten()))
        assert rest == (seed if n else seed + bytes(2))


# ---- without the mirror: slices of at most one pair under ORBITS_NONE
def _bit_len(x):
    return int(x).bit_length()


def _chain(m, n, edges, loops):
    """Autoregressive::push of a graph whose slices hold at most one pair, as the oracle's own steps.
    Slice v (v = n-1 .. 0) of the pair (v, j): the 1-vector's plain_shuffle_codec is a Uniform(1) pop and a
    Uniform(1) push; j is pushed under the urn over the positions v + !loops .. n-1, mass 1 + the
    neighbours among the positions < v; then the size: Uniform(1) of 0 and Uniform(bitlen(s_v) + 2) of 1.
    An empty slice pushes 0 under Uniform(bitlen(s_v) + 2) alone."""
    adj = [set() for _ in range(n)]
    for i, j in edges:
        adj[i].add(j)
        adj[j].add(i)
    for v in reversed(range(n)):
        mine = [j for j in adj[v] if j >= v]
        assert len(mine) <= 1
        s_v = n - v - 1 + int(loops)
        if mine:
            j = mine[0]
            assert orc.uniform_pop(m, 1) == 0
            orc.uniform_push(m, 1, 0)
            masses = np.zeros(n, np.uint64)
            for k in range(v + (0 if loops else 1), n):
                masses[k] = 1 + sum(1 for w in adj[k] if w < v)
            assert orc.Categorical(masses).push(m, j) == 0
            orc.uniform_push(m, 1, 0)
            orc.uniform_push(m, _bit_len(s_v) + 2, 1)
        else:
            orc.uniform_push(m, _bit_len(s_v) + 2, 0)
        assert not m.err


@pytest.mark.parametrize("loops", [False, True])
def test_none_with_single_pair_slices_is_a_chain_of_the_oracles_steps(loops):
    graphs = [("n=0", 0, []), ("n=1", 1, []), ("n=2", 2, [(0, 1)]), ("n=2 empty", 2, []),
              ("empty graph", 9, []), ("path in label order", 9, [(v, v + 1) for v in range(8)]),
              ("perfect matching", 10, [(v, v + 1) for v in range(0, 10, 2)]),
              ("crossed matching", 10, [(v, 9 - v) for v in range(5)])]
    if loops:
        graphs += [("n=1 with its loop", 1, [(0, 0)]), ("every loop", 5, [(v, v) for v in range(5)])]
    for name, n, edges in graphs:
        for sname, seed in _seeds():
            m = orc.Message.unflatten(seed, orc.EMPTY)
            _chain(m, n, edges, loops)
            got = A.Message.unflatten(seed, A.GEN_EMPTY)
            perm = A.AutoregressivePolya(n, loops, A.ORBITS_NONE).push(got, edges)
            assert got.flatten() == m.flatten(), f"{name} from {sname}"
            assert list(perm) == list(range(n))
            back = A.AutoregressivePolya(n, loops, A.ORBITS_NONE).pop(got)
            assert back == sorted(edges), name


@pytest.mark.parametrize("orbits", ORBITS)
def test_order_of_the_pairs_does_not_matter(orbits):
    rng = np.random.default_rng(5)
    seed = _seeds()[0][1]
    for name, n, edges, loops in PM2.shapes():
        codec = A.AutoregressivePolya(n, loops, orbits)
        want = _expected(orbits)[name, "seed"]
        for order in (edges[::-1], sorted(edges), [edges[k] for k in rng.permutation(len(edges))]):
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            perm = codec.push(m, order)
            assert m.flatten() == want[0] and list(perm) == want[1], name


def _code_of(fn):
    with pytest.raises(A.AnsError) as e:
        fn()
    return e.value.code


def test_every_error_is_a_status():
    zeros = A.Message.zeros
    seed = _seeds()[0][1]
    for orbits in ORBITS:
        def push(n, loops, edges, o=orbits):
            return lambda: A.AutoregressivePolya(n, loops, o).push(zeros(), edges)
        # the alphabet: i > j, a node >= n, a loop without loops, a pair given twice (also a loop)
        assert _code_of(push(4, True, [(2, 1)])) == A.ANS_E_SYMBOL
        assert _code_of(push(4, True, [(1, 4)])) == A.ANS_E_SYMBOL
        assert _code_of(push(4, False, [(1, 1)])) == A.ANS_E_SYMBOL
        assert _code_of(push(4, True, [(0, 1), (2, 3), (0, 1)])) == A.ANS_E_SYMBOL
        assert _code_of(push(4, True, [(1, 1), (0, 1), (1, 1)])) == A.ANS_E_SYMBOL
        # a pop from an empty message under the Empty tail; a message cut to 2 bytes; a cap one short
        assert _code_of(lambda: A.AutoregressivePolya(6, False, orbits).pop(A.Message.unflatten(b"", A.GEN_EMPTY))) \
            == A.ANS_E_EXHAUSTED
        m = A.Message.unflatten(seed, A.GEN_EMPTY)
        edges = [(0, 1), (0, 3), (2, 3), (4, 5), (1, 5)]
        A.AutoregressivePolya(6, False, orbits).push(m, edges)
        data = m.flatten()
        assert _code_of(lambda: A.AutoregressivePolya(6, False, orbits).pop(A.Message.unflatten(data[:2], A.GEN_EMPTY))) \
            == A.ANS_E_EXHAUSTED
        assert _code_of(lambda: A.AutoregressivePolya(6, False, orbits).pop(A.Message.unflatten(data, A.GEN_EMPTY),
                                                                         cap=len(edges) - 1)) == A.ANS_E_LEN
        assert len(A.AutoregressivePolya(6, False, orbits).pop(A.Message.unflatten(data, A.GEN_EMPTY),
                                                               cap=len(edges))) == len(edges)
    with pytest.raises(PM2.Fail) as f:
        PM2.Mirror(4, False, PM2.DEGREE).push(orc.Message.unflatten(seed, orc.EMPTY), [(1, 1)])
    assert f.value.code == PM2.E_SYMBOL  # as the mirror reports
    # an orbits value outside the three
    assert _code_of(lambda: A.AutoregressivePolya(3, False, 3).push(zeros(), [(0, 1)])) == A.ANS_E_ARG
    assert _code_of(lambda: A.AutoregressivePolya(3, False, 3).pop(zeros())) == A.ANS_E_ARG
    assert _code_of(lambda: A.AutoregressivePolya(3, False, -1).pop(zeros())) == A.ANS_E_ARG


@pytest.mark.parametrize("orbits", ORBITS)
def test_a_pop_of_random_bytes_is_a_status_or_a_graph(orbits):
    """Bytes no push wrote: a graph of the alphabet, or one of the statuses; never a crash."""
    rng = np.random.default_rng(77 + orbits)
    seen = set()
    for k in range(100):
        n, loops = int(rng.integers(0, 41)), bool(k & 1)
        data = rng.integers(0, 256, int(rng.integers(1, 48)), dtype=np.uint8).tobytes()
        try:
            got = A.AutoregressivePolya(n, loops, orbits).pop(A.Message.unflatten(data, A.GEN_EMPTY))
        except A.AnsError as e:
            assert e.code in (A.ANS_E_EXHAUSTED, A.ANS_E_SYMBOL), e.code
            seen.add(e.code)
            continue
        seen.add(A.ANS_OK)
        assert got == sorted(set(got)), "pairs in the documented order, none twice"
        assert all(i <= j < n and (loops or i != j) for i, j in got)
    assert A.ANS_E_EXHAUSTED in seen and A.ANS_E_SYMBOL in seen
