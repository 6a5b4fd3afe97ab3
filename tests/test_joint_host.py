"""Joint shuffle coding of graphs with Weisfeiler-Lehman orbits on the host (include/ans_capi.h section 3:
ans_joint_er_wl_push / _pop, ans_joint_polya_wl_push / _pop; ans_amd.JointERWL, JointPolyaWL) against the
expected-bytes mirror of tests/joint_mirror.py, the mirror's dense loop against the oracle's GraphIID,
the reference's incremental ids against apply, and what the orbits save, measured on the library's own
messages.

The seed is 320 bytes where test_wl_host._seeds has 96: a joint push pops the whole order (log2 n! bits,
and under the urn log2 E! more for the order of the pairs) before its ordered codec pushes the first
bit, 296 + 1,245 bits for "n=64 E=200", and the Empty generator gives none back."""
import math

import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

import arer_mirror as AM
import joint_mirror as JM
import mset_mirror as MM
from polya_mirror import random_graph

MASS, NORM = JM.MASS, JM.NORM
SETTINGS = [(w, h) for w in range(4) for h in (True, False)]
CASES = [("er", False)] + [("pu", r) for r in (False, True)]  # (model, redraws)


def _seeds():
    """test_wl_host._seeds() with a longer seed: a random seed message, and the same with zero bytes on top."""
    seed = MM.seeds(np.random.default_rng(11), 1, 320)[0]
    return [("seed", seed), ("seed + zeros", seed + b"\x00\x00\x00")]


def _codec(model, n, loops, wl_iter, half_iter, redraws=False):
    if model == "er":
        return A.JointERWL(A.Bernoulli(MASS, NORM), n, loops, wl_iter, half_iter)
    return A.JointPolyaWL(n, loops, redraws, wl_iter, half_iter)


def _pop(codec, m, num_edges):
    return codec.pop(m) if isinstance(codec, A.JointERWL) else codec.pop(m, num_edges)


# ---- 1. the mirror's dense loop is GraphIID without labels
def test_the_mirrors_dense_loop_is_the_oracles_graph_iid():
    masses = np.array([NORM - MASS, MASS], np.uint64)
    seed = _seeds()[0][1]
    for name, n, edges, loops in JM.shapes():
        a, b = orc.Message.unflatten(seed, orc.EMPTY), orc.Message.unflatten(seed, orc.EMPTY)
        JM.dense_push(a, masses, n, loops, edges)
        assert orc.graph_iid_push(b, n, None, np.asarray(edges, np.int64).reshape(-1, 2), None, masses, None, None, False,
                                  loops) == 0
        assert a.flatten() == b.flatten(), name
        popped = JM.dense_pop(a, masses, n, loops)
        _, indices, _ = orc.graph_iid_pop(b, n, masses, None, None, False, loops)
        assert sorted(popped) == [tuple(e) for e in indices] == sorted(edges) and a.flatten() == b.flatten(), name
        assert popped == [e for e in JM.all_edge_indices(n, loops) if e in set(edges)], name


# ---- 2. update_around(full, [the node that changed sides]) carries what apply computes
@pytest.mark.parametrize("wl_iter", range(4))
def test_carried_ids_equal_apply_at_every_step(wl_iter):
    rng = np.random.default_rng(23 + wl_iter)
    graphs = [(name, n, edges) for name, n, edges, _ in JM.shapes()]
    for k in range(30):
        n = int(rng.integers(1, 24))
        loops = bool(k & 1)
        most = n * (n - 1) // 2 + (n if loops else 0)
        graphs.append((f"random {k}", n, random_graph(rng, n, int(rng.integers(0, min(most, 3 * n) + 1)), loops=loops)))
    for half_iter in (True, False):
        for name, n, edges in graphs:
            steps, bad = JM.joint_carried_against_apply(n, edges, wl_iter, half_iter, rng)
            assert steps == 2 * n and bad == 0, f"{name} wl_iter={wl_iter} half={half_iter}: {bad} of {steps} steps differ"


# ---- 3. the library against the mirror
@pytest.mark.parametrize("model,redraws", CASES)
@pytest.mark.parametrize("wl_iter,half_iter", SETTINGS)
def test_push_pop_bytes_equal_the_mirror(model, redraws, wl_iter, half_iter):
    want = JM.expected(model, wl_iter, half_iter, redraws, tuple(_seeds()))
    rng = np.random.default_rng(5)
    for name, n, edges, loops in JM.shapes():
        codec = _codec(model, n, loops, wl_iter, half_iter, redraws)
        for sname, seed in _seeds():
            where = f"{name} from {sname}"
            pushed, perm, popped, rest = want[name, sname]
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            got_perm = codec.push(m, edges)
            assert m.flatten() == pushed, f"{where}: push"
            assert list(got_perm) == perm, f"{where}: perm"
            m = A.Message.unflatten(pushed, A.GEN_EMPTY)
            got = _pop(codec, m, len(edges))
            assert got == popped, f"{where}: the pairs as the codec returns them"
            assert m.flatten() == rest, f"{where}: what remains"
            assert sorted(got) == AM.relabelled(edges, perm), where
        # the order of the input pairs does not matter
        seed = _seeds()[0][1]
        for order in (edges[::-1], [edges[k] for k in rng.permutation(len(edges))]):
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            got_perm = codec.push(m, order)
            assert m.flatten() == want[name, "seed"][0] and list(got_perm) == want[name, "seed"][1], name


# ---- 4. without a mirror: what the orbits save under the Erdős–Rényi ordered codec, wl_iter 1 + half
def _log2_factorial(n):
    return math.lgamma(n + 1) / math.log(2)


SAVED = {"er: n=40 E=90": _log2_factorial(40), "er: n=64 E=200": _log2_factorial(64), "er: K1,7": math.log2(8),
         "er: K6": 0.0, "K1,33": math.log2(34)}


def test_saved_bits_and_round_trips():
    seed = _seeds()[0][1]
    bern = A.Bernoulli(MASS, NORM)
    seen = set()
    for name, n, edges, loops in JM.shapes():
        codec = A.JointERWL(bern, n, loops, 1, True)
        m = A.Message.unflatten(seed, A.GEN_EMPTY)
        before = m.virtual_bits()
        perm = codec.push(m, edges)
        joint_bits = m.virtual_bits() - before
        o = A.Message.unflatten(seed, A.GEN_EMPTY)
        A.ErdosRenyi(bern, n, False, loops).push(o, edges)
        ordered_bits = o.virtual_bits() - before
        saved = ordered_bits - joint_bits
        print(f"{name}: ordered {ordered_bits:.3f} bits, joint {joint_bits:.3f}, saved {saved:.3f}")
        if name in SAVED:
            A.assert_bits_eq(SAVED[name], saved)
            seen.add(name)
        m = A.Message.unflatten(m.flatten(), A.GEN_EMPTY)  # (as the mirror pops: from the flattened bytes)
        got = codec.pop(m)
        assert sorted(got) == AM.relabelled(edges, list(perm)), name
        if n >= 1:
            assert m.flatten() == seed, name
        else:  # nothing was coded: the untouched seed reflattens with a zero byte more each time
            assert m.flatten() == JM.expected("er", 1, True, False, tuple(_seeds()))[name, "seed"][3], name
    assert seen == set(SAVED)


# ---- 5. every error is a status, and the message is left as it was
def _fails(fn, m, code):
    before = m.flatten()
    with pytest.raises(A.AnsError) as e:
        fn(m)
    assert e.value.code == code
    assert m.flatten() == before  # (flatten clones: calling it changes nothing)


@pytest.mark.parametrize("model,redraws", CASES)
def test_every_error_is_a_status_and_leaves_the_message(model, redraws):
    seed = _seeds()[0][1]

    def fresh():
        return A.Message.unflatten(seed, A.GEN_EMPTY)

    for half_iter in (True, False):
        _fails(lambda m: _codec(model, 3, False, 4, half_iter, redraws).push(m, [(0, 1)]), fresh(), A.ANS_E_ARG)
        _fails(lambda m: _pop(_codec(model, 3, False, 4, half_iter, redraws), m, 1), fresh(), A.ANS_E_ARG)
        _fails(lambda m: _pop(_codec(model, 3, False, -1, half_iter, redraws), m, 1), fresh(), A.ANS_E_ARG)
    for wl_iter, half_iter in SETTINGS:
        def push(n, loops, edges):
            return lambda m: _codec(model, n, loops, wl_iter, half_iter, redraws).push(m, edges)
        _fails(push(4, True, [(2, 1)]), fresh(), A.ANS_E_SYMBOL)
        _fails(push(4, True, [(1, 4)]), fresh(), A.ANS_E_SYMBOL)  # out of range
        _fails(push(4, False, [(1, 1)]), fresh(), A.ANS_E_SYMBOL)  # a loop without `loops`
        _fails(push(4, True, [(0, 1), (2, 3), (0, 1)]), fresh(), A.ANS_E_SYMBOL)  # a pair twice
        _fails(push(4, True, [(1, 1), (0, 1), (1, 1)]), fresh(), A.ANS_E_SYMBOL)
        edges = [(0, 1), (0, 3), (2, 3), (4, 5), (1, 5)]
        codec = _codec(model, 6, False, wl_iter, half_iter, redraws)
        m = fresh()
        codec.push(m, edges)
        data = m.flatten()
        # a pop of a message cut to 2 bytes
        _fails(lambda m: _pop(codec, m, len(edges)), A.Message.unflatten(data[:2], A.GEN_EMPTY), A.ANS_E_EXHAUSTED)
        # a push that runs out of bits to pop: the order of six nodes needs more than a byte
        _fails(lambda m: codec.push(m, edges), A.Message.unflatten(b"\x01", A.GEN_EMPTY), A.ANS_E_EXHAUSTED)
        if model == "er":  # a pop with cap one short (the urn takes the count itself: it has no capacity)
            _fails(lambda m: codec.pop(m, cap=len(edges) - 1), A.Message.unflatten(data, A.GEN_EMPTY), A.ANS_E_LEN)
            assert len(codec.pop(A.Message.unflatten(data, A.GEN_EMPTY), cap=len(edges))) == len(edges)
    if model == "er":
        for wl_iter, half_iter in SETTINGS:
            def er(b):
                return A.JointERWL(b, 3, False, wl_iter, half_iter)
            _fails(lambda m: er(A.Bernoulli(0, NORM)).push(m, [(0, 1)]), fresh(), A.ANS_E_ZERO_MASS)
            _fails(lambda m: er(A.Bernoulli(NORM, NORM)).push(m, [(0, 1)]), fresh(), A.ANS_E_ZERO_MASS)
            three = A.Categorical([1, 2, 3])
            _fails(lambda m: er(three).push(m, [(0, 1)]), fresh(), A.ANS_E_ARG)
            _fails(lambda m: er(three).pop(m), fresh(), A.ANS_E_ARG)
