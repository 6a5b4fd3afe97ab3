"""One lane, several graphs: the kernels of ans_joint.hip keep a lane's state (the prefix graph or the
decoded adjacency, the orbit stage, and over it the ordered urn's arrays) in the context's workspace,
entry i of lane l at i * lanes + l, and a lane that codes a second graph finds the first one's state
there.  These cases declare bounds so large that the 256 MiB cap leaves one workgroup (read back from
the launch record, Gpu.last_launch_grid, so that the reuse is known to have happened), code 200 graphs
on its 64 lanes, small ones and ones with a hub of 12 to 33 neighbours in turn on every lane (both sides
of the urn's plain / joint switch at 11 pairs and of the 32 words at which the hash's length byte wraps),
and compare every graph with the host entries byte for byte, at wl_iter 1 with the half iteration, for
both ordered codecs.  The expected grids follow from kWsMax = 256 MiB and ans_joint.hpp's *_entries as
include/ans_capi.h section 5h states them."""
import functools

import numpy as np
import pytest

import ans_amd as A

import polya_mirror as PM
from test_gpu_arer import _seeds
from test_gpu_joint import Dev, _codec, _host_codec, _slack

pytestmark = pytest.mark.gpu

MODELS = ["er", "pu"]
WL_ITER, HALF = 1, True
WS_MAX = 256 << 20
NUM_GRAPHS = 200  # 3 * 64 + 8: every lane codes three graphs, eight of them four
MAX_NODES = 64
MAX_EDGES = {"er": 400000, "pu": 120000}
SEED_BYTES = 128  # the order of 38 nodes and 45 pairs is 334 bits


def _orbit(n, w):
    return (2 * (w + 1) + 6) * n if w else 5 * n + 1


ENTRIES = {  # include/ans_capi.h section 5h
    ("er", "push"): lambda n, e, w: 3 * n + 2 * e + 1 + _orbit(n, w),
    ("er", "pop"): lambda n, e, w: 2 * n + 2 * e + _orbit(n, w),
    ("pu", "push"): lambda n, e, w: 3 * n + 2 * e + 1 + max(_orbit(n, w), 2 * n + 6 * e + 2),
    ("pu", "pop"): lambda n, e, w: max(2 * n + 2 * e + _orbit(n, w), 2 * n + 5 * e + 2 + min(e, 11)),
}


def test_the_declared_bounds_give_the_grids_asserted_below():
    for (model, what), entries in ENTRIES.items():
        assert WS_MAX // (256 * entries(MAX_NODES, MAX_EDGES[model], WL_ITER)) == 1, (model, what)


def _large(g):
    """Neighbours in a wave differ in size, and so do g and g + 64 (the graph a lane codes next)."""
    return (g // 64 + g) % 2 == 1


@functools.lru_cache(maxsize=None)
def _graphs(model, loops):
    rng = np.random.default_rng(800 + loops)
    graphs = []
    for g in range(NUM_GRAPHS):
        if _large(g):
            hub = 12 + (g // 2) % 22  # 12 .. 33 neighbours
            n = hub + 1 + int(rng.integers(0, 5))
            centre = int(rng.integers(0, n))
            others = [v for v in range(n) if v != centre]
            star = {(min(centre, v), max(centre, v)) for v in others[:hub]}
            extra = [e for e in PM.random_graph(rng, n, 12, loops) if e not in star and centre not in e]
            graphs.append((n, sorted(star) + extra))
        else:
            n = int(rng.integers(0, 7))
            alphabet = n * (n - 1) // 2 + (n if loops else 0)
            graphs.append((n, PM.random_graph(rng, n, int(rng.integers(0, min(11, alphabet) + 1)), loops)))
    seeds = _seeds(rng, NUM_GRAPHS, SEED_BYTES)
    want = []
    for (n, e), s in zip(graphs, seeds):
        host = _host_codec(model, n, loops, WL_ITER, HALF)
        m = A.Message.unflatten(s, A.GEN_EMPTY)
        perm = [int(p) for p in host.push(m, e)]
        pushed = m.flatten()
        m = A.Message.unflatten(pushed, A.GEN_EMPTY)
        pairs = host.pop(m) if model == "er" else host.pop(m, len(e))
        want.append((pushed, perm, pairs, m.flatten()))
    return graphs, seeds, want


def test_the_graphs_cross_the_plain_switch_and_the_wrap():
    graphs, _, _ = _graphs("pu", False)
    sizes = {len(e) for _, e in graphs}
    assert min(sizes) <= 11 < max(sizes)
    degrees = {max(sum(1 for e in edges if v in e) for v in range(n)) for n, edges in graphs if n}
    assert {12, 29, 30, 33} <= degrees  # 2 + 30 words is the first hash whose length byte wraps


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_a_lanes_code_several_graphs(gpu, model, loops):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _graphs(model, loops)
    codec = _codec(gpu, model, loops, WL_ITER, HALF)
    d = Dev(torch, graphs, seeds, SEED_BYTES + _slack(codec, 38, 60), MAX_NODES)
    assert d.push(codec, MAX_EDGES[model]) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got = d.messages()
    for c in range(NUM_GRAPHS):
        assert got[c] == want[c][0], f"push, graph {c} (lane {c % 64}, its graph number {c // 64})"
    assert d.perms([n for n, _ in graphs]) == [w[1] for w in want]
    assert d.pop(codec, MAX_EDGES[model]) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got, pairs = d.messages(), d.popped()
    for c in range(NUM_GRAPHS):
        assert pairs[c] == want[c][2], f"pop, graph {c}"
        assert got[c] == want[c][3], f"what remains, graph {c}"


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)
