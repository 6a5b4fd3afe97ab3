"""One lane, several labelled graphs: the kernels of ans_wl_labelled.hip keep a lane's state (that of
ans_wl.hip's kernels and, under an edge table, the label of each adjacency entry, the slice's positions
and labels and the wider sort scratch) in the context's workspace, entry i of lane l at i * lanes + l,
and a lane that codes a second graph finds the first one's state there.  As
test_gpu_wl_lane_reuse.py: bounds so large that the 256 MiB cap leaves one workgroup (read back from
the launch record), 200 graphs on its 64 lanes, a large labelled graph and then a small one on every
lane, every slot compared with the host codec's (itself pinned to the mirror by test_labelled_host.py)."""
import functools

import numpy as np
import pytest

import ans_amd as A

import labelled_mirror as LM
import polya_mirror as PM
from test_gpu_arer import _seeds, SEED_BYTES
from test_gpu_labelled import Dev, _cat, _codec

pytestmark = pytest.mark.gpu

MODELS = ["er", "pu"]
WL_ITER, HALF = 1, True
NUM_GRAPHS = 200  # 3 * 64 + 8: every lane codes three graphs, eight of them four
# one wave's state is more than half of 256 MiB, so one workgroup: a push holds 4 dwords a pair under an
# edge table (include/ans_capi.h 5g), a pop 2
MAX_NODES, PUSH_EDGES, POP_EDGES = 64, 200000, 400000


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _large(g):
    """Neighbours in a wave differ in size, and so do g and g + 64 (the graph a lane codes next)."""
    return (g // 64 + g) % 2 == 1


def _host(model, n, loops):
    if model == "er":
        return A.AutoregressiveERLabelled(A.Bernoulli(LM.MASS, LM.NORM), n, loops, WL_ITER, HALF, _cat(LM.NODE_MASSES),
                                          _cat(LM.EDGE_MASSES))
    return A.AutoregressivePolyaLabelled(n, loops, WL_ITER, HALF, _cat(LM.NODE_MASSES), _cat(LM.EDGE_MASSES))


@functools.lru_cache(maxsize=None)
def _graphs(model, loops):
    rng = np.random.default_rng(900 + loops)
    node_alphabet = [s for s, p in enumerate(LM.NODE_MASSES) if p]
    edge_alphabet = [s for s, p in enumerate(LM.EDGE_MASSES) if p]
    graphs = []
    for g in range(NUM_GRAPHS):
        n = int(rng.integers(14, 25)) if _large(g) else int(rng.integers(0, 7))
        alphabet = n * (n - 1) // 2 + (n if loops else 0)
        low = 12 if _large(g) else 0
        pairs = PM.random_graph(rng, n, int(rng.integers(low, max(low, min(60, alphabet)) + 1)), loops)
        graphs.append((n, [int(v) for v in rng.choice(node_alphabet, n)],
                       [(e, int(l)) for e, l in zip(pairs, rng.choice(edge_alphabet, len(pairs)))]))
    seeds = _seeds(rng, NUM_GRAPHS)
    want = []
    for (n, labels, edges), s in zip(graphs, seeds):
        codec = _host(model, n, loops)
        m = A.Message.unflatten(s, A.GEN_EMPTY)
        perm = [int(v) for v in codec.push(m, A.Graph(labels, edges))]
        pushed = m.flatten()
        m = A.Message.unflatten(pushed, A.GEN_EMPTY)  # (as the slot holds it: a flattened message)
        popped = codec.pop(m)
        want.append((pushed, perm, (list(popped.node_labels), popped.edges), m.flatten()))
    return graphs, seeds, want


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_lanes_code_several_labelled_graphs(gpu, model, loops):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _graphs(model, loops)
    codec = _codec(gpu, model, loops, WL_ITER, HALF, LM.NODE_MASSES, LM.EDGE_MASSES, (LM.MASS, LM.NORM))
    d = Dev(torch, graphs, seeds, SEED_BYTES + codec.slack(24, 60), MAX_NODES)
    assert d.push(codec, PUSH_EDGES) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got = d.messages()
    for c in range(NUM_GRAPHS):
        assert got[c] == want[c][0], f"push, graph {c} (lane {c % 64}, its graph number {c // 64})"
    assert d.perms([g[0] for g in graphs]) == [w[1] for w in want]
    assert d.pop(codec, POP_EDGES) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got, popped = d.messages(), d.popped_graphs([g[0] for g in graphs], True, True)
    for c in range(NUM_GRAPHS):
        assert popped[c] == want[c][2], f"pop, graph {c}"
        assert got[c] == want[c][3], f"what remains, graph {c}"
