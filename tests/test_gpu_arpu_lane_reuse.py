"""One lane, several graphs: the kernels of ans_arpu.hip keep a lane's state in the context's
workspace, entry i of lane l at i * lanes + l, and a lane that codes a second graph finds the first
one's state there.  These cases declare bounds so large that the 256 MiB cap leaves one workgroup
(read back from the launch record, Gpu.last_launch_grid, so that the reuse is known to have
happened), code 200 graphs on its 64 lanes, small ones and larger ones with a hub (a joint slice) in
turn on every lane, and compare every graph with the mirror of tests/arpu_mirror.py bit for bit.  The
expected grids follow from kWsMax = 256 MiB and ans_arpu.hpp push_entries / pop_entries as they
stand."""
import functools

import numpy as np
import pytest

import ans_amd as A

from polya_mirror import random_graph
from test_gpu_arer import _seeds, SEED_BYTES
from test_gpu_arpu import Dev, expect

pytestmark = pytest.mark.gpu

ORBITS = [A.ORBITS_NONE, A.ORBITS_ONE_CLASS, A.ORBITS_DEGREE]
WS_MAX = 256 << 20
NUM_GRAPHS = 200  # 3 * 64 + 8: every lane codes three graphs, eight of them four
PUSH_BOUNDS = (64, 400000)  # max_nodes, max_edges: 800,834 entries a lane
POP_NODES = 80000           # 720,012 entries a lane
BAD = (5, 70, 135)          # g + 64 (and g + 128 for the first) follow them on their lanes
MOST_EDGES = 130


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _push_entries(max_nodes, max_edges):
    return 13 * max_nodes + 2 * max_edges + 2


def _pop_entries(max_nodes):
    return 9 * max_nodes + min(max_nodes, 11) + 1


def test_the_declared_bounds_give_the_grids_asserted_below():
    assert WS_MAX // (256 * _push_entries(*PUSH_BOUNDS)) == 1
    assert WS_MAX // (256 * _pop_entries(POP_NODES)) == 1
    assert 256 * _push_entries(64, 523871) == WS_MAX
    assert 256 * _pop_entries(116507) < WS_MAX < 256 * _pop_entries(116508)


def _large(g):
    """Neighbours in a wave differ in size, and so do g and g + 64 (the graph a lane codes next)."""
    return (g // 64 + g) % 2 == 1


@functools.lru_cache(maxsize=None)
def _graphs(loops, orbits):
    rng = np.random.default_rng(510 + loops)
    graphs = []
    for g in range(NUM_GRAPHS):
        if _large(g):  # a hub of 12 to 20 neighbours: its slice, or its neighbours' sum, is joint
            n = int(rng.integers(24, 41))
            edges = set(random_graph(rng, n, int(rng.integers(12, 101)), loops))
            hub = int(rng.integers(0, n))
            others = [v for v in range(n) if v != hub]
            edges |= {tuple(sorted((hub, int(v)))) for v in rng.choice(others, int(rng.integers(12, 21)), replace=False)}
            edges = [sorted(edges)[k] for k in rng.permutation(len(edges))]
        else:
            n = int(rng.integers(0, 9))
            alphabet = n * (n - 1) // 2 + (n if loops else 0)
            edges = random_graph(rng, n, int(rng.integers(0, alphabet + 1)), loops)
        assert len(edges) <= MOST_EDGES
        graphs.append((n, edges))
    seeds = _seeds(rng, NUM_GRAPHS)
    return graphs, seeds, [expect(n, e, s, loops, orbits) for (n, e), s in zip(graphs, seeds)]


def _cap(codec):
    """The slots' size: by the graphs coded, not by the declared bounds (which size the state only)."""
    return SEED_BYTES + codec.slack(40, MOST_EDGES)


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("orbits", ORBITS)
def test_a_lanes_code_several_graphs(gpu, orbits, loops):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _graphs(loops, orbits)
    codec = A.GpuAutoregressivePolya(gpu, loops, orbits)
    d = Dev(torch, graphs, seeds, _cap(codec), PUSH_BOUNDS[0])
    assert d.push(codec, PUSH_BOUNDS[1]) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got = d.messages()
    for c in range(NUM_GRAPHS):
        assert got[c] == want[c][0], f"push, graph {c} (lane {c % 64}, its graph number {c // 64})"
    assert d.perms([n for n, _ in graphs]) == [w[1] for w in want]
    d.max_nodes = POP_NODES
    assert d.pop(codec, MOST_EDGES) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got, pairs = d.messages(), d.popped()
    for c in range(NUM_GRAPHS):
        assert pairs[c] == want[c][2], f"pop, graph {c}"
        assert got[c] == want[c][3], f"what remains, graph {c}"


def _with(items, replacement):
    out = list(items)
    for g in BAD:
        out[g] = replacement(g)
    return out


def _others_equal(got, want, what):
    for c in range(NUM_GRAPHS):
        if c not in BAD:
            assert got[c] == want[c], f"{what}, graph {c}"


@pytest.mark.parametrize("orbits", [A.ORBITS_NONE, A.ORBITS_DEGREE])
def test_b_a_failed_graph_then_good_ones_on_its_lane(gpu, orbits):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _graphs(False, orbits)
    assert all(_large(g) for g in BAD) and all(g + 64 < NUM_GRAPHS for g in BAD)
    codec = A.GpuAutoregressivePolya(gpu, False, orbits)
    pushed = [w[0] for w in want]
    twice = lambda g: (graphs[g][0], graphs[g][1] + [graphs[g][1][0]])  # found after the adjacency is written
    for kind, bad_graphs, bad_seeds in (
            (A.ANS_E_EXHAUSTED, graphs, _with(seeds, lambda g: b"")),  # nothing to pull for the first renorm
            (A.ANS_E_SYMBOL, _with(graphs, twice), seeds)):
        d = Dev(torch, bad_graphs, bad_seeds, _cap(codec), PUSH_BOUNDS[0])
        assert d.push(codec, PUSH_BOUNDS[1]) == kind
        assert gpu.last_launch_grid() == 1
        assert all(d.lens()[g] == 0 for g in BAD), kind
        _others_equal(d.messages(), pushed, f"push beside status {kind}")
    # ... and on pop: two bytes of the message
    d = Dev(torch, graphs, _with(pushed, lambda g: pushed[g][:2]), _cap(codec), POP_NODES)
    assert d.pop(codec, MOST_EDGES) == A.ANS_E_EXHAUSTED
    assert gpu.last_launch_grid() == 1
    assert all(d.lens()[g] == 0 and d.counts()[g] == 0 for g in BAD)
    _others_equal(d.messages(), [w[3] for w in want], "what remains beside ANS_E_EXHAUSTED")
    _others_equal(d.popped(), [w[2] for w in want], "pop beside ANS_E_EXHAUSTED")


def test_c_the_largest_state_of_one_wave_and_the_first_refused(gpu):
    torch = pytest.importorskip("torch")
    graphs = [(4, [(0, 1), (2, 3), (1, 2)]), (3, []), (4, [(0, 3)])]
    seeds = _seeds(np.random.default_rng(541), 3)
    orbits = A.ORBITS_DEGREE
    want = [expect(n, e, s, False, orbits) for (n, e), s in zip(graphs, seeds)]
    codec = A.GpuAutoregressivePolya(gpu, False, orbits)
    d = Dev(torch, graphs, seeds, _cap(codec), 64)
    assert d.push(codec, 523871) == A.ANS_OK  # 2^20 entries a lane, 256 MiB a wave
    assert gpu.last_launch_grid() == 1
    assert d.messages() == [w[0] for w in want]
    # one node more: refused by the launch plan, before the record is cleared and any kernel starts
    before = d.messages()
    d.max_nodes = 65
    d.d_perm = d.d_perm.new_full((3 * 65,), -1)
    with pytest.raises(A.AnsError) as e:
        d.push(codec, 523871)
    assert e.value.code == A.ANS_E_ARG
    assert gpu.last_launch() == f"k_arpu_push<orbits={orbits}>" and gpu.last_launch_grid() == 1
    assert gpu.status(d.status, d.stream) == A.ANS_OK and int(d.status.cpu()[0]) == 0
    assert d.messages() == before
    # pop: 9 * 116,507 + 12 entries a lane fit, one node more does not
    d.max_nodes = 116507
    assert d.pop(codec, 4) == A.ANS_OK and gpu.last_launch_grid() == 1
    assert d.popped() == [w[2] for w in want] and d.messages() == [w[3] for w in want]
    before = d.messages()
    d.max_nodes = 116508
    with pytest.raises(A.AnsError) as e:
        d.pop(codec, 4)
    assert e.value.code == A.ANS_E_ARG
    assert gpu.last_launch() == f"k_arpu_pop<orbits={orbits}>" and gpu.last_launch_grid() == 1
    assert d.messages() == before
