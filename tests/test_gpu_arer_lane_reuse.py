"""One lane, several graphs: the kernels of ans_arer.hip keep a lane's state in the context's
workspace, entry i of lane l at i * lanes + l, and a lane that codes a second graph finds the first
one's state there.  These cases declare bounds so large that the 256 MiB cap leaves one workgroup
(read back from the launch record, Gpu.last_launch_grid, so that the reuse is known to have
happened), code 200 graphs on its 64 lanes, small and larger ones in turn on every lane, and compare
every graph with the mirror of tests/arer_mirror.py bit for bit.  The expected grids follow from
kWsMax = 256 MiB and ans_arer.hpp push_entries / pop_entries as they stand; no two degrees up to
524,288 share a class id (checked on the CPU when this was written), so the rank table of the
largest bound exists."""
import functools

import numpy as np
import pytest

import ans_amd as A

import arer_mirror as AM
import polya_mirror as PM
from test_gpu_arer import Dev, _expect, _seeds, SEED_BYTES

pytestmark = pytest.mark.gpu

ORBITS = [A.ORBITS_NONE, A.ORBITS_ONE_CLASS, A.ORBITS_DEGREE]
TABLE = (100, 1000)
WS_MAX = 256 << 20
NUM_GRAPHS = 200  # 3 * 64 + 8: every lane codes three graphs, eight of them four
PUSH_BOUNDS = (64, 400000)  # max_nodes, max_edges: 800,386 entries a lane
POP_NODES = 300000          # 600,001 entries a lane
BAD = (5, 70, 135)          # g + 64 (and g + 128 for the first) follow them on their lanes


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _push_entries(max_nodes, max_edges):
    return 6 * max_nodes + 2 * max_edges + 2


def _pop_entries(max_nodes):
    return 2 * max_nodes + 1


def test_the_declared_bounds_give_the_grids_asserted_below():
    assert WS_MAX // (256 * _push_entries(*PUSH_BOUNDS)) == 1
    assert WS_MAX // (256 * _pop_entries(POP_NODES)) == 1
    assert 256 * _push_entries(64, 524095) == WS_MAX and 256 * _pop_entries(524287) < WS_MAX < 256 * _pop_entries(524288)


def _large(g):
    """Neighbours in a wave differ in size, and so do g and g + 64 (the graph a lane codes next)."""
    return (g // 64 + g) % 2 == 1


@functools.lru_cache(maxsize=None)
def _graphs(loops, orbits):
    rng = np.random.default_rng(500 + loops)
    graphs = []
    for g in range(NUM_GRAPHS):
        n = int(rng.integers(24, 41)) if _large(g) else int(rng.integers(0, 9))
        alphabet = n * (n - 1) // 2 + (n if loops else 0)
        low = 12 if _large(g) else 0
        graphs.append((n, PM.random_graph(rng, n, int(rng.integers(low, max(low, min(100, alphabet)) + 1)), loops)))
    seeds = _seeds(rng, NUM_GRAPHS)
    return graphs, seeds, [_expect(TABLE, n, e, s, loops, orbits) for (n, e), s in zip(graphs, seeds)]


def _cap(codec):
    """The slots' size: by the graphs coded, not by the declared bounds (which size the state only)."""
    return SEED_BYTES + codec.slack(40)


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("orbits", ORBITS)
def test_a_lanes_code_several_graphs(gpu, orbits, loops):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _graphs(loops, orbits)
    codec = A.GpuAutoregressiveER(gpu, A.Bernoulli(*TABLE), loops, orbits)
    d = Dev(torch, graphs, seeds, _cap(codec), PUSH_BOUNDS[0])
    assert d.push(codec, PUSH_BOUNDS[1]) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got = d.messages()
    for c in range(NUM_GRAPHS):
        assert got[c] == want[c][0], f"push, graph {c} (lane {c % 64}, its graph number {c // 64})"
    assert d.perms([n for n, _ in graphs]) == [w[1] for w in want]
    d.max_nodes = POP_NODES
    assert d.pop(codec) == A.ANS_OK
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
    codec = A.GpuAutoregressiveER(gpu, A.Bernoulli(*TABLE), False, orbits)
    pushed = [w[0] for w in want]
    twice = lambda g: (graphs[g][0], graphs[g][1] + [graphs[g][1][0]])  # found after the adjacency is written
    for kind, bad_graphs, bad_seeds in (
            (A.ANS_E_EXHAUSTED, graphs, _with(seeds, lambda g: b"")),  # nothing to pull for the first renorm
            (A.ANS_E_SYMBOL, _with(graphs, twice), seeds)):
        assert all(len(bad_graphs[g][1]) for g in BAD)
        d = Dev(torch, bad_graphs, bad_seeds, _cap(codec), PUSH_BOUNDS[0])
        assert d.push(codec, PUSH_BOUNDS[1]) == kind
        assert gpu.last_launch_grid() == 1
        assert all(d.lens()[g] == 0 for g in BAD), kind
        _others_equal(d.messages(), pushed, f"push beside status {kind}")
    # ... and on pop: two bytes of the message
    d = Dev(torch, graphs, _with(pushed, lambda g: pushed[g][:2]), _cap(codec), POP_NODES)
    assert d.pop(codec) == A.ANS_E_EXHAUSTED
    assert gpu.last_launch_grid() == 1
    assert all(d.lens()[g] == 0 and d.counts()[g] == 0 for g in BAD)
    _others_equal(d.messages(), [w[3] for w in want], "what remains beside ANS_E_EXHAUSTED")
    _others_equal(d.popped(), [w[2] for w in want], "pop beside ANS_E_EXHAUSTED")


def test_c_the_largest_state_of_one_wave_and_the_first_refused(gpu):
    torch = pytest.importorskip("torch")
    graphs = [(4, [(0, 1), (2, 3), (1, 2)]), (3, []), (4, [(0, 3)])]
    seeds = _seeds(np.random.default_rng(540), 3)
    orbits = A.ORBITS_DEGREE
    want = [_expect(TABLE, n, e, s, False, orbits) for (n, e), s in zip(graphs, seeds)]
    codec = A.GpuAutoregressiveER(gpu, A.Bernoulli(*TABLE), False, orbits)
    d = Dev(torch, graphs, seeds, _cap(codec), 64)
    assert d.push(codec, 524095) == A.ANS_OK  # 2^20 entries a lane, 256 MiB a wave
    assert gpu.last_launch_grid() == 1
    assert d.messages() == [w[0] for w in want]
    # one node more: refused by the launch plan, before the record is cleared and any kernel starts
    before = d.messages()
    d.max_nodes = 65
    d.d_perm = d.d_perm.new_full((3 * 65,), -1)
    with pytest.raises(A.AnsError) as e:
        d.push(codec, 524095)
    assert e.value.code == A.ANS_E_ARG
    assert gpu.last_launch() == f"k_arer_push<orbits={orbits}>" and gpu.last_launch_grid() == 1
    assert gpu.status(d.status, d.stream) == A.ANS_OK and int(d.status.cpu()[0]) == 0
    assert d.messages() == before
    # pop: 2 * 524,287 + 1 entries a lane fit, one node more does not
    d.max_nodes = 524287
    assert d.pop(codec) == A.ANS_OK and gpu.last_launch_grid() == 1
    assert d.popped() == [w[2] for w in want] and d.messages() == [w[3] for w in want]
    before = d.messages()
    d.max_nodes = 524288
    with pytest.raises(A.AnsError) as e:
        d.pop(codec)
    assert e.value.code == A.ANS_E_ARG
    assert gpu.last_launch() == f"k_arer_pop<orbits={orbits}>" and gpu.last_launch_grid() == 1
    assert d.messages() == before
