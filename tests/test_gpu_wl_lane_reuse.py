"""One lane, several graphs: the kernels of ans_wl.hip keep a lane's state (the slice model's, the
ids, the ordered known positions, the dirty list, the sort scratch, on a pop the decoded prefix's
adjacency) in the context's workspace, entry i of lane l at i * lanes + l, and a lane that codes a
second graph finds the first one's state there.  These cases declare bounds so large that the 256 MiB
cap leaves one workgroup (read back from the launch record, Gpu.last_launch_grid, so that the reuse is
known to have happened), code 200 graphs on its 64 lanes, small and larger ones in turn on every
lane, and compare every graph with the mirror of tests/wl_mirror.py bit for bit, at wl_iter 1 with
the half iteration, for both slice models.  The expected grids follow from kWsMax = 256 MiB and
ans_wl.hpp's *_entries as they stand."""
import functools

import numpy as np
import pytest

import ans_amd as A

import polya_mirror as PM
import wl_mirror as WM
from test_gpu_arer import _seeds, SEED_BYTES
from test_gpu_wl import Dev, _codec, _slack

pytestmark = pytest.mark.gpu

MODELS = ["er", "pu"]
WL_ITER, HALF = 1, True
WS_MAX = 256 << 20
NUM_GRAPHS = 200  # 3 * 64 + 8: every lane codes three graphs, eight of them four
MAX_NODES, MAX_EDGES = 64, 400000


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _orbit(n, wl_iter):
    return (2 * (wl_iter + 1) + 4 + (2 if wl_iter else 0)) * n


ENTRIES = {  # include/ans_capi.h section 5f
    ("er", "push"): lambda n, e, w: 4 * n + 2 * e + 1 + _orbit(n, w),
    ("er", "pop"): lambda n, e, w: 2 * n + 2 * e + _orbit(n, w),
    ("pu", "push"): lambda n, e, w: 11 * n + 2 * e + 1 + _orbit(n, w),
    ("pu", "pop"): lambda n, e, w: 9 * n + min(n, 11) + 2 * e + _orbit(n, w),
}


def _most_edges(model, what):
    """The largest max_edges whose state of one wave fits the cap at MAX_NODES."""
    fixed = ENTRIES[model, what](MAX_NODES, 0, WL_ITER)
    return (WS_MAX // 256 - fixed) // 2


def test_the_declared_bounds_give_the_grids_asserted_below():
    for key, entries in ENTRIES.items():
        assert WS_MAX // (256 * entries(MAX_NODES, MAX_EDGES, WL_ITER)) == 1, key
        most = _most_edges(*key)
        assert 256 * entries(MAX_NODES, most, WL_ITER) <= WS_MAX < 256 * entries(MAX_NODES, most + 1, WL_ITER), key


def _large(g):
    """Neighbours in a wave differ in size, and so do g and g + 64 (the graph a lane codes next)."""
    return (g // 64 + g) % 2 == 1


@functools.lru_cache(maxsize=None)
def _graphs(model, loops):
    rng = np.random.default_rng(700 + loops)
    graphs = []
    for g in range(NUM_GRAPHS):
        n = int(rng.integers(14, 25)) if _large(g) else int(rng.integers(0, 7))
        alphabet = n * (n - 1) // 2 + (n if loops else 0)
        low = 12 if _large(g) else 0
        graphs.append((n, PM.random_graph(rng, n, int(rng.integers(low, max(low, min(60, alphabet)) + 1)), loops)))
    seeds = _seeds(rng, NUM_GRAPHS)
    want = []
    for (n, e), s in zip(graphs, seeds):
        mirror = WM.mirror_of(model, n, loops, WL_ITER, HALF)
        pushed, perm = mirror.push_bytes(s, e)
        want.append((pushed, perm) + mirror.pop_bytes(pushed))
    return graphs, seeds, want


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_a_lanes_code_several_graphs(gpu, model, loops):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _graphs(model, loops)
    codec = _codec(gpu, model, loops, WL_ITER, HALF)
    d = Dev(torch, graphs, seeds, SEED_BYTES + _slack(codec, 24, 60), MAX_NODES)
    assert d.push(codec, MAX_EDGES) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got = d.messages()
    for c in range(NUM_GRAPHS):
        assert got[c] == want[c][0], f"push, graph {c} (lane {c % 64}, its graph number {c // 64})"
    assert d.perms([n for n, _ in graphs]) == [w[1] for w in want]
    assert d.pop(codec, MAX_EDGES) == A.ANS_OK
    assert gpu.last_launch_grid() == 1
    got, pairs = d.messages(), d.popped()
    for c in range(NUM_GRAPHS):
        assert pairs[c] == want[c][2], f"pop, graph {c}"
        assert got[c] == want[c][3], f"what remains, graph {c}"


@pytest.mark.parametrize("model", MODELS)
def test_b_the_largest_state_of_one_wave_and_the_first_refused(gpu, model):
    torch = pytest.importorskip("torch")
    graphs = [(4, [(0, 1), (2, 3), (1, 2)]), (3, []), (4, [(0, 3)])]
    seeds = _seeds(np.random.default_rng(740), 3)
    want = []
    for (n, e), s in zip(graphs, seeds):
        mirror = WM.mirror_of(model, n, False, WL_ITER, HALF)
        pushed, perm = mirror.push_bytes(s, e)
        want.append((pushed, perm) + mirror.pop_bytes(pushed))
    codec = _codec(gpu, model, False, WL_ITER, HALF)
    d = Dev(torch, graphs, seeds, SEED_BYTES + _slack(codec, 4, 3), MAX_NODES)
    most = _most_edges(model, "push")
    assert d.push(codec, most) == A.ANS_OK and gpu.last_launch_grid() == 1
    assert d.messages() == [w[0] for w in want]
    # one pair more: refused by the launch plan, before the record is cleared and any kernel starts
    before, launched = d.messages(), gpu.last_launch()
    with pytest.raises(A.AnsError) as e:
        d.push(codec, most + 1)
    assert e.value.code == A.ANS_E_ARG
    assert gpu.last_launch() == launched and gpu.last_launch_grid() == 1
    assert gpu.status(d.status, d.stream) == A.ANS_OK and int(d.status.cpu()[0]) == 0
    assert d.messages() == before
    most = _most_edges(model, "pop")
    assert d.pop(codec, most) == A.ANS_OK and gpu.last_launch_grid() == 1
    assert d.popped() == [w[2] for w in want] and d.messages() == [w[3] for w in want]
    before, launched = d.messages(), gpu.last_launch()
    with pytest.raises(A.AnsError) as e:
        d.pop(codec, most + 1)
    assert e.value.code == A.ANS_E_ARG
    assert gpu.last_launch() == launched and gpu.last_launch_grid() == 1
    assert d.messages() == before
