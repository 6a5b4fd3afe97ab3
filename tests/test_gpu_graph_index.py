"""The graph index kernels (csrc/ans_graph.hip) at tile and graph boundaries: the tile compaction
(k_tile_count, k_excl_scan, k_tile_emit, k_tile_emit_multi), the per-graph ranges
(k_graph_edge_offsets), the labelled-graph ranking (k_graph_edges_in, k_graph_sort_labels,
k_graph_slots_to_rows, k_graph_emit_rows) and the edge_slot / slot_edge / row_slot / row_edge
arithmetic.

The reference is `_alphabet`: AllEdgeIndices order (src/graph_codec.rs:187-199) built by plain
enumeration in numpy, no square root and no closed form, checked on CPU against the oracle's
literal Python loop.  Everything is exact equality: bytes, edges, offsets, counts, status codes.

1. The compaction alone through ans_dev_dense_to_edges / ans_dev_edges_to_dense on hand-built
   dense vectors: alphabet lengths on the 4096-slot tile grid, both branches of the last 16-byte
   word, the cap contract, slot_edge at every triangular-number boundary of n = 3000.
2. Dataset layouts through GpuDenseSets and GpuGraphs: totals that are multiples of the tile, graph
   boundaries on tile boundaries, zero-slot graphs before, on and after them; every stream
   byte-equal to the oracle's, every decoded edge, label and the raw edge_offsets array equal to
   the reference.  Labels are 251-valued functions of the edge, so a label beside the wrong edge
   shows.
3. GpuGraphs.encode refuses label lists of the wrong length before the library reads them.
"""
import ctypes

import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc
from test_graph_iid import _oracle_stream

TILE = 4096  # kTileSlots: 256 threads x 16 bytes
NORM = 1 << 28
MASS = int(0.3 * NORM)
BERN = [NORM - MASS, MASS]
SPACES = [(False, False), (True, False), (False, True), (True, True)]
UND, DL = (False, False), (True, True)
NLAB = 251  # label alphabet: a prime, so (31 i + 17 j) mod 251 separates neighbouring edges


# ---------------------------------------------------------------- the reference (CPU)
def _alen(n, directed, loops):  # num_all_edge_indices (src/graph_codec.rs:203-205)
    pairs = n * (n - 1) // 2
    return (n if loops else 0) + (2 * pairs if directed else pairs)


def _alphabet(n, directed, loops):
    """AllEdgeIndices order as a (len, 2) uint32 array, by enumeration: the loops (v, v), then
    for j in 0..n the pairs (i, j) with i in 0..j, each followed by (j, i) when directed."""
    cnt = np.arange(n, dtype=np.int64)  # column j holds j pairs
    j = np.repeat(cnt, cnt)
    i = np.arange(len(j), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)  # 0..j-1 within column j
    pairs = np.stack([i, j], 1)
    if directed:
        pairs = np.stack([pairs, pairs[:, ::-1]], 1).reshape(-1, 2)
    if loops:
        pairs = np.concatenate([np.stack([cnt, cnt], 1), pairs])
    assert len(pairs) == _alen(n, directed, loops)
    return pairs.astype(np.uint32)


_small = {}


def _alpha(n, directed, loops):
    """_alphabet, kept for the small spaces the dataset cases share (read-only)."""
    key = (n, directed, loops)
    if key not in _small:
        a = _alphabet(n, directed, loops)
        a.setflags(write=False)
        _small[key] = a
    return _small[key]


def _by_index(e):
    """Rows of e sorted by (i, j): EdgesIID's order (src/graph_codec.rs:67-71, 82-85)."""
    return e[np.lexsort((e[:, 1], e[:, 0]))]


def _lib_alen(n, directed, loops):
    out = A.u64(0)
    A._check(A.lib().ans_edge_alphabet_len(n, int(directed), int(loops), ctypes.byref(out)))
    return out.value


def _fill(lens, rest, k, top):
    """k node counts <= top, largest first, whose alphabet lengths sum to rest (None if none do)."""
    for n in range(top, 1, -1):
        if lens[n] == rest and k == 1:
            return [n]
        if lens[n] < rest and k > 1:
            more = _fill(lens, rest - lens[n], k - 1, n)
            if more:
                return [n] + more
    return None


def _case_a_counts(directed, loops):
    """Node counts shaped like the undirected [128, 11, 4, 3, 0, 1]: one graph that spans slot 4096,
    three small ones (four in the directed space with loops, whose lengths are squares: 8192 is
    no sum of four non-zero squares) and two trailing zero-slot graphs, 8192 slots (two full tiles)
    in all."""
    lens = {n: _alen(n, directed, loops) for n in range(2, 130)}
    tail = [0, 0] if loops else [0, 1]  # one node has a slot of its own only with loops
    for k in (3, 4):
        for n0 in sorted((n for n, v in lens.items() if TILE < v < 2 * TILE), reverse=True):
            small = _fill(lens, 2 * TILE - lens[n0], k, n0)
            if small:
                return [n0] + small + tail
    raise AssertionError("no node counts with 8192 slots")


CASE_A = {sp: _case_a_counts(*sp) for sp in SPACES}

# name, space -> node counts (cases a, g, h share CASE_A)
LAYOUTS = {
    ("b", DL): [64, 0, 0],  # 4096 slots: exactly one tile, trailing zero-slot graphs
    ("c", UND): [91, 2, 0, 1, 0, 91, 5],  # graphs 2..5 start at slot 4096
    ("c", DL): [63, 11, 2, 1, 1, 0, 0, 0, 64, 5],  # graphs 5..8 start at slot 4096
    ("d", UND): [0, 1, 0, 128, 3],  # leading zero-slot graphs
    ("e", UND): [60, 91, 40],  # graph 1 spans slot 4096, graphs 1 and 2 start deep in a tile
    ("e", DL): [40, 60, 30],
    ("f", UND): [0, 1, 0, 1],  # no slots at all
}


def _nums(name, space):
    return CASE_A[space] if name in "agh" else LAYOUTS[(name, space)]


def _bounds(nums, space):
    return np.concatenate([[0], np.cumsum([_alen(n, *space) for n in nums])]).astype(np.int64)


def _layout(name, space):
    """-> (node counts, per graph the sorted local slots that are set).  Apart from g (nothing set)
    and h (everything set): every graph's first and last slot, the two slots on either side of
    every tile boundary, slots 0 and 1, and a seeded random 300 of the rest."""
    nums = _nums(name, space)
    S = _bounds(nums, space)
    total = int(S[-1])
    if name == "g" or total == 0:
        glob = np.zeros(0, np.int64)
    elif name == "h":
        glob = np.arange(total)
    else:
        has = S[1:] > S[:-1]
        cuts = np.arange(TILE, total + 1, TILE)
        near = (cuts[:, None] + np.arange(-2, 2)[None, :]).ravel()
        rng = np.random.default_rng(sum(map(ord, name)) + 2 * space[0] + space[1])
        glob = np.concatenate([S[:-1][has], S[1:][has] - 1, near, [0, 1],
                               rng.choice(total, min(total, 300), replace=False)])
        glob = np.unique(glob[(glob >= 0) & (glob < total)])
    return nums, [glob[(glob >= S[g]) & (glob < S[g + 1])] - S[g] for g in range(len(nums))]


@pytest.mark.parametrize("directed,loops", SPACES)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 64])
def test_reference_alphabet_matches_oracle(n, directed, loops):
    want = orc.all_edge_indices(n, directed, loops)
    got = _alphabet(n, directed, loops)
    assert got.shape == (len(want), 2)
    assert [tuple(map(int, e)) for e in got] == want
    assert [tuple(map(int, e)) for e in _by_index(got)] == sorted(want)
    assert _lib_alen(n, directed, loops) == len(want) == _alen(n, directed, loops)


def test_layouts_sit_on_the_tile_grid():
    """The shapes the GPU cases rely on, asserted where no GPU is needed."""
    assert CASE_A[UND] == [128, 11, 4, 3, 0, 1]
    for sp in SPACES:
        nums = CASE_A[sp]
        S = _bounds(nums, sp)
        assert [_lib_alen(n, *sp) for n in nums] == list(np.diff(S))
        assert S[-1] == 2 * TILE and S[0] < TILE < S[1]  # two full tiles, graph 0 spans the boundary
        assert S[-3] == S[-2] == S[-1] == 2 * TILE and all(S[g + 1] > S[g] for g in range(len(nums) - 2))
    assert list(_bounds(LAYOUTS[("b", DL)], DL)) == [0, TILE, TILE, TILE]
    S = _bounds(LAYOUTS[("c", UND)], UND)
    assert list(S) == [0, 4095, 4096, 4096, 4096, 4096, 8191, 8201]
    S = _bounds(LAYOUTS[("c", DL)], DL)
    assert list(S[4:10]) == [4095, 4096, 4096, 4096, 4096, 8192]
    assert list(_bounds(LAYOUTS[("d", UND)], UND)) == [0, 0, 0, 0, 8128, 8131]
    for sp in (UND, DL):
        S = _bounds(LAYOUTS[("e", sp)], sp)
        assert 0 < S[1] < TILE < S[2] < 2 * TILE and S[1] % TILE and S[2] % TILE
        local = _layout("e", sp)[1]
        assert len(local[0]) > 2 and (local[1] >= TILE - S[1]).sum() > 2  # set slots for the partial-tile loops
    assert _bounds(LAYOUTS[("f", UND)], UND)[-1] == 0
    assert all(_lib_alen(*sp) == L for sp, L in GRID_SPACES.items())
    assert GRID_SPACES[(7, False, False)] % 16 and GRID_SPACES[(16, True, False)] % 16 == 0  # both last-word paths


# ---------------------------------------------------------------- 1. the compaction alone (GPU)
GUARD = 8  # rows past cap, which no call may touch
SENTINEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _dense_to_edges(g, space, dense, cap):
    """ans_dev_dense_to_edges on a host dense vector.  The 16 bytes after it are set, so a last
    word read past the alphabet is counted and shows.  -> (status, status word, count, edge rows)"""
    import torch
    n, directed, loops = space
    buf = np.ones(len(dense) + 16, np.uint8)
    buf[:len(dense)] = dense
    d_dense = torch.from_numpy(buf).cuda()
    d_edges = torch.full((cap + GUARD, 2), -1, dtype=torch.int32, device="cuda")
    d_count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    A._check(A.lib().ans_dev_dense_to_edges(g.h, n, int(directed), int(loops), d_dense.data_ptr(), d_edges.data_ptr(),
                                            cap, d_count.data_ptr(), d_status.data_ptr(), None), "dense_to_edges")
    st = g.status(d_status)  # waits for the context's stream
    word = int(d_status.cpu().numpy().view(np.uint32)[0])
    return st, word, int(d_count.cpu().numpy()[0]), d_edges.cpu().numpy().view(np.uint32)


def _edges_to_dense(g, space, edges):
    """ans_dev_edges_to_dense -> (status, the dense vector); nothing past the alphabet is written."""
    import torch
    n, directed, loops = space
    L = _alen(*space)
    e = np.ascontiguousarray(edges, dtype=np.uint32).reshape(-1, 2)
    d_edges = torch.from_numpy(e.view(np.int32)).cuda()
    d_dense = torch.full((L + 16,), 7, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    A._check(A.lib().ans_dev_edges_to_dense(g.h, n, int(directed), int(loops), d_edges.data_ptr() if len(e) else None,
                                            len(e), d_dense.data_ptr(), d_status.data_ptr(), None), "edges_to_dense")
    st = g.status(d_status)
    out = d_dense.cpu().numpy()
    assert (out[L:] == 7).all()
    return st, out[:L]


def _indicator(L, slots):
    d = np.zeros(L, np.uint8)
    d[slots] = 1
    return d


def _patterns(L):
    none = np.zeros(0, np.int64)
    tiles = np.arange(0, L, TILE)
    waves = (tiles[:, None] + np.asarray([1023, 1024, 2047, 2048, 3071, 3072])[None, :]).ravel()
    return {"none": none, "all": np.arange(L), "slot_0": np.asarray([0]), "slot_last": np.asarray([L - 1]),
            "tile_first": tiles, "tile_last": np.minimum(tiles + TILE, L) - 1, "wave_edges": waves[waves < L]}


def _check_exact(g, space, slots):
    """cap == count: every edge right, no ANS_E_LEN, nothing past cap; and the way back."""
    L = _alen(*space)
    ref = _alphabet(*space) if L > (1 << 20) else _alpha(*space)
    dense = _indicator(L, slots)
    st, word, count, rows = _dense_to_edges(g, space, dense, len(slots))
    assert (st, word, count) == (A.ANS_OK, 0, len(slots))
    assert np.array_equal(rows[:count], ref[slots])
    assert (rows[count:] == SENTINEL).all()
    st, back = _edges_to_dense(g, space, rows[:count])
    assert st == A.ANS_OK
    assert back.tobytes() == dense.tobytes()


# (n, directed, loops) -> alphabet length; the first four sit on the tile grid, 21 and 4225 end in
# a partial 16-byte word, 240 and 16384 in a full one
GRID_SPACES = {(91, False, False): 4095, (64, True, True): 4096, (65, True, True): 4225, (128, True, True): 16384,
               (7, False, False): 21, (16, True, False): 240, (10, False, True): 55, (130, False, False): 8385}


@pytest.mark.gpu
@pytest.mark.parametrize("space", list(GRID_SPACES), ids=lambda s: f"n{s[0]}-d{int(s[1])}-l{int(s[2])}")
def test_gpu_compaction_patterns(gpu, space):
    L = GRID_SPACES[space]
    assert _lib_alen(*space) == L
    for name, slots in _patterns(L).items():
        try:
            _check_exact(gpu, space, slots)
        except AssertionError as e:
            raise AssertionError(f"pattern {name}") from e


@pytest.mark.gpu
@pytest.mark.parametrize("space", list(GRID_SPACES), ids=lambda s: f"n{s[0]}-d{int(s[1])}-l{int(s[2])}")
def test_gpu_compaction_cap(gpu, space):
    """One short of the count, and none at all: ANS_E_LEN, the true count, the first cap edges and
    nothing past them."""
    L = GRID_SPACES[space]
    ref = _alpha(*space)
    for name, slots in _patterns(L).items():
        if len(slots) == 0:
            continue
        dense = _indicator(L, slots)
        for cap in sorted({len(slots) - 1, 0}):
            st, word, count, rows = _dense_to_edges(gpu, space, dense, cap)
            assert st == A.ANS_E_LEN and word & (1 << A.ANS_E_LEN), (name, cap, st, word)
            assert count == len(slots), (name, cap)
            assert np.array_equal(rows[:cap], ref[slots[:cap]]), (name, cap)
            assert (rows[cap:] == SENTINEL).all(), (name, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("directed,loops", SPACES)
def test_gpu_slot_edge_triangular_boundaries(gpu, directed, loops):
    """slot_edge's square root at its rounding edges: for every b in 2..n-1 the last pair of
    column b - 1 and the first of column b (pair indices b(b-1)/2 - 1 and b(b-1)/2), both
    orientations when directed, and the first and last loop."""
    n = 3000
    b = np.arange(2, n, dtype=np.int64)
    tri = b * (b - 1) // 2
    pair = np.unique(np.concatenate([tri - 1, tri]))
    base = n if loops else 0
    slots = base + (np.concatenate([2 * pair, 2 * pair + 1]) if directed else pair)
    if loops:
        slots = np.concatenate([[0, n - 1], slots])
    slots = np.unique(slots)
    assert slots[-1] < _lib_alen(n, directed, loops) <= 9_003_000
    _check_exact(gpu, (n, directed, loops), slots)


# ---------------------------------------------------------------- 2. dataset layouts (GPU)
def _expected_offsets(local):
    return np.concatenate([[0], np.cumsum([len(p) for p in local])]).astype(np.uint64)


DENSE_SETS_CASES = ([("a", sp) for sp in SPACES] + [("b", DL), ("c", UND), ("c", DL), ("d", UND), ("e", UND),
                                                    ("e", DL), ("f", UND), ("g", UND), ("h", UND), ("h", DL)])


def _case_id(c):
    return f"{c[0]}-d{int(c[1][0])}-l{int(c[1][1])}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", DENSE_SETS_CASES, ids=_case_id)
def test_gpu_dense_sets_layouts(gpu, case):
    name, space = case
    nums, local = _layout(name, space)
    want_edges = [_alpha(n, *space)[p] for n, p in zip(nums, local)]  # alphabet order
    want_eo = _expected_offsets(local)
    ds = A.GpuDenseSets(gpu, A.Bernoulli(MASS, NORM), *space)
    data, offsets, lens = ds.encode(nums, [e[::-1] for e in want_edges])  # a set: any order in
    assert len(lens) == len(nums)
    for g, (n, e) in enumerate(zip(nums, want_edges)):
        dense = orc.dense_set(e, n, *space)
        assert np.array_equal(np.flatnonzero(dense), local[g]), g  # the oracle's slots are the reference's
        od, _, _ = orc.encode_chunks(BERN, dense, max(len(dense), 1))
        want = od.tobytes() if len(dense) else bytes(orc.Message.zeros().flatten())
        assert data[int(offsets[g]):int(offsets[g] + lens[g])].tobytes() == want, g
    back, eo = ds.decode(nums, data, offsets, lens, cap=int(want_eo[-1]), return_offsets=True)  # the exact count
    assert eo.tolist() == want_eo.tolist()
    for g, e in enumerate(want_edges):
        assert np.array_equal(back[g], e), g


def _labelled_graphs(nums, local, space, order):
    """Per graph (n, node labels, edges in the given input order, edge labels); labels are
    functions of the node / edge they belong to, so they can be recomputed after decoding."""
    rng = np.random.default_rng(97)
    graphs = []
    for g, (n, p) in enumerate(zip(nums, local)):
        e = _by_index(_alpha(n, *space)[p])
        e = e[::-1] if order == "descending" else e[rng.permutation(len(e))]
        graphs.append((n, _node_labels(n, g), np.ascontiguousarray(e), _edge_labels(e)))
    return graphs


def _node_labels(n, g):
    return ((7 * np.arange(n, dtype=np.int64) + g) % NLAB).astype(np.uint32)


def _edge_labels(e):
    return ((31 * e[:, 0].astype(np.int64) + 17 * e[:, 1].astype(np.int64)) % NLAB).astype(np.uint32)


GRAPHS_CASES = [("a", sp) for sp in SPACES] + [(name, sp) for name in "ceh" for sp in (UND, DL)]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["descending", "shuffled"])
@pytest.mark.parametrize("case", GRAPHS_CASES, ids=_case_id)
def test_gpu_graphs_layouts_with_labels(gpu, case, order):
    name, space = case
    nums, local = _layout(name, space)
    graphs = _labelled_graphs(nums, local, space, order)
    want_eo = _expected_offsets(local)
    gg = A.GpuGraphs(gpu, A.Bernoulli(MASS, NORM), A.Uniform(NLAB), A.Uniform(NLAB), *space)
    data, offsets, lens = gg.encode(graphs)
    assert len(lens) == len(nums)
    for k, g in enumerate(graphs):
        got = data[int(offsets[k]):int(offsets[k] + lens[k])].tobytes()
        assert got == _oracle_stream(g, BERN, ("uniform", NLAB), ("uniform", NLAB), *space), k
    back, eo = gg.decode(nums, data, offsets, lens, cap=int(want_eo[-1]), return_offsets=True)  # the exact count
    assert eo.tolist() == want_eo.tolist()
    for k, (n, p) in enumerate(zip(nums, local)):
        bn, be, bl = back[k]
        e = _by_index(_alpha(n, *space)[p])
        assert np.array_equal(be, e), k
        assert np.array_equal(bl, _edge_labels(e)), k  # every label beside its own edge
        assert np.array_equal(bn, _node_labels(n, k)), k


# ---------------------------------------------------------------- 3. label list lengths (GPU context only)
@pytest.mark.gpu
def test_gpu_graphs_encode_refuses_wrong_label_lengths(gpu, monkeypatch):
    """ANS_E_ARG before the library is called: it would read num_nodes node labels and one label
    per edge out of whatever it is given."""
    gg = A.GpuGraphs(gpu, A.Bernoulli(MASS, NORM), A.Uniform(NLAB), A.Uniform(NLAB))

    def never(*args):
        raise AssertionError("ans_gpu_graphs_encode was called with short label buffers")

    monkeypatch.setattr(A.lib(), "ans_gpu_graphs_encode", never)
    e = np.asarray([[0, 1], [0, 2], [1, 3]], np.uint32)
    nl, el = np.zeros(4, np.uint32), np.zeros(3, np.uint32)
    for bad in ((4, None, e, el), (4, nl[:3], e, el), (4, nl, e, None), (4, nl, e, el[:2])):
        with pytest.raises(A.AnsError) as err:
            gg.encode([bad])
        assert err.value.code == A.ANS_E_ARG
