"""The Pólya urn edge-index codec in bulk on the GPU (include/ans_capi.h section 5c:
ans_dev_polya_push / _pop and the ans_gpu_polya_*_graphs host-buffer calls): one graph per message,
coded onto / from the message already in the graph's slot.  Every case compares every graph's bytes
after push with the mirror of tests/polya_mirror.py, the popped edges with the mirror's, and what
remains after pop with the mirror's (the seed message)."""
import functools

import numpy as np
import pytest

import ans_amd as A

import polya_mirror as PM

pytestmark = pytest.mark.gpu

LT, LF = True, False


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _seeds(rng, count, nbytes=64):
    s = rng.integers(0, 256, (count, nbytes), dtype=np.uint8)
    s[:, -1] = rng.integers(1, 256, count)  # a nonzero top byte: the seed comes back byte for byte
    return [row.tobytes() for row in s]


def _expect(n, edges, seed, loops, redraws):
    """(bytes after push, edges as pop returns them, bytes after pop) of one graph."""
    mirror = PM.Mirror(n, loops, redraws)
    pushed = mirror.push_bytes(seed, edges)
    popped, rest = mirror.pop_bytes(pushed, len(edges))
    assert sorted(popped) == sorted(edges)
    return pushed, popped, rest


def _u32(t):
    return np.ascontiguousarray(t, dtype=np.uint32).view(np.int32)


class Dev:
    """The graphs and their slots on the device."""

    def __init__(self, torch, nn, edge_lists, seeds, cap):
        self.torch, self.cap, self.g = torch, cap, len(nn)
        eo = np.zeros(len(nn) + 1, np.uint64)
        np.cumsum([len(e) for e in edge_lists], out=eo[1:])
        self.eo = eo
        flat = [p for e in edge_lists for p in e] or [(0, 0)]
        self.d_nn = torch.from_numpy(_u32(nn)).cuda()
        self.d_edges = torch.from_numpy(_u32(flat).reshape(-1)).cuda()
        self.d_eo = torch.from_numpy(eo.view(np.int64)).cuda()
        h = np.zeros((self.g, cap), np.uint8)
        for c, b in enumerate(seeds):
            h[c, :len(b)] = np.frombuffer(b, np.uint8)
        self.d_slots = torch.from_numpy(h.reshape(-1)).cuda()
        self.d_lens = torch.from_numpy(_u32([len(b) for b in seeds])).cuda()
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.Stream()

    def lens(self):
        return self.d_lens.cpu().numpy().view(np.uint32)

    def messages(self):
        h, ln = self.d_slots.cpu().numpy().reshape(-1, self.cap), self.lens()
        return [bytes(h[c, :ln[c]]) for c in range(self.g)]

    def edges_of(self, d_out):
        e = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
        return [[(int(i), int(j)) for i, j in e[int(self.eo[c]):int(self.eo[c + 1])]] for c in range(self.g)]


def _dev_roundtrip(torch, gpu, loops, redraws, nn, edge_lists, seeds, want, max_nodes=None, max_edges=None):
    """ans_dev_polya_push then ans_dev_polya_pop on device slots against `want`."""
    max_nodes = max_nodes or max(nn)
    max_edges = max_edges if max_edges is not None else max(len(e) for e in edge_lists)
    cap = max(len(s) for s in seeds) + A.GpuPolyaUrn.slack(max_nodes, max_edges)
    codec = A.GpuPolyaUrn(gpu, loops, redraws)
    d = Dev(torch, nn, edge_lists, seeds, cap)
    codec.dev_push(d.g, d.d_nn, d.d_edges, d.d_eo, max_nodes, max_edges, d.d_slots, cap, d.d_lens, d.status, d.stream)
    assert gpu.last_launch() == f"k_polya_push<redraws={int(redraws)}>"
    assert gpu.status(d.status, d.stream) == A.ANS_OK
    got = d.messages()
    for c in range(d.g):
        assert got[c] == want[c][0], f"push, graph {c}: length {len(got[c])}, want {len(want[c][0])}"
    d_out = torch.zeros_like(d.d_edges)
    codec.dev_pop(d.g, d.d_nn, d_out, d.d_eo, max_nodes, max_edges, d.d_slots, cap, d.d_lens, d.status, d.stream)
    assert gpu.last_launch() == f"k_polya_pop<redraws={int(redraws)}>"
    assert gpu.status(d.status, d.stream) == A.ANS_OK
    got, edges = d.messages(), d.edges_of(d_out)
    for c in range(d.g):
        assert edges[c] == want[c][1], f"pop, graph {c}"
        assert got[c] == want[c][2], f"what remains, graph {c}"
        if edge_lists[c]:
            assert got[c] == seeds[c], f"seed, graph {c}"
        else:  # no edges: each call is flatten(unflatten(B)) = B ++ [0]
            assert got[c] == seeds[c] + bytes(2), f"seed, graph {c}"


def _check(torch, gpu, loops, redraws, graphs, seed=1, **kw):
    nn = [n for n, _ in graphs]
    edge_lists = [e for _, e in graphs]
    seeds = _seeds(np.random.default_rng(seed), len(graphs))
    want = [_expect(n, e, s, loops, redraws) for (n, e), s in zip(graphs, seeds)]
    _dev_roundtrip(torch, gpu, loops, redraws, nn, edge_lists, seeds, want, **kw)
    return nn, edge_lists, seeds, want


# ---- 1: across the plain / joint switch, and the empty graph
@pytest.mark.parametrize("loops,redraws", [(LT, LT), (LF, LF)])
def test_case1_edge_counts_across_the_switch(gpu, loops, redraws):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(201)
    graphs = [(6, PM.random_graph(rng, 6, num_edges)) for num_edges in (0, 1, 2, 11, 12, 13)]
    _check(torch, gpu, loops, redraws, graphs)


# ---- 2: the i == j branch of the per-edge shuffle
def test_case2_loops(gpu):
    torch = pytest.importorskip("torch")
    _check(torch, gpu, LT, LT, [(1, [(0, 0)]), (2, [(0, 0), (0, 1), (1, 1)])])
    _check(torch, gpu, LT, LF, [(1, [(0, 0)]), (2, [(1, 1), (0, 0), (0, 1)])])


# ---- 3: the norms go down to 1
def test_case3_complete_graphs_without_redraws(gpu):
    torch = pytest.importorskip("torch")
    _check(torch, gpu, LF, LF, [(5, PM.complete(5)), (6, PM.complete(6))])


# ---- 4: a long exclusion list; Fenwick sizes that are no powers of two
@pytest.mark.parametrize("loops,redraws", [(LF, LF), (LT, LF)])
def test_case4_star_and_path(gpu, loops, redraws):
    torch = pytest.importorskip("torch")
    star = [(0, v) for v in range(1, 40)]
    path = [(v, v + 1) for v in range(32)]
    _check(torch, gpu, loops, redraws, [(40, star), (33, path)])


# ---- 5: rank / select and swaps at depth
def test_case5_a_thousand_edges(gpu):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(205)
    edges = PM.random_graph(rng, 300, 1000)
    seeds = _seeds(rng, 1, 2048)  # the orbit pops take log2(1000!) + 1000 bits out before any push
    want = [_expect(300, edges, seeds[0], LF, LF)]
    _dev_roundtrip(torch, gpu, LF, LF, [300], [edges], seeds, want)


# ---- 6: many graphs in one call
@functools.lru_cache(maxsize=None)
def _mixed():
    rng = np.random.default_rng(206)
    graphs = []
    for _ in range(200):
        n = int(rng.integers(1, 51))
        graphs.append((n, PM.random_graph(rng, n, int(rng.integers(0, min(60, n * (n - 1) // 2) + 1)))))
    seeds = _seeds(rng, 200, 96)
    want = [_expect(n, e, s, LF, LF) for (n, e), s in zip(graphs, seeds)]
    return graphs, seeds, want


def test_case6_mixed_graphs_device_call(gpu):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _mixed()
    _dev_roundtrip(torch, gpu, LF, LF, [n for n, _ in graphs], [e for _, e in graphs], seeds, want,
                   max_nodes=64, max_edges=100)


def test_case6_mixed_graphs_host_buffers(gpu):
    pytest.importorskip("torch")
    graphs, seeds, want = _mixed()
    nn, lists = [n for n, _ in graphs], [e for _, e in graphs]
    codec = A.GpuPolyaUrn(gpu, LF, LF)
    lens = np.array([len(s) for s in seeds], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    data, offs, ln = codec.push_graphs(nn, lists, np.frombuffer(b"".join(seeds), np.uint8), offsets, lens)
    for c in range(len(graphs)):
        assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[c][0], f"push, graph {c}"
    edges, (data, offs, ln) = codec.pop_graphs(nn, [len(e) for e in lists], data, offs, ln)
    for c in range(len(graphs)):
        assert [(int(i), int(j)) for i, j in edges[c]] == want[c][1], f"pop, graph {c}"
        assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[c][2], f"what remains, graph {c}"


def test_case6_more_graphs_than_resident_lanes(gpu):
    """n = 3, E = 2, 140,000 graphs: above the 256 CUs x 8 waves x 64 lanes the launch keeps
    resident, so the grid-stride wraps and a lane's state is reused.  A 1-in-997 sample, the first
    and the last graph against the mirror; every graph round-trips."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(207)
    count, nbytes = 140000, 16
    pairs = np.array([(0, 1), (0, 2), (1, 2)], np.uint32)
    order = np.argsort(rng.random((count, 3)), axis=1)[:, :2]  # two of the three pairs, in random order
    edges = pairs[order]  # (count, 2, 2)
    seeds = rng.integers(0, 256, (count, nbytes), dtype=np.uint8)
    seeds[:, -1] = rng.integers(1, 256, count)
    cap = nbytes + A.GpuPolyaUrn.slack(3, 2)
    slots = np.zeros((count, cap), np.uint8)
    slots[:, :nbytes] = seeds
    d_slots = torch.from_numpy(slots.reshape(-1)).cuda()
    d_lens = torch.from_numpy(np.full(count, nbytes, np.int32)).cuda()
    d_nn = torch.from_numpy(np.full(count, 3, np.int32)).cuda()
    d_edges = torch.from_numpy(edges.reshape(-1).view(np.int32)).cuda()
    d_eo = torch.from_numpy(np.arange(0, 2 * count + 1, 2, dtype=np.int64)).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    codec = A.GpuPolyaUrn(gpu, LF, LF)
    codec.dev_push(count, d_nn, d_edges, d_eo, 3, 2, d_slots, cap, d_lens, status, stream)
    assert gpu.status(status, stream) == A.ANS_OK
    h, ln = d_slots.cpu().numpy().reshape(-1, cap), d_lens.cpu().numpy().view(np.uint32)
    for c in sorted(set(range(0, count, 997)) | {0, count - 1}):
        want = PM.Mirror(3, LF, LF).push_bytes(seeds[c].tobytes(), [tuple(int(v) for v in p) for p in edges[c]])
        assert bytes(h[c, :ln[c]]) == want, f"push, graph {c}"
    d_out = torch.zeros_like(d_edges)
    codec.dev_pop(count, d_nn, d_out, d_eo, 3, 2, d_slots, cap, d_lens, status, stream)
    assert gpu.status(status, stream) == A.ANS_OK
    out = d_out.cpu().numpy().view(np.uint32).reshape(count, 2, 2)
    flat = edges.astype(np.int64)[:, :, 0] * 3 + edges[:, :, 1]
    assert np.array_equal(out[:, :, 0].astype(np.int64) * 3 + out[:, :, 1], np.sort(flat, axis=1))  # E <= 11: sorted
    assert np.all(d_lens.cpu().numpy().view(np.uint32) == nbytes)
    assert np.array_equal(d_slots.cpu().numpy().reshape(-1, cap)[:, :nbytes], seeds)


# ---- 7: statuses, graph by graph
def _push_status(torch, gpu, loops, redraws, graphs, seeds, max_nodes, max_edges, cap):
    d = Dev(torch, [n for n, _ in graphs], [e for _, e in graphs], seeds, cap)
    A.GpuPolyaUrn(gpu, loops, redraws).dev_push(d.g, d.d_nn, d.d_edges, d.d_eo, max_nodes, max_edges, d.d_slots, cap,
                                                d.d_lens, d.status, d.stream)
    return gpu.status(d.status, d.stream), d


def test_case7_statuses(gpu):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(208)
    good = (6, PM.random_graph(rng, 6, 9))
    seeds = _seeds(rng, 3)
    want = [_expect(good[0], good[1], s, LT, LT)[0] for s in seeds]
    cap = 64 + A.GpuPolyaUrn.slack(6, 20)

    def others_intact(d, bad):
        got = d.messages()
        for c in range(3):
            assert got[c] == (b"" if c == bad else want[c]), f"graph {c}"

    # a seed too short for the orientation pop: exhausted, that graph alone
    st, d = _push_status(torch, gpu, LT, LT, [good] * 3, [seeds[0], b"\x07", seeds[2]], 6, 20, cap)
    assert st == A.ANS_E_EXHAUSTED and d.lens()[1] == 0
    others_intact(d, 1)
    # ... and on pop
    d2 = Dev(torch, [6] * 3, [good[1]] * 3, [want[0], b"\x07\x07", want[2]], cap)
    d_out = torch.zeros_like(d2.d_edges)
    A.GpuPolyaUrn(gpu, LT, LT).dev_pop(3, d2.d_nn, d_out, d2.d_eo, 6, 20, d2.d_slots, cap, d2.d_lens, d2.status,
                                        d2.stream)
    assert gpu.status(d2.status, d2.stream) == A.ANS_E_EXHAUSTED
    assert d2.lens()[1] == 0 and d2.messages()[0] == seeds[0] and d2.messages()[2] == seeds[2]
    # a slot with the slack holds the result; one a byte short of the result does not
    big = (40, PM.random_graph(rng, 40, 90))
    long_seed = _seeds(rng, 1, 128)[0]  # the orbit pops take log2(90!) + 90 bits out before any push
    grown = _expect(big[0], big[1], long_seed, LT, LT)[0]
    assert len(grown) > len(long_seed)
    st, d = _push_status(torch, gpu, LT, LT, [big], [long_seed], 40, 90, len(long_seed) + A.GpuPolyaUrn.slack(40, 90))
    assert st == A.ANS_OK and d.messages()[0] == grown
    st, d = _push_status(torch, gpu, LT, LT, [big], [long_seed], 40, 90, len(grown) - 1)
    assert st == A.ANS_E_LEN and d.lens()[0] == 0
    # a graph over max_edges (and one over max_nodes)
    seeds3 = [seeds[0], long_seed, seeds[2]]
    st, d = _push_status(torch, gpu, LT, LT, [good, big, good], seeds3, 40, 89, 256)
    assert st == A.ANS_E_ARG and d.lens()[1] == 0
    others_intact(d, 1)
    st, d = _push_status(torch, gpu, LT, LT, [good, big, good], seeds3, 39, 90, 256)
    assert st == A.ANS_E_ARG and d.lens()[1] == 0
    # a pair given twice (on both sides of the switch), i > j, a loop without loops
    twice = (6, good[1] + [good[1][3]])
    many = (6, PM.complete(6) + [(2, 3)])
    for loops, bad in ((LT, twice), (LT, many), (LT, (6, [(0, 1), (3, 2)])), (LF, (6, [(0, 1), (2, 2)])),
                       (LT, (6, [(0, 6)]))):
        ok = _expect(good[0], good[1], seeds[0], loops, LT)[0]
        st, d = _push_status(torch, gpu, loops, LT, [good, bad, good], seeds, 6, 20, cap)
        assert st == A.ANS_E_SYMBOL and d.lens()[1] == 0, bad
        assert d.messages()[0] == ok


# ---- 8: GraphIID<Categorical, Categorical, PolyaUrn> out of three calls on the same messages
def test_case8_composes_into_graph_iid(gpu):
    pytest.importorskip("torch")
    rng = np.random.default_rng(209)
    node_masses = rng.integers(1, 1 << 12, 5).astype(np.uint64)
    edge_masses = rng.integers(1, 1 << 12, 3).astype(np.uint64)
    node_cat, edge_cat = A.Categorical(node_masses), A.Categorical(edge_masses)
    ts = A.GpuTableSet(gpu, [node_cat, edge_cat])
    codec = A.GpuPolyaUrn(gpu, LF, LF)
    graphs = []
    for _ in range(20):
        n = int(rng.integers(2, 12))
        edges = sorted(PM.random_graph(rng, n, int(rng.integers(1, min(20, n * (n - 1) // 2) + 1))))
        graphs.append((n, edges, rng.integers(0, 5, n).astype(np.uint32), rng.integers(0, 3, len(edges)).astype(np.uint32)))
    seeds = _seeds(rng, 20, 96)
    nn, lists = [g[0] for g in graphs], [g[1] for g in graphs]
    node_labels, edge_labels = np.concatenate([g[2] for g in graphs]), np.concatenate([g[3] for g in graphs])
    node_starts = np.concatenate([[0], np.cumsum(nn)]).astype(np.uint64)
    edge_starts = np.concatenate([[0], np.cumsum([len(e) for e in lists])]).astype(np.uint64)
    # the reference's order: edge labels (sorted by edge index), edge indices, node labels
    # (src/graph_codec.rs:31-34, 61-65), on one message per graph
    want = []
    for (n, edges, nl, el), seed in zip(graphs, seeds):
        m = A.Message.unflatten(seed, A.GEN_EMPTY)
        A.IID(edge_cat, len(edges)).push(m, el)
        A.PolyaUrn(n, len(edges), LF, LF).push(m, edges)
        A.IID(node_cat, n).push(m, nl)
        want.append(m.flatten())
    lens = np.array([len(s) for s in seeds], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    box = (np.frombuffer(b"".join(seeds), np.uint8), offsets, lens)
    box = ts.push_var_chunks(np.ones(len(edge_labels), np.uint32), edge_labels, edge_starts, *box)
    box = codec.push_graphs(nn, lists, *box)
    box = ts.push_var_chunks(np.zeros(len(node_labels), np.uint32), node_labels, node_starts, *box)
    for c in range(20):
        assert bytes(box[0][int(box[1][c]):int(box[1][c] + box[2][c])]) == want[c], f"graph {c}"
    # ... and back, in the reverse order
    got_nodes, box = ts.pop_var_chunks(np.zeros(len(node_labels), np.uint32), *box, node_starts)
    got_edges, box = codec.pop_graphs(nn, [len(e) for e in lists], *box)
    got_labels, box = ts.pop_var_chunks(np.ones(len(edge_labels), np.uint32), *box, edge_starts)
    assert np.array_equal(got_nodes, node_labels) and np.array_equal(got_labels, edge_labels)
    for c in range(20):
        assert sorted((int(i), int(j)) for i, j in got_edges[c]) == lists[c], f"edges, graph {c}"
        assert bytes(box[0][int(box[1][c]):int(box[1][c] + box[2][c])]) == seeds[c], f"seed, graph {c}"
