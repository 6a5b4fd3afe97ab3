"""Graph shuffle coding with node and edge labels in bulk on the GPU (include/ans_capi.h section 5g:
ans_dev_ar_er_wl_labelled_push / _pop, ans_dev_ar_polya_wl_labelled_push / _pop and the host-buffer
calls): one graph per message, coded onto / from the message already in the graph's slot.  The bytes
after push, the permutation, the popped graph and what remains after pop are compared with the mirror
of tests/labelled_mirror.py; with no label table with the kernels of ans_wl.hip."""
import numpy as np
import pytest

import ans_amd as A

import labelled_mirror as LM
from polya_mirror import complete
from test_gpu_arer import Dev as ArerDev, _seeds, _u32, SMALL
from test_gpu_wl import Dev as WlDev

pytestmark = pytest.mark.gpu

MODELS = ["er", "pu"]
SETTINGS = LM.SETTINGS  # wl_iter 0 .. 3 x the half iteration: each its own size of the sort scratch
SEED = ("seed", _seeds(np.random.default_rng(801), 1)[0])  # not empty: the message is already in the slot


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _cat(masses):
    return A.Categorical(np.asarray(masses, np.uint64)) if masses is not None else None


def _codec(gpu, model, loops, wl_iter, half_iter, node_masses, edge_masses, table=SMALL):
    if model == "er":
        return A.GpuAutoregressiveERLabelled(gpu, A.Bernoulli(*table), loops, wl_iter, half_iter, _cat(node_masses),
                                             _cat(edge_masses))
    return A.GpuAutoregressivePolyaLabelled(gpu, loops, wl_iter, half_iter, _cat(node_masses), _cat(edge_masses))


def _kernel(codec, what):
    model = "arer" if codec.model == "er" else "arpu"
    return (f"k_{model}_wll_{what}(wl_iter={codec.wl_iter},half_iter={codec.half_iter},"
            f"node={int(codec.node_cat is not None)},edge={int(codec.edge_cat is not None)})")


class Dev(ArerDev):
    """test_gpu_arer.Dev with the labels: graphs are (n, node labels or None, [((i, j), label or None)])."""

    def __init__(self, torch, graphs, msgs, cap, max_nodes, pair_caps=None):
        super().__init__(torch, [(n, [e for e, _ in edges]) for n, _, edges in graphs], msgs, cap, max_nodes, pair_caps)
        nl = np.zeros((self.g, max(max_nodes, 1)), np.uint32)
        for c, (n, labels, _) in enumerate(graphs):
            if labels is not None and n <= max_nodes:
                nl[c, :n] = labels
        el = [l if l is not None else 0 for _, _, edges in graphs for _, l in edges] + [0]
        self.d_nl = torch.from_numpy(_u32(nl.reshape(-1))).cuda()
        self.d_el = torch.from_numpy(_u32(el)).cuda()
        self.d_nl_out = torch.full((self.g * max(max_nodes, 1),), -1, dtype=torch.int32, device="cuda")
        self.d_el_out = torch.full((int(self.po[-1]) + 1,), -1, dtype=torch.int32, device="cuda")

    def push(self, codec, max_edges):
        self.status.zero_()
        codec.dev_push(self.g, self.d_nn, self.d_edges, self.d_eo, self.d_nl if codec.node_cat is not None else None,
                       self.d_el if codec.edge_cat is not None else None, self.max_nodes, max_edges, self.d_slots,
                       self.cap, self.d_lens, self.status, self.stream, d_perm=self.d_perm)
        assert codec.gpu.last_launch() == _kernel(codec, "push")
        return codec.gpu.status(self.status, self.stream)

    def pop(self, codec, max_edges):
        self.status.zero_()
        codec.dev_pop(self.g, self.d_nn, self.d_out, self.d_po, self.d_count,
                      self.d_nl_out if codec.node_cat is not None else None,
                      self.d_el_out if codec.edge_cat is not None else None, self.max_nodes, max_edges, self.d_slots,
                      self.cap, self.d_lens, self.status, self.stream)
        assert codec.gpu.last_launch() == _kernel(codec, "pop")
        return codec.gpu.status(self.status, self.stream)

    def popped_graphs(self, nn, nl, el):
        """Per graph (node labels by position or None, [((v, w), label or None)])."""
        pairs, k = self.popped(), self.counts()
        nodes = self.d_nl_out.cpu().numpy().view(np.uint32).reshape(self.g, -1)
        labels = self.d_el_out.cpu().numpy().view(np.uint32)
        out = []
        for c in range(self.g):
            a = int(self.po[c])
            out.append(([int(v) for v in nodes[c, :nn[c]]] if nl else None,
                        [(e, int(labels[a + i]) if el else None) for i, e in enumerate(pairs[c])]))
        return out


def _batches(nl, el):
    """The shapes of a label setting in batches of one launch: by `loops` and by their tables."""
    out = {}
    for s in LM.shapes_of(nl, el):
        out.setdefault((s[4], repr(s[5])), []).append(s)
    return [(loops, shapes[0][5], shapes) for (loops, _), shapes in out.items()]


# ---- 1: every shape against the mirror, the message already in the slot
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("wl_iter,half_iter", SETTINGS)
@pytest.mark.parametrize("nl,el", LM.LABELS[:3])
def test_case1_bytes_equal_the_mirror(gpu, model, wl_iter, half_iter, nl, el):
    torch = pytest.importorskip("torch")
    want = LM.expected(model, wl_iter, half_iter, nl, el, (SEED,))
    for loops, (node_masses, edge_masses), shapes in _batches(nl, el):
        graphs = [(n, labels, edges) for _, n, labels, edges, _, _ in shapes]
        w = [want[s[0], "seed"] for s in shapes]
        max_nodes, max_edges = 32, 80
        codec = _codec(gpu, model, loops, wl_iter, half_iter, node_masses, edge_masses)
        d = Dev(torch, graphs, [SEED[1]] * len(graphs), len(SEED[1]) + codec.slack(max_nodes, max_edges), max_nodes)
        assert d.push(codec, max_edges) == A.ANS_OK
        got = d.messages()
        for c, s in enumerate(shapes):
            assert got[c] == w[c][0], f"push, {s[0]}: length {len(got[c])}, want {len(w[c][0])}"
        assert d.perms([g[0] for g in graphs]) == [x[1] for x in w]
        assert d.pop(codec, max_edges) == A.ANS_OK
        got, popped = d.messages(), d.popped_graphs([g[0] for g in graphs], nl, el)
        for c, s in enumerate(shapes):
            assert popped[c] == (w[c][2], w[c][3]), f"pop, {s[0]}"
            assert got[c] == w[c][4], f"what remains, {s[0]}"
        assert (d.d_out.cpu().numpy()[2 * int(d.po[-1]):] == -1).all() and int(d.d_el_out.cpu()[-1]) == -1


@pytest.mark.parametrize("model", MODELS)
def test_case1_host_buffers(gpu, model):
    pytest.importorskip("torch")
    wl_iter, half_iter = 1, True
    want = LM.expected(model, wl_iter, half_iter, True, True, (SEED,))
    for loops, (node_masses, edge_masses), shapes in _batches(True, True):
        codec = _codec(gpu, model, loops, wl_iter, half_iter, node_masses, edge_masses)
        lens = np.full(len(shapes), len(SEED[1]), np.uint64)
        offsets = (np.arange(len(shapes)) * len(SEED[1])).astype(np.uint64)
        perms, (data, offs, ln) = codec.push_graphs([A.Graph(labels, edges) for _, _, labels, edges, _, _ in shapes],
                                                    np.frombuffer(SEED[1] * len(shapes), np.uint8), offsets, lens)
        for c, s in enumerate(shapes):
            assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[s[0], "seed"][0], f"push, {s[0]}"
            assert list(perms[c]) == want[s[0], "seed"][1], f"perm, {s[0]}"
        graphs, (data, offs, ln) = codec.pop_graphs([s[1] for s in shapes], data, offs, ln)
        for c, s in enumerate(shapes):
            assert (list(graphs[c].node_labels), graphs[c].edges) == want[s[0], "seed"][2:4], f"pop, {s[0]}"
            assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[s[0], "seed"][4], f"what remains, {s[0]}"


# ---- 2: without a table the slots, lens and perm of the kernels of ans_wl.hip, byte for byte
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("wl_iter,half_iter", [(0, True), (0, False), (1, True), (2, False), (3, True)])
def test_case2_without_tables_equals_the_wl_kernels(gpu, model, wl_iter, half_iter):
    torch = pytest.importorskip("torch")
    for loops in (False, True):
        shapes = [s for s in LM.shapes_of(True, True) if s[4] == loops]
        graphs = [(n, None, [(e, None) for e, _ in edges]) for _, n, _, edges, _, _ in shapes]
        seeds = _seeds(np.random.default_rng(802), len(graphs))
        new = _codec(gpu, model, loops, wl_iter, half_iter, None, None)
        old = A.GpuAutoregressiveERWL(gpu, A.Bernoulli(*SMALL), loops, wl_iter, half_iter) if model == "er" \
            else A.GpuAutoregressivePolyaWL(gpu, loops, wl_iter, half_iter)
        cap = len(seeds[0]) + new.slack(32, 80)
        assert new.slack(32, 80) >= (old.slack(32) if model == "er" else old.slack(32, 80))
        a, b = Dev(torch, graphs, seeds, cap, 32), WlDev(torch, [(n, [e for e, _ in edges]) for n, _, edges in graphs], seeds, cap, 32)
        assert a.push(new, 80) == A.ANS_OK and b.push(old, 80) == A.ANS_OK
        assert torch.equal(a.d_lens, b.d_lens) and a.messages() == b.messages() and torch.equal(a.d_perm, b.d_perm)
        assert all(a.lens() > 0)
        assert a.pop(new, 80) == A.ANS_OK and b.pop(old, 80) == A.ANS_OK
        assert torch.equal(a.d_lens, b.d_lens) and a.messages() == b.messages() and torch.equal(a.d_count, b.d_count)
        # the pairs are equal once each node's slice is sorted (a labelled pop gives the loop first)
        assert a.popped() == [sorted(p) for p in b.popped()]


# ---- 3: a failing graph between good ones
@pytest.mark.parametrize("model", MODELS)
def test_case3_a_failing_graph_between_good_ones(gpu, model):
    torch = pytest.importorskip("torch")
    name, n, labels, edges, loops, (node_masses, edge_masses) = [s for s in LM.shapes() if s[0] == "random 0"][0]
    good = (n, labels, edges)
    mirror = LM.mirror_of(model, n, loops, 1, True, node_masses, edge_masses)
    pushed, perm = mirror.push_bytes(SEED[1], labels, edges)
    popped_nodes, popped_edges, rest = mirror.pop_bytes(pushed)
    codec = _codec(gpu, model, loops, 1, True, node_masses, edge_masses)
    cap = len(SEED[1]) + codec.slack(16, 40)
    seeds = [SEED[1]] * 3

    def push_fails(bad, code):
        d = Dev(torch, [good, bad, good], seeds, cap, 16)
        assert d.push(codec, 40) == code and d.lens()[1] == 0
        assert d.messages() == [pushed, b"", pushed]
        assert d.perms([n, 0, n])[0] == perm

    push_fails((n, [7] + labels[1:], edges), A.ANS_E_SYMBOL)             # a node label outside its table
    push_fails((n, labels, [(edges[0][0], 4)] + edges[1:]), A.ANS_E_SYMBOL)  # an edge label outside its table
    push_fails((n, [4] + labels[1:], edges), A.ANS_E_ZERO_MASS)          # labels of mass 0
    push_fails((n, labels, edges[:-1] + [(edges[-1][0], 2)]), A.ANS_E_ZERO_MASS)
    push_fails((17, [0] * 17, []), A.ANS_E_ARG)                          # more nodes than max_nodes
    # a stream cut to 2 bytes
    d = Dev(torch, [good] * 3, [pushed, pushed[:2], pushed], cap, 16)
    assert d.pop(codec, 40) == A.ANS_E_EXHAUSTED and d.lens()[1] == 0 and d.counts()[1] == 0
    assert d.messages() == [rest, b"", rest]
    got = d.popped_graphs([n] * 3, True, True)
    assert got[0] == got[2] == (popped_nodes, popped_edges) and got[1][1] == []
    # a pop capacity one short
    d = Dev(torch, [good] * 3, [pushed] * 3, cap, 16, pair_caps=[len(edges), len(edges) - 1, len(edges)])
    assert d.pop(codec, 40) == A.ANS_E_LEN and d.lens()[1] == 0 and d.counts()[1] == 0
    assert d.messages() == [rest, b"", rest]
    got = d.popped_graphs([n] * 3, True, True)
    assert got[0] == got[2] == (popped_nodes, popped_edges)
    # a table without its array: before any launch
    d = Dev(torch, [good] * 3, seeds, cap, 16)
    with pytest.raises(A.AnsError) as e:
        codec.dev_push(d.g, d.d_nn, d.d_edges, d.d_eo, None, d.d_el, 16, 40, d.d_slots, d.cap, d.d_lens, d.status, d.stream)
    assert e.value.code == A.ANS_E_ARG and d.messages() == seeds


# ---- 4: the slack holds the worst graphs: every label the table's rarest
@pytest.mark.parametrize("model", MODELS)
def test_case4_slack_holds_the_worst_graphs(gpu, model):
    torch = pytest.importorskip("torch")
    n = 40
    rare_node, rare_edge = len(LM.NODE_MASSES) - 1, len(LM.EDGE_MASSES) - 1
    assert LM.NODE_MASSES[rare_node] == min(p for p in LM.NODE_MASSES if p) and LM.EDGE_MASSES[rare_edge] == min(p for p in LM.EDGE_MASSES if p)
    for pairs in (complete(n), []):
        graph = (n, [rare_node] * n, [(e, rare_edge) for e in pairs])
        codec = _codec(gpu, model, False, 1, True, LM.NODE_MASSES, LM.EDGE_MASSES)
        seeds = _seeds(np.random.default_rng(806), 2, 16)
        slack = codec.slack(n, len(pairs))
        d = Dev(torch, [graph] * 2, seeds, 16 + slack, n)
        assert d.push(codec, len(pairs)) == A.ANS_OK
        grown = d.lens().copy()
        assert all(grown > 16)
        pushed = d.messages()
        d2 = Dev(torch, [graph] * 2, pushed, int(grown.max()) + slack, n)
        assert d2.pop(codec, len(pairs)) == A.ANS_OK and d2.messages() == seeds
        assert [int(c) for c in d2.counts()] == [len(pairs)] * 2
        d3 = Dev(torch, [graph] * 2, seeds, int(grown.max()) - 1, n)
        assert d3.push(codec, len(pairs)) == A.ANS_E_LEN
        assert all(ln == 0 for ln, g in zip(d3.lens(), grown) if g == grown.max())
