"""Joint shuffle coding of graphs with Weisfeiler-Lehman orbits in bulk on the GPU (include/ans_capi.h
section 5h: ans_dev_joint_er_wl_push / _pop, ans_dev_joint_polya_wl_push / _pop and the *_graphs
host-buffer calls): one graph per message, coded onto / from the message already in the graph's slot.
The bytes after push, the permutation, the popped pairs, their counts and what remains after pop are
compared with the mirror of tests/joint_mirror.py (computed once per setting for the module); at
wl_iter = 0 with the host entries, there being no older kernel.

The seeds are longer than test_gpu_wl's: a joint push pops the whole order of the nodes (and under the
urn that of the pairs) before its ordered codec pushes the first bit, and the slots' tail is Empty."""
import math

import numpy as np
import pytest

import ans_amd as A

import joint_mirror as JM
from polya_mirror import complete, random_graph
from test_gpu_wl import Dev as WlDev, _seeds, HUGE, SMALL

pytestmark = pytest.mark.gpu

MODELS = ["er", "pu"]
SETTINGS = [(w, h) for w in (1, 2) for h in (True, False)]
SEED = ("seed", _seeds(np.random.default_rng(701), 1, 320)[0])  # not empty: the message is already in the slot


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _redraws(model, wl_iter):
    return model == "pu" and wl_iter == 2  # (both settings of redraws are run)


def _want(model, wl_iter, half_iter):
    return JM.expected(model, wl_iter, half_iter, _redraws(model, wl_iter), (SEED,))


def _codec(gpu, model, loops, wl_iter, half_iter, table=SMALL):
    if model == "er":
        return A.GpuJointERWL(gpu, A.Bernoulli(*table), loops, wl_iter, half_iter)
    return A.GpuJointPolyaWL(gpu, loops, _redraws(model, wl_iter), wl_iter, half_iter)


def _host_codec(model, n, loops, wl_iter, half_iter):
    if model == "er":
        return A.JointERWL(A.Bernoulli(*SMALL), n, loops, wl_iter, half_iter)
    return A.JointPolyaWL(n, loops, _redraws(model, wl_iter), wl_iter, half_iter)


def _slack(codec, max_nodes, max_edges):
    return codec.slack(max_nodes) if isinstance(codec, A.GpuJointERWL) else codec.slack(max_nodes, max_edges)


def _kernel(codec, what):
    if isinstance(codec, A.GpuJointERWL):
        return f"k_joint_er_{what}(wl_iter={codec.wl_iter},half_iter={codec.half_iter})"
    return f"k_joint_pu_{what}(wl_iter={codec.wl_iter},half_iter={codec.half_iter},redraws={codec.redraws})"


class Dev(WlDev):
    """test_gpu_wl's device buffers.  A pop's offsets are the graphs' own pair counts unless given: the
    Erdős–Rényi codec's capacities, the urn's parameter."""

    def push(self, codec, max_edges, with_perm=True):
        self.status.zero_()
        codec.dev_push(self.g, self.d_nn, self.d_edges, self.d_eo, self.max_nodes, max_edges, self.d_slots, self.cap,
                       self.d_lens, self.status, self.stream, d_perm=self.d_perm if with_perm else None)
        assert codec.gpu.last_launch() == _kernel(codec, "push")
        return codec.gpu.status(self.status, self.stream)

    def pop(self, codec, max_edges):
        self.status.zero_()
        codec.dev_pop(self.g, self.d_nn, self.d_out, self.d_po, self.d_count, self.max_nodes, max_edges, self.d_slots,
                      self.cap, self.d_lens, self.status, self.stream)
        assert codec.gpu.last_launch() == _kernel(codec, "pop")
        return codec.gpu.status(self.status, self.stream)


def _shapes(loops):
    return [(name, n, edges) for name, n, edges, needs_loops in JM.shapes() if needs_loops == loops]


# ---- 1: every shape against the mirror, the message already in the slot
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("wl_iter,half_iter", SETTINGS)
def test_case1_bytes_equal_the_mirror(gpu, model, wl_iter, half_iter):
    torch = pytest.importorskip("torch")
    want = _want(model, wl_iter, half_iter)
    for loops in (False, True):
        shapes = _shapes(loops)
        graphs = [(n, edges) for _, n, edges in shapes]
        w = [want[name, "seed"] for name, _, _ in shapes]
        max_nodes, max_edges = 64, 200
        codec = _codec(gpu, model, loops, wl_iter, half_iter)
        d = Dev(torch, graphs, [SEED[1]] * len(graphs), len(SEED[1]) + _slack(codec, max_nodes, max_edges), max_nodes)
        assert d.push(codec, max_edges) == A.ANS_OK
        got = d.messages()
        for c, (name, _, _) in enumerate(shapes):
            assert got[c] == w[c][0], f"push, {name}: length {len(got[c])}, want {len(w[c][0])}"
        assert d.perms([n for n, _ in graphs]) == [x[1] for x in w]
        assert d.pop(codec, max_edges) == A.ANS_OK
        got, pairs, counts = d.messages(), d.popped(), d.counts()
        for c, (name, _, edges) in enumerate(shapes):
            assert int(counts[c]) == len(edges), f"d_num_edges, {name}"
            assert pairs[c] == w[c][2], f"pop, {name}"
            assert got[c] == w[c][3], f"what remains, {name}"
        assert (d.d_out.cpu().numpy()[2 * int(d.po[-1]):] == -1).all()


@pytest.mark.parametrize("model", MODELS)
def test_case1_host_buffers(gpu, model):
    pytest.importorskip("torch")
    wl_iter, half_iter = 1, True
    want = _want(model, wl_iter, half_iter)
    for loops in (False, True):
        shapes = _shapes(loops)
        nn, lists = [n for _, n, _ in shapes], [e for _, _, e in shapes]
        codec = _codec(gpu, model, loops, wl_iter, half_iter)
        lens = np.full(len(shapes), len(SEED[1]), np.uint64)
        offsets = (np.arange(len(shapes)) * len(SEED[1])).astype(np.uint64)
        perms, (data, offs, ln) = codec.push_graphs(nn, lists, np.frombuffer(SEED[1] * len(shapes), np.uint8), offsets, lens)
        for c, (name, _, _) in enumerate(shapes):
            assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[name, "seed"][0], f"push, {name}"
            assert list(perms[c]) == want[name, "seed"][1], f"perm, {name}"
        if model == "er":
            pairs, (data, offs, ln) = codec.pop_graphs(nn, data, offs, ln)
        else:
            pairs, (data, offs, ln) = codec.pop_graphs(nn, [len(e) for e in lists], data, offs, ln)
        for c, (name, _, _) in enumerate(shapes):
            assert [(int(i), int(j)) for i, j in pairs[c]] == want[name, "seed"][2], f"pop, {name}"
            assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[name, "seed"][3], f"what remains, {name}"


# ---- 2: at wl_iter = 0 the host entries' bytes
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("half_iter", [True, False])
def test_case2_wl0_equals_the_host_entries(gpu, model, half_iter):
    torch = pytest.importorskip("torch")
    for loops in (False, True):
        shapes = _shapes(loops)
        graphs = [(n, edges) for _, n, edges in shapes]
        seeds = _seeds(np.random.default_rng(702), len(graphs), 320)
        codec = _codec(gpu, model, loops, 0, half_iter)
        d = Dev(torch, graphs, seeds, len(seeds[0]) + _slack(codec, 64, 200), 64)
        assert d.push(codec, 200) == A.ANS_OK
        pushed, perms = d.messages(), d.perms([n for n, _ in graphs])
        assert d.pop(codec, 200) == A.ANS_OK
        rest, pairs = d.messages(), d.popped()
        for c, (name, n, edges) in enumerate(shapes):
            host = _host_codec(model, n, loops, 0, half_iter)
            m = A.Message.unflatten(seeds[c], A.GEN_EMPTY)
            perm = host.push(m, edges)
            assert pushed[c] == m.flatten() and perms[c] == list(perm), f"push, {name}"
            m = A.Message.unflatten(pushed[c], A.GEN_EMPTY)
            got = host.pop(m) if model == "er" else host.pop(m, len(edges))
            assert pairs[c] == got and rest[c] == m.flatten(), f"pop, {name}"


# ---- 3: slots of exactly d_lens + slack hold the worst graphs
def _slack_case(torch, codec, n, edges):
    """Slots of exactly d_lens + slack for the push, then for the pop; then a slot one byte shorter than
    the result: ANS_E_LEN for that slot, as a status.  The seed holds the bits the push pops before it
    pushes any: the order of the nodes and, under the urn, of the pairs (log2 n! + log2 E! bits)."""
    E = len(edges)
    need = (math.lgamma(n + 1) + (0 if isinstance(codec, A.GpuJointERWL) else math.lgamma(E + 1))) / math.log(2) / 8
    nbytes = int(need) + 32
    seeds = _seeds(np.random.default_rng(706), 2, nbytes)
    slack = _slack(codec, n, E)
    d = Dev(torch, [(n, edges)] * 2, seeds, nbytes + slack, n)
    assert d.push(codec, E) == A.ANS_OK
    grown = d.lens().copy()
    assert all(grown > 0)
    pushed = d.messages()
    d2 = Dev(torch, [(n, edges)] * 2, pushed, int(grown.max()) + slack, n)
    assert d2.pop(codec, E) == A.ANS_OK and d2.messages() == seeds
    assert [int(c) for c in d2.counts()] == [E] * 2
    if int(grown.max()) > nbytes:
        d3 = Dev(torch, [(n, edges)] * 2, seeds, int(grown.max()) - 1, n)
        assert d3.push(codec, E) == A.ANS_E_LEN
        assert all(ln == 0 for ln, g in zip(d3.lens(), grown) if g == grown.max())
        assert all(ln == g for ln, g in zip(d3.lens(), grown) if g < grown.max())
    return int(grown.max()) > nbytes


@pytest.mark.parametrize("table,loops", [(SMALL, True), ((900, 1000), False), (HUGE, True), (((1 << 55) + 3, (1 << 56) - 1), True)])
def test_case3_er_slack_holds_the_worst_graph(gpu, table, loops):
    """The worst graph of tests/test_gpu_wl.py case 3: complete (with every loop) when an edge is the
    rarer symbol, empty otherwise."""
    torch = pytest.importorskip("torch")
    n = 40
    rare_edge = table[0] * 2 < table[1]
    edges = [(i, j) for j in range(n) for i in range(j + 1 if loops else j)] if rare_edge else []
    assert _slack_case(torch, _codec(gpu, "er", loops, 1, True, table), n, edges)  # (both grow: the short slot was run)


@pytest.mark.parametrize("loops", [False, True])
def test_case3_polya_slack_holds_the_worst_graph(gpu, loops):
    torch = pytest.importorskip("torch")
    n = 40
    grew = [_slack_case(torch, _codec(gpu, "pu", loops, 1, True), n, edges)
            for edges in (complete(n) + ([(v, v) for v in range(n)] if loops else []), [])]
    assert grew == [True, False]  # (an empty graph pushes nothing: its message only shrinks)


# ---- 4: a failing graph between good ones
@pytest.mark.parametrize("model", MODELS)
def test_case4_a_failing_graph_between_good_ones(gpu, model):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(705)
    good = (12, random_graph(rng, 12, 20))
    mirror = JM.Mirror(model, 12, False, 1, True, False)
    pushed, perm = mirror.push_bytes(SEED[1], good[1])
    popped, rest = mirror.pop_bytes(pushed, 20)
    codec = _codec(gpu, model, False, 1, True)
    cap = len(SEED[1]) + _slack(codec, 16, 40)
    seeds = [SEED[1]] * 3

    def others_intact(got, want):
        assert got == [want, b"", want]

    # a pair out of range
    d = Dev(torch, [good, (12, [(0, 12)]), good], seeds, cap, 16)
    assert d.push(codec, 40) == A.ANS_E_SYMBOL and d.lens()[1] == 0
    others_intact(d.messages(), pushed)
    assert d.perms([12, 0, 12])[0] == perm
    # more nodes than max_nodes
    d = Dev(torch, [good, (17, []), good], seeds, cap, 16)
    assert d.push(codec, 40) == A.ANS_E_ARG and d.lens()[1] == 0
    others_intact(d.messages(), pushed)
    # a stream cut to 2 bytes
    d = Dev(torch, [good] * 3, [pushed, pushed[:2], pushed], cap, 16)
    assert d.pop(codec, 40) == A.ANS_E_EXHAUSTED and d.lens()[1] == 0 and d.counts()[1] == 0
    others_intact(d.messages(), rest)
    assert d.popped() == [popped, [], popped]
    if model == "er":
        # a pop capacity one short
        d = Dev(torch, [good] * 3, [pushed] * 3, cap, 16, pair_caps=[20, 19, 20])
        assert d.pop(codec, 40) == A.ANS_E_LEN and d.lens()[1] == 0 and d.counts()[1] == 0
        others_intact(d.messages(), rest)
        assert d.popped() == [popped, [], popped]
        # ... and a state one pair short of the graphs': every graph
        d = Dev(torch, [good] * 3, [pushed] * 3, cap, 16)
        assert d.pop(codec, 19) == A.ANS_E_LEN and all(d.lens() == 0)
    else:
        # the urn has no capacity (the pair count is its parameter); a count the state cannot hold
        d = Dev(torch, [good] * 3, [pushed] * 3, cap, 16, pair_caps=[20, 41, 20])
        assert d.pop(codec, 40) == A.ANS_E_ARG and d.lens()[1] == 0 and d.counts()[1] == 0
        others_intact(d.messages(), rest)
        assert d.popped() == [popped, [], popped]
        # ... and a state one pair short of the graphs': every graph
        d = Dev(torch, [good] * 3, [pushed] * 3, cap, 16)
        assert d.pop(codec, 19) == A.ANS_E_ARG and all(d.lens() == 0)
    # wl_iter above ANS_WL_MAX_ITER: before any launch
    d = Dev(torch, [good] * 3, seeds, cap, 16)
    with pytest.raises(A.AnsError) as e:
        d.push(_codec(gpu, model, False, 4, True), 40)
    assert e.value.code == A.ANS_E_ARG and d.messages() == seeds
