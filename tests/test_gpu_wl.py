"""Graph shuffle coding with Weisfeiler-Lehman orbits in bulk on the GPU (include/ans_capi.h section
5f: ans_dev_ar_er_wl_push / _pop, ans_dev_ar_polya_wl_push / _pop and the *_wl_*_graphs host-buffer
calls): one graph per message, coded onto / from the message already in the graph's slot.  The bytes
after push, the permutation, the popped pairs, their counts and what remains after pop are compared
with the mirror of tests/wl_mirror.py (computed once per setting for the module); at wl_iter = 0
with the kernels of ans_arer.hip / ans_arpu.hip."""
import numpy as np
import pytest

import ans_amd as A

import wl_mirror as WM
from polya_mirror import complete, random_graph
from test_gpu_arer import Dev as ArerDev, _seeds, HUGE, SMALL

pytestmark = pytest.mark.gpu

MODELS = ["er", "pu"]
SETTINGS = [(w, h) for w in (1, 2) for h in (True, False)]
SEED = ("seed", _seeds(np.random.default_rng(601), 1)[0])  # not empty: the message is already in the slot


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _want(model, wl_iter, half_iter):
    return WM.expected(model, wl_iter, half_iter, (SEED,))  # (remembered: the host-buffer case reads it again)


def _codec(gpu, model, loops, wl_iter, half_iter, table=SMALL):
    if model == "er":
        return A.GpuAutoregressiveERWL(gpu, A.Bernoulli(*table), loops, wl_iter, half_iter)
    return A.GpuAutoregressivePolyaWL(gpu, loops, wl_iter, half_iter)


def _slack(codec, max_nodes, max_edges):
    return codec.slack(max_nodes) if isinstance(codec, A.GpuAutoregressiveERWL) else codec.slack(max_nodes, max_edges)


def _kernel(codec, what):
    model = "arer" if isinstance(codec, A.GpuAutoregressiveERWL) else "arpu"
    return f"k_{model}_wl_{what}(wl_iter={codec.wl_iter},half_iter={codec.half_iter})"


class Dev(ArerDev):
    def push(self, codec, max_edges, with_perm=True):
        self.status.zero_()
        codec.dev_push(self.g, self.d_nn, self.d_edges, self.d_eo, self.max_nodes, max_edges, self.d_slots, self.cap,
                       self.d_lens, self.status, self.stream, d_perm=self.d_perm if with_perm else None)
        if hasattr(codec, "wl_iter"):
            assert codec.gpu.last_launch() == _kernel(codec, "push")
        return codec.gpu.status(self.status, self.stream)

    def pop(self, codec, max_edges):
        self.status.zero_()
        if isinstance(codec, A.GpuAutoregressiveER) and not hasattr(codec, "wl_iter"):
            codec.dev_pop(self.g, self.d_nn, self.d_out, self.d_po, self.d_count, self.max_nodes, self.d_slots,
                          self.cap, self.d_lens, self.status, self.stream)
        else:
            codec.dev_pop(self.g, self.d_nn, self.d_out, self.d_po, self.d_count, self.max_nodes, max_edges,
                          self.d_slots, self.cap, self.d_lens, self.status, self.stream)
        if hasattr(codec, "wl_iter"):
            assert codec.gpu.last_launch() == _kernel(codec, "pop")
        return codec.gpu.status(self.status, self.stream)


def _shapes(loops):
    return [(name, n, edges) for name, n, edges, needs_loops in WM.all_shapes() if needs_loops == loops]


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
        pairs, (data, offs, ln) = codec.pop_graphs(nn, data, offs, ln)
        for c, (name, _, _) in enumerate(shapes):
            assert [(int(i), int(j)) for i, j in pairs[c]] == want[name, "seed"][2], f"pop, {name}"
            assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[name, "seed"][3], f"what remains, {name}"


# ---- 2: at wl_iter = 0 the slots of the degree kernels, byte for byte
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("half_iter", [True, False])
def test_case2_wl0_equals_the_degree_kernels(gpu, model, half_iter):
    torch = pytest.importorskip("torch")
    orbits = A.ORBITS_DEGREE if half_iter else A.ORBITS_ONE_CLASS
    for loops in (False, True):
        shapes = _shapes(loops)
        graphs = [(n, edges) for _, n, edges in shapes]
        seeds = _seeds(np.random.default_rng(602), len(graphs))
        new = _codec(gpu, model, loops, 0, half_iter)
        old = A.GpuAutoregressiveER(gpu, A.Bernoulli(*SMALL), loops, orbits) if model == "er" \
            else A.GpuAutoregressivePolya(gpu, loops, orbits)
        cap = len(seeds[0]) + _slack(new, 64, 200)
        a, b = Dev(torch, graphs, seeds, cap, 64), Dev(torch, graphs, seeds, cap, 64)
        assert a.push(new, 200) == A.ANS_OK and b.push(old, 200) == A.ANS_OK
        assert torch.equal(a.d_lens, b.d_lens) and a.messages() == b.messages() and torch.equal(a.d_perm, b.d_perm)
        assert all(a.lens() > 0)
        assert a.pop(new, 200) == A.ANS_OK and b.pop(old, 200) == A.ANS_OK
        assert torch.equal(a.d_lens, b.d_lens) and a.messages() == b.messages()
        assert torch.equal(a.d_out, b.d_out) and torch.equal(a.d_count, b.d_count)


# ---- 3: the slack of the wl_iter = 0 codecs holds at wl_iter = 1
def _slack_case(torch, codec, n, edges):
    """Slots of exactly d_lens + slack for the push, then for the pop; then a slot one byte shorter than
    the result: ANS_E_LEN for that slot, as a status."""
    seeds = _seeds(np.random.default_rng(606), 2, 16)
    slack = _slack(codec, n, len(edges))
    d = Dev(torch, [(n, edges)] * 2, seeds, 16 + slack, n)
    assert d.push(codec, len(edges)) == A.ANS_OK
    grown = d.lens().copy()
    assert all(grown > 0)
    pushed = d.messages()
    d2 = Dev(torch, [(n, edges)] * 2, pushed, int(grown.max()) + slack, n)
    assert d2.pop(codec, len(edges)) == A.ANS_OK and d2.messages() == seeds
    assert [int(c) for c in d2.counts()] == [len(edges)] * 2
    if int(grown.max()) > 16:
        d3 = Dev(torch, [(n, edges)] * 2, seeds, int(grown.max()) - 1, n)
        assert d3.push(codec, len(edges)) == A.ANS_E_LEN
        assert all(ln == 0 for ln, g in zip(d3.lens(), grown) if g == grown.max())


@pytest.mark.parametrize("table,loops", [(SMALL, True), ((900, 1000), False), (HUGE, True), (((1 << 55) + 3, (1 << 56) - 1), True)])
def test_case3_er_slack_holds_the_worst_graph(gpu, table, loops):
    """The worst graph of tests/test_gpu_arer.py case 6: complete (with every loop) when an edge is the
    rarer symbol, empty otherwise."""
    torch = pytest.importorskip("torch")
    n = 40
    rare_edge = table[0] * 2 < table[1]
    edges = [(i, j) for j in range(n) for i in range(j + 1 if loops else j)] if rare_edge else []
    _slack_case(torch, _codec(gpu, "er", loops, 1, True, table), n, edges)


@pytest.mark.parametrize("loops", [False, True])
def test_case3_polya_slack_holds_the_worst_graph(gpu, loops):
    """The worst graphs of tests/test_gpu_arpu.py case 5: complete, and empty (all slice sizes)."""
    torch = pytest.importorskip("torch")
    n = 40
    for edges in (complete(n) + ([(v, v) for v in range(n)] if loops else []), []):
        _slack_case(torch, _codec(gpu, "pu", loops, 1, True), n, edges)


# ---- 4: a failing graph between good ones
@pytest.mark.parametrize("model", MODELS)
def test_case4_a_failing_graph_between_good_ones(gpu, model):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(605)
    good = (12, random_graph(rng, 12, 20))
    mirror = WM.mirror_of(model, 12, False, 1, True)
    pushed, perm = mirror.push_bytes(SEED[1], good[1])
    popped, rest = mirror.pop_bytes(pushed)
    codec = _codec(gpu, model, False, 1, True)
    cap = len(SEED[1]) + _slack(codec, 16, 40)
    seeds = [SEED[1]] * 3

    def others_intact(got, want):
        assert got == [want, b"", want]

    # an edge out of range
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
    # a pop capacity one short
    d = Dev(torch, [good] * 3, [pushed] * 3, cap, 16, pair_caps=[20, 19, 20])
    assert d.pop(codec, 40) == A.ANS_E_LEN and d.lens()[1] == 0 and d.counts()[1] == 0
    others_intact(d.messages(), rest)
    assert d.popped() == [popped, [], popped]
    # ... and a state one pair short of the graphs': every graph
    d = Dev(torch, [good] * 3, [pushed] * 3, cap, 16)
    assert d.pop(codec, 19) == A.ANS_E_LEN and all(d.lens() == 0)
    # wl_iter above ANS_WL_MAX_ITER: before any launch
    d = Dev(torch, [good] * 3, seeds, cap, 16)
    with pytest.raises(A.AnsError) as e:
        d.push(_codec(gpu, model, False, 4, True), 40)
    assert e.value.code == A.ANS_E_ARG and d.messages() == seeds
