"""The autoregressive Erdős–Rényi graph codecs in bulk on the GPU (include/ans_capi.h section 5d:
ans_dev_ar_er_push / _pop and the ans_gpu_ar_er_*_graphs host-buffer calls): one graph per message,
coded onto / from the message already in the graph's slot.  Every case compares every graph's bytes
after push with the mirror of tests/arer_mirror.py and with the host codec, the permutation and the
popped pairs with the mirror's, and what remains after pop with the mirror's (the seed message)."""
import functools

import numpy as np
import pytest

import ans_amd as A

import arer_mirror as AM
import polya_mirror as PM

pytestmark = pytest.mark.gpu

ORBITS = [A.ORBITS_NONE, A.ORBITS_ONE_CLASS, A.ORBITS_DEGREE]
SMALL = (100, 1000)                      # (mass, norm)
WIDE = (3 << 28, (3 << 30) + 7)          # a norm above 2^31, below 2^32: the u32 table
HUGE = ((1 << 40) - 5, (1 << 42) + 11)   # ... and above 2^32: the table the exact kernels take
SEED_BYTES = 96


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _seeds(rng, count, nbytes=SEED_BYTES):
    s = rng.integers(0, 256, (count, nbytes), dtype=np.uint8)
    s[:, -1] = rng.integers(1, 256, count)  # a nonzero top byte: the seed comes back byte for byte
    return [row.tobytes() for row in s]


def _steps(n, loops, orbits):
    """Blanket steps of one call: without any, the call is flatten(unflatten(B)) = B ++ [0]."""
    return n if orbits != A.ORBITS_NONE else n * (n - 1) // 2 + (n if loops else 0)


def _expect(table, n, edges, seed, loops, orbits):
    """(bytes after push, perm, pairs as pop returns them, bytes after pop) of one graph."""
    mirror = AM.Mirror(*table, n, loops, orbits)
    pushed, perm = mirror.push_bytes(seed, edges)
    popped, rest = mirror.pop_bytes(pushed)
    assert sorted(popped) == AM.relabelled(edges, perm)
    assert rest == (seed if _steps(n, loops, orbits) else seed + bytes(2))
    # the host codec agrees (ans_ar_er_push)
    m = A.Message.unflatten(seed, A.GEN_EMPTY)
    host_perm = A.AutoregressiveER(A.Bernoulli(*table), n, loops, orbits).push(m, edges)
    assert m.flatten() == pushed and list(host_perm) == perm
    return pushed, perm, popped, rest


def _u32(t):
    return np.ascontiguousarray(t, dtype=np.uint32).view(np.int32)


class Dev:
    """Graphs (n, pairs), their messages and the room for what pop returns, on the device."""

    def __init__(self, torch, graphs, msgs, cap, max_nodes, pair_caps=None):
        self.cap, self.g, self.max_nodes = cap, len(graphs), max_nodes
        lists = [e for _, e in graphs]
        self.eo = np.zeros(self.g + 1, np.uint64)
        np.cumsum([len(e) for e in lists], out=self.eo[1:])
        self.po = np.zeros(self.g + 1, np.uint64)  # pop: capacities (the graph's own pair count unless given)
        np.cumsum(pair_caps if pair_caps is not None else [len(e) for e in lists], out=self.po[1:])
        flat = [p for e in lists for p in e] + [(0, 0)]
        self.d_nn = torch.from_numpy(_u32([n for n, _ in graphs])).cuda()
        self.d_edges = torch.from_numpy(_u32(flat).reshape(-1)).cuda()
        self.d_eo = torch.from_numpy(self.eo.view(np.int64)).cuda()
        self.d_po = torch.from_numpy(self.po.view(np.int64)).cuda()
        h = np.zeros((self.g, cap), np.uint8)
        for c, b in enumerate(msgs):
            h[c, :len(b)] = np.frombuffer(b, np.uint8)
        self.d_slots = torch.from_numpy(h.reshape(-1)).cuda()
        self.d_lens = torch.from_numpy(_u32([len(b) for b in msgs])).cuda()
        self.d_perm = torch.full((self.g * max(max_nodes, 1),), -1, dtype=torch.int32, device="cuda")
        self.d_out = torch.full((2 * int(self.po[-1]) + 2,), -1, dtype=torch.int32, device="cuda")
        self.d_count = torch.full((self.g,), -1, dtype=torch.int32, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.Stream()

    def lens(self):
        return self.d_lens.cpu().numpy().view(np.uint32)

    def messages(self):
        h, ln = self.d_slots.cpu().numpy().reshape(-1, self.cap), self.lens()
        return [bytes(h[c, :ln[c]]) for c in range(self.g)]

    def perms(self, nn):
        p = self.d_perm.cpu().numpy().view(np.uint32).reshape(self.g, -1)
        assert all((p[c, nn[c]:] == 0xFFFFFFFF).all() for c in range(self.g))  # nothing past a graph's nodes
        return [[int(v) for v in p[c, :nn[c]]] for c in range(self.g)]

    def counts(self):
        return self.d_count.cpu().numpy().view(np.uint32)

    def popped(self):
        e, k = self.d_out.cpu().numpy().view(np.uint32).reshape(-1, 2), self.counts()
        return [[(int(i), int(j)) for i, j in e[int(self.po[c]):int(self.po[c]) + int(k[c])]] for c in range(self.g)]

    def push(self, codec, max_edges, with_perm=True):
        codec.dev_push(self.g, self.d_nn, self.d_edges, self.d_eo, self.max_nodes, max_edges, self.d_slots, self.cap,
                       self.d_lens, self.status, self.stream, d_perm=self.d_perm if with_perm else None)
        assert codec.gpu.last_launch() == f"k_arer_push<orbits={codec.orbits}>"
        return codec.gpu.status(self.status, self.stream)

    def pop(self, codec):
        self.status.zero_()
        codec.dev_pop(self.g, self.d_nn, self.d_out, self.d_po, self.d_count, self.max_nodes, self.d_slots, self.cap,
                      self.d_lens, self.status, self.stream)
        assert codec.gpu.last_launch() == f"k_arer_pop<orbits={codec.orbits}>"
        return codec.gpu.status(self.status, self.stream)


def _dev_roundtrip(torch, gpu, table, loops, orbits, graphs, seeds, want, max_nodes, max_edges, with_perm=True):
    """ans_dev_ar_er_push then ans_dev_ar_er_pop on device slots against `want`."""
    codec = A.GpuAutoregressiveER(gpu, A.Bernoulli(*table), loops, orbits)
    d = Dev(torch, graphs, seeds, max(len(s) for s in seeds) + codec.slack(max_nodes), max_nodes)
    nn = [n for n, _ in graphs]
    assert d.push(codec, max_edges, with_perm) == A.ANS_OK
    got = d.messages()
    for c in range(d.g):
        assert got[c] == want[c][0], f"push, graph {c}: length {len(got[c])}, want {len(want[c][0])}"
    if with_perm:
        assert d.perms(nn) == [w[1] for w in want]
    else:
        assert (d.d_perm.cpu().numpy() == -1).all()
    assert d.pop(codec) == A.ANS_OK
    got, pairs = d.messages(), d.popped()
    for c in range(d.g):
        assert pairs[c] == want[c][2], f"pop, graph {c}"
        assert got[c] == want[c][3], f"what remains, graph {c}"
    assert (d.d_out.cpu().numpy()[2 * int(d.po[-1]):] == -1).all()


# ---- 1: the named shapes in one launch
@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("orbits", ORBITS)
def test_case1_named_shapes(gpu, orbits, loops):
    torch = pytest.importorskip("torch")
    graphs = [(n, edges) for _, n, edges, needs_loops in AM.shapes() if loops or not needs_loops]
    seeds = _seeds(np.random.default_rng(401), len(graphs))
    seeds[3] += bytes(3)  # zero bytes on top: the first pull runs through them
    want = [_expect(SMALL, n, e, s, loops, orbits) if i != 3 else None for i, ((n, e), s) in enumerate(zip(graphs, seeds))]
    mirror = AM.Mirror(*SMALL, graphs[3][0], loops, orbits)
    pushed, perm = mirror.push_bytes(seeds[3], graphs[3][1])
    want[3] = (pushed, perm) + mirror.pop_bytes(pushed)
    _dev_roundtrip(torch, gpu, SMALL, loops, orbits, graphs, seeds, want, 64, 200)


# ---- 2: divergent lanes, more than one wave
@functools.lru_cache(maxsize=None)
def _mixed(table, loops, orbits, count=300):
    rng = np.random.default_rng(402 + loops)
    graphs = []
    for _ in range(count):
        n = int(rng.integers(0, 41))
        alphabet = n * (n - 1) // 2 + (n if loops else 0)
        graphs.append((n, PM.random_graph(rng, n, int(rng.integers(0, min(120, alphabet) + 1)), loops)))
    seeds = _seeds(rng, count)
    return graphs, seeds, [_expect(table, n, e, s, loops, orbits) for (n, e), s in zip(graphs, seeds)]


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("orbits", ORBITS)
def test_case2_mixed_graphs(gpu, orbits, loops):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _mixed(SMALL, loops, orbits)
    _dev_roundtrip(torch, gpu, SMALL, loops, orbits, graphs, seeds, want, 40, 120)


# ---- 3: the other norms; d_perm NULL
@pytest.mark.parametrize("table", [WIDE, HUGE])
@pytest.mark.parametrize("orbits", ORBITS)
def test_case3_norms_above_2_31(gpu, orbits, table):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = _mixed(table, True, orbits, 80)
    _dev_roundtrip(torch, gpu, table, True, orbits, graphs, seeds, want, 40, 120, with_perm=False)


# ---- 4: host buffers
@pytest.mark.parametrize("orbits", ORBITS)
def test_case4_host_buffers(gpu, orbits):
    pytest.importorskip("torch")
    graphs, seeds, want = _mixed(SMALL, True, orbits)
    nn, lists = [n for n, _ in graphs], [e for _, e in graphs]
    codec = A.GpuAutoregressiveER(gpu, A.Bernoulli(*SMALL), True, orbits)
    lens = np.array([len(s) for s in seeds], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    perms, (data, offs, ln) = codec.push_graphs(nn, lists, np.frombuffer(b"".join(seeds), np.uint8), offsets, lens)
    for c in range(len(graphs)):
        assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[c][0], f"push, graph {c}"
        assert list(perms[c]) == want[c][1], f"perm, graph {c}"
    pairs, (data, offs, ln) = codec.pop_graphs(nn, data, offs, ln)
    for c in range(len(graphs)):
        got = [(int(i), int(j)) for i, j in pairs[c]]
        assert got == want[c][2], f"pop, graph {c}"
        assert sorted(got) == AM.relabelled(lists[c], list(perms[c])), f"the relabelling, graph {c}"
        rest = bytes(data[int(offs[c]):int(offs[c] + ln[c])])
        assert rest == (seeds[c] if _steps(nn[c], True, orbits) else seeds[c] + bytes(2)), f"seed, graph {c}"


# ---- 5: statuses, graph by graph
@pytest.mark.parametrize("orbits", ORBITS)
def test_case5_statuses(gpu, orbits):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(405)
    good = (12, PM.random_graph(rng, 12, 20))
    seeds = _seeds(rng, 3)
    want = [_expect(SMALL, *good, s, False, orbits) for s in seeds]
    codec = A.GpuAutoregressiveER(gpu, A.Bernoulli(*SMALL), False, orbits)
    cap = SEED_BYTES + codec.slack(16)

    def others_intact(got, bad, k):
        for c in range(3):
            assert got[c] == (b"" if c == bad else want[c][k]), f"graph {c}"

    # a bad pair of each kind, among good neighbours on the same wave
    for bad in ([(0, 1), (3, 2)], [(0, 12)], [(0, 1), (2, 2)], good[1] + [good[1][7]]):
        d = Dev(torch, [good, (12, bad), good], seeds, cap, 16)
        assert d.push(codec, 40) == A.ANS_E_SYMBOL and d.lens()[1] == 0, bad
        others_intact(d.messages(), 1, 0)
    # more nodes or pairs than declared
    d = Dev(torch, [good, (17, []), good], seeds, cap, 16)
    assert d.push(codec, 40) == A.ANS_E_ARG and d.lens()[1] == 0
    others_intact(d.messages(), 1, 0)
    d = Dev(torch, [good, good, good], seeds, cap, 16)
    assert d.push(codec, 19) == A.ANS_E_ARG and all(d.lens() == 0)
    # a slot cut to 2 bytes on pop
    pushed = [w[0] for w in want]
    d = Dev(torch, [good] * 3, [pushed[0], pushed[1][:2], pushed[2]], cap, 16)
    assert d.pop(codec) == A.ANS_E_EXHAUSTED and d.lens()[1] == 0 and d.counts()[1] == 0
    others_intact(d.messages(), 1, 3)
    assert d.popped()[0] == want[0][2] and d.popped()[2] == want[2][2]
    # pair capacity one short
    d = Dev(torch, [good] * 3, pushed, cap, 16, pair_caps=[20, 19, 20])
    assert d.pop(codec) == A.ANS_E_LEN and d.lens()[1] == 0 and d.counts()[1] == 0
    others_intact(d.messages(), 1, 3)
    assert d.popped()[0] == want[0][2] and d.popped()[2] == want[2][2]
    # a result past slot_cap; a length above it
    d = Dev(torch, [good] * 3, seeds, len(pushed[1]) - 1, 16)
    assert d.push(codec, 40) == A.ANS_E_LEN and d.lens()[1] == 0
    # arguments: a table of three symbols, an orbits value outside the three
    for make in (lambda: A.GpuAutoregressiveER(gpu, A.Categorical([1, 2, 3]), False, orbits),
                 lambda: A.GpuAutoregressiveER(gpu, A.Bernoulli(*SMALL), False, 3)):
        d = Dev(torch, [good] * 3, seeds, cap, 16)
        with pytest.raises(A.AnsError) as e:
            d.push(make(), 40)
        assert e.value.code == A.ANS_E_ARG and d.messages() == seeds


# ---- 6: the slack holds the worst graph of the table
@pytest.mark.parametrize("table,loops", [(SMALL, True), ((900, 1000), False), (HUGE, True), (((1 << 55) + 3, (1 << 56) - 1), True)])
def test_case6_slack_holds_the_worst_graph(gpu, table, loops):
    """Complete (with every loop) when an edge is the rarer symbol, empty otherwise; NONE pops
    nothing first, so the message only grows."""
    torch = pytest.importorskip("torch")
    n = 40
    rare_edge = table[0] * 2 < table[1]
    edges = [(i, j) for j in range(n) for i in range(j + 1 if loops else j)] if rare_edge else []
    seeds = _seeds(np.random.default_rng(406), 2, 16)
    for orbits in (A.ORBITS_NONE, A.ORBITS_DEGREE):
        codec = A.GpuAutoregressiveER(gpu, A.Bernoulli(*table), loops, orbits)
        d = Dev(torch, [(n, edges)] * 2, seeds, 16 + codec.slack(n), n)
        assert d.push(codec, len(edges)) == A.ANS_OK
        grown = d.lens().copy()
        assert all(grown > 16)
        # ... and a pop in a slot of its length + slack
        d2 = Dev(torch, [(n, edges)] * 2, d.messages(), int(grown.max()) + codec.slack(n), n)
        assert d2.pop(codec) == A.ANS_OK and d2.messages() == seeds
