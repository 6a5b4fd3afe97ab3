"""The autoregressive Pólya urn graph codecs in bulk on the GPU (include/ans_capi.h section 5e:
ans_dev_ar_polya_push / _pop and the ans_gpu_ar_polya_*_graphs host-buffer calls): one graph per
message, coded onto / from the message already in the graph's slot.  Every case compares every
graph's bytes after push with the mirror of tests/arpu_mirror.py and with the host codec, the
permutation and the popped pairs with the mirror's, and what remains after pop with the seed."""
import functools

import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

import arpu_mirror as PM2
from polya_mirror import complete, random_graph
from test_gpu_arer import Dev as ArerDev, _seeds  # the device buffers of a batch of graphs

pytestmark = pytest.mark.gpu

ORBITS = [A.ORBITS_NONE, A.ORBITS_ONE_CLASS, A.ORBITS_DEGREE]
SEED_BYTES = 96


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def expect(n, edges, seed, loops, orbits):
    """(bytes after push, perm, pairs as pop returns them, bytes after pop) of one graph: the mirror's,
    which the host codec has to give as well (ans_ar_polya_push / _pop)."""
    mirror = PM2.Mirror(n, loops, orbits)
    m = orc.Message.unflatten(seed, orc.EMPTY)
    perm = mirror.push(m, edges)
    pushed = m.flatten()
    m = orc.Message.unflatten(pushed, orc.EMPTY)
    popped = mirror.pop(m)
    rest = m.flatten()
    assert popped == PM2.relabelled(edges, perm)
    assert rest == (seed if n else seed + bytes(2))  # without a node the calls are two flattens
    codec = A.AutoregressivePolya(n, loops, orbits)
    m = A.Message.unflatten(seed, A.GEN_EMPTY)
    host_perm = codec.push(m, edges)
    assert m.flatten() == pushed and list(host_perm) == perm
    m = A.Message.unflatten(pushed, A.GEN_EMPTY)
    assert codec.pop(m) == popped and m.flatten() == rest
    return pushed, perm, popped, rest


class Dev(ArerDev):
    def push(self, codec, max_edges, with_perm=True):
        codec.dev_push(self.g, self.d_nn, self.d_edges, self.d_eo, self.max_nodes, max_edges, self.d_slots, self.cap,
                       self.d_lens, self.status, self.stream, d_perm=self.d_perm if with_perm else None)
        assert codec.gpu.last_launch() == f"k_arpu_push<orbits={codec.orbits}>"
        return codec.gpu.status(self.status, self.stream)

    def pop(self, codec, max_edges):
        self.status.zero_()
        codec.dev_pop(self.g, self.d_nn, self.d_out, self.d_po, self.d_count, self.max_nodes, max_edges, self.d_slots,
                      self.cap, self.d_lens, self.status, self.stream)
        assert codec.gpu.last_launch() == f"k_arpu_pop<orbits={codec.orbits}>"
        return codec.gpu.status(self.status, self.stream)


def dev_roundtrip(torch, gpu, loops, orbits, graphs, seeds, want, max_nodes, max_edges, with_perm=True):
    """ans_dev_ar_polya_push then ans_dev_ar_polya_pop on device slots against `want`."""
    codec = A.GpuAutoregressivePolya(gpu, loops, orbits)
    d = Dev(torch, graphs, seeds, max(len(s) for s in seeds) + codec.slack(max_nodes, max_edges), max_nodes)
    nn = [n for n, _ in graphs]
    assert d.push(codec, max_edges, with_perm) == A.ANS_OK
    got = d.messages()
    for c in range(d.g):
        assert got[c] == want[c][0], f"push, graph {c}: length {len(got[c])}, want {len(want[c][0])}"
    if with_perm:
        assert d.perms(nn) == [w[1] for w in want]
    else:
        assert (d.d_perm.cpu().numpy() == -1).all()
    assert d.pop(codec, max_edges) == A.ANS_OK
    got, pairs = d.messages(), d.popped()
    for c in range(d.g):
        assert pairs[c] == want[c][2], f"pop, graph {c}"
        assert got[c] == want[c][3], f"what remains, graph {c}"
    assert (d.d_out.cpu().numpy()[2 * int(d.po[-1]):] == -1).all()


# ---- 1: the host test's named shapes in one launch
@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("orbits", ORBITS)
def test_case1_named_shapes(gpu, orbits, loops):
    torch = pytest.importorskip("torch")
    graphs = [(n, edges) for _, n, edges, needs_loops in PM2.shapes() if loops or not needs_loops]
    seeds = _seeds(np.random.default_rng(411), len(graphs))
    seeds[3] += bytes(3)  # zero bytes on top: the first pull runs through them
    want = [expect(n, e, s, loops, orbits) if i != 3 else None for i, ((n, e), s) in enumerate(zip(graphs, seeds))]
    mirror = PM2.Mirror(graphs[3][0], loops, orbits)
    m = orc.Message.unflatten(seeds[3], orc.EMPTY)
    perm = mirror.push(m, graphs[3][1])
    pushed = m.flatten()
    m = orc.Message.unflatten(pushed, orc.EMPTY)
    want[3] = (pushed, perm, mirror.pop(m), m.flatten())
    dev_roundtrip(torch, gpu, loops, orbits, graphs, seeds, want, 40, 120)


# ---- 2: divergent lanes, more than one wave; sparse and dense (joint slices) in turn
@functools.lru_cache(maxsize=None)
def mixed(loops, orbits, count=150):
    rng = np.random.default_rng(412 + loops)
    graphs = []
    for k in range(count):
        n = int(rng.integers(0, 41)) if k % 2 else int(rng.integers(0, 17))
        alphabet = n * (n - 1) // 2 + (n if loops else 0)
        graphs.append((n, random_graph(rng, n, int(rng.integers(0, min(120, alphabet) + 1)), loops)))
    seeds = _seeds(rng, count)
    return graphs, seeds, [expect(n, e, s, loops, orbits) for (n, e), s in zip(graphs, seeds)]


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("orbits", ORBITS)
def test_case2_mixed_graphs(gpu, orbits, loops):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = mixed(loops, orbits)
    dev_roundtrip(torch, gpu, loops, orbits, graphs, seeds, want, 40, 120, with_perm=orbits != A.ORBITS_ONE_CLASS)


# ---- 3: host buffers
@pytest.mark.parametrize("orbits", ORBITS)
def test_case3_host_buffers(gpu, orbits):
    pytest.importorskip("torch")
    graphs, seeds, want = mixed(True, orbits)
    nn, lists = [n for n, _ in graphs], [e for _, e in graphs]
    codec = A.GpuAutoregressivePolya(gpu, True, orbits)
    lens = np.array([len(s) for s in seeds], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    perms, (data, offs, ln) = codec.push_graphs(nn, lists, np.frombuffer(b"".join(seeds), np.uint8), offsets, lens)
    assert gpu.last_launch() == f"k_arpu_push<orbits={orbits}>"
    for c in range(len(graphs)):
        assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[c][0], f"push, graph {c}"
        assert list(perms[c]) == want[c][1], f"perm, graph {c}"
    pairs, (data, offs, ln) = codec.pop_graphs(nn, data, offs, ln, caps=[len(e) for e in lists])
    assert gpu.last_launch() == f"k_arpu_pop<orbits={orbits}>"
    for c in range(len(graphs)):
        got = [(int(i), int(j)) for i, j in pairs[c]]
        assert got == want[c][2], f"pop, graph {c}"
        assert bytes(data[int(offs[c]):int(offs[c] + ln[c])]) == want[c][3], f"what remains, graph {c}"


# ---- 4: statuses, graph by graph
@pytest.mark.parametrize("orbits", ORBITS)
def test_case4_statuses(gpu, orbits):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(415)
    good = (12, random_graph(rng, 12, 20))
    seeds = _seeds(rng, 3)
    want = [expect(*good, s, False, orbits) for s in seeds]
    codec = A.GpuAutoregressivePolya(gpu, False, orbits)
    cap = SEED_BYTES + codec.slack(16, 40)

    def others_intact(got, bad, k):
        for c in range(3):
            assert got[c] == (b"" if c == bad else want[c][k]), f"graph {c}"

    # a bad pair of each kind, among good neighbours on the same wave
    for bad in ([(0, 1), (3, 2)], [(0, 12)], [(0, 1), (2, 2)], good[1] + [good[1][7]]):
        d = Dev(torch, [good, (12, bad), good], seeds, cap, 16)
        assert d.push(codec, 40) == A.ANS_E_SYMBOL and d.lens()[1] == 0, bad
        others_intact(d.messages(), 1, 0)
    # more nodes or pairs than declared, each alone among good graphs
    d = Dev(torch, [good, (17, []), good], seeds, cap, 16)
    assert d.push(codec, 40) == A.ANS_E_ARG and d.lens()[1] == 0
    others_intact(d.messages(), 1, 0)
    d = Dev(torch, [good, (12, complete(7)), good], seeds, cap, 16)
    assert d.push(codec, 20) == A.ANS_E_ARG and d.lens()[1] == 0
    others_intact(d.messages(), 1, 0)
    # a slot cut to 2 bytes on pop
    pushed = [w[0] for w in want]
    d = Dev(torch, [good] * 3, [pushed[0], pushed[1][:2], pushed[2]], cap, 16)
    assert d.pop(codec, 40) == A.ANS_E_EXHAUSTED and d.lens()[1] == 0 and d.counts()[1] == 0
    others_intact(d.messages(), 1, 3)
    assert d.popped()[0] == want[0][2] and d.popped()[2] == want[2][2]
    # pair capacity one short
    d = Dev(torch, [good] * 3, pushed, cap, 16, pair_caps=[20, 19, 20])
    assert d.pop(codec, 40) == A.ANS_E_LEN and d.lens()[1] == 0 and d.counts()[1] == 0
    others_intact(d.messages(), 1, 3)
    assert d.popped()[0] == want[0][2] and d.popped()[2] == want[2][2]
    # a slot too small for one result alone: a larger graph between two small ones, in slots one byte
    # short of its result (the small ones' results are 10 bytes or more below that: room for the few
    # bytes a message can stand above its final length between steps)
    small, big = (5, [(0, 1), (2, 3)]), (16, random_graph(rng, 16, 75))
    shorts = [expect(*small, s, False, orbits)[0] for s in seeds]
    long = expect(*big, seeds[1], False, orbits)[0]
    assert len(long) - 1 >= max(len(p) for p in shorts) + 10
    d = Dev(torch, [small, big, small], seeds, len(long) - 1, 16)
    assert d.push(codec, 75) == A.ANS_E_LEN and d.lens()[1] == 0
    assert [d.messages()[c] for c in (0, 2)] == [shorts[0], shorts[2]]
    d = Dev(torch, [good] * 3, seeds, min(len(p) for p in pushed) - 1, 16)
    assert d.push(codec, 40) == A.ANS_E_LEN and all(d.lens() == 0)
    # an orbits value outside the three: before any launch, the slots as they were
    d = Dev(torch, [good] * 3, seeds, cap, 16)
    with pytest.raises(A.AnsError) as e:
        d.push(A.GpuAutoregressivePolya(gpu, False, 3), 40)
    assert e.value.code == A.ANS_E_ARG and d.messages() == seeds


# ---- 5: the slack holds the worst graphs
@pytest.mark.parametrize("loops", [False, True])
def test_case5_slack_holds_the_worst_graph(gpu, loops):
    """Slots of exactly seed + ans_gpu_ar_polya_slack.  The complete graph has the most urn symbols
    under the largest norms (a push), and the most permutation steps to put back (a pop); the empty
    graph is all slice sizes."""
    torch = pytest.importorskip("torch")
    n = 40
    full = complete(n) + ([(v, v) for v in range(n)] if loops else [])
    seeds = _seeds(np.random.default_rng(416), 2, 16)
    for edges in (full, []):
        for orbits in (A.ORBITS_NONE, A.ORBITS_DEGREE):
            codec = A.GpuAutoregressivePolya(gpu, loops, orbits)
            slack = codec.slack(n, len(edges))
            d = Dev(torch, [(n, edges)] * 2, seeds, 16 + slack, n)
            assert d.push(codec, len(edges)) == A.ANS_OK
            grown = d.lens().copy()
            assert all(grown > 16)
            # ... and a pop in a slot of its length + slack
            d2 = Dev(torch, [(n, edges)] * 2, d.messages(), int(grown.max()) + slack, n)
            assert d2.pop(codec, len(edges)) == A.ANS_OK and d2.messages() == seeds
            if orbits == A.ORBITS_NONE:
                assert d2.popped() == [sorted(edges)] * 2
