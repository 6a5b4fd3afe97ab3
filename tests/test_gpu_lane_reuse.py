"""One lane, several items: the multiset and Pólya urn kernels (ans_mset.hip cnt=global,
ans_polya.hip) keep a lane's state in the context's workspace, entry i of lane l at i * lanes + l,
and a lane that codes a second item finds the first one's state there.  These cases force few lanes
(by a large declared bound, or a large alphabet: the launch cuts the lanes until their state fits
256 MiB), read the workgroup count back from the launch record (Gpu.last_launch_grid) so that the
reuse is known to have happened, and compare with the mirrors of tests/polya_mirror.py and
tests/mset_mirror.py bit for bit:
  (a) Pólya, 273 graphs on 64 and on 192 lanes, all four (loops, redraws) settings; a lane's graphs
      alternate between the plain path (E <= 11, few nodes) and the joint one (E >= 12, many nodes);
  (b) a graph that fails, then good ones on the same lane;
  (c) multisets over 65,536 symbols, 2,148 chunks on 1,024 lanes;
  (d) both units in turn on one context: the workspace grows, and is then larger than needed and
      full of the other unit's state;
  (e) the largest state one wave may have, and the first that is refused.
The expected grids follow from kWsMax = 256 MiB and ans_polya.hpp ws_entries as they stand."""
import functools

import numpy as np
import pytest

import ans_amd as A

import mset_mirror as MM
import polya_mirror as PM

pytestmark = pytest.mark.gpu

SETTINGS = [(True, True), (True, False), (False, True), (False, False)]
WS_MAX = 256 << 20
NUM_GRAPHS = 273  # 4 * 64 + 17
SEED_BYTES = 96
BAD = (5, 70, 135)  # graphs of (b); g + 64 and g + 128 follow them on their lanes


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _ws_entries(max_nodes, max_edges):
    return 2 * max_nodes + 6 * max_edges + 2


def test_the_declared_bounds_give_the_grids_asserted_below():
    assert _ws_entries(64, 100000) == 600130 and WS_MAX // (256 * 600130) == 1
    assert _ws_entries(64, 50000) == 300130 and WS_MAX // (256 * 300130) == 3
    assert _ws_entries(4, 174761) == 1 << 20 and 256 * _ws_entries(5, 174761) > WS_MAX
    assert WS_MAX // (4 * 65536 * 64) == 16


# ---- the graphs
def _large(g):
    """Graph g is a large one (E >= 12) or a small one (E <= 11): neighbours in a wave differ, and so
    do g and g + 64, and g and g + 192 (the graph a lane codes next on 64 and on 192 lanes)."""
    return (g // 64 + g) % 2 == 1


@functools.lru_cache(maxsize=None)
def _graphs(loops, redraws, count=300):
    """(graphs, seeds, expectations): the first NUM_GRAPHS are the graphs of (a) and (b)."""
    rng = np.random.default_rng(300 + 2 * loops + redraws)
    graphs = []
    for g in range(count):
        n = int(rng.integers(20, 41)) if _large(g) else int(rng.integers(1, 13))
        alphabet = n * (n - 1) // 2 + (n if loops else 0)
        low, high = (12, min(60, alphabet)) if _large(g) else (0, min(11, alphabet))
        edges = PM.random_graph(rng, n, int(rng.integers(low, high + 1)), loops)
        if loops and edges and all(i != j for i, j in edges):
            edges[int(rng.integers(len(edges)))] = (n - 1, n - 1)
        graphs.append((n, edges))
    assert all(_large(g) != _large(g + 64) for g in range(count - 64))
    assert all(_large(g) != _large(g + 192) for g in range(count - 192))
    seeds = _seeds(rng, count)
    return graphs, seeds, [_expect(n, e, s, loops, redraws) for (n, e), s in zip(graphs, seeds)]


def _seeds(rng, count, nbytes=SEED_BYTES):
    s = rng.integers(0, 256, (count, nbytes), dtype=np.uint8)
    s[:, -1] = rng.integers(1, 256, count)  # a nonzero top byte: the seed comes back byte for byte
    return [row.tobytes() for row in s]


def _expect(n, edges, seed, loops, redraws):
    """(bytes after push, edges as pop returns them, bytes after pop) of one graph."""
    mirror = PM.Mirror(n, loops, redraws)
    pushed = mirror.push_bytes(seed, edges)
    popped, rest = mirror.pop_bytes(pushed, len(edges))
    assert sorted(popped) == sorted(edges)
    assert rest == (seed if edges else seed + bytes(2))
    return pushed, popped, rest


class Dev:
    """Graphs (n, E x 2 array or list of pairs) and their messages on the device."""

    def __init__(self, torch, graphs, msgs, cap):
        self.cap, self.g = cap, len(graphs)
        arrays = [np.asarray(e, np.uint32).reshape(-1, 2) for _, e in graphs]
        self.eo = np.zeros(self.g + 1, np.uint64)
        np.cumsum([len(a) for a in arrays], out=self.eo[1:])
        flat = np.concatenate(arrays + [np.zeros((1, 2), np.uint32)]).reshape(-1)
        self.d_nn = torch.from_numpy(np.array([n for n, _ in graphs], np.uint32).view(np.int32)).cuda()
        self.d_edges = torch.from_numpy(flat.view(np.int32)).cuda()
        self.d_eo = torch.from_numpy(self.eo.view(np.int64)).cuda()
        h = np.zeros((self.g, cap), np.uint8)
        for c, b in enumerate(msgs):
            h[c, :len(b)] = np.frombuffer(b, np.uint8)
        self.d_slots = torch.from_numpy(h.reshape(-1)).cuda()
        self.d_lens = torch.from_numpy(np.array([len(b) for b in msgs], np.uint32).view(np.int32)).cuda()
        self.d_out = torch.zeros_like(self.d_edges)
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.Stream()

    def lens(self):
        return self.d_lens.cpu().numpy().view(np.uint32)

    def messages(self):
        h, ln = self.d_slots.cpu().numpy().reshape(-1, self.cap), self.lens()
        return [bytes(h[c, :ln[c]]) for c in range(self.g)]

    def popped(self):
        e = self.d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
        return [[(int(i), int(j)) for i, j in e[int(self.eo[c]):int(self.eo[c + 1])]] for c in range(self.g)]

    def push(self, gpu, loops, redraws, max_nodes, max_edges):
        A.GpuPolyaUrn(gpu, loops, redraws).dev_push(self.g, self.d_nn, self.d_edges, self.d_eo, max_nodes, max_edges,
                                                    self.d_slots, self.cap, self.d_lens, self.status, self.stream)
        assert gpu.last_launch() == f"k_polya_push<redraws={int(redraws)}>"
        return gpu.status(self.status, self.stream)

    def pop(self, gpu, loops, redraws, max_nodes, max_edges):
        self.status.zero_()
        A.GpuPolyaUrn(gpu, loops, redraws).dev_pop(self.g, self.d_nn, self.d_out, self.d_eo, max_nodes, max_edges,
                                                   self.d_slots, self.cap, self.d_lens, self.status, self.stream)
        assert gpu.last_launch() == f"k_polya_pop<redraws={int(redraws)}>"
        return gpu.status(self.status, self.stream)


def _cap():
    """The slots' size: by the graphs coded, not by the declared bounds (which size the state only)."""
    return SEED_BYTES + A.GpuPolyaUrn.slack(40, 60)


def _polya_roundtrip(torch, gpu, loops, redraws, count, max_nodes, max_edges, grid):
    graphs, seeds, want = (x[:count] for x in _graphs(loops, redraws))
    d = Dev(torch, graphs, seeds, _cap())
    assert d.push(gpu, loops, redraws, max_nodes, max_edges) == A.ANS_OK
    assert gpu.last_launch_grid() == grid
    got = d.messages()
    for c in range(count):
        assert got[c] == want[c][0], f"push, graph {c} (lane {c % (64 * grid)}, its graph number {c // (64 * grid)})"
    assert d.pop(gpu, loops, redraws, max_nodes, max_edges) == A.ANS_OK
    assert gpu.last_launch_grid() == grid
    got, edges = d.messages(), d.popped()
    for c in range(count):
        assert edges[c] == want[c][1], f"pop, graph {c}"
        assert got[c] == want[c][2], f"what remains, graph {c}"


# ---- (a)
@pytest.mark.parametrize("max_edges,grid", [(100000, 1), (50000, 3)])
@pytest.mark.parametrize("loops,redraws", SETTINGS)
def test_a_polya_lanes_code_several_graphs(gpu, loops, redraws, max_edges, grid):
    torch = pytest.importorskip("torch")
    _polya_roundtrip(torch, gpu, loops, redraws, NUM_GRAPHS, 64, max_edges, grid)


# ---- (b)
def _with(items, replacement):
    out = list(items)
    for g in BAD:
        out[g] = replacement(g)
    return out


def _others_equal(got, want, what):
    for c in range(NUM_GRAPHS):
        if c not in BAD:
            assert got[c] == want[c], f"{what}, graph {c}"


@pytest.mark.parametrize("loops,redraws", [(True, True), (False, False)])
def test_b_push_a_failed_graph_then_good_ones_on_its_lane(gpu, loops, redraws):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = (x[:NUM_GRAPHS] for x in _graphs(loops, redraws))
    assert all(_large(g) for g in BAD) and all(g + 128 < NUM_GRAPHS for g in BAD)
    pushed = [w[0] for w in want]
    rng = np.random.default_rng(310)
    twice = PM.random_graph(rng, 8, 12, loops)
    twice = (8, twice + [twice[4]])  # 13 pairs: found after the ranking has written ord and next
    over = (40, np.zeros((100001, 2), np.uint32))  # more pairs than max_edges: refused before any is read
    for kind, bad_graphs, bad_seeds in (
            (A.ANS_E_EXHAUSTED, graphs, _with(seeds, lambda g: b"\x07")),  # in the middle of the push
            (A.ANS_E_SYMBOL, _with(graphs, lambda g: twice), seeds),
            (A.ANS_E_ARG, _with(graphs, lambda g: over), seeds)):
        d = Dev(torch, bad_graphs, bad_seeds, _cap())
        assert d.push(gpu, loops, redraws, 64, 100000) == kind
        assert gpu.last_launch_grid() == 1
        assert all(d.lens()[g] == 0 for g in BAD), kind
        _others_equal(d.messages(), pushed, f"push beside status {kind}")


@pytest.mark.parametrize("loops,redraws", [(True, True), (False, False)])
def test_b_pop_a_failed_graph_then_good_ones_on_its_lane(gpu, loops, redraws):
    torch = pytest.importorskip("torch")
    graphs, seeds, want = (x[:NUM_GRAPHS] for x in _graphs(loops, redraws))
    pushed = [w[0] for w in want]
    cap = _cap()
    # two bytes of the message: exhausted within the ordered pops
    d = Dev(torch, graphs, _with(pushed, lambda g: pushed[g][:2]), cap)
    assert d.pop(gpu, loops, redraws, 64, 100000) == A.ANS_E_EXHAUSTED
    assert gpu.last_launch_grid() == 1
    assert all(d.lens()[g] == 0 for g in BAD)
    _others_equal(d.messages(), [w[2] for w in want], "what remains beside ANS_E_EXHAUSTED")
    _others_equal(d.popped(), [w[1] for w in want], "pop beside ANS_E_EXHAUSTED")
    # a full slot whose result is a byte longer: no pairs, so the pop is flatten(unflatten(B)) = B ++ [0]
    full = _seeds(np.random.default_rng(311), 1, cap)[0]
    d = Dev(torch, _with(graphs, lambda g: (3, [])), _with(pushed, lambda g: full), cap)
    assert d.pop(gpu, loops, redraws, 64, 100000) == A.ANS_E_LEN
    assert gpu.last_launch_grid() == 1
    assert all(d.lens()[g] == 0 for g in BAD)
    _others_equal(d.messages(), [w[2] for w in want], "what remains beside ANS_E_LEN")
    _others_equal(d.popped(), [w[1] for w in want], "pop beside ANS_E_LEN")


# ---- (c)
NUM_CHUNKS = 2148  # two full wraps of 1,024 lanes and 100 chunks
SAMPLE = sorted({0, 1023, 1024, 2047, 2048, 2147} | set(range(0, NUM_CHUNKS, 97)))


@functools.lru_cache(maxsize=None)
def _wide_multisets():
    rng = np.random.default_rng(320)
    masses = rng.integers(1, 16, 65536).astype(np.uint64)  # the norm stays below 2^20
    lens = rng.integers(0, 41, NUM_CHUNKS)
    lens[[0, 1023, 1024]] = (40, 0, 33)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    values = rng.integers(0, 65536, int(starts[-1])).astype(np.uint32)
    seeds = MM.seeds(rng, NUM_CHUNKS)
    mirror = MM.Mirror(masses)
    want = {}
    for c in SAMPLE:
        a, b = int(starts[c]), int(starts[c + 1])
        pushed = mirror.push_bytes(seeds[c], values[a:b])
        want[c] = (pushed,) + mirror.pop_bytes(pushed, b - a)
    # chunk c + 1,024, the next on c's lane, repeats few of c's symbols: counts left behind would show
    shared = [len(set(values[int(starts[c]):int(starts[c + 1])]) & set(values[int(starts[c + 1024]):int(starts[c + 1025])]))
              for c in range(NUM_CHUNKS - 1024)]
    assert max(shared) <= 2
    return masses, starts, values, seeds, want


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_c_multiset_lanes_code_several_chunks(gpu, dtype):
    torch = pytest.importorskip("torch")
    masses, starts, values, seeds, want = _wide_multisets()
    values = values.astype(dtype)
    w = values.dtype.itemsize
    name = {2: "u16", 4: "u32"}[w]
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    cap = 64 + ts.slot_capacity(40) + ts.mset_pop_slack(40)
    h = np.zeros((NUM_CHUNKS, cap), np.uint8)
    h[:, :64] = np.frombuffer(b"".join(seeds), np.uint8).reshape(NUM_CHUNKS, 64)
    d_slots = torch.from_numpy(h.reshape(-1)).cuda()
    d_lens = torch.from_numpy(np.full(NUM_CHUNKS, 64, np.int32)).cuda()
    d_syms = torch.from_numpy(values.view({2: np.int16, 4: np.int32}[w])).cuda()
    d_starts = torch.from_numpy(starts.view(np.int64)).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()

    def messages():
        m, ln = d_slots.cpu().numpy().reshape(-1, cap), d_lens.cpu().numpy().view(np.uint32)
        return [bytes(m[c, :ln[c]]) for c in range(NUM_CHUNKS)]

    ts.dev_mset_push(0, d_syms, w, 0, 0, d_slots, cap, d_lens, status, stream, d_starts=d_starts, nchunks=NUM_CHUNKS)
    assert gpu.last_launch() == f"k_mset_push<{name},cnt=global>"
    assert gpu.last_launch_grid() == 16
    assert gpu.status(status, stream) == A.ANS_OK
    got = messages()
    for c in SAMPLE:
        assert got[c] == want[c][0], f"push, chunk {c}"
    d_out = torch.zeros_like(d_syms)
    ts.dev_mset_pop(0, d_slots, cap, d_lens, 0, 0, d_out, w, status, stream, d_starts=d_starts, nchunks=NUM_CHUNKS)
    assert gpu.last_launch() == f"k_mset_pop<{name},cnt=global>"
    assert gpu.last_launch_grid() == 16
    assert gpu.status(status, stream) == A.ANS_OK
    got, out = messages(), d_out.cpu().numpy().view(dtype)
    for c in SAMPLE:
        assert [int(v) for v in out[int(starts[c]):int(starts[c + 1])]] == want[c][1], f"pop order, chunk {c}"
        assert got[c] == want[c][2], f"what remains, chunk {c}"
    for c in range(NUM_CHUNKS):  # every chunk: the multiset, and the seed byte for byte
        a, b = int(starts[c]), int(starts[c + 1])
        assert np.array_equal(np.sort(out[a:b]), np.sort(values[a:b])), f"values, chunk {c}"
        assert got[c] == (seeds[c] if b > a else seeds[c] + bytes(2)), f"seed, chunk {c}"


# ---- (d)
@functools.lru_cache(maxsize=None)
def _narrow_multisets():
    rng = np.random.default_rng(330)
    masses = rng.integers(1, 1 << 12, 1030).astype(np.uint64)
    n, chunk_len = 70 * 96, 96
    values = rng.integers(0, 1030, n).astype(np.uint16)
    seeds = MM.seeds(rng, 70)
    mirror = MM.Mirror(masses)
    want = []
    for c, seed in enumerate(seeds):
        pushed = mirror.push_bytes(seed, values[c * chunk_len:(c + 1) * chunk_len])
        want.append((pushed,) + mirror.pop_bytes(pushed, chunk_len))
    return masses, values, seeds, want


def _narrow_roundtrip(torch, gpu, ts):
    _, values, seeds, want = _narrow_multisets()
    n, chunk_len = len(values), 96
    cap = 64 + ts.slot_capacity(chunk_len) + ts.mset_pop_slack(chunk_len)
    h = np.zeros((70, cap), np.uint8)
    h[:, :64] = np.frombuffer(b"".join(seeds), np.uint8).reshape(70, 64)
    d_slots = torch.from_numpy(h.reshape(-1)).cuda()
    d_lens = torch.from_numpy(np.full(70, 64, np.int32)).cuda()
    d_syms = torch.from_numpy(values.view(np.int16)).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()

    def messages():
        m, ln = d_slots.cpu().numpy().reshape(-1, cap), d_lens.cpu().numpy().view(np.uint32)
        return [bytes(m[c, :ln[c]]) for c in range(70)]

    ts.dev_mset_push(0, d_syms, 2, n, chunk_len, d_slots, cap, d_lens, status, stream)
    assert gpu.last_launch() == "k_mset_push<u16,cnt=global>" and gpu.last_launch_grid() == 2
    assert gpu.status(status, stream) == A.ANS_OK
    assert messages() == [w[0] for w in want]
    d_out = torch.zeros_like(d_syms)
    ts.dev_mset_pop(0, d_slots, cap, d_lens, n, chunk_len, d_out, 2, status, stream)
    assert gpu.last_launch() == "k_mset_pop<u16,cnt=global>" and gpu.last_launch_grid() == 2
    assert gpu.status(status, stream) == A.ANS_OK
    assert [int(v) for v in d_out.cpu().numpy().view(np.uint16)] == [v for w in want for v in w[1]]
    assert messages() == [w[2] for w in want] == seeds


def test_d_both_units_share_one_workspace():
    torch = pytest.importorskip("torch")
    gpu = A.Gpu(0)  # a context of its own: its workspace starts empty
    ts = A.GpuTableSet(gpu, [A.Categorical(_narrow_multisets()[0])])
    _narrow_roundtrip(torch, gpu, ts)  # a small workspace: 2 workgroups x 1,030 counts
    _polya_roundtrip(torch, gpu, False, False, NUM_GRAPHS, 64, 100000, 1)  # it grows: freed and allocated anew
    _narrow_roundtrip(torch, gpu, ts)  # larger than needed, and full of the urn codec's state
    _polya_roundtrip(torch, gpu, False, False, 300, 40, 60, 5)  # other lanes over the same memory


# ---- (e)
def test_e_the_largest_state_of_one_wave_and_the_first_refused(gpu):
    torch = pytest.importorskip("torch")
    graphs = [(4, [(0, 1), (2, 3), (1, 2)]), (3, []), (4, [(0, 3)])]
    seeds = _seeds(np.random.default_rng(340), 3)
    want = [_expect(n, e, s, False, False) for (n, e), s in zip(graphs, seeds)]
    d = Dev(torch, graphs, seeds, _cap())
    assert d.push(gpu, False, False, 4, 174761) == A.ANS_OK  # 2^20 entries a lane, 256 MiB a wave
    assert gpu.last_launch_grid() == 1
    assert d.messages() == [w[0] for w in want]
    # one entry more: refused by the launch plan, before the record is cleared and any kernel starts
    before = d.messages()
    with pytest.raises(A.AnsError) as e:
        A.GpuPolyaUrn(gpu, False, False).dev_pop(3, d.d_nn, d.d_out, d.d_eo, 5, 174761, d.d_slots, d.cap, d.d_lens,
                                                 d.status, d.stream)
    assert e.value.code == A.ANS_E_ARG
    assert gpu.last_launch() == "k_polya_push<redraws=0>" and gpu.last_launch_grid() == 1
    assert gpu.status(d.status, d.stream) == A.ANS_OK and int(d.status.cpu()[0]) == 0
    assert d.messages() == before
    with pytest.raises(A.AnsError) as e:
        gpu.last_launch_grid(1)
    assert e.value.code == A.ANS_E_ARG


def test_records_that_keep_no_grid_read_zero(gpu):
    table = A.GpuTable(gpu, A.Categorical(np.arange(1, 257, dtype=np.uint64)))
    table.encode_chunks(np.arange(4096, dtype=np.uint8), 4096)
    assert gpu.last_launch().startswith("k_encode") and gpu.last_launch_grid() == 0
