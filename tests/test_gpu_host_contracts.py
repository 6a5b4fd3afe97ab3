"""The container contracts of the synchronous host entries (include/ans_capi.h), through the C ABI
with explicit buffers.

Encode side, for every entry: an output buffer one byte short is ANS_E_LEN with *total still the
exact container size; the full size gives the oracle's container (bytes, offsets, lens); and the
out = NULL size query reports the same total.  Decode side, for the matching entry: a chunk ending
one byte past the input (offsets[c] + lens[c] == in_len + 1) and a chunk of 2^32 bytes are both
ANS_E_LEN.  Both are refused on the host, before anything is launched.

(ans_gpu_encode_chunks has the same checks in test_gpu_parity.py's pipeline tests.)
"""
import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

P = A._np_ptr


class Case:
    """encode(out, out_cap, offsets, lens, total) -> rc and decode(in, in_len, offsets, lens) -> rc
    of one entry pair, with the oracle's container (data, offsets, lens)."""

    def __init__(self, encode, decode, streams, keep):
        self.encode, self.decode, self.keep = encode, decode, keep
        self.lens = np.asarray([len(s) for s in streams], np.uint64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.uint64)
        self.data = np.frombuffer(b"".join(streams), np.uint8)


def _split(data, lens):
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [data[cuts[c]:cuts[c + 1]].tobytes() for c in range(len(lens))]


def _var_chunks(gpu):
    masses = A.c3_masses()
    gt = A.GpuTable(gpu, A.Categorical(masses))
    sizes = [0, 1, 300, 4096, 77]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(starts[-1])
    syms = orc.gen_iid(masses, 21, 0, n).astype(np.uint8)
    streams = []
    for c in range(len(sizes)):
        a, b = int(starts[c]), int(starts[c + 1])
        od, _, _ = orc.encode_chunks(masses, syms[a:b], max(b - a, 1))
        streams.append(od.tobytes() if b > a else bytes(orc.Message.zeros().flatten()))
    back = np.zeros(n, np.uint8)

    def encode(out, cap, offs, lens, total):
        return A.lib().ans_gpu_encode_var_chunks(gt.h, P(syms), 1, len(sizes), P(starts), out, cap, offs, lens, total)

    def decode(data, in_len, offs, lens):
        return A.lib().ans_gpu_decode_var_chunks(gt.h, data, in_len, offs, lens, len(sizes), P(starts), A.GEN_ZEROS,
                                                 P(back), 1)

    return Case(encode, decode, streams, (gt, syms, starts, back))


def _indep_tables():
    rng = np.random.default_rng(5)
    tables = [(1 + rng.integers(0, 1000, 256)).astype(np.uint64) for _ in range(3)]
    n = 3 * 256 + 5
    tids = rng.integers(0, 3, n).astype(np.uint32)
    syms = rng.integers(0, 256, n).astype(np.uint32)
    return tables, tids, syms, n


def _independent(gpu):
    tables, tids, syms, n = _indep_tables()
    ts = A.GpuTableSet(gpu, [A.Categorical(t) for t in tables])
    L = 256
    od, _, ol = orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, syms, L, tables=tables, tids=tids)
    back = np.zeros(n, np.uint32)

    def encode(out, cap, offs, lens, total):
        return A.lib().ans_gpu_independent_encode_chunks(ts.h, P(tids), P(syms), 4, n, L, A.GEN_ZEROS, 0, out, cap,
                                                         offs, lens, total)

    def decode(data, in_len, offs, lens):
        return A.lib().ans_gpu_independent_decode_chunks(ts.h, P(tids), data, in_len, offs, lens, n, L, A.GEN_ZEROS, 0,
                                                         P(back), 4)

    return Case(encode, decode, _split(od, ol), (ts, tids, syms, back))


def _independent_var(gpu):
    tables, tids, syms, n = _indep_tables()
    ts = A.GpuTableSet(gpu, [A.Categorical(t) for t in tables])
    starts = np.asarray([0, 256, 256, 257, 768, n], np.uint64)  # an empty and a one-symbol chunk among them
    nchunks = len(starts) - 1
    streams = []
    for c in range(nchunks):
        a, b = int(starts[c]), int(starts[c + 1])
        if b == a:
            streams.append(bytes(orc.Message.zeros().flatten()))
            continue
        od, _, _ = orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, syms[a:b], b - a, tables=tables, tids=tids[a:b])
        streams.append(od.tobytes())
    back = np.zeros(n, np.uint32)

    def encode(out, cap, offs, lens, total):
        return A.lib().ans_gpu_independent_encode_var_chunks(ts.h, P(tids), P(syms), 4, nchunks, P(starts),
                                                             A.GEN_ZEROS, 0, out, cap, offs, lens, total)

    def decode(data, in_len, offs, lens):
        return A.lib().ans_gpu_independent_decode_var_chunks(ts.h, P(tids), data, in_len, offs, lens, nchunks,
                                                             P(starts), A.GEN_ZEROS, 0, P(back), 4)

    return Case(encode, decode, streams, (ts, tids, syms, starts, back))


def _uniform(gpu):
    size, n, L = 1000, 1000, 128
    syms = np.random.default_rng(6).integers(0, size, n).astype(np.uint32)
    od, _, ol = orc.codec_encode_chunks(orc.CODEC_UNIFORM, syms, L, param=size)
    back = np.zeros(n, np.uint32)

    def encode(out, cap, offs, lens, total):
        return A.lib().ans_gpu_uniform_encode_chunks(gpu.h, size, P(syms), 4, n, L, A.GEN_ZEROS, 0, out, cap, offs,
                                                     lens, total)

    def decode(data, in_len, offs, lens):
        return A.lib().ans_gpu_uniform_decode_chunks(gpu.h, size, data, in_len, offs, lens, n, L, A.GEN_ZEROS, 0,
                                                     P(back), 4)

    return Case(encode, decode, _split(od, ol), (syms, back))


def _dense_set(gpu):
    nodes, L = 40, 128
    bern = A.Bernoulli(1 << 17, 1 << 20)
    masses = [(1 << 20) - (1 << 17), 1 << 17]
    gt = A.GpuTable(gpu, bern.categorical)
    rng = np.random.default_rng(7)
    alpha = np.asarray(orc.all_edge_indices(nodes, False, False), np.uint32)
    edges = np.ascontiguousarray(alpha[rng.random(len(alpha)) < 0.125])
    od, _, ol = orc.encode_chunks(masses, orc.dense_set(edges, nodes, False, False), L)
    back = np.zeros((len(alpha), 2), np.uint32)
    count = A.u64(0)

    def encode(out, cap, offs, lens, total):
        return A.lib().ans_gpu_dense_set_encode(gt.h, nodes, 0, 0, P(edges), len(edges), L, out, cap, offs, lens, total)

    def decode(data, in_len, offs, lens):
        return A.lib().ans_gpu_dense_set_decode(gt.h, nodes, 0, 0, data, in_len, offs, lens, L, P(back), len(alpha),
                                                A.ctypes.byref(count))

    return Case(encode, decode, _split(od, ol), (gt, bern, edges, back, count))


def _graphs(gpu):
    rng = np.random.default_rng(8)
    nums = [6, 3, 0, 5]
    graphs = []
    for n in nums:
        alpha = np.asarray(orc.all_edge_indices(n, False, False), np.uint32).reshape(-1, 2)
        e = alpha[rng.random(len(alpha)) < 0.4]
        graphs.append((n, rng.integers(0, 3, n).astype(np.uint32), e, rng.integers(0, 2, len(e)).astype(np.uint32)))
    bern = [30, 10]
    nodes, elabels = np.asarray([5, 2, 1], np.uint64), np.asarray([3, 1], np.uint64)
    ts = A.GpuTableSet(gpu, [A.Categorical(bern), A.Categorical(nodes), A.Categorical(elabels)])
    streams = []
    for n, nl, e, el in graphs:
        m = orc.Message.zeros()
        assert orc.graph_iid_push(m, n, nl, e, el, bern, ("cat", nodes), ("cat", elabels), False, False) == 0
        streams.append(bytes(m.flatten()))
    nn = np.asarray(nums, np.uint32)
    nl = np.ascontiguousarray(np.concatenate([g[1] for g in graphs]))
    edges = np.ascontiguousarray(np.concatenate([g[2] for g in graphs]))
    el = np.ascontiguousarray(np.concatenate([g[3] for g in graphs]))
    eo = np.concatenate([[0], np.cumsum([len(g[2]) for g in graphs])]).astype(np.uint64)
    cap = max(len(edges), 1)
    bnl, bedges, bel = np.zeros(max(len(nl), 1), np.uint32), np.zeros((cap, 2), np.uint32), np.zeros(cap, np.uint32)
    beo = np.zeros(len(nums) + 1, np.uint64)

    def encode(out, cap_, offs, lens, total):
        return A.lib().ans_gpu_graphs_encode(ts.h, 1, 2, 0, 0, 0, len(nums), P(nn), P(nl), P(edges), P(el), P(eo),
                                             A.GEN_ZEROS, 0, out, cap_, offs, lens, total)

    def decode(data, in_len, offs, lens):
        return A.lib().ans_gpu_graphs_decode(ts.h, 1, 2, 0, 0, 0, len(nums), P(nn), data, in_len, offs, lens,
                                             A.GEN_ZEROS, 0, P(bnl), P(bedges), P(bel), cap, P(beo))

    return Case(encode, decode, streams, (ts, nn, nl, edges, el, eo, bnl, bedges, bel, beo))


CASES = {"var_chunks": _var_chunks, "independent": _independent, "independent_var": _independent_var,
         "uniform": _uniform, "dense_set": _dense_set, "graphs": _graphs}


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


@pytest.fixture(scope="module", params=list(CASES))
def case(request, gpu):
    return CASES[request.param](gpu)


def _encode(case, cap, with_out=True):
    n = len(case.lens)
    out = np.zeros(max(cap, 1), np.uint8)
    offs, lens = np.full(n, 0xEE, np.uint64), np.full(n, 0xEE, np.uint64)
    total = A.u64(0xEE)
    if with_out:
        rc = case.encode(P(out), cap, P(offs), P(lens), A.ctypes.byref(total))
    else:
        rc = case.encode(None, 0, None, None, A.ctypes.byref(total))
    return rc, total.value, out, offs, lens


def test_encode_one_byte_short_is_e_len_with_the_exact_total(case):
    assert len(case.data) > 0
    rc, total, _, _, _ = _encode(case, len(case.data) - 1)
    assert rc == A.ANS_E_LEN
    assert total == len(case.data)


def test_encode_exact_capacity_gives_the_oracle_container(case):
    rc, total, out, offs, lens = _encode(case, len(case.data))
    assert rc == A.ANS_OK
    assert total == len(case.data)
    assert np.array_equal(lens, case.lens)
    assert np.array_equal(offs, case.offsets)
    assert out[:total].tobytes() == case.data.tobytes()


def test_encode_size_query_reports_the_same_total(case):
    rc, total, _, _, _ = _encode(case, 0, with_out=False)
    assert rc == A.ANS_OK
    assert total == len(case.data)


def test_decode_accepts_the_oracle_container(case):
    """The decode closure itself is sound: the untouched container decodes."""
    data = case.data.copy()
    assert case.decode(P(data), len(data), P(case.offsets.copy()), P(case.lens.copy())) == A.ANS_OK


@pytest.mark.parametrize("which", ["one_past_the_input", "two_to_the_32"])
def test_decode_bad_chunk_bounds_are_e_len(case, which):
    data = case.data.copy()
    offs, lens = case.offsets.copy(), case.lens.copy()
    c = len(lens) - 1  # the last stream ends at in_len
    assert int(offs[c] + lens[c]) == len(data)
    lens[c] = lens[c] + np.uint64(1) if which == "one_past_the_input" else np.uint64(1 << 32)
    assert case.decode(P(data), len(data), P(offs), P(lens)) == A.ANS_E_LEN
