"""Multisets in bulk on the GPU (include/ans_capi.h section 4b: ans_dev_mset_push / _pop, their
_var forms and the ans_gpu_mset_*_chunks host-buffer calls): one multiset per chunk, coded by
recursive shuffle coding onto / from the message already in the chunk's slot.  Every case compares
every chunk's bytes and length after push with the mirror of tests/mset_mirror.py, the popped
values with the mirror's pop order, and what remains after pop with the seed messages; the count
path (LDS or global) is read from the launch record."""
import numpy as np
import pytest

import ans_amd as A

import mset_mirror as MM

pytestmark = pytest.mark.gpu

_VIEW = {1: np.uint8, 2: np.int16, 4: np.int32}  # torch.from_numpy takes the signed twins


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _to_slots(torch, msgs, cap, lens=None):
    h = np.zeros((len(msgs), cap), np.uint8)
    for c, b in enumerate(msgs):
        h[c, :min(len(b), cap)] = np.frombuffer(b, np.uint8)[:cap]
    ln = np.array([len(b) for b in msgs] if lens is None else lens, np.int64).astype(np.uint32).view(np.int32)
    return torch.from_numpy(h.reshape(-1)).cuda(), torch.from_numpy(ln).cuda()


def _from_slots(d_slots, d_lens, cap):
    h = d_slots.cpu().numpy().reshape(-1, cap)
    ln = d_lens.cpu().numpy().view(np.uint32)
    return [bytes(h[c, :ln[c]]) for c in range(len(ln))]


def _chunks(n, chunk_len=None, starts=None):
    if starts is not None:
        return [(int(starts[c]), int(starts[c + 1])) for c in range(len(starts) - 1)]
    return [(a, min(a + chunk_len, n)) for a in range(0, n, chunk_len)]


def _expected(mirror, seeds, values, chunks):
    """Per chunk: (bytes after push, values in pop order, bytes after pop), or None where the
    mirror reports exhaustion."""
    out = []
    for seed, (a, b) in zip(seeds, chunks):
        pushed = mirror.push_bytes(seed, values[a:b])
        if pushed is None:
            out.append(None)
            continue
        popped = mirror.pop_bytes(pushed, b - a)
        assert popped is not None
        out.append((pushed, popped[0], popped[1]))
    return out


def _dev_roundtrip(torch, gpu, ts, table, values, seeds, want, path, chunk_len=None, starts=None, cap=None,
                   status_push=A.ANS_OK):
    """ans_dev_mset_push then ans_dev_mset_pop on device slots against `want`; returns nothing."""
    n = len(values)
    w = values.dtype.itemsize
    chunks = _chunks(n, chunk_len, starts)
    nchunks = len(chunks)
    longest = max([b - a for a, b in chunks] + [1])
    if cap is None:
        cap = max(len(s) for s in seeds) + ts.slot_capacity(longest) + ts.mset_pop_slack(longest)
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_slots, d_lens = _to_slots(torch, seeds, cap)
    d_syms = torch.from_numpy(values.view(_VIEW[w])).cuda()
    var = {}
    if starts is not None:
        var = dict(d_starts=torch.from_numpy(np.asarray(starts, np.uint64).view(np.int64)).cuda(), nchunks=nchunks)
    ts.dev_mset_push(table, d_syms, w, n, chunk_len or 0, d_slots, cap, d_lens, status, stream, **var)
    name = {1: "u8", 2: "u16", 4: "u32"}[w]
    assert gpu.last_launch() == f"k_mset_push<{name},cnt={path}>"
    assert gpu.status(status, stream) == status_push
    got = _from_slots(d_slots, d_lens, cap)
    for c in range(nchunks):
        assert got[c] == (want[c][0] if want[c] else b""), f"push chunk {c}: length {len(got[c])}"
    # pop from what the push left (a failed chunk left an empty message: its pop is exhausted too,
    # unless it holds no symbols)
    status.zero_()
    d_out = torch.zeros(max(n, 1), dtype=d_syms.dtype, device="cuda")
    ts.dev_mset_pop(table, d_slots, cap, d_lens, n, chunk_len or 0, d_out, w, status, stream, **var)
    assert gpu.last_launch() == f"k_mset_pop<{name},cnt={path}>"
    failed = [c for c in range(nchunks) if want[c] is None and chunks[c][1] > chunks[c][0]]
    assert gpu.status(status, stream) == (A.ANS_E_EXHAUSTED if failed else A.ANS_OK)
    got = _from_slots(d_slots, d_lens, cap)
    out = d_out.cpu().numpy().view(values.dtype)
    for c, (a, b) in enumerate(chunks):
        if want[c] is None:
            continue
        assert [int(v) for v in out[a:b]] == want[c][1], f"pop order, chunk {c}"
        assert got[c] == want[c][2], f"what remains, chunk {c}"
        if b == a:  # no symbols: each call is flatten(unflatten(B)) = B ++ [0]
            assert got[c] == seeds[c] + bytes(2), f"seed, chunk {c}"
        elif seeds[c][-1]:  # a seed with a nonzero top byte comes back byte for byte
            assert got[c] == seeds[c], f"seed, chunk {c}"


def _no_exhaustion(want):
    assert all(w is not None for w in want), "the mirror reports exhaustion on a shape that must not exhaust"


def _table1(rng):
    return rng.integers(1, 1 << 16, 256).astype(np.uint64)


# ---- the five shapes
def test_case1_u8_256_symbols_lds(gpu):
    """256 symbols, chunk_len 64, 130 chunks and a ragged 17: three workgroups, one partly filled."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(101)
    masses = _table1(rng)
    n, L = 130 * 64 + 17, 64
    values = rng.integers(0, 256, n).astype(np.uint8)
    seeds = MM.seeds(rng, 131)
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(n, L))
    _no_exhaustion(want)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    _dev_roundtrip(torch, gpu, ts, 0, values, seeds, want, "lds", chunk_len=L)


@pytest.fixture(scope="module")
def case2(multiset_masses, multiset_vectors):
    """The multiset table (1,024 symbols exactly) over multiset_10000.txt as 10 chunks of 1,000."""
    rng = np.random.default_rng(102)
    values = np.asarray(multiset_vectors[10000], np.uint32)
    seeds = MM.seeds(rng, 10)
    want = _expected(MM.Mirror(multiset_masses), seeds, values, _chunks(10000, 1000))
    return values, seeds, want


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_case2_multiset_table_1024_symbols_lds(gpu, multiset_masses, case2, dtype):
    torch = pytest.importorskip("torch")
    values, seeds, want = case2
    assert len(multiset_masses) == 1024
    _no_exhaustion(want)
    # The counts take 128 KiB of the 160.  Alone, the table's image (8 KiB of cdf, 16 KiB of icdf
    # buckets) still fits beside them; with a second table of 4,096 buckets the set's image is above
    # 32 KiB and its LDS staging has to yield.
    ts = A.GpuTableSet(gpu, [A.Categorical(multiset_masses)])
    _dev_roundtrip(torch, gpu, ts, 0, values.astype(dtype), seeds, want, "lds", chunk_len=1000)
    ts = A.GpuTableSet(gpu, [A.Categorical([1 << 15, 1 << 15]), A.Categorical(multiset_masses)])
    _dev_roundtrip(torch, gpu, ts, 1, values.astype(dtype), seeds, want, "lds", chunk_len=1000)


def test_case3_1030_symbols_global(gpu):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(103)
    masses = rng.integers(1, 1 << 12, 1030).astype(np.uint64)
    n, L = 70 * 96, 96
    values = rng.integers(0, 1030, n).astype(np.uint16)
    seeds = MM.seeds(rng, 70)
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(n, L))
    _no_exhaustion(want)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    _dev_roundtrip(torch, gpu, ts, 0, values, seeds, want, "global", chunk_len=L)


def test_case4_long_chunk_counts_past_16_bits_global(gpu):
    """One chunk of 70,000 values of 4 symbols (a count passes 2^16) and 65 chunks of 64, in one
    variable-chunk call."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(104)
    masses = np.array([700, 100, 150, 50], np.uint64)
    starts = np.concatenate([[0], 70000 + 64 * np.arange(66)]).astype(np.uint64)
    values = rng.choice(4, int(starts[-1]), p=[0.97, 0.01, 0.015, 0.005]).astype(np.uint8)
    assert np.bincount(values[:70000])[0] > 65536
    seeds = [MM.seeds(rng, 1, 256)[0]] + MM.seeds(rng, 65)
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(len(values), starts=starts))
    _no_exhaustion(want)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    _dev_roundtrip(torch, gpu, ts, 0, values, seeds, want, "global", starts=starts)
    # the host-buffer call knows the longest chunk: the same path, the same bytes
    data = np.frombuffer(b"".join(seeds), np.uint8)
    lens = np.array([len(s) for s in seeds], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    out, o, ln = ts.mset_push_var_chunks(0, values, starts, data, offs, lens)
    assert gpu.last_launch() == "k_mset_push<u8,cnt=global>"
    assert [bytes(out[int(o[c]):int(o[c] + ln[c])]) for c in range(66)] == [w[0] for w in want]


def test_case5_long_runs_of_one_value(gpu):
    """[65000, 500]: 66 chunks of 200, runs of one value, pmf = count up to 200."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(105)
    masses = np.array([65000, 500], np.uint64)
    n, L = 66 * 200, 200
    values = (rng.random(n) < 0.01).astype(np.uint8)
    values[:200] = 0
    values[200:400] = 1
    seeds = MM.seeds(rng, 66)
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(n, L))
    _no_exhaustion(want)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    _dev_roundtrip(torch, gpu, ts, 0, values, seeds, want, "lds", chunk_len=L)


# ---- the other cases
VAR_LENS = [0, 1, 2, 11, 12, 300, 64, 65, 0]


def test_variable_chunks_device_and_host(gpu):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(106)
    masses = _table1(rng)
    starts = np.concatenate([[0], np.cumsum(VAR_LENS)]).astype(np.uint64)
    values = rng.integers(0, 256, int(starts[-1])).astype(np.uint8)
    seeds = MM.seeds(rng, len(VAR_LENS))
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(len(values), starts=starts))
    _no_exhaustion(want)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    # device-resident: the chunk lengths are on the device, the counts global
    _dev_roundtrip(torch, gpu, ts, 0, values, seeds, want, "global", starts=starts)
    # host buffers: the longest chunk is known, the counts in LDS
    data, offs, lens = _container(seeds)
    out, o, ln = ts.mset_push_var_chunks(0, values, starts, data, offs, lens)
    assert gpu.last_launch() == "k_mset_push<u8,cnt=lds>"
    assert _messages(out, o, ln) == [w[0] for w in want]
    back, (rest, ro, rl) = ts.mset_pop_var_chunks(0, out, o, ln, starts, np.uint8)
    assert gpu.last_launch() == "k_mset_pop<u8,cnt=lds>"
    assert [int(v) for v in back] == [v for w in want for v in w[1]]
    assert _messages(rest, ro, rl) == [w[2] for w in want]


def _container(msgs):
    lens = np.array([len(b) for b in msgs], np.uint64)
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    return np.frombuffer(b"".join(msgs), np.uint8), offs, lens


def _messages(data, offsets, lens):
    return [bytes(data[int(o):int(o + n)]) for o, n in zip(offsets, lens)]


def test_dense_container_host_calls(gpu):
    """Fixed chunks through host buffers, and the out == NULL size query."""
    import ctypes
    rng = np.random.default_rng(107)
    masses = _table1(rng)
    n, L = 9 * 64 + 5, 64
    values = rng.integers(0, 256, n).astype(np.uint16)
    seeds = MM.seeds(rng, 10)
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(n, L))
    _no_exhaustion(want)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    data, offs, lens = _container(seeds)
    out, o, ln = ts.mset_push_chunks(0, values, L, data, offs, lens)
    assert _messages(out, o, ln) == [w[0] for w in want]
    total = ctypes.c_uint64(0)
    A._check(A.lib().ans_gpu_mset_push_chunks(ts.h, 0, A._np_ptr(values), 2, n, L, A._np_ptr(data), data.size,
                                              A._np_ptr(offs), A._np_ptr(lens), None, 0, None, None,
                                              ctypes.byref(total)), "size query")
    assert total.value == len(out) == sum(len(w[0]) for w in want)
    back, (rest, ro, rl) = ts.mset_pop_chunks(0, out, o, ln, n, L, np.uint16)
    assert [int(v) for v in back] == [v for w in want for v in w[1]]
    assert _messages(rest, ro, rl) == [w[2] for w in want] == seeds
    syms = np.zeros(n, np.uint16)
    A._check(A.lib().ans_gpu_mset_pop_chunks(ts.h, 0, A._np_ptr(out), out.size, A._np_ptr(o), A._np_ptr(ln), n, L,
                                             A._np_ptr(syms), 2, None, 0, None, None, ctypes.byref(total)), "size query")
    assert total.value == len(rest) and np.array_equal(syms, back)


def test_exhaustion_is_a_status_not_a_fault(gpu):
    """Three of 130 chunks carry 1-byte seeds: ANS_E_EXHAUSTED, their d_lens 0, every other chunk
    still the mirror's."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(108)
    masses = _table1(rng)
    n, L = 130 * 64, 64
    values = rng.integers(0, 256, n).astype(np.uint8)
    seeds = MM.seeds(rng, 130)
    short = (0, 64, 129)
    for c in short:
        seeds[c] = bytes([7 + c % 5])
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(n, L))
    assert [c for c in range(130) if want[c] is None] == list(short)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    _dev_roundtrip(torch, gpu, ts, 0, values, seeds, want, "lds", chunk_len=L, status_push=A.ANS_E_EXHAUSTED)


def test_seeds_with_zero_bytes_on_top(gpu):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(109)
    masses = _table1(rng)
    n, L = 70 * 64, 64
    values = rng.integers(0, 256, n).astype(np.uint8)
    seeds = [s[:64 - c % 4] + bytes(c % 4) for c, s in enumerate(MM.seeds(rng, 70))]
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(n, L))
    _no_exhaustion(want)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    _dev_roundtrip(torch, gpu, ts, 0, values, seeds, want, "lds", chunk_len=L)


def test_slot_bound_is_ans_e_len(gpu):
    """slot_cap 16 B short of the longest result on push; a d_lens[c] above slot_cap."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(110)
    masses = _table1(rng)
    n, L = 66 * 64, 64
    values = rng.integers(0, 256, n).astype(np.uint8)
    seeds = MM.seeds(rng, 66)
    want = _expected(MM.Mirror(masses), seeds, values, _chunks(n, L))
    _no_exhaustion(want)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    need = max(len(w[0]) for w in want)
    cap = need - 16
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_slots, d_lens = _to_slots(torch, seeds, cap)
    d_syms = torch.from_numpy(values).cuda()
    ts.dev_mset_push(0, d_syms, 1, n, L, d_slots, cap, d_lens, status, stream)
    assert gpu.status(status, stream) == A.ANS_E_LEN
    got = _from_slots(d_slots, d_lens, cap)
    over = [c for c in range(66) if len(want[c][0]) > cap]
    assert over
    for c in range(66):
        if c in over:
            assert got[c] == b"", f"chunk {c}"
        elif len(want[c][0]) <= cap - 16:  # (a push's message is never 16 B above where it ends)
            assert got[c] == want[c][0], f"chunk {c}"
        else:
            assert got[c] in (b"", want[c][0]), f"chunk {c}"
    # a length above slot_cap going in: push and pop both refuse that chunk alone
    cap = 64 + ts.slot_capacity(L) + ts.mset_pop_slack(L)
    for op in ("push", "pop"):
        status.zero_()
        msgs = seeds if op == "push" else [w[0] for w in want]
        lens = [len(b) for b in msgs]
        lens[5] = cap + 1
        d_slots, d_lens = _to_slots(torch, msgs, cap, lens)
        d_out = torch.zeros(n, dtype=torch.uint8, device="cuda")
        if op == "push":
            ts.dev_mset_push(0, d_syms, 1, n, L, d_slots, cap, d_lens, status, stream)
        else:
            ts.dev_mset_pop(0, d_slots, cap, d_lens, n, L, d_out, 1, status, stream)
        assert gpu.status(status, stream) == A.ANS_E_LEN, op
        got = _from_slots(d_slots, d_lens, cap)
        assert got[5] == b"", op
        for c in (0, 4, 6, 65):
            assert got[c] == (want[c][0] if op == "push" else want[c][2]), f"{op} chunk {c}"


def test_symbol_and_zero_mass_statuses(gpu):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(111)
    masses = np.array([9, 0, 4, 11, 6], np.uint64)
    mirror = MM.Mirror(masses)
    n, L = 66 * 16, 16
    seeds = MM.seeds(rng, 66)
    ts = A.GpuTableSet(gpu, [A.Categorical(masses)])
    cap = 64 + ts.slot_capacity(L) + ts.mset_pop_slack(L)
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for bad, code in ((5, A.ANS_E_SYMBOL), (255, A.ANS_E_SYMBOL), (1, A.ANS_E_ZERO_MASS)):
        values = rng.choice([0, 2, 3, 4], n).astype(np.uint8)
        values[3 * L + 7] = bad
        values[65 * L] = bad
        status.zero_()
        d_slots, d_lens = _to_slots(torch, seeds, cap)
        ts.dev_mset_push(0, torch.from_numpy(values).cuda(), 1, n, L, d_slots, cap, d_lens, status, stream)
        assert gpu.status(status, stream) == code
        got = _from_slots(d_slots, d_lens, cap)
        for c in range(66):
            if c in (3, 65):
                assert got[c] == b"", f"chunk {c}"
            else:
                assert got[c] == mirror.push_bytes(seeds[c], values[c * L:(c + 1) * L]), f"chunk {c}"
    # arguments: a table outside the set, a symbol width the call does not take
    with pytest.raises(A.AnsError) as e:
        ts.dev_mset_push(1, d_slots, 1, n, L, d_slots, cap, d_lens, status, stream)
    assert e.value.code == A.ANS_E_ARG
    with pytest.raises(A.AnsError) as e:
        ts.dev_mset_push(0, d_slots, 8, n, L, d_slots, cap, d_lens, status, stream)
    assert e.value.code == A.ANS_E_ARG
