"""GPU resume (include/ans_capi.h section 4b, ans_dev_independent_push / _pop and their host
forms): pushing onto and popping from messages that already exist, one per chunk, each
Message::unflatten(bytes) with the Empty generator.  The reference is the rule: every result must
equal the oracle's unflatten + Categorical push_iid / pop_iid + flatten byte for byte
(oracle/ans_oracle.c, the restatement of src/ans.rs:96-116,233-264 and src/codec.rs:388-399).

Two identities give expected bytes from the oracle's bulk calls:
  split (push): encode X[:, h:], then push X[:, :h] onto it == encode X;
  split (pop):  pop h symbols from encode(X) returns X[:, :h] and leaves encode(X[:, h:]).
The other cases compare with the oracle's Message API chunk by chunk."""
import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _sample(rng, masses, n):
    nz = np.flatnonzero(masses)
    p = masses[nz].astype(np.float64)
    return rng.choice(nz, size=n, p=p / p.sum())


def _indep_case(rng, tables, n):
    tids = rng.integers(0, len(tables), size=n).astype(np.uint32)
    syms = np.zeros(n, np.uint64)
    for t, m in enumerate(tables):
        sel = tids == t
        syms[sel] = _sample(rng, m, int(sel.sum()))
    return tids, syms


def _fast_tables(rng):
    """Five 256-symbol tables in the fast range, as tools/codecs_bench.py codes them."""
    return [rng.integers(1, 1 << 16, size=256).astype(np.uint64) for _ in range(5)]


def _small_norm_tables(rng):
    return [np.array([31000, 3400], np.uint64), np.array([2395, 345, 593, 0, 23, 12, 2], np.uint64),
            np.array([1, 1], np.uint64), rng.integers(1, 200, size=256).astype(np.uint64),
            np.array([65000, 1, 1, 7], np.uint64)]


def _big_norm_tables(rng):
    t = [rng.integers(1 << 23, 1 << 24, size=256).astype(np.uint64),
         np.array([(1 << 31) + 12345, 1, 77, 1 << 30], np.uint64),
         np.array([(1 << 32) - 2, 1], np.uint64)]
    t[0] = (t[0] * ((1 << 32) - 99) // int(t[0].sum())).astype(np.uint64)
    return t


def _two_range_tables(rng):
    """Norms from two ranges in one set: the exact kernels only (ans_gpu_tableset_fast == 0)."""
    return [rng.integers(1, 1 << 16, size=256).astype(np.uint64), np.array([3, 5], np.uint64)]


# ---- containers and the per-chunk oracle
def _container(msgs):
    lens = np.array([len(m) for m in msgs], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(msgs) else np.zeros(0, np.uint64)
    data = np.frombuffer(b"".join(msgs), np.uint8).copy()
    return data, offsets, lens


def _messages(data, offsets, lens):
    return [bytes(data[int(o):int(o) + int(n)]) for o, n in zip(offsets, lens)]


def _orc_push(ocats, msg, tids, syms):
    """unflatten (Empty) + Independent::push (last position first, src/codec.rs:388-391; runs of
    one table as one push_iid) + flatten; None where the reference reports exhaustion."""
    m = orc.Message.unflatten(msg, orc.EMPTY)
    k = len(syms)
    while k > 0:
        j = k
        while j > 0 and tids[j - 1] == tids[k - 1]:
            j -= 1
        rc = ocats[int(tids[k - 1])].push_iid(m, syms[j:k])
        if rc:
            assert rc == A.ANS_E_EXHAUSTED, rc
            return None
        k = j
    return m.flatten()


def _orc_pop(ocats, msg, tids):
    """unflatten (Empty) + forward pops + flatten: (symbols, bytes), or None on exhaustion."""
    m = orc.Message.unflatten(msg, orc.EMPTY)
    out = []
    k = 0
    while k < len(tids):
        j = k
        while j < len(tids) and tids[j] == tids[k]:
            j += 1
        try:
            out.extend(int(v) for v in ocats[int(tids[k])].pop_iid(m, j - k))
        except RuntimeError:
            assert m.err == A.ANS_E_EXHAUSTED, m.err
            return None
        k = j
    return np.array(out, np.uint64), m.flatten()


def _initial(kind, seed):
    m = orc.Message.random(seed) if kind == A.GEN_RANDOM else orc.Message.zeros()
    return m.flatten()


def _split_case(rng, tables, L, h, nfull, ragged):
    """X: nfull chunks of L symbols and a last one of `ragged` <= h; its heads X[:, :h] (the last
    chunk whole) and tails X[:, h:] as flat arrays with their table ids."""
    n = nfull * L + ragged
    tids, syms = _indep_case(rng, tables, n)
    full = np.arange(nfull * L).reshape(nfull, L)
    head_idx = np.concatenate([full[:, :h].reshape(-1), np.arange(nfull * L, n)])
    tail_idx = full[:, h:].reshape(-1)
    return tids, syms, head_idx, tail_idx


def _check_split(ts, tables, dtype, L, h, nfull, ragged, kind, seed, rng):
    tids, syms, hi, ti = _split_case(rng, tables, L, h, nfull, ragged)
    od, oo, ol = orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, syms, L, tables=tables, tids=tids, kind=kind, seed=seed)
    # push: the tails through the existing encoder (the ragged chunk's tail is its initial message)
    td, to, tl = ts.encode_chunks(tids[ti], syms[ti].astype(dtype), L - h, kind, seed)
    tails = _messages(td, to, tl) + ([_initial(kind, seed + nfull)] if ragged else [])
    pd, po, pl = ts.push_chunks(tids[hi], syms[hi].astype(dtype), h, *_container(tails))
    assert np.array_equal(pl, ol), "push: stream lengths"
    assert pd.tobytes() == od.tobytes(), "push: stream bytes"
    assert np.array_equal(po, oo)
    # pop: the heads back off the whole messages
    back, (rd, ro, rl) = ts.pop_chunks(tids[hi], od, oo, ol, h, dtype)
    assert np.array_equal(back, syms[hi].astype(dtype)), "pop: symbols"
    assert _messages(rd, ro, rl) == tails, "pop: what remains"


@pytest.mark.parametrize("lanes,nfull,ragged", [(256, 37, 29), (1024, 1061, 0)])
@pytest.mark.parametrize("dtype,L,h", [(np.uint8, 256, 128), (np.uint8, 4096, 2048), (np.uint16, 128, 64)])
def test_resume_split_identities(gpu, dtype, L, h, lanes, nfull, ragged):
    rng = np.random.default_rng(L + h + nfull)
    tables = _fast_tables(rng)
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    ts.lanes(lanes)
    for kind, seed in [(A.GEN_ZEROS, 0), (A.GEN_RANDOM, 9)]:
        _check_split(ts, tables, dtype, L, h, nfull, ragged, kind, seed, rng)


@pytest.mark.parametrize("which", ["small", "big", "two_ranges"])
def test_resume_split_other_table_sets(gpu, which):
    rng = np.random.default_rng(300 + len(which))
    tables = {"small": _small_norm_tables, "big": _big_norm_tables, "two_ranges": _two_range_tables}[which](rng)
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    assert (ts.fast() == 0) == (which == "two_ranges")
    for kind, seed in [(A.GEN_ZEROS, 0), (A.GEN_RANDOM, 4)]:
        _check_split(ts, tables, np.uint8, 256, 128, 37, 29, kind, seed, rng)


def _block_tids(rng, ntables, nchunks, L, block=16):
    """Table ids constant per 16-position block: a few push_iid calls per chunk in the oracle."""
    return np.repeat(rng.integers(0, ntables, size=nchunks * L // block), block).astype(np.uint32)


def _block_syms(rng, tables, tids):
    syms = np.zeros(len(tids), np.uint64)
    for t, m in enumerate(tables):
        sel = tids == t
        syms[sel] = _sample(rng, m, int(sel.sum()))
    return syms


def test_resume_push_every_start_position(gpu):
    """First-stage messages of 0..300 symbols: the input lengths cover every residue mod 128 and
    both parities of the 128-B page index; then a fixed 128-symbol u8 push onto each."""
    rng = np.random.default_rng(41)
    tables = _fast_tables(rng)
    ocats = [orc.Categorical(m) for m in tables]
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    nchunks, L = 2 * 301, 128
    first = []
    for c in range(nchunks):
        m = orc.Message.zeros()
        assert ocats[c % 5].push_iid(m, _sample(rng, tables[c % 5], c % 301)) == 0
        first.append(m.flatten())
    lens = np.array([len(b) for b in first])
    assert len(set(lens % 128)) == 128 and set((lens // 128) % 2) == {0, 1}
    tids = _block_tids(rng, len(tables), nchunks, L)
    syms = _block_syms(rng, tables, tids)
    pd, po, pl = ts.push_chunks(tids, syms.astype(np.uint8), L, *_container(first))
    got = _messages(pd, po, pl)
    for c in range(nchunks):
        assert got[c] == _orc_push(ocats, first[c], tids[c * L:(c + 1) * L], syms[c * L:(c + 1) * L]), f"chunk {c}"


def _to_slots(torch, msgs, cap):
    h = np.zeros((len(msgs), cap), np.uint8)
    for c, b in enumerate(msgs):
        h[c, :len(b)] = np.frombuffer(b, np.uint8)
    return (torch.from_numpy(h.reshape(-1)).cuda(),
            torch.from_numpy(np.array([len(b) for b in msgs], np.int32)).cuda())


def _from_slots(d_slots, d_lens, cap):
    h = d_slots.cpu().numpy().reshape(-1, cap)
    ln = d_lens.cpu().numpy()
    return [bytes(h[c, :ln[c]]) for c in range(len(ln))]


def _odd_messages(rng, ocats, tables, nchunks):
    """Valid messages with, in the same waves: lengths 0-9 of random bytes, nine zero bytes, and
    zero bytes on top of a valid message."""
    msgs = []
    for c in range(nchunks):
        m = orc.Message.zeros()
        ocats[c % 5].push_iid(m, _sample(rng, tables[c % 5], 150 + c % 60))
        valid = m.flatten()
        kind = c % 4
        if kind == 0:
            msgs.append(valid)
        elif kind == 1:
            msgs.append(rng.integers(0, 256, size=(c // 4) % 10, dtype=np.uint8).tobytes())
        elif kind == 2:
            msgs.append(bytes(9) if c % 8 == 2 else valid + bytes(1 + (c // 8) % 11))
        else:
            msgs.append(valid[:(c // 4) % 10])
    return msgs


def test_resume_short_and_odd_messages(gpu):
    """Where the oracle under EMPTY reports exhaustion the GPU reports ANS_E_EXHAUSTED and
    lens[c] == 0; every other chunk matches the oracle's bytes (zero bytes on top of a message are
    consumed by the first pull)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(43)
    tables = _fast_tables(rng)
    ocats = [orc.Categorical(m) for m in tables]
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    nchunks, L, P = 160, 128, 128  # (both 128-B multiples: the fast kernels, which hand such chunks over)
    msgs = _odd_messages(rng, ocats, tables, nchunks)
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    # push L symbols onto each
    tids = _block_tids(rng, len(tables), nchunks, L)
    syms = _block_syms(rng, tables, tids)
    cap = 128 + ts.slot_capacity(L)
    d_slots, d_lens = _to_slots(torch, msgs, cap)
    d_tids = torch.from_numpy(tids.astype(np.uint8)).cuda()
    d_syms = torch.from_numpy(syms.astype(np.uint8)).cuda()
    ts.dev_push(d_tids, d_syms, 1, nchunks * L, L, d_slots, cap, d_lens, status, stream)
    assert gpu.status(status, stream) == A.ANS_E_EXHAUSTED
    got = _from_slots(d_slots, d_lens, cap)
    want = [_orc_push(ocats, msgs[c], tids[c * L:(c + 1) * L], syms[c * L:(c + 1) * L]) for c in range(nchunks)]
    assert any(w is None for w in want) and sum(w is not None for w in want) > nchunks // 4
    for c in range(nchunks):
        assert got[c] == (want[c] or b""), f"push chunk {c}"
    # pop P symbols from each (the valid ones hold at least 150)
    ptids = _block_tids(rng, len(tables), nchunks, P)
    for c in range(0, nchunks, 4):  # the valid messages' first symbols came from table c % 5
        ptids[c * P:(c + 1) * P] = c % 5
    status.zero_()
    d_slots, d_lens = _to_slots(torch, msgs, cap)
    d_ptids = torch.from_numpy(ptids.astype(np.uint8)).cuda()
    d_out = torch.zeros(nchunks * P, dtype=torch.uint8, device="cuda")
    ts.dev_pop(d_ptids, d_slots, cap, d_lens, nchunks * P, P, d_out, 1, status, stream)
    assert gpu.status(status, stream) == A.ANS_E_EXHAUSTED
    got = _from_slots(d_slots, d_lens, cap)
    out = d_out.cpu().numpy()
    want = [_orc_pop(ocats, msgs[c], ptids[c * P:(c + 1) * P]) for c in range(nchunks)]
    assert any(w is None for w in want) and sum(w is not None for w in want) > nchunks // 4
    for c in range(nchunks):
        if want[c] is None:
            assert got[c] == b"", f"pop chunk {c}"
        else:
            assert got[c] == want[c][1] and np.array_equal(out[c * P:(c + 1) * P], want[c][0]), f"pop chunk {c}"


def _renorm_tables():
    """As test_gpu_codecs_fast.py: after E, C's pushes the head is 2^56 - 2^25, below D's
    p K = 2^56 - 1, so D's push takes a byte back and, decoding, C's pop hands one back."""
    return [np.array([1 << 15, 1 << 15], np.uint64),         # E: norm 2^16, p = 2^15
            np.array([1, (1 << 31) - 2], np.uint64),         # C: norm 2^31 - 1, p = 1 (K = 2^25)
            np.array([71755], np.uint64),                    # D: norm 71755 | 2^56 - 1: p K = 2^56 - 1
            np.array([1, (1 << 16) - 1], np.uint64),         # F: norm 2^16, p = 1: 2 bytes, head back to 2^56
            np.array([1, (1 << 24) - 1], np.uint64),         # G: norm 2^24, p = 1: 3 bytes, head back to 2^56
            np.arange(1, 257, dtype=np.uint64) * 97]         # A: an ordinary table for the rest


def test_resume_pop_hands_a_byte_back(gpu):
    """Chunk c is A-table symbols, then D, C, E and a run of F / G (see _renorm_tables): the
    resumed pop of everything up to and including C ends on the pop whose renorm_down hands a byte
    back to the stream (src/ans.rs:246-253; the oracle's tail grows by one there).  The run varies
    per chunk, so that byte lands at every offset of an 8-byte word.  What remains (E and the run
    on the initial message) and the popped symbols equal the oracle's."""
    rng = np.random.default_rng(5)
    tables = _renorm_tables()
    ocats = [orc.Categorical(m) for m in tables]
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    E, C, D, F, G, Atab = range(6)
    nchunks, L = 96, 128
    tids, syms, starts = [], [], [0]
    for c in range(nchunks):
        a, b = c % 17, (c // 17) % 6
        run = [F] * a + [G] * b
        rng.shuffle(run)
        tail = [D, C, E] + run
        head = L - len(tail)
        ss = np.zeros(L, np.uint64)
        ss[:head] = _sample(rng, tables[Atab], head)
        ss[head + 2] = 1
        tids.append(np.concatenate([np.full(head, Atab), np.array(tail)]).astype(np.uint32))
        syms.append(ss)
        starts.append(starts[-1] + head + 2)  # pop through D and C
    alltids, allsyms = np.concatenate(tids), np.concatenate(syms)
    od, oo, ol = orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, allsyms, L, tables=tables, tids=alltids)
    msgs = _messages(od, oo, ol)
    ptids = np.concatenate([t[:s1 - s0] for t, s0, s1 in zip(tids, starts, starts[1:])])
    # the oracle hands a byte back at C's pop
    m = orc.Message.unflatten(msgs[0], orc.EMPTY)
    ocats[Atab].pop_iid(m, starts[1] - 2)
    ocats[D].pop_iid(m, 1)
    before = orc.lib().orc_msg_tail_len(m.h)
    ocats[C].pop_iid(m, 1)
    assert orc.lib().orc_msg_tail_len(m.h) == before + 1
    back, (rd, ro, rl) = ts.pop_var_chunks(ptids, od, oo, ol, np.array(starts, np.uint64), np.uint8)
    got = _messages(rd, ro, rl)
    for c in range(nchunks):
        want_syms, want = _orc_pop(ocats, msgs[c], ptids[starts[c]:starts[c + 1]])
        assert got[c] == want and np.array_equal(back[starts[c]:starts[c + 1]], want_syms), f"chunk {c}"


def test_resume_empty_chunks_grow_by_one_zero_byte(gpu):
    """flatten(unflatten(B)) == B ++ [0]: zero-symbol chunks through the _var entries."""
    rng = np.random.default_rng(6)
    tables = _fast_tables(rng)
    ocats = [orc.Categorical(m) for m in tables]
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    msgs = []
    for c in range(70):
        m = orc.Message.zeros()
        ocats[0].push_iid(m, _sample(rng, tables[0], 20 + c))
        msgs.append(m.flatten())
    msgs[3], msgs[5] = b"", bytes(4)
    counts = np.array([0 if c % 3 else 7 for c in range(70)])
    counts[3] = counts[5] = 0
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n = int(starts[-1])
    tids = np.zeros(n, np.uint32)
    syms = _sample(rng, tables[0], n).astype(np.uint64)
    pd, po, pl = ts.push_var_chunks(tids, syms.astype(np.uint8), starts, *_container(msgs))
    got = _messages(pd, po, pl)
    back, (rd, ro, rl) = ts.pop_var_chunks(tids, *_container(msgs), starts, np.uint8)
    rem = _messages(rd, ro, rl)
    for c in range(70):
        a, b = int(starts[c]), int(starts[c + 1])
        if a == b:
            assert got[c] == msgs[c] + b"\0" and rem[c] == msgs[c] + b"\0", f"chunk {c}"
        else:
            assert got[c] == _orc_push(ocats, msgs[c], tids[a:b], syms[a:b]), f"chunk {c}"
            want_syms, want = _orc_pop(ocats, msgs[c], tids[a:b])
            assert rem[c] == want and np.array_equal(back[a:b], want_syms), f"chunk {c}"


def test_resume_composes_graph_iid(gpu):
    """GraphIID::push (src/graph_codec.rs:31-34, 61-65) as three pushes of different alphabets
    onto one message per graph: sorted edge labels, the dense indicator vector, node labels.  A
    MUTAG-shaped set (10-28 nodes, 7 node labels, 4 edge labels)."""
    rng = np.random.default_rng(7)
    G = 30
    graphs = []
    for _ in range(G):
        n = int(rng.integers(10, 29))
        pairs = [(i, j) for j in range(n) for i in range(j)]
        pick = rng.choice(len(pairs), size=min(len(pairs), n + int(rng.integers(0, 4))), replace=False)
        edges = sorted(pairs[k] for k in pick)
        graphs.append((n, rng.choice(7, size=n, p=[0.72, 0.10, 0.12, 0.02, 0.02, 0.01, 0.01]), edges,
                       rng.choice(4, size=len(edges), p=[0.6, 0.3, 0.08, 0.02])))
    slots = sum(n * (n - 1) // 2 for n, _, _, _ in graphs)
    nedges = sum(len(e) for _, _, e, _ in graphs)
    bern = np.array([slots - nedges, nedges], np.uint64)
    node = np.bincount(np.concatenate([g[1] for g in graphs]), minlength=7).astype(np.uint64)
    edge = np.bincount(np.concatenate([g[3] for g in graphs]), minlength=4).astype(np.uint64)
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in (bern, node, edge)])
    cont = _container([orc.Message.zeros().flatten()] * G)
    stages = [(2, [g[3] for g in graphs]),
              (0, [orc.dense_set(np.array(g[2]).reshape(-1, 2), g[0], False, False) for g in graphs]),
              (1, [g[1] for g in graphs])]
    for t, parts in stages:
        starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
        syms = np.concatenate(parts).astype(np.uint8)
        cont = ts.push_var_chunks(np.full(len(syms), t, np.uint32), syms, starts, *cont)
    got = _messages(*cont)
    for k, (n, nl, edges, el) in enumerate(graphs):
        m = orc.Message.zeros()
        assert orc.graph_iid_push(m, n, nl, edges, el, bern, ("cat", node), ("cat", edge), False, False) == 0
        assert got[k] == m.flatten(), f"graph {k}"


def test_resume_device_entries_and_slot_bound(gpu):
    """ans_dev_independent_push / _pop in place on slots give the host forms' bytes; a slot_cap one
    byte short of the longest result is ANS_E_LEN with lens[c] == 0 for that chunk alone."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(8)
    tables = _fast_tables(rng)
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    L, h, nchunks = 256, 128, 70
    tids, syms, hi, ti = _split_case(rng, tables, L, h, nchunks, 0)
    td, to, tl = ts.encode_chunks(tids[ti], syms[ti].astype(np.uint8), L - h)
    tails = _messages(td, to, tl)
    pd, po, pl = ts.push_chunks(tids[hi], syms[hi].astype(np.uint8), h, td, to, tl)
    whole = _messages(pd, po, pl)
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_tids = torch.from_numpy(tids[hi].astype(np.uint8)).cuda()
    d_syms = torch.from_numpy(syms[hi].astype(np.uint8)).cuda()
    cap = int(tl.max()) + ts.slot_capacity(h)
    d_slots, d_lens = _to_slots(torch, tails, cap)
    ts.dev_push(d_tids, d_syms, 1, nchunks * h, h, d_slots, cap, d_lens, status, stream)
    assert gpu.status(status, stream) == 0
    assert _from_slots(d_slots, d_lens, cap) == whole
    d_out = torch.zeros_like(d_syms)
    ts.dev_pop(d_tids, d_slots, cap, d_lens, nchunks * h, h, d_out, 1, status, stream)
    assert gpu.status(status, stream) == 0
    assert torch.equal(d_out, d_syms)
    assert _from_slots(d_slots, d_lens, cap) == tails
    # one byte short of the longest result (an odd slot_cap: slots at every alignment)
    short = int(pl.max()) - 1
    d_slots, d_lens = _to_slots(torch, tails, short)
    ts.dev_push(d_tids, d_syms, 1, nchunks * h, h, d_slots, short, d_lens, status, stream)
    assert gpu.status(status, stream) == A.ANS_E_LEN
    got = _from_slots(d_slots, d_lens, short)
    for c in range(nchunks):
        assert got[c] == (whole[c] if len(whole[c]) <= short else b""), f"chunk {c}"
    assert sum(g == b"" for g in got) >= 1


def _dev_resume(torch, gpu, ts, msgs, tids, syms, L, cap):
    """ans_dev_independent_push and _pop of L u8 symbols per chunk on copies of msgs in slots of
    cap bytes: (status, messages) of the push, (status, messages, symbols) of the pop."""
    n = len(msgs) * L
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_tids = torch.from_numpy(tids.astype(np.uint8)).cuda()
    d_syms = torch.from_numpy(syms.astype(np.uint8)).cuda()
    d_slots, d_lens = _to_slots(torch, msgs, cap)
    ts.dev_push(d_tids, d_syms, 1, n, L, d_slots, cap, d_lens, status, stream)
    pushed = (gpu.status(status, stream), _from_slots(d_slots, d_lens, cap))
    status.zero_()
    d_slots, d_lens = _to_slots(torch, msgs, cap)
    d_out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ts.dev_pop(d_tids, d_slots, cap, d_lens, n, L, d_out, 1, status, stream)
    return pushed, (gpu.status(status, stream), _from_slots(d_slots, d_lens, cap), d_out.cpu().numpy())


@pytest.mark.parametrize("which,lanes", [("fast", 256), ("fast", 1024), ("small", 256), ("big", 256), ("renorm", 256)])
def test_resume_fast_and_exact_paths_agree_on_arbitrary_messages(gpu, which, lanes):
    """Messages of random bytes (nothing any coder here produced: every handed-back byte is new
    data), a quarter of them topped with eight 0xFF bytes (the push prologue's head just below
    2^64, the top of the renorm word's range).  Slots of a 128-byte multiple take the fast kernels,
    slots one byte wider the exact ones: the same bytes and symbols, and the oracle's."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(900 + len(which) + lanes)
    tables = {"fast": _fast_tables, "small": _small_norm_tables, "big": _big_norm_tables,
              "renorm": lambda r: _renorm_tables()}[which](rng)
    ocats = [orc.Categorical(m) for m in tables]
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    assert ts.fast() != 0
    ts.lanes(lanes)
    nchunks, L = 1061 if lanes == 1024 else 300, 128
    msgs = []
    for c in range(nchunks):
        b = rng.integers(0, 256, size=int(rng.integers(600, 900)), dtype=np.uint8)
        if c % 4 == 0:
            b[-8:] = 0xFF
        msgs.append(b.tobytes())
    tids = _block_tids(rng, len(tables), nchunks, L)
    syms = _block_syms(rng, tables, tids)
    cap = 1024 + ts.slot_capacity(L)
    assert cap % 128 == 0
    fast_push, fast_pop = _dev_resume(torch, gpu, ts, msgs, tids, syms, L, cap)
    exact_push, exact_pop = _dev_resume(torch, gpu, ts, msgs, tids, syms, L, cap + 1)
    assert fast_push[0] == exact_push[0] == 0 and fast_pop[0] == exact_pop[0] == 0
    assert fast_push[1] == exact_push[1], "push: fast and exact bytes"
    assert fast_pop[1] == exact_pop[1] and np.array_equal(fast_pop[2], exact_pop[2]), "pop: fast and exact"
    for c in range(0, nchunks, 7 if lanes == 1024 else 1):
        t, x = tids[c * L:(c + 1) * L], syms[c * L:(c + 1) * L]
        assert fast_push[1][c] == _orc_push(ocats, msgs[c], t, x), f"push chunk {c}"
        want_syms, want = _orc_pop(ocats, msgs[c], t)
        assert fast_pop[1][c] == want and np.array_equal(fast_pop[2][c * L:(c + 1) * L], want_syms), f"pop chunk {c}"


def test_resume_fast_pop_stores_a_new_handed_back_byte(gpu):
    """The fast decoder's hand-back with a byte the stream never held.  Chunk c pops C
    (norm 2^31 - 1, bound 2^56 - 2^25), then X (norm 2,147,437,313: 2^56 mod norm is almost 2^31,
    so its bound lies 2^31 below 2^56), then 126 ordinary symbols, from random bytes topped with
    F0 FF FF FF: the unflatten's head is just under 2^64 - 2^36, C's pop (head = p q + r,
    p / norm = 1 - 2^-31) rewrites its low bytes and leaves head >> 8 above X's bound, and X's
    renorm_down hands the new low byte back (src/ans.rs:246-253; the oracle's tail grows by one
    there and its byte differs from the message's).  The message lengths put that byte in every
    ring row, row 0 and its mirror included.  Fixed 128-symbol chunks: the fast kernel; the same
    chunks in slots one byte wider: the exact one."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(12)
    norm_x = 2147437313
    assert (1 << 56) % norm_x > 1 << 30
    tables = [np.array([1, (1 << 31) - 2], np.uint64), np.array([1, norm_x - 1], np.uint64),
              rng.integers(1 << 15, 1 << 16, size=256).astype(np.uint64)]
    ocats = [orc.Categorical(m) for m in tables]
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    assert ts.fast() != 0
    nchunks, L = 160, 128
    tids = np.tile(np.array([0, 1] + [2] * (L - 2), np.uint32), nchunks)
    msgs = []
    for c in range(nchunks):
        b = rng.integers(0, 256, size=300 + c, dtype=np.uint8)
        b[-4:] = [0xF0, 0xFF, 0xFF, 0xFF]
        msgs.append(b.tobytes())
        m = orc.Message.unflatten(msgs[c], orc.EMPTY)
        ocats[0].pop_iid(m, 1)
        at = orc.lib().orc_msg_tail_len(m.h)
        ocats[1].pop_iid(m, 1)
        assert orc.lib().orc_msg_tail_len(m.h) == at + 1 and m.flatten()[at] != msgs[c][at], f"chunk {c}"
    syms = np.zeros(nchunks * L, np.uint64)  # (the push half of _dev_resume: any valid symbols)
    cap = 512 + ts.slot_capacity(L)
    _, fast = _dev_resume(torch, gpu, ts, msgs, tids, syms, L, cap)
    _, exact = _dev_resume(torch, gpu, ts, msgs, tids, syms, L, cap + 1)
    assert fast[0] == exact[0] == 0
    for c in range(nchunks):
        want_syms, want = _orc_pop(ocats, msgs[c], tids[c * L:(c + 1) * L])
        assert fast[1][c] == want and np.array_equal(fast[2][c * L:(c + 1) * L], want_syms), f"fast chunk {c}"
        assert exact[1][c] == want and np.array_equal(exact[2][c * L:(c + 1) * L], want_syms), f"exact chunk {c}"
