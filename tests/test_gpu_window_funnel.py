"""The LDS-row encoder's sliding-window byte funnel on the GPU (ans_funnel.hpp WindowFunnelT in
ans_fast.hpp k_encode) against the oracle, byte for byte.

k_encode takes the window funnel in every instantiation whose pushes emit at most three bytes
(KMAX <= 3) and keeps the dword-aligned funnel for KMAX = 4.  Each case here names the
instantiation that must run through the context's launch record and compares every
chunk's length and every stream byte up to that length with oracle.encode_chunks; the slot bytes
past a stream's end are unspecified (stale ring rows) and are not compared.

Shapes: 520 chunks, so two 512-lane workgroups run and the second is partly filled.
  * 320 u8 symbols a chunk: streams of more than four 64-byte pages, so the two-page ring laps
    more than twice and pages leave both as pairs and as a last odd one.  320 bytes are not a
    multiple of the encoder's 128-byte symbol groups, so this call runs the staged (var=1) form;
  * 384 u8 symbols a chunk (three groups): the fixed-chunk form (var=0, the mass word's top byte
    carrying the renorm count where every mass is below 2^24), which is the bench's C3 kernel;
  * variable chunks of 0, 1, 15, 16, 17 and 320 symbols in turn: the empty stream (the flatten
    alone), chunks below, at and just past one 16-symbol unit, and the long one.
Tables of kmax 1, 2 and 3 (the ladder instantiates KMAX = max(kmax, 2), so the records read
kmax=2, kmax=2 and kmax=3) on the window funnel and one of kmax 4 on the old funnel, each from
Message::zeros() and Message::random(seed + c) initial messages.
"""
import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

NCHUNKS = 520
M18 = 1 << 18
TABLES = {
    # name: (masses, kmax the reference's renorm gives the table)
    "k1": (np.asarray([M18] * 256, np.uint64), 1),
    "k2": (np.asarray([1 << 12] * 8 + [M18] * 248, np.uint64), 2),
    "k3": (np.asarray([256] + [M18] * 255, np.uint64), 3),
    "k4": (np.asarray([1] + [M18] * 255, np.uint64), 4),
}
GENS = [("zeros", A.GEN_ZEROS, orc.ZEROS, 0), ("random", A.GEN_RANDOM, orc.RANDOM, 77)]
VAR_LENGTHS = [0, 1, 15, 16, 17, 320]


def _kmax(masses):
    m = [int(x) for x in masses]
    K = (1 << 56) // sum(m)
    return max(max(j for j in range(1, 5) if p * K << (8 * j) < 1 << 64) for p in m)


def _record(kmax, var):
    # (every table here: 2^16 <= norm <= 2^31, K < 2^32, every mass below 2^24)
    return f"k_encode<u8,kmax={max(kmax, 2)},k32=1,grows=0,var={int(var)},nr=std,m24={int(not var)}>"


def _draw(masses, n, seed):
    """Half iid from the table, half uniform over its symbols, so the rare rows that emit the
    table's kmax bytes are coded many times in every chunk."""
    rng = np.random.default_rng(seed)
    syms = orc.gen_iid(masses, seed, 0, n)
    mask = rng.random(n) < 0.5
    syms[mask] = rng.integers(0, len(masses), size=int(mask.sum()))
    return syms.astype(np.uint8)


def test_tables_have_the_declared_kmax():
    for name, (masses, kmax) in TABLES.items():
        assert _kmax(masses) == kmax, name
        assert (1 << 16) <= int(masses.sum()) <= (1 << 31) and int(masses.max()) < (1 << 24)
        assert (1 << 56) // int(masses.sum()) < (1 << 32)


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


_tables_on_gpu = {}


def _gpu_table(gpu, name):
    if name not in _tables_on_gpu:
        _tables_on_gpu[name] = A.GpuTable(gpu, A.Categorical(TABLES[name][0]))
    return _tables_on_gpu[name]


@pytest.mark.gpu
@pytest.mark.parametrize("gen", GENS, ids=[g[0] for g in GENS])
@pytest.mark.parametrize("chunk_len", [320, 384])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_chunks_match_oracle(gpu, name, chunk_len, gen):
    torch = pytest.importorskip("torch")
    _, gkind, okind, seed = gen
    masses, kmax = TABLES[name]
    gt = _gpu_table(gpu, name)
    n = NCHUNKS * chunk_len
    syms = _draw(masses, n, 3)
    cap = gt.slot_capacity(chunk_len)
    stream = torch.cuda.Stream()
    d_syms = torch.from_numpy(syms).cuda()
    slots = torch.zeros(NCHUNKS * cap, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(NCHUNKS, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    gt.dev_encode(d_syms, 1, n, chunk_len, slots, cap, d_lens, status, stream, gen_kind=gkind, seed=seed)
    assert gpu.last_launch() == _record(kmax, var=chunk_len % 128 != 0)
    assert gpu.status(status, stream) == 0
    odata, _, olens = orc.encode_chunks(masses, syms, chunk_len, kind=okind, seed=seed)
    lens = d_lens.cpu().numpy().astype(np.int64)
    assert np.array_equal(lens, olens.astype(np.int64)), "every chunk's stream length"
    assert int(lens.min()) > 4 * 64, "streams of more than four pages"
    s = slots.cpu().numpy().reshape(NCHUNKS, cap)
    got = s[np.arange(cap)[None, :] < lens[:, None]]  # every stream's bytes up to its length
    assert got.tobytes() == odata.tobytes(), "every chunk's bytes"
    out = torch.zeros_like(d_syms)
    gt.dev_decode(slots, None, cap, d_lens, n, chunk_len, out, 1, status, stream, gen_kind=gkind, seed=seed)
    assert gpu.status(status, stream) == 0
    assert torch.equal(out, d_syms), "decode returns the symbols"


@pytest.mark.gpu
@pytest.mark.parametrize("gen", GENS, ids=[g[0] for g in GENS])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_variable_chunks_match_oracle(gpu, name, gen):
    _, gkind, okind, seed = gen
    masses, kmax = TABLES[name]
    gt = _gpu_table(gpu, name)
    sizes = np.asarray([VAR_LENGTHS[c % len(VAR_LENGTHS)] for c in range(NCHUNKS)], np.uint64)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    syms = _draw(masses, int(starts[-1]), 5)
    data, offs, lens = gt.encode_var_chunks(syms, starts, gen_kind=gkind, seed=seed)
    assert gpu.last_launch() == _record(kmax, var=True)
    assert np.array_equal(offs, np.cumsum(lens) - lens)
    for c in range(NCHUNKS):
        a, b = int(starts[c]), int(starts[c + 1])
        if b > a:
            od, _, _ = orc.encode_chunks(masses, syms[a:b], b - a, kind=okind, seed=seed + c)
            want = od.tobytes()
        else:
            m0 = orc.Message.zeros() if okind == orc.ZEROS else orc.Message.random(seed + c)
            want = bytes(m0.flatten())
        assert int(lens[c]) == len(want), c
        assert data[int(offs[c]):int(offs[c] + lens[c])].tobytes() == want, c
    back = gt.decode_var_chunks(data, offs, lens, starts, syms.dtype, gen_kind=gkind, seed=seed)
    assert np.array_equal(back, syms)
