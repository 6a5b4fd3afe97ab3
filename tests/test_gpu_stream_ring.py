"""The shared stream ring (csrc/ans_ring.hpp DecRingT: start / fetch_top / fetch_pair / point) at
its boundaries, on each of its four layouts.

One ring serves every fast decoder, so it is pinned where it can go wrong: the top pair that must
not read past the stream's last line, the page-landing rule, the zero pair below a stream's start
and the four byte phases of a stream's start in a dense container.  Each case codes 1,025 chunks
(one more than the widest workgroup) of one fixed chunk_len.  Chunk c takes its first
c * chunk_len // 1024 symbols from draws of the table and fills the rest with the table's most
probable symbol, so the stream lengths sweep from the shortest possible stream (under one page)
to past three 128-B pairs, across the lanes of every wave.  The draws are the census' (half iid
from the table, half uniform over its symbols): a table whose commonest symbol is cheap enough for
a one-page stream has too little entropy for iid draws alone to pass three pairs at the same
chunk_len.  The tables give that symbol three quarters of the norm.

Everything is compared with the oracle (oracle/oracle.py encode_chunks / codec_encode_chunks): the
bytes and lengths of the GPU encode, and the symbols of two GPU decodes, from slots and from a
dense container.  That the input reaches the boundaries is asserted from the oracle's lengths alone
(_assert_sweep; also a CPU test): every top page index 0..5 (both parities), stream lengths in each
of the residues 0, 1, 60, 61, 63 mod 64, and dense offsets of all four values mod 4.
"""
import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

NCHUNKS = 1025
RESIDUES = (0, 1, 60, 61, 63)


def _heavy(nsym, light):
    """nsym symbols: symbol 0 holds three quarters of the norm, the others `light` each."""
    return np.asarray([3 * light * (nsym - 1)] + [light] * (nsym - 1), dtype=np.uint64)


# id -> (tables, symbol bytes, chunk_len, lanes).  chunk_len: the smallest multiple of a 128-B symbol
# group at which the sweep's longest streams pass 384 bytes (checked by _assert_sweep).
LAYOUTS = {
    "fast-1024": ([_heavy(256, 1 << 10)], 1, 512, None),              # k_decode: 256 symbols, u8
    "wide-512": ([_heavy(32769, 64)], 2, 320, None),                  # k_decode_w: norm 2^23, u16
    "mfast-256": ([_heavy(256, 1 << 10), _heavy(256, 1 << 10)[::-1].copy()], 1, 512, 256),
    "mfast-1024": ([_heavy(256, 1 << 10), _heavy(256, 1 << 10)[::-1].copy()], 1, 512, 1024),
}
_cases = {}


def _draw(masses, n, seed):
    rng = np.random.default_rng(seed)
    syms = orc.gen_iid(masses, seed, 0, n)
    mask = rng.random(n) < 0.5
    syms[mask] = rng.integers(0, len(masses), size=int(mask.sum()))
    return syms.astype(np.uint64)


def _case(name):
    """(tables, w, L, lanes, tids, syms, the oracle's container), computed once per layout."""
    if name not in _cases:
        tables, w, L, lanes = LAYOUTS[name]
        n = NCHUNKS * L
        tids = np.random.default_rng(2).integers(0, len(tables), size=n).astype(np.uint32)
        syms = np.zeros(n, np.uint64)
        for t, m in enumerate(tables):
            sel = tids == t
            syms[sel] = _draw(m, int(sel.sum()), 5 + t)
        keep = np.arange(L)[None, :] < (np.arange(NCHUNKS) * L // 1024)[:, None]  # chunk c: its first c L / 1024
        common = np.asarray([int(np.argmax(m)) for m in tables], np.uint64)[tids]
        syms = np.where(keep.ravel(), syms, common)
        if len(tables) == 1:
            want = orc.encode_chunks(tables[0], syms, L)
        else:
            want = orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, syms, L, tables=tables, tids=tids)
        _cases[name] = (tables, w, L, lanes, tids, syms, want)
    return _cases[name]


def _assert_sweep(lens, offsets):
    lens, offsets = np.asarray(lens, np.int64), np.asarray(offsets, np.int64)
    top = (lens - 1) >> 6
    assert set(range(6)) <= set(top.tolist()), "every top page index 0..5 (both parities)"
    assert lens.max() > 384, "past three pairs"
    assert set(RESIDUES) <= set((lens % 64).tolist()), "lengths at the page boundaries"
    assert set((offsets & 3).tolist()) == {0, 1, 2, 3}, "dense stream starts on all four byte phases"


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_sweep_reaches_the_ring_boundaries(name):
    """(CPU) the oracle's lengths of each layout's input cover the boundaries the GPU cases pin."""
    _, _, _, _, _, _, (_, ooffs, olens) = _case(name)
    _assert_sweep(olens, ooffs)


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


def _dev(torch, a, w):
    dt = {1: np.uint8, 2: np.int16}[w]
    return torch.from_numpy(np.ascontiguousarray(a.astype({1: np.uint8, 2: np.uint16}[w]).view(dt))).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_ring_layout_sweep(gpu, name):
    torch = pytest.importorskip("torch")
    tables, w, L, lanes, tids, syms, (odata, ooffs, olens) = _case(name)
    _assert_sweep(olens, ooffs)
    n = NCHUNKS * L
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_syms = _dev(torch, syms, w)
    d_lens = torch.zeros(NCHUNKS, dtype=torch.int32, device="cuda")
    if lanes is None:
        coder = A.GpuTable(gpu, A.Categorical(tables[0]))
        want_dec = "k_decode<u8" if name == "fast-1024" else "k_decode_w<u16"
        enc = lambda slots, cap: coder.dev_encode(d_syms, w, n, L, slots, cap, d_lens, status, stream)  # noqa: E731
        dec = lambda src, offs, cap, out: coder.dev_decode(src, offs, cap, d_lens, n, L, out, w, status, stream)  # noqa: E731
    else:
        coder = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
        assert coder.fast() != 0
        coder.lanes(lanes)
        want_dec = f"k_mdec<indep,u8,spp=16,lanes={lanes},res=0"
        d_tids = torch.from_numpy(tids.astype(np.uint8)).cuda()
        enc = lambda slots, cap: coder.dev_encode(d_tids, d_syms, w, n, L, slots, cap, d_lens, status, stream)  # noqa: E731
        dec = lambda src, offs, cap, out: coder.dev_decode(d_tids, src, offs, cap, d_lens, n, L, out, w, status, stream)  # noqa: E731
    cap = -(-coder.slot_capacity(L) // 128) * 128
    slots = torch.zeros(NCHUNKS * cap, dtype=torch.uint8, device="cuda")
    enc(slots, cap)
    assert gpu.status(status, stream) == 0
    lens = d_lens.cpu().numpy().astype(np.int64)
    assert np.array_equal(lens, olens.astype(np.int64)), "every chunk's stream length"
    s = slots.cpu().numpy().reshape(NCHUNKS, cap)
    assert s[np.arange(cap)[None, :] < lens[:, None]].tobytes() == odata.tobytes(), "every chunk's bytes"
    # decode from the slots, then from the dense container (stream starts at any byte phase)
    out = torch.zeros_like(d_syms)
    dec(slots, None, cap, out)
    assert gpu.last_launch().startswith(want_dec), gpu.last_launch()
    assert gpu.status(status, stream) == 0
    assert torch.equal(out, d_syms), "decode from slots returns the symbols"
    d_offs = torch.from_numpy(ooffs.astype(np.int64)).cuda()
    dense = torch.zeros(len(odata) + 16, dtype=torch.uint8, device="cuda")
    gpu.compact(slots, cap, d_lens, d_offs, NCHUNKS, dense, stream)
    out.zero_()
    dec(dense, d_offs, cap, out)
    assert gpu.last_launch().startswith(want_dec), gpu.last_launch()
    assert gpu.status(status, stream) == 0
    assert dense.cpu().numpy()[:len(odata)].tobytes() == odata.tobytes(), "the dense container"
    assert torch.equal(out, d_syms), "decode from the dense container returns the symbols"


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [256, 1024])
def test_resume_ring_sweep(gpu, lanes):
    """The resume ring (MChainT<kL, true>): half of each chunk popped off the sweep's messages; the
    popped symbols and what remains equal the oracle's, and the rest decodes."""
    tables, w, L, _, tids, syms, (odata, ooffs, olens) = _case(f"mfast-{lanes}")
    _assert_sweep(olens, ooffs)
    h = L // 2
    first = lambda a: a.reshape(NCHUNKS, L)[:, :h].ravel().copy()  # noqa: E731
    second = lambda a: a.reshape(NCHUNKS, L)[:, h:].ravel().copy()  # noqa: E731
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    ts.lanes(lanes)
    back, (rd, ro, rl) = ts.pop_chunks(first(tids), odata, ooffs, olens, h, np.uint8)
    assert f"k_mdec<indep,u8,spp=16,lanes={lanes},res=1" in gpu.last_launch(), gpu.last_launch()
    assert np.array_equal(back, first(syms).astype(np.uint8)), "pop: the first halves"
    wd, wo, wl = orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, second(syms), h, tables=tables, tids=second(tids))
    assert np.array_equal(rl, wl) and np.array_equal(ro, wo) and rd.tobytes() == wd.tobytes(), "pop: what remains"
    rest = ts.decode_chunks(second(tids), rd, ro, rl, h, np.uint8)
    assert np.array_equal(rest, second(syms).astype(np.uint8)), "the rest decodes"
