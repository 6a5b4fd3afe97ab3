"""The decoders' bucket-word lookups on the device against the oracle's streams (the u-domain
decoder's additive words, ans_dec_u.hpp / ans_fast.hpp k_decode kModeU; the
Independent decoder's, ans_mfast.hpp).

Three tables at the ends and the middle of the u-domain's range: norm 2^16 + 1 (the narrowest
buckets), C3's masses, and a norm just under 3,072 * 2^17 (us = 18, the widest; its masses
reach 2^24, so the kernel without the 24-bit product runs too).  Each has a mass-1 symbol and a
zero-mass symbol, set between large neighbours so that no bucket holds a fourth candidate and
the table keeps its u-domain image.  130 chunks of 256 symbols (two waves and a partial one)
in which every positive-mass symbol occurs are encoded by the oracle, laid out in slots,
decoded on the device and compared symbol by symbol.  The Independent decoder reads the same
three tables and two more (position k codes with table k mod 5) over 37 chunks.
"""
import numpy as np
import pytest

import ans_amd as A
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

L = 256
TOP = 3072 << 17  # the largest norm the u-domain takes (bucket width 2^18)


def _with_rare_rows(m, norm=None):
    """m with a zero-mass and a mass-1 symbol, each between the largest neighbours available
    (apart from each other), and the last mass taking up the difference to `norm`."""
    m = np.asarray(m, np.int64).copy()
    near = np.minimum(m[:-4], m[2:-2])  # near[i]: the smaller neighbour of symbol i + 1
    z = 1 + int(np.argmax(near))
    near[max(0, z - 4):z + 3] = 0
    o = 1 + int(np.argmax(near))
    m[z], m[o] = 0, 1
    if norm is not None:
        m[-1] += norm - int(m.sum())
    assert m[-1] > 0 and m[z - 1] > 1 and m[z + 1] > 1 and m[o - 1] > 1 and m[o + 1] > 1
    return m.astype(np.uint64)


def _draws(s):
    return A.splitmix64_np(np.uint64(0xD0C) ^ np.arange(s, s + 256, dtype=np.uint64))


TABLES = {
    "norm_2^16+1": lambda: _with_rare_rows(200 + (_draws(0) & np.uint64(63)), (1 << 16) + 1),
    "c3": lambda: _with_rare_rows(A.c3_masses()),
    "us_18": lambda: _with_rare_rows((1 << 20) + (_draws(256) & np.uint64((1 << 19) - 1)), TOP - 12345),
    "norm_2^20": lambda: _with_rare_rows(3000 + (_draws(512) & np.uint64(2047)), 1 << 20),
    "norm_2^24+3": lambda: _with_rare_rows((1 << 15) + (_draws(768) & np.uint64((1 << 15) - 1)), (1 << 24) + 3),
}


def _symbols(masses, n, seed):
    """Half iid from the table, half uniform over its coded symbols, every one of them present."""
    rng = np.random.default_rng(seed)
    nz = np.flatnonzero(masses)
    syms = orc.gen_iid(masses, seed, 0, n)
    mask = rng.random(n) < 0.5
    syms[mask] = rng.choice(nz, size=int(mask.sum()))
    syms[rng.choice(n, size=len(nz), replace=False)] = nz
    assert set(np.unique(syms)) == set(nz)
    return syms.astype(np.uint32)


def _slots(torch, data, offsets, lens, cap):
    """The oracle's dense streams as fixed slots of `cap` bytes on the device."""
    nch = len(lens)
    assert int(lens.max()) <= cap
    host = np.zeros((nch, cap), np.uint8)
    for c in range(nch):
        host[c, :int(lens[c])] = data[int(offsets[c]):int(offsets[c] + lens[c])]
    return torch.from_numpy(host.ravel()).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()


@pytest.fixture(scope="module")
def gpu():
    return A.Gpu(0)


@pytest.mark.parametrize("name", ["norm_2^16+1", "c3", "us_18"])
def test_u_domain_decoder_reads_the_oracles_streams(gpu, name):
    torch = pytest.importorskip("torch")
    masses = TABLES[name]()
    norm = int(masses.sum())
    assert norm == {"norm_2^16+1": (1 << 16) + 1, "us_18": TOP - 12345}.get(name, norm)
    assert (masses == 0).sum() == 1 and (masses == 1).sum() >= 1
    gt = A.GpuTable(gpu, A.Categorical(masses))
    assert gt.paths() & A.ANS_PATH_DEC_U, hex(gt.paths())
    nch = 130
    syms = _symbols(masses, nch * L, 5)
    data, offsets, lens = orc.encode_chunks(masses, syms, L)
    cap = -(-gt.slot_capacity(L) // 128) * 128
    stream = torch.cuda.Stream()
    slots, d_lens = _slots(torch, data, offsets, lens, cap)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(nch * L, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gt.dev_decode(slots, None, cap, d_lens, nch * L, L, out, 1, status, stream)
    launched = gpu.last_launch()
    assert launched.startswith("k_decode<u8,") and "mode=u," in launched, launched
    assert ("p24=0" in launched) == (name == "us_18"), launched
    assert gpu.status(status, stream) == 0
    assert np.array_equal(out.cpu().numpy(), syms.astype(np.uint8))


def test_independent_decoder_reads_the_oracles_streams(gpu):
    torch = pytest.importorskip("torch")
    tables = [TABLES[k]() for k in ("norm_2^16+1", "c3", "us_18", "norm_2^20", "norm_2^24+3")]
    nch = 37
    n = nch * L
    tids = (np.arange(n) % 5).astype(np.uint32)
    syms = np.zeros(n, np.uint64)
    for t, m in enumerate(tables):
        syms[t::5] = _symbols(m, len(syms[t::5]), 7 + t)
    ts = A.GpuTableSet(gpu, [A.Categorical(m) for m in tables])
    assert ts.fast() != 0
    data, offsets, lens = orc.codec_encode_chunks(orc.CODEC_INDEPENDENT, syms, L, tables=tables, tids=tids)
    cap = -(-ts.slot_capacity(L) // 128) * 128
    stream = torch.cuda.Stream()
    slots, d_lens = _slots(torch, data, offsets, lens, cap)
    d_tids = torch.from_numpy(tids.astype(np.uint8)).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ts.dev_decode(d_tids, slots, None, cap, d_lens, n, L, out, 1, status, stream)
    launched = gpu.last_launch()
    assert launched.startswith("k_mdec<indep,u8,"), launched
    assert gpu.status(status, stream) == 0
    assert np.array_equal(out.cpu().numpy(), syms.astype(np.uint8))
