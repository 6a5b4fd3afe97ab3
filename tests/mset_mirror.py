"""The expected-bytes mirror of recursive multiset shuffle coding, shared by test_mset_host.py and
test_gpu_mset.py (not a test module).  A Python loop over the oracle's Message, written from the
reference (src/recursive/mod.rs:117-148, src/recursive/multiset.rs:13-91, src/recursive/
prefix_orbit.rs:42-136, src/codec.rs:145-181) and sharing no code with the library:
  * T, the values' codec, is orc.Categorical(masses);
  * the orbit distribution over the current prefix is one orc.Categorical(counts in rank order)
    per step (its pop / push are the blanket ones), the rank of a symbol being its position when
    the alphabet is sorted by ascending orbit id;
  * the orbit id is this file's own SipHash-1-3 (std's DefaultHasher::new(), keys 0, 0, fed the
    usize as 8 little-endian bytes)."""
import functools

import numpy as np

from oracle import oracle as orc

M64 = (1 << 64) - 1


def _rotl(v, s):
    return ((v << s) | (v >> (64 - s))) & M64


def siphash13_usize(x):
    v = [0x736f6d6570736575, 0x646f72616e646f6d, 0x6c7967656e657261, 0x7465646279746573]

    def rnd():
        v[0] = (v[0] + v[1]) & M64
        v[1] = _rotl(v[1], 13) ^ v[0]
        v[0] = _rotl(v[0], 32)
        v[2] = (v[2] + v[3]) & M64
        v[3] = _rotl(v[3], 16) ^ v[2]
        v[0] = (v[0] + v[3]) & M64
        v[3] = _rotl(v[3], 21) ^ v[0]
        v[2] = (v[2] + v[1]) & M64
        v[1] = _rotl(v[1], 17) ^ v[2]
        v[2] = _rotl(v[2], 32)

    for block in (x & M64, 8 << 56):  # the value's 8 bytes, then the final block: length in the top byte
        v[3] ^= block
        rnd()
        v[0] ^= block
    v[2] ^= 0xFF
    rnd()
    rnd()
    rnd()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


@functools.lru_cache(maxsize=None)
def ranks(nsym):
    """(rank[s], sym_of_rank[r]) of the alphabet 0 .. nsym-1."""
    ids = [siphash13_usize(s) for s in range(nsym)]
    assert len(set(ids)) == nsym
    sym_of_rank = sorted(range(nsym), key=ids.__getitem__)
    rank = [0] * nsym
    for r, s in enumerate(sym_of_rank):
        rank[s] = r
    return rank, sym_of_rank


class Mirror:
    def __init__(self, masses):
        self.masses = np.asarray(masses, dtype=np.uint64)
        self.T = orc.Categorical(self.masses)
        self.nsym = len(self.masses)
        self.rank, self.sym_of_rank = ranks(self.nsym)

    def push(self, m, values):
        """ShuffleCodec::push of the multiset onto the oracle Message m; False on exhaustion."""
        cnt = np.zeros(self.nsym, np.uint64)
        for x in values:
            cnt[self.rank[int(x)]] += 1
        for _ in range(len(values)):
            try:
                r = orc.Categorical(cnt).pop(m)  # the blanket pop, norm = the values left
            except RuntimeError:
                return False
            if m.err:
                return False
            cnt[r] -= 1
            if self.T.push(m, self.sym_of_rank[r]) or m.err:
                return False
        return True

    def pop(self, m, n):
        """ShuffleCodec::pop of n values: the values in pop order, or None on exhaustion."""
        cnt = np.zeros(self.nsym, np.uint64)
        out = []
        for _ in range(n):
            try:
                s = self.T.pop(m)
            except RuntimeError:
                return None
            if m.err:
                return None
            out.append(s)
            r = self.rank[s]
            cnt[r] += 1
            if orc.Categorical(cnt).push(m, r) or m.err:  # the blanket push, norm = the values so far
                return None
        return out

    def push_bytes(self, seed, values):
        """flatten(push(unflatten(seed, EMPTY), values)), or None on exhaustion."""
        m = orc.Message.unflatten(seed, orc.EMPTY)
        return m.flatten() if self.push(m, values) else None

    def pop_bytes(self, data, n):
        """(values in pop order, flatten of what remains) from unflatten(data, EMPTY), or None."""
        m = orc.Message.unflatten(data, orc.EMPTY)
        vals = self.pop(m, n)
        return None if vals is None else (vals, m.flatten())


def seeds(rng, nchunks, nbytes=64):
    """Random seed messages with a nonzero top byte."""
    out = []
    for _ in range(nchunks):
        b = rng.integers(0, 256, nbytes, dtype=np.uint8)
        b[-1] = rng.integers(1, 256)
        out.append(b.tobytes())
    return out
