"""The expected-bytes mirror of the autoregressive Erdős–Rényi graph codecs, shared by
test_arer_host.py, test_gpu_arer.py and test_gpu_arer_lane_reuse.py (not a test module).
Autoregressive(ErdosRenyiSliceCodecs) and ShuffleCodec<ErdosRenyiSliceCodecs, WLOrbitCodecs<
GraphPrefix>> with wl_iter = 0 as a Python loop over the oracle's Message, written from the
reference line by line (src/recursive/mod.rs:117-148, 190-216, src/recursive/graph/mod.rs:28-104,
src/recursive/graph/slice.rs:16-59, src/recursive/graph/incomplete.rs:45-51, 189-236,
src/recursive/prefix_orbit.rs:42-136, src/graph.rs:304-331, src/graph_codec.rs:105-171,
src/codec.rs:405-424) and sharing no code with the library.  Deliberately naive:
  * the graph is one Python set of neighbours per position, the swap is the reference's;
  * the ids of the known nodes are computed afresh from the prefix's graph at every step
    (WLOrbitCodecs::apply), not carried along, so nothing here assumes that a known node's
    degree is its degree in the whole graph;
  * the orbit distribution is the sorted list of the prefix's ids, one orc.Categorical per step;
  * the ids are this file's own SipHash-1-3 over the words a tuple feeds DefaultHasher."""
import functools

import numpy as np

from oracle import oracle as orc

from polya_mirror import E_EXHAUSTED, E_SYMBOL, E_ZERO_MASS, Fail, _pop, _push  # noqa: F401  (the blanket steps)

NONE, ONE_CLASS, DEGREE = 0, 1, 2
M64 = (1 << 64) - 1


def _rotl(v, s):
    return ((v << s) | (v >> (64 - s))) & M64


def siphash13_words(words):
    """DefaultHasher::new() (SipHash-1-3, keys 0, 0) fed the 8-byte little-endian words in turn."""
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

    for block in [w & M64 for w in words] + [(8 * len(words)) << 56]:
        v[3] ^= block
        rnd()
        v[0] ^= block
    v[2] ^= 0xFF
    rnd()
    rnd()
    rnd()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


# hash(((), None::<usize>)), incomplete.rs:195-196: () feeds nothing, None its isize discriminant 0
H0 = siphash13_words([0])


@functools.lru_cache(maxsize=None)
def degree_id(d):
    """hash((h0, vec![&(); d])), incomplete.rs:49-51: h0, then the vector's usize length prefix."""
    return siphash13_words([H0, d])


class Mirror:
    def __init__(self, mass, norm, num_nodes, loops, orbits):
        self.masses = np.array([norm - mass, mass], np.uint64)  # Bernoulli::new, src/codec.rs:125-128
        self.has_edge = orc.Categorical(self.masses)
        self.n, self.loops, self.orbits = num_nodes, loops, orbits

    # ---- ErdosRenyiSliceCodecs::apply (slice.rs:37-50) and DenseSetIID (graph_codec.rs:111-138)
    def _alphabet(self, node):
        return [(node, j) for j in range(node + 1, self.n)] + ([(node, node)] if self.loops else [])

    def _slice_push(self, m, node, edges):
        dense = [e in edges for e in self._alphabet(node)]
        assert sum(dense) == len(edges)  # graph_codec.rs:136
        for b in reversed(dense):  # IID::push, src/codec.rs:415-420
            if int(self.masses[int(b)]) == 0:
                raise Fail(E_ZERO_MASS)  # src/ans.rs:98
            if self.has_edge.push(m, int(b)) or m.err:
                raise Fail(E_EXHAUSTED)

    def _slice_pop(self, m, node):
        try:
            dense = [self.has_edge.pop(m) for _ in self._alphabet(node)]  # IID::pop, src/codec.rs:422-424
        except RuntimeError:
            raise Fail(E_EXHAUSTED)
        if m.err:
            raise Fail(E_EXHAUSTED)
        return [e for e, b in zip(self._alphabet(node), dense) if b]

    # ---- WLOrbitCodecs::apply over the known positions (incomplete.rs:193-210, num_iter = 0)
    def _orbit_masses(self, adj, length):
        if self.orbits == DEGREE:
            ids = [degree_id(len(adj[p])) for p in range(length)]
        else:
            ids = [H0] * length
        present = sorted(set(ids))  # MutCategorical: ascending ids, src/codec.rs:145-181
        return ids, present, [ids.count(i) for i in present]

    def push(self, m, edges):
        """Returns perm: perm[position] = the input node that ended there."""
        n = self.n
        edges = [(int(i), int(j)) for i, j in edges]
        for i, j in edges:
            if i > j or j >= n or (i == j and not self.loops):
                raise Fail(E_SYMBOL)
        if len(set(edges)) != len(edges):
            raise Fail(E_SYMBOL)
        adj = [set() for _ in range(n)]
        for i, j in edges:
            adj[i].add(j)
            adj[j].add(i)
        perm = list(range(n))
        for length in range(n, 0, -1):
            last = length - 1
            if self.orbits != NONE:  # recursive/mod.rs:123-127
                ids, present, counts = self._orbit_masses(adj, length)
                index = ids.index(present[_pop(m, counts)])  # prefix_orbit.rs:117-119
                if index != last:  # graph.rs:304-331
                    adj[index], adj[last] = adj[last], adj[index]
                    nei, nej = set(adj[index]), set(adj[last])
                    for v in sorted(nei | nej | {index, last}):
                        ei, ej = last in adj[v], index in adj[v]
                        adj[v].discard(last)
                        adj[v].discard(index)
                        if ei:
                            adj[v].add(index)
                        if ej:
                            adj[v].add(last)
                    perm[index], perm[last] = perm[last], perm[index]
            # pop_slice, graph/mod.rs:57-66: the edges to the unknown positions (last included)
            slice_edges = [(last, j) for j in sorted(adj[last]) if j >= last]
            for _, j in slice_edges:
                adj[last].discard(j)
                adj[j].discard(last)
            self._slice_push(m, last, slice_edges)
        assert not any(adj)  # empty_prefix is a ConstantCodec, slice.rs:55-58
        return perm

    def pop(self, m):
        """The pairs in pop order."""
        adj = [set() for _ in range(self.n)]
        out = []
        for v in range(self.n):
            for i, j in self._slice_pop(m, v):  # push_slice, graph/mod.rs:82-95
                assert j not in adj[i]
                adj[i].add(j)
                adj[j].add(i)
                out.append((i, j))
            if self.orbits != NONE:  # recursive/mod.rs:143-145
                ids, present, counts = self._orbit_masses(adj, v + 1)
                _push(m, counts, present.index(ids[v]))
        return out

    def push_bytes(self, seed, edges):
        """(flatten(push(unflatten(seed, EMPTY), edges)), perm)."""
        m = orc.Message.unflatten(seed, orc.EMPTY)
        perm = self.push(m, edges)
        return m.flatten(), perm

    def pop_bytes(self, data):
        """(pairs, flatten of what remains) from unflatten(data, EMPTY)."""
        m = orc.Message.unflatten(data, orc.EMPTY)
        edges = self.pop(m)
        return edges, m.flatten()


def relabelled(edges, perm):
    """The input graph as the decoder sees it: the pair of positions of every input pair, sorted."""
    pos = {node: p for p, node in enumerate(perm)}
    return sorted(tuple(sorted((pos[i], pos[j]))) for i, j in edges)


# ---- the shapes the tests share: (name, n, edges, loops)
def shapes():
    from polya_mirror import complete, random_graph
    rng = np.random.default_rng(41)
    return [
        ("n=0", 0, [], False),
        ("n=1", 1, [], False),
        ("n=1 with its loop", 1, [(0, 0)], True),
        ("n=2", 2, [(0, 1)], False),
        ("C8", 8, [(v, v + 1) for v in range(7)] + [(0, 7)], False),
        ("K1,7", 8, [(0, v) for v in range(1, 8)], False),
        ("path of 6", 6, [(v, v + 1) for v in range(5)], False),
        ("K6", 6, complete(6), False),
        ("five isolated nodes", 5, [], False),
        ("n=40 E=90", 40, random_graph(rng, 40, 90), False),
        ("n=9 E=20 with loops", 9, random_graph(rng, 9, 20, loops=True), True),
        ("n=64 E=200", 64, random_graph(rng, 64, 200), False),
    ]
