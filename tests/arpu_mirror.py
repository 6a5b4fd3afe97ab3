"""The expected-bytes mirror of the autoregressive Pólya urn graph codecs, shared by
test_arpu_host.py, test_gpu_arpu.py and test_gpu_arpu_lane_reuse.py (not a test module).
Autoregressive(PolyaUrnSliceCodecs) and ShuffleCodec<PolyaUrnSliceCodecs, WLOrbitCodecs<GraphPrefix>>
with wl_iter = 0 as a Python loop over the oracle's Message, written from the reference line by line
(src/recursive/graph/slice.rs:61-230, src/recursive/mod.rs:117-148, 190-216,
src/recursive/graph/mod.rs:53-104, src/graph_codec.rs:58-94, src/codec.rs:549-611,
src/recursive/multiset.rs:126-136) and sharing no code with the library.  Deliberately naive:
  * the urn is a plain list of masses over the positions, zero outside the urn's keys, and it is
    built afresh from the prefix's graph by PolyaUrnSliceCodec::from_graph's formula before every
    slice; nothing here carries an urn from one slice to the next, so nothing assumes what
    update_after_pop_slice / update_after_push_slice are argued to leave behind;
  * the plain layer of a slice's multiset codec is polya_mirror's perm_pop / rcoset_* / canon on the
    slice's pairs, the joint layer its loop over sorted ids with polya_mirror's SipHash of a pair;
  * the shuffle loop over the graph, the swap and the orbit masses are arer_mirror's, restated here
    around this model's slices (arer_mirror's loop does not hand the prefix's graph to its slices)."""
import numpy as np

from oracle import oracle as orc

import arer_mirror as AM
from polya_mirror import (E_EXHAUSTED, E_SYMBOL, Fail, _pop, _push, _uniform, _inverse,  # noqa: F401
                          canon, chain_of, permuted, rcoset_pop, rcoset_push, siphash13_pair)

NONE, ONE_CLASS, DEGREE = AM.NONE, AM.ONE_CLASS, AM.DEGREE
relabelled = AM.relabelled


def get_bits(x):  # LogUniform::get_bits, src/codec.rs:608-610
    return int(x).bit_length()


def log_uniform_push(m, excl_max_bits, x):  # src/codec.rs:569-577, 597-601
    bits = get_bits(x)
    assert bits < excl_max_bits + 1
    if bits != 0:
        size = 1 << (bits - 1)
        _push(m, _uniform(size), x & ~size)
    _push(m, _uniform(excl_max_bits + 1), bits)


def log_uniform_pop(m, excl_max_bits):  # src/codec.rs:579-585
    bits = _pop(m, _uniform(excl_max_bits + 1))
    if bits == 0:
        return 0
    size = 1 << (bits - 1)
    return _pop(m, _uniform(size)) | size


class Mirror(AM.Mirror):
    """arer_mirror's Mirror lends _orbit_masses (WLOrbitCodecs::apply); the slices are this file's."""

    def __init__(self, num_nodes, loops, orbits):
        self.n, self.loops, self.orbits = num_nodes, loops, orbits

    # ---- PolyaUrnSliceCodec::from_graph (slice.rs:78-86): the prefix holds `node` known positions
    def _urn(self, adj, node):
        masses = [0] * self.n
        for j in range(node + (0 if self.loops else 1), self.n):
            masses[j] = len(adj[j]) + 1
        return masses

    def _slice_len(self, node):  # len_codec, slice.rs:72-76
        return int(self.loops) + (self.n - node - 1)

    # ---- PolyaUrnSliceEdgeIndicesCodec (slice.rs:137-173) on the urn `masses`
    @staticmethod
    def _ordered_push(m, masses, node, x):
        masses = list(masses)
        taken = []
        for node_, j in x:
            assert node_ == node
            taken.append(masses[j])  # remove_all
            masses[j] = 0
        for (_, j), mass in zip(reversed(x), reversed(taken)):
            masses[j] += mass  # insert
            _push(m, masses, j)

    @staticmethod
    def _ordered_pop(m, masses, node, length):
        masses = list(masses)
        edges = []
        for _ in range(length):
            j = _pop(m, masses)
            masses[j] = 0
            edges.append((node, j))
        return edges

    # ---- multiset_shuffle_codec (src/recursive/multiset.rs:126-136) around it
    def _multiset_push(self, m, masses, node, edges):
        if len(edges) <= 11:  # plain_shuffle_codec, src/plain/mod.rs:111-116
            x = permuted(edges, canon(edges))
            x = permuted(x, rcoset_pop(m, chain_of(x)))
            self._ordered_push(m, masses, node, x)
            return
        x = list(edges)  # PrefixShuffleCodec::push over JointPrefix, src/recursive/mod.rs:117-134
        ids = [siphash13_pair(i, j) for i, j in x]
        assert len(set(ids)) == len(ids)
        for length in range(len(x), 0, -1):
            present = sorted(ids[:length])
            index = ids.index(present[_pop(m, _uniform(length))])
            last = length - 1
            x[index], x[last] = x[last], x[index]
            ids[index], ids[last] = ids[last], ids[index]
        self._ordered_push(m, masses, node, x)

    def _multiset_pop(self, m, masses, node, length):
        y = self._ordered_pop(m, masses, node, length)
        if length <= 11:  # src/plain/mod.rs:118-123
            c = canon(y)
            x = permuted(y, c)
            rcoset_push(m, chain_of(x), _inverse(c))
            return x
        ids = [siphash13_pair(i, j) for i, j in y]  # src/recursive/mod.rs:136-148
        assert len(set(ids)) == len(ids)
        for k in range(length):
            present = sorted(ids[:k + 1])
            _push(m, _uniform(k + 1), present.index(ids[k]))
        return y

    # ---- PolyaUrnSliceCodec under EdgesIID (slice.rs:99-117, graph_codec.rs:58-72; unit labels)
    def _slice_push(self, m, adj, node, edges):
        masses = self._urn(adj, node)
        edges = sorted(edges)  # EdgesIID::split
        if len(edges) > 0:
            self._multiset_push(m, masses, node, edges)
        log_uniform_push(m, get_bits(self._slice_len(node)) + 1, len(edges))

    def _slice_pop(self, m, adj, node):
        masses = self._urn(adj, node)
        length = log_uniform_pop(m, get_bits(self._slice_len(node)) + 1)
        if length > sum(1 for x in masses if x):
            raise Fail(E_SYMBOL)  # the reference would panic in the urn; only bytes no push wrote get here
        edges = self._multiset_pop(m, masses, node, length) if length > 0 else []
        return sorted(edges)  # EdgesIID::pop sorts

    # ---- the shuffle loop (recursive/mod.rs:117-148), as arer_mirror has it
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
                    for v in sorted(set(adj[index]) | set(adj[last]) | {index, last}):
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
            self._slice_push(m, adj, last, slice_edges)
        assert not any(adj)
        return perm

    def pop(self, m):
        """The pairs in pop order."""
        adj = [set() for _ in range(self.n)]
        out = []
        for v in range(self.n):
            for i, j in self._slice_pop(m, adj, v):  # push_slice, graph/mod.rs:82-95
                assert j not in adj[i]
                adj[i].add(j)
                adj[j].add(i)
                out.append((i, j))
            if self.orbits != NONE:  # recursive/mod.rs:143-145
                ids, present, counts = self._orbit_masses(adj, v + 1)
                _push(m, counts, present.index(ids[v]))
        return out


# ---- the shapes the tests share: (name, n, edges, loops)
def star(n, centre):
    return [tuple(sorted((centre, v))) for v in range(n) if v != centre]


def shapes():
    from polya_mirror import complete, random_graph
    rng = np.random.default_rng(43)
    out = [
        ("n=0", 0, [], False),
        ("n=1", 1, [], False),
        ("n=1 with its loop", 1, [(0, 0)], True),
        ("n=2", 2, [(0, 1)], False),
        ("n=2 without its edge", 2, [], False),
        ("n=3 path", 3, [(0, 1), (1, 2)], False),
        ("n=13 E=30", 13, random_graph(rng, 13, 30), False),
        ("n=14 E=40 with loops", 14, random_graph(rng, 14, 40, loops=True), True),
        ("n=40 E=90", 40, random_graph(rng, 40, 90), False),
        ("K14", 14, complete(14), False),
        ("K14 with every loop", 14, complete(14) + [(v, v) for v in range(14)], True),
    ]
    for pairs in (11, 12, 13):  # the centre's slice: the plain / joint switch
        out.append((f"star of {pairs}, centre first", pairs + 1, star(pairs + 1, 0), False))
        out.append((f"star of {pairs}, centre last", pairs + 1, star(pairs + 1, pairs), False))
    return out
