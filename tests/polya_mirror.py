"""The expected-bytes mirror of the Pólya urn edge-index codec, shared by test_polya_host.py and
test_gpu_polya.py (not a test module).  multiset_shuffle_codec(PolyaUrnEdgeIndicesCodec<Undirected>)
as a Python loop over the oracle's Message, written from the reference line by line
(src/graph_codec.rs:210-375, src/recursive/multiset.rs:94-136, src/recursive/mod.rs:117-148,
src/recursive/joint.rs, src/recursive/prefix_orbit.rs, src/plain/mod.rs:111-123, 206-347,
src/permutable.rs:26-41, 184-212, src/multiset.rs:21-53) and sharing no code with the library.
Deliberately naive:
  * every blanket step is orc.Categorical(masses): all-ones masses are Uniform, the urn is a plain
    list of masses with the excluded nodes' set to zero;
  * permutations are lists acted on as the reference's Permutation is, the stabiliser chain of a
    2-vector is written out, the orbit distribution is the sorted list of the prefix's ids;
  * the adjacency is one Python set per node;
  * the orbit id is this file's own SipHash-1-3 over the tuple's 16 bytes."""
import numpy as np

from oracle import oracle as orc

M64 = (1 << 64) - 1
E_ZERO_MASS, E_EXHAUSTED, E_SYMBOL = 1, 2, 4


class Fail(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def _rotl(v, s):
    return ((v << s) | (v >> (64 - s))) & M64


def siphash13_pair(i, j):
    """DefaultHasher::new() fed (i, j): two usizes, 16 little-endian bytes, then the length block."""
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

    for block in (i & M64, j & M64, 16 << 56):
        v[3] ^= block
        rnd()
        v[0] ^= block
    v[2] ^= 0xFF
    rnd()
    rnd()
    rnd()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


# ---- the blanket codec on the oracle's message
def _push(m, masses, x):
    a = np.asarray(masses, dtype=np.uint64)
    if int(a[x]) == 0:
        raise Fail(E_ZERO_MASS)  # src/ans.rs:98
    if orc.Categorical(a).push(m, x) or m.err:
        raise Fail(E_EXHAUSTED)


def _pop(m, masses):
    a = np.asarray(masses, dtype=np.uint64)
    if int(a.sum()) == 0:
        raise Fail(E_ZERO_MASS)  # the reference divides by a norm of zero
    try:
        x = orc.Categorical(a).pop(m)
    except RuntimeError:
        raise Fail(E_EXHAUSTED)
    if m.err:
        raise Fail(E_EXHAUSTED)
    return x


def _uniform(size):
    return [1] * size


# ---- Permutation as a list of images (src/permutable.rs:68-160)
def _swap(p, i, j):  # Permutable for Permutation: the images at i and j change places
    p[i], p[j] = p[j], p[i]


def _inverse(p):
    q = [0] * len(p)
    for i, x in enumerate(p):
        q[x] = i
    return q


def _mul(a, b):  # (a * b)(i) = a(b(i))
    return [a[x] for x in b]


def permuted(x, perm):  # _permuted_from_swap, src/permutable.rs:26-41
    n = len(x)
    p, p_inv, out = list(range(n)), list(range(n)), list(x)
    for i in reversed(range(n)):
        xi = perm[i]
        j = p_inv[xi]
        pi = p[i]
        _swap(p_inv, pi, xi)
        out[pi], out[xi] = out[xi], out[pi]
        _swap(p, i, j)
    return out


def perm_pop(m, n):  # PermutationUniform::pop, src/permutable.rs:202-212
    p = list(range(n))
    for i in reversed(range(n)):
        _swap(p, i, _pop(m, _uniform(i + 1)))
    return p


def perm_push(m, x):  # PermutationUniform::push, src/permutable.rs:184-200
    n = len(x)
    p, p_inv, js = list(range(n)), list(range(n)), []
    for i in reversed(range(n)):
        xi = x[i]
        j = p_inv[xi]
        _swap(p_inv, p[i], xi)
        _swap(p, i, j)
        js.append(j)
    for i, j in enumerate(reversed(js)):
        _push(m, _uniform(i + 1), j)


def canon(x):  # src/multiset.rs:26-30 (a stable sort: [v, v] has the identity, :101)
    return _inverse(sorted(range(len(x)), key=lambda k: x[k]))


def chain_of(x):
    """lex_stabilizer_chain of x's automorphism group (src/multiset.rs:40-46, src/plain/mod.rs:458-468)
    as [(sorted orbit, {element: from[element]})], for the two cases the codec meets: all of x
    distinct (trivial group) and the 2-vector [v, v]."""
    n = len(x)
    ident = list(range(n))
    if len(set(x)) == n:
        return [([b], {b: ident}) for b in range(n)]
    assert n == 2 and x[0] == x[1]
    return [([0, 1], {0: [0, 1], 1: [1, 0]}), ([1], {1: [0, 1]})]


def coset_min_and_restore_aut(chain, labels):  # src/plain/mod.rs:328-347
    labels = list(labels)
    min_elements, base_to_min = [], []
    for base, (orbit, frm) in enumerate(chain):
        _, min_element = min((labels[e], e) for e in orbit)
        b2m = _inverse(frm[min_element])
        min_elements.append(min_element)
        base_to_min.append(b2m)
        labels = _mul(labels, b2m)
    return labels, (min_elements, base_to_min)


def rcoset_pop(m, chain):  # RCosetUniform::pop, src/plain/mod.rs:258-263
    perm = perm_pop(m, len(chain))
    coset_min, (min_elements, _) = coset_min_and_restore_aut(chain, perm)
    for (orbit, _), e in reversed(list(zip(chain, min_elements))):  # AutomorphismUniform::push, :209-214
        _push(m, _uniform(len(orbit)), orbit.index(e))
    return coset_min


def rcoset_push(m, chain, x):  # RCosetUniform::push, src/plain/mod.rs:251-256
    coset_min, _ = coset_min_and_restore_aut(chain, x)
    total = list(range(len(chain)))  # AutomorphismUniform::pop (:216-223) and Automorphism::total (:307-313)
    base_to_min = []
    for orbit, frm in chain:
        e = orbit[_pop(m, _uniform(len(orbit)))]
        base_to_min.append(_inverse(frm[e]))
    for b2m in reversed(base_to_min):
        total = _mul(b2m, total)
    perm_push(m, _mul(coset_min, _inverse(total)))  # apply_to, :316-318


class Mirror:
    def __init__(self, num_nodes, loops, redraws):
        self.n, self.loops, self.redraws = num_nodes, loops, redraws

    # ---- PolyaUrnEdgeIndexCodec (src/graph_codec.rs:211-291)
    def _graph(self, edges):
        self.adj = [set() for _ in range(self.n)]
        for i, j in edges:
            self._insert(i, j)

    def _insert(self, i, j):
        if j in self.adj[i]:
            raise Fail(E_SYMBOL)  # insert_plain_edge asserts, :257
        self.adj[i].add(j)
        self.adj[j].add(i)

    def _remove(self, i, j):
        self.adj[i].remove(j)
        if i != j:
            self.adj[j].remove(i)

    def _masses(self, without=None):  # :224 and use_codec_without, :229-245
        masses = [len(a) + 1 for a in self.adj]
        if without is not None:
            if not self.loops:
                masses[without] = 0
            if not self.redraws:
                for v in self.adj[without]:
                    masses[v] = 0
        return masses

    def _edge_push(self, m, i, j):  # plain_shuffle_codec(self).push of Unordered([i, j])
        x = permuted([i, j], canon([i, j]))
        x = permuted(x, rcoset_pop(m, chain_of(x)))
        node, node_ = x  # :269-276
        _push(m, self._masses(node), node_)
        _push(m, self._masses(), node)

    def _edge_pop(self, m):
        node = _pop(m, self._masses())  # :278-282
        node_ = _pop(m, self._masses(node))
        y = [node, node_]
        c = canon(y)
        x = permuted(y, c)
        rcoset_push(m, chain_of(x), _inverse(c))
        return tuple(x)

    # ---- PolyaUrnEdgeIndicesCodec (src/graph_codec.rs:315-342)
    def _ordered_push(self, m, edges):
        self._graph(edges)
        for i, j in reversed(edges):
            self._remove(i, j)
            self._edge_push(m, i, j)

    def _ordered_pop(self, m, num_edges):
        self._graph([])
        edges = []
        for _ in range(num_edges):
            i, j = self._edge_pop(m)
            self._insert(i, j)
            edges.append((i, j))
        return edges

    # ---- multiset_shuffle_codec (src/recursive/multiset.rs:126-136)
    def push(self, m, edges):
        edges = [(int(i), int(j)) for i, j in edges]
        for i, j in edges:
            if i > j or j >= self.n or (i == j and not self.loops):
                raise Fail(E_SYMBOL)
        if len(set(edges)) != len(edges):
            raise Fail(E_SYMBOL)
        if len(edges) <= 11:  # plain_shuffle_codec, src/plain/mod.rs:111-116
            x = permuted(edges, canon(edges))
            x = permuted(x, rcoset_pop(m, chain_of(x)))
            self._ordered_push(m, x)
            return
        # PrefixShuffleCodec::push over JointPrefix, src/recursive/mod.rs:117-134
        x = list(edges)
        ids = [siphash13_pair(i, j) for i, j in x]
        assert len(set(ids)) == len(ids)
        for length in range(len(x), 0, -1):
            present = sorted(ids[:length])
            index = ids.index(present[_pop(m, _uniform(length))])  # pop_element: singleton orbits
            last = length - 1
            x[index], x[last] = x[last], x[index]
            ids[index], ids[last] = ids[last], ids[index]
        self._ordered_push(m, x)

    def pop(self, m, num_edges):
        """The edges as the codec returns them: sorted for E <= 11, in pop order beyond."""
        if num_edges <= 11:  # src/plain/mod.rs:118-123
            y = self._ordered_pop(m, num_edges)
            c = canon(y)
            x = permuted(y, c)
            rcoset_push(m, chain_of(x), _inverse(c))
            return x
        x = self._ordered_pop(m, num_edges)  # src/recursive/mod.rs:136-148
        ids = [siphash13_pair(i, j) for i, j in x]
        assert len(set(ids)) == len(ids)
        for k in range(num_edges):
            present = sorted(ids[:k + 1])
            _push(m, _uniform(k + 1), present.index(ids[k]))
        return x

    def push_bytes(self, seed, edges):
        """flatten(push(unflatten(seed, EMPTY), edges))."""
        m = orc.Message.unflatten(seed, orc.EMPTY)
        self.push(m, edges)
        return m.flatten()

    def pop_bytes(self, data, num_edges):
        """(edges, flatten of what remains) from unflatten(data, EMPTY)."""
        m = orc.Message.unflatten(data, orc.EMPTY)
        edges = self.pop(m, num_edges)
        return edges, m.flatten()


# ---- graphs the tests share
def random_graph(rng, n, num_edges, loops=False):
    """num_edges distinct pairs (i, j), i <= j < n, in random order."""
    pairs = [(i, j) for j in range(n) for i in range(j + 1 if loops else j)]
    pick = rng.choice(len(pairs), size=num_edges, replace=False)
    return [pairs[k] for k in pick]


def complete(n):
    return [(i, j) for j in range(n) for i in range(j)]
