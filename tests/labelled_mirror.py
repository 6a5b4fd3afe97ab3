"""The expected-bytes mirror of graph shuffle coding with node and edge labels, shared by
test_labelled_host.py, test_gpu_labelled.py and test_gpu_labelled_lane_reuse.py (not a test module).
ShuffleCodec<ErdosRenyiSliceCodecs<NodeC, EdgeC, _> | PolyaUrnSliceCodecs<NodeC, EdgeC, _>,
WLOrbitCodecs<GraphPrefix<N, E, Undirected>, N, E, _>> over Graph<N, E, Undirected>, N and E each usize
under a Categorical or () under EmptyCodec, written from the reference line by line
(src/recursive/graph/mod.rs:53-104, src/recursive/graph/slice.rs:33-51, 185-192,
src/graph_codec.rs:58-94, src/codec.rs:415-424, 468-479, src/recursive/graph/incomplete.rs:45-57,
97-151, 193-210) and sharing no code with the library.  The index codecs of a slice, the blanket steps
and SipHash are the unlabelled mirrors' (arer_mirror, arpu_mirror, wl_mirror), subclassed, not edited.
  * The prefix's graph is a dict {neighbour: edge label} per position and a node label per position
    (0 once pop_slice has taken it: N::default()); the swap renames the two positions everywhere.
  * _orbit_masses is WLOrbitCodecs::apply: every id of every position afresh at every step.  The
    bytes are defined by it.
  * Carried is the reference's incremental form; carried_against_apply compares the two at every step
    down and up."""
import functools

import numpy as np

import arer_mirror as AM
import arpu_mirror as PM
import wl_mirror as WM
from polya_mirror import E_EXHAUSTED, E_SYMBOL, E_ZERO_MASS, Fail, _pop, _push, random_graph  # noqa: F401

sip = WM.sip


def level0(i, length, label, node_labels):
    """hash((n, if i < len { None } else { Some(i) })) (incomplete.rs:116-117, 195-196): a usize label
    feeds a word, () nothing; None its discriminant 0, Some(i) 1 and i."""
    return sip(([label] if node_labels else []) + ([0] if i < length else [1, i]))


def half_step(h, row, edge_labels):
    """half_wl_node_iter (:49-51): h, the Vec<&E>'s length, the labels sorted (() feeds nothing)."""
    return sip([h, len(row)] + (sorted(row.values()) if edge_labels else []))


def full_step(h, row, prev, edge_labels):
    """wl_iter (:53-57): h, the Vec's length, the (hash, &e) pairs sorted, each a word or two."""
    if edge_labels:
        return sip([h, len(row)] + [w for pair in sorted((prev(j), l) for j, l in row.items()) for w in pair])
    return sip([h, len(row)] + sorted(prev(j) for j in row))


def apply_ids(adj, labels, length, wl_iter, half_iter, node_labels, edge_labels):
    """WLOrbitCodecs::apply (incomplete.rs:193-210) of the prefix (adj, labels) with `length` known
    positions: the id of every position."""
    n = len(adj)
    hashes = [level0(i, length, labels[i], node_labels) for i in range(n)]
    if half_iter:
        hashes = [half_step(hashes[i], adj[i], edge_labels) for i in range(n)]
    ids = [[h] for h in hashes]
    for _ in range(wl_iter):
        hashes = [full_step(hashes[i], adj[i], hashes.__getitem__, edge_labels) for i in range(n)]
        for id_, h in zip(ids, hashes):
            id_.append(h)
    return [tuple(id_) for id_ in ids]


def swap_positions(adj, labels, index, last):
    """x.swap(index, last) (graph.rs:304-331): the two nodes change places, labels and edges with them."""
    def to(k):
        return last if k == index else index if k == last else k
    adj[index], adj[last] = adj[last], adj[index]
    for v in range(len(adj)):
        adj[v] = {to(k): l for k, l in adj[v].items()}
    labels[index], labels[last] = labels[last], labels[index]


def graph_of(n, node_labels, edges):
    adj = [{} for _ in range(n)]
    for (i, j), l in edges:
        adj[i][j] = l
        adj[j][i] = l
    return adj, [0] * n if node_labels is None else [int(v) for v in node_labels]


class LabelledMixin:
    """The shuffle loop over a labelled graph.  node_masses / edge_masses: the Categorical's masses,
    None for EmptyCodec.  A symbol is (node_labels or None, [((i, j), label or None)])."""
    node_masses = edge_masses = None

    def _orbit_masses(self, adj, labels, length):
        ids = apply_ids(adj, labels, length, self.wl_iter, self.half_iter, self.node_masses is not None,
                        self.edge_masses is not None)[:length]
        present = sorted(set(ids))
        return ids, present, [ids.count(i) for i in present]

    def _check(self, node_labels, edges):
        n = self.n
        pairs = [e for e, _ in edges]
        for i, j in pairs:
            if i > j or j >= n or (i == j and not self.loops):
                raise Fail(E_SYMBOL)
        if len(set(pairs)) != len(pairs):
            raise Fail(E_SYMBOL)
        # Categorical::pmf asserts the symbol, the blanket push its mass (src/codec.rs:63, src/ans.rs:98)
        for masses, values in ((self.node_masses, node_labels), (self.edge_masses, [l for _, l in edges])):
            if masses is not None:
                if any(v >= len(masses) for v in values):
                    raise Fail(E_SYMBOL)
                if any(masses[v] == 0 for v in values):
                    raise Fail(E_ZERO_MASS)

    def push(self, m, node_labels, edges):
        """Returns perm: perm[position] = the input node that ended there."""
        n = self.n
        edges = [((int(i), int(j)), l) for (i, j), l in edges]
        self._check(node_labels, edges)
        adj, labels = graph_of(n, node_labels, edges)
        perm = list(range(n))
        for length in range(n, 0, -1):
            last = length - 1
            ids, present, counts = self._orbit_masses(adj, labels, length)  # recursive/mod.rs:123-127
            index = ids.index(present[_pop(m, counts)])
            if index != last:
                swap_positions(adj, labels, index, last)
                perm[index], perm[last] = perm[last], perm[index]
            # pop_slice, graph/mod.rs:57-80: the edges to the unknown positions, the label taken out
            sl = sorted((j, l) for j, l in adj[last].items() if j >= last)
            for j, _ in sl:
                del adj[last][j]
                if j != last:
                    del adj[j][last]
            label, labels[last] = labels[last], 0
            # (NodeC, EdgesIID<EdgeC, indices>)::push: .1 first (codec.rs:468-479); EdgesIID the labels
            # in the order of the index, IID last first (graph_codec.rs:61-65, 82-85, codec.rs:415-420)
            if self.edge_masses is not None:
                for _, l in reversed(sl):
                    _push(m, self.edge_masses, l)
            self._indices_push(m, adj, last, [(last, j) for j, _ in sl])
            if self.node_masses is not None:
                _push(m, self.node_masses, label)
        assert not any(adj) and not any(labels)
        return perm

    def pop(self, m):
        """(node labels by position or None, [((v, w), label or None)] in pop order)."""
        n = self.n
        adj, labels = graph_of(n, None, [])
        out = []
        for v in range(n):
            if self.node_masses is not None:  # the tuple pops .0 first
                labels[v] = _pop(m, self.node_masses)
            for i, j in sorted(self._indices_pop(m, adj, v)):  # graph_codec.rs:67-72: sort_unstable
                l = _pop(m, self.edge_masses) if self.edge_masses is not None else None
                assert j not in adj[i]
                adj[i][j] = l
                adj[j][i] = l
                out.append(((i, j), l))
            ids, present, counts = self._orbit_masses(adj, labels, v + 1)  # recursive/mod.rs:143-145
            _push(m, counts, present.index(ids[v]))
        return (labels if self.node_masses is not None else None), out

    def push_bytes(self, seed, node_labels, edges):
        m = AM.orc.Message.unflatten(seed, AM.orc.EMPTY)
        perm = self.push(m, node_labels, edges)
        return m.flatten(), perm

    def pop_bytes(self, data):
        m = AM.orc.Message.unflatten(data, AM.orc.EMPTY)
        return self.pop(m) + (m.flatten(),)


class ERMirror(LabelledMixin, WM.ERMirror):
    def __init__(self, mass, norm, num_nodes, loops, wl_iter, half_iter, node_masses, edge_masses):
        WM.ERMirror.__init__(self, mass, norm, num_nodes, loops, wl_iter, half_iter)
        self.node_masses, self.edge_masses = node_masses, edge_masses

    def _indices_push(self, m, adj, node, pairs):
        AM.Mirror._slice_push(self, m, node, pairs)

    def _indices_pop(self, m, adj, node):
        return AM.Mirror._slice_pop(self, m, node)


class PolyaMirror(LabelledMixin, WM.PolyaMirror):
    def __init__(self, num_nodes, loops, wl_iter, half_iter, node_masses, edge_masses):
        WM.PolyaMirror.__init__(self, num_nodes, loops, wl_iter, half_iter)
        self.node_masses, self.edge_masses = node_masses, edge_masses

    def _indices_push(self, m, adj, node, pairs):  # (the urn reads the prefix's degrees alone)
        PM.Mirror._slice_push(self, m, adj, node, pairs)

    def _indices_pop(self, m, adj, node):
        return PM.Mirror._slice_pop(self, m, adj, node)


class Carried(WM.Carried):
    """PrefixOrbitCodec<Vec<usize>>'s ids under WLOrbitCodecs' incremental updates, with labels."""

    def __init__(self, ids, length, wl_iter, half_iter, node_labels, edge_labels):
        WM.Carried.__init__(self, ids, length, wl_iter, half_iter)
        self.node_labels, self.edge_labels = node_labels, edge_labels

    def update_around(self, adj, labels, indices):  # incomplete.rs:97-151
        by_distance = [{i: list(self.ids[i]) for i in sorted(indices)}]
        for _ in range(self.wl_iter):  # :103-111
            more = {}
            for p in by_distance[-1]:
                for i in adj[p]:
                    if all(i not in ids for ids in by_distance):
                        more[i] = list(self.ids[i])
            by_distance.append(dict(sorted(more.items())))
        for i, new_id in by_distance[0].items():  # :114-124
            h = level0(i, self.length, labels[i], self.node_labels)
            if self.half_iter:
                h = half_step(h, adj[i], self.edge_labels)
            new_id[0] = h
        for it in range(self.wl_iter):  # :127-145
            def prev(i):
                for new_id in by_distance:
                    if i in new_id:
                        return new_id[i][it]
                return self.ids[i][it]

            for u, i in [(u, i) for u, x in enumerate(by_distance[:it + 2]) for i in x]:
                by_distance[u][i][it + 1] = full_step(prev(i), adj[i], prev, self.edge_labels)
        touched = 0
        for x in by_distance:  # :148-150
            for i, new_id in x.items():
                self.ids[i] = new_id
                touched += 1
        return touched


def carried_against_apply(n, node_labels, edges, wl_iter, half_iter, rng):
    """wl_mirror.carried_against_apply with labels: (steps compared, mismatches, most ids touched)."""
    nl, el = node_labels is not None, any(l is not None for _, l in edges)
    adj, labels = graph_of(n, node_labels, edges)

    def fresh(length):
        return apply_ids(adj, labels, length, wl_iter, half_iter, nl, el)

    car = Carried(fresh(n), n, wl_iter, half_iter, nl, el)
    steps = bad = most = 0
    slices = []
    for length in range(n, 0, -1):
        last = length - 1
        known = [tuple(i) for i in car.ids[:length]]
        present = sorted(set(known))
        index = known.index(present[int(rng.integers(len(present)))])
        if index != last:
            swap_positions(adj, labels, index, last)
            car.swap(index, last)
        sl = sorted((j, l) for j, l in adj[last].items() if j >= last)
        for j, _ in sl:
            del adj[last][j]
            if j != last:
                del adj[j][last]
        slices.append((labels[last], sl))
        labels[last] = 0
        car.length = last
        most = max(most, car.update_around(adj, labels, [j for j, _ in sl] + [last]))
        steps += 1
        bad += [tuple(i) for i in car.ids] != fresh(last)
    assert not any(adj)
    for v in range(n):
        labels[v], sl = slices.pop()
        for j, l in sl:
            adj[v][j] = l
            adj[j][v] = l
        car.length = v + 1
        most = max(most, car.update_around(adj, labels, [j for j, _ in sl] + [v]))
        steps += 1
        bad += [tuple(i) for i in car.ids] != fresh(v + 1)
    return steps, bad, most


# ---- what the tests share
MASS, NORM = WM.MASS, WM.NORM
NODE_MASSES = [50, 30, 10, 7, 0, 2, 1]  # seven node labels, symbol 4 of mass 0; the rarest is the largest
EDGE_MASSES = [6, 3, 0, 1]              # four edge labels, symbol 2 of mass 0
SETTINGS = [(w, h) for w in range(4) for h in (True, False)]
LABELS = [(True, True), (True, False), (False, True), (False, False)]  # (node labels, edge labels)


def _labelled(pairs, labels):
    return [(tuple(e), int(l)) for e, l in zip(pairs, labels)]


@functools.lru_cache(maxsize=None)
def shapes():
    """(name, n, node labels, [((i, j), label)], loops, (node masses, edge masses))."""
    both = (NODE_MASSES, EDGE_MASSES)
    rng = np.random.default_rng(47)
    star15 = [(0, v) for v in range(1, 16)]
    star31 = [(0, v) for v in range(1, 32)]
    out = [
        ("n=0", 0, [], [], False, both),
        ("n=1", 1, [3], [], False, both),
        ("n=1 with its loop", 1, [3], [((0, 0), 1)], True, both),
        ("two equal nodes joined", 2, [1, 1], [((0, 1), 0)], False, both),
        ("3-path, ends alike, edges differ", 3, [0, 1, 0], [((0, 1), 0), ((1, 2), 1)], False, both),
        ("star, leaves alike, two edge labels", 7, [2] + [0] * 6, _labelled([(0, v) for v in range(1, 7)], [0, 1, 0, 1, 1, 0]),
         False, both),
        ("triangle, one odd edge", 3, [0, 0, 0], [((0, 1), 0), ((1, 2), 0), ((0, 2), 3)], False, both),
        ("C6, alternating edges", 6, [1] * 6, _labelled([(v, v + 1) for v in range(5)] + [(0, 5)], [0, 1, 0, 1, 0, 1]), False, both),
        ("two equal triangles", 6, [0, 1, 3] * 2,
         _labelled([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5)], [0, 1, 3] * 2), False, both),
        ("labelled loops", 4, [0, 0, 1, 1], _labelled([(0, 0), (1, 1), (0, 1), (2, 2), (2, 3)], [0, 1, 0, 0, 3]), True, both),
        ("degree 15", 16, [0] + [int(v) % 2 for v in range(15)], _labelled(star15, [v % 2 for v in range(15)]), False, both),
        ("degree 31", 32, [1] + [0] * 31, _labelled(star31 + [(1, 2), (3, 4)], [(v * v) % 2 for v in range(33)]), False, both),
        ("all labels equal", 7, [0] * 7, _labelled(random_graph(rng, 7, 10), [0] * 10), False, both),
        ("the largest symbols", 5, [6] * 5, _labelled(random_graph(rng, 5, 6, loops=True), [3] * 6), True, both),
        ("one-symbol tables", 5, [0] * 5, _labelled(random_graph(rng, 5, 7), [0] * 7), False, ([9], [4])),
        ("K13: a slice of 12", 13, [int(v) for v in rng.choice([0, 1], 13)],
         _labelled([(i, j) for j in range(13) for i in range(j)], rng.choice([0, 1, 3], 78)), False, both),
    ]
    node_alphabet = [s for s, p in enumerate(NODE_MASSES) if p]
    edge_alphabet = [s for s, p in enumerate(EDGE_MASSES) if p]
    for k in range(20):
        loops = bool(k & 1)
        pairs = random_graph(rng, 12, 20, loops=loops)
        out.append((f"random {k}", 12, [int(v) for v in rng.choice(node_alphabet, 12)],
                    _labelled(pairs, rng.choice(edge_alphabet, 20)), loops, both))
    return tuple(out)


# the shapes the setting without labels runs (the rest repeat what wl_mirror's shapes cover)
UNLABELLED_SUBSET = ("n=0", "n=1 with its loop", "labelled loops", "degree 31", "K13: a slice of 12", "random 0", "random 1")


def project(shape, nl, el):
    """A shape under a label setting: the labels a setting lacks are dropped, with their table."""
    name, n, node_labels, edges, loops, (node_masses, edge_masses) = shape
    return (name, n, node_labels if nl else None, [(e, l if el else None) for e, l in edges], loops,
            (node_masses if nl else None, edge_masses if el else None))


def shapes_of(nl, el):
    return [project(s, nl, el) for s in shapes() if nl or el or s[0] in UNLABELLED_SUBSET]


def mirror_of(model, n, loops, wl_iter, half_iter, node_masses, edge_masses):
    if model == "er":
        return ERMirror(MASS, NORM, n, loops, wl_iter, half_iter, node_masses, edge_masses)
    return PolyaMirror(n, loops, wl_iter, half_iter, node_masses, edge_masses)


def relabelled(node_labels, edges, perm):
    """The input as the decoder sees it: (labels by position or None, the pairs of positions with
    their labels, sorted)."""
    pos = {node: p for p, node in enumerate(perm)}
    return (None if node_labels is None else [node_labels[v] for v in perm],
            sorted((tuple(sorted((pos[i], pos[j]))), l) for (i, j), l in edges))


@functools.lru_cache(maxsize=None)
def expected(model, wl_iter, half_iter, nl, el, seeds):
    """{(shape, seed name): (bytes after push, perm, popped node labels, popped edges, bytes after pop)}."""
    out = {}
    for name, n, node_labels, edges, loops, (node_masses, edge_masses) in shapes_of(nl, el):
        mirror = mirror_of(model, n, loops, wl_iter, half_iter, node_masses, edge_masses)
        for sname, seed in seeds:
            pushed, perm = mirror.push_bytes(seed, node_labels, edges)
            out[name, sname] = (pushed, perm) + mirror.pop_bytes(pushed)
    return out
