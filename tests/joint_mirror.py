"""The expected-bytes mirror of joint shuffle coding of graphs with Weisfeiler-Lehman orbits, shared by
test_joint_host.py, test_gpu_joint.py and test_gpu_joint_lane_reuse.py (not a test module).
ShuffleCodec<JointSliceCodecs<C>, WLOrbitCodecs<JointPrefix<Graph>>> as a Python loop over the oracle's
Message, written from the reference line by line (src/recursive/mod.rs:117-148, src/recursive/joint.rs,
src/recursive/graph/incomplete.rs:154-187, 193-210, src/recursive/prefix_orbit.rs:23-39, 117-119,
src/graph_codec.rs:104-139, 184-199, 405-450) and sharing no code with the library.  Deliberately naive:
  * the full graph is one Python set of neighbours per position and never loses an edge; the swap is
    the reference's (wl_mirror._swap_positions);
  * the ids are WLOrbitCodecs::apply (wl_mirror.apply_ids) of the full graph with `len` known positions,
    computed afresh at every step.  The bytes are defined by it;
  * the ordered codec C is polya_mirror.Mirror for the urn and, for the dense set, a Bernoulli loop over
    AllEdgeIndices written out here (dense_push / dense_pop; test_joint_host.py holds it against
    oracle.graph_iid_push);
  * joint_carried_against_apply walks a graph down and up with the reference's incremental form
    (wl_mirror.Carried.update_around(adj, [the node that changed sides])) and compares it with apply."""
import functools

import numpy as np

from oracle import oracle as orc

import polya_mirror as PM
import wl_mirror as WM
from polya_mirror import E_EXHAUSTED, E_SYMBOL, E_ZERO_MASS, Fail, _pop, _push

MASS, NORM = WM.MASS, WM.NORM


def all_edge_indices(n, loops):
    """AllEdgeIndices::into_iter for an undirected graph (src/graph_codec.rs:187-199): the loops, then
    (0..n).flat_map(|j| (0..j).map(|i| (i, j)))."""
    return ([(i, i) for i in range(n)] if loops else []) + [(i, j) for j in range(n) for i in range(j)]


def dense_push(m, masses, n, loops, edges):
    """IID<Bernoulli>::push of DenseSetIID::dense(edges) (src/graph_codec.rs:111-138, src/codec.rs:415-420):
    the last slot first."""
    has_edge = orc.Categorical(masses)
    present = set(edges)
    for slot in reversed(all_edge_indices(n, loops)):
        b = int(slot in present)
        if int(masses[b]) == 0:
            raise Fail(E_ZERO_MASS)  # src/ans.rs:98
        if has_edge.push(m, b) or m.err:
            raise Fail(E_EXHAUSTED)


def dense_pop(m, masses, n, loops):
    """... and its pop (src/codec.rs:422-424): the pairs in the alphabet's order."""
    has_edge = orc.Categorical(masses)
    out = []
    for slot in all_edge_indices(n, loops):
        try:
            b = has_edge.pop(m)
        except RuntimeError:
            raise Fail(E_EXHAUSTED)
        if m.err:
            raise Fail(E_EXHAUSTED)
        if b:
            out.append(slot)
    return out


def _adjacency(n, edges):
    adj = [set() for _ in range(n)]
    for i, j in edges:
        adj[i].add(j)
        adj[j].add(i)
    return adj


def _pairs(adj):
    return sorted((i, j) for i in range(len(adj)) for j in adj[i] if i <= j)


class Mirror:
    """model: "er" (the dense indicator under Bernoulli(MASS, NORM)) or "pu" (the ordered urn)."""

    def __init__(self, model, num_nodes, loops, wl_iter, half_iter, redraws=False):
        self.model, self.n, self.loops, self.wl_iter, self.half_iter = model, num_nodes, loops, wl_iter, half_iter
        self.redraws = redraws
        self.masses = np.array([NORM - MASS, MASS], np.uint64)  # Bernoulli::new, src/codec.rs:125-128

    def _orbit_masses(self, adj, length):
        ids = WM.apply_ids(adj, length, self.wl_iter, self.half_iter)[:length]  # incomplete.rs:158-162
        present = sorted(set(ids))
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
        adj = _adjacency(n, edges)
        perm = list(range(n))
        for length in range(n, 0, -1):  # recursive/mod.rs:120-130
            ids, present, counts = self._orbit_masses(adj, length)
            index = ids.index(present[_pop(m, counts)])  # prefix_orbit.rs:117-119
            last = length - 1
            if index != last:  # joint.rs:40-44
                WM._swap_positions(adj, index, last)
                perm[index], perm[last] = perm[last], perm[index]
        # EmptyJointPrefixCodec::push (joint.rs:87-89): the whole permuted graph
        if self.model == "er":
            dense_push(m, self.masses, n, self.loops, _pairs(adj))
        else:
            # (the urn codes a multiset of pairs: any order of the list gives the same bytes)
            PM.Mirror(n, self.loops, self.redraws).push(m, _pairs(adj))
        return perm

    def pop(self, m, num_edges=None):
        """The pairs as the ordered codec returns them; num_edges: the urn's parameter."""
        n = self.n
        if self.model == "er":
            edges = dense_pop(m, self.masses, n, self.loops)
        else:
            edges = [tuple(e) for e in PM.Mirror(n, self.loops, self.redraws).pop(m, num_edges)]
        adj = _adjacency(n, edges)
        for v in range(n):  # recursive/mod.rs:139-146
            ids, present, counts = self._orbit_masses(adj, v + 1)
            _push(m, counts, present.index(ids[v]))
        return edges

    def push_bytes(self, seed, edges):
        m = orc.Message.unflatten(seed, orc.EMPTY)
        perm = self.push(m, edges)
        return m.flatten(), perm

    def pop_bytes(self, data, num_edges=None):
        m = orc.Message.unflatten(data, orc.EMPTY)
        edges = self.pop(m, num_edges)
        return edges, m.flatten()


def joint_carried_against_apply(n, edges, wl_iter, half_iter, rng):
    """Walks the graph down (a class drawn by rng at every step, its smallest position swapped to the end,
    which leaves the known positions) and up again, carrying the ids as the reference does
    (incomplete.rs:164-182).  Returns (steps compared, mismatches)."""
    adj = _adjacency(n, edges)
    car = WM.Carried(WM.apply_ids(adj, n, wl_iter, half_iter), n, wl_iter, half_iter)
    steps = bad = 0
    for length in range(n, 0, -1):
        last = length - 1
        known = [tuple(i) for i in car.ids[:length]]
        present = sorted(set(known))
        index = known.index(present[int(rng.integers(len(present)))])
        if index != last:
            WM._swap_positions(adj, index, last)
            car.swap(index, last)  # incomplete.rs:184-186
        car.length = last  # pop_id, then update_around(&x.full, orbits, vec![x.len()]) (:170-171)
        car.update_around(adj, [last])
        steps += 1
        bad += [tuple(i) for i in car.ids] != WM.apply_ids(adj, last, wl_iter, half_iter)
    for v in range(n):
        car.length = v + 1  # push_id, then update_around(&x.full, orbits, vec![x.last_index()]) (:180-181)
        car.update_around(adj, [v])
        steps += 1
        bad += [tuple(i) for i in car.ids] != WM.apply_ids(adj, v + 1, wl_iter, half_iter)
    return steps, bad


# ---- what the tests share
def shapes():
    """wl_mirror's shapes and a star whose centre feeds 35 words to its hash (the length byte wraps)."""
    return WM.all_shapes() + [("K1,33", 34, [(0, v) for v in range(1, 34)], False)]


@functools.lru_cache(maxsize=None)
def expected(model, wl_iter, half_iter, redraws, seeds):
    """{(shape, seed name): (bytes after push, perm, pairs as pop returns them, bytes after pop)};
    seeds: a tuple of (name, bytes)."""
    out = {}
    for name, n, edges, loops in shapes():
        mirror = Mirror(model, n, loops, wl_iter, half_iter, redraws)
        for sname, seed in seeds:
            pushed, perm = mirror.push_bytes(seed, edges)
            popped, rest = mirror.pop_bytes(pushed, len(edges))
            out[name, sname] = (pushed, perm, popped, rest)
    return out
