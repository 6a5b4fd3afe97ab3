"""The expected-bytes mirror of graph shuffle coding with Weisfeiler-Lehman orbits at any wl_iter,
shared by test_wl_host.py, test_gpu_wl.py and test_gpu_wl_lane_reuse.py (not a test module).
ShuffleCodec<ErdosRenyiSliceCodecs | PolyaUrnSliceCodecs, WLOrbitCodecs<GraphPrefix>> with
num_iter = wl_iter and extra_half_iter = half_iter: the shuffle loops, the swap and the slices are
arer_mirror's and arpu_mirror's; this file replaces the orbit stage alone, written from the
reference line by line (src/recursive/graph/incomplete.rs:45-57, 87-151, 189-236,
src/recursive/prefix_orbit.rs:42-120) and sharing no code with the library.
  * WLMixin._orbit_masses is WLOrbitCodecs::apply: every id of every position computed afresh from
    the prefix's graph at every step.  The bytes are defined by it.
  * Carried is the reference's incremental form (update_around after every slice, the ids' swap);
    carried_against_apply walks a graph down and up again and compares the two at every step."""
import functools

import arer_mirror as AM
import arpu_mirror as PM

M64 = AM.M64


def _sip_long(words):
    """SipHash-1-3, keys 0, 0, over 8-byte words, the final block's length byte taken mod 256 (as
    the hasher has it): arer_mirror.siphash13_words leaves that byte unreduced, which is the same
    below 32 words, all its own callers feed."""
    v = [0x736f6d6570736575, 0x646f72616e646f6d, 0x6c7967656e657261, 0x7465646279746573]

    def rnd():
        v[0] = (v[0] + v[1]) & M64
        v[1] = AM._rotl(v[1], 13) ^ v[0]
        v[0] = AM._rotl(v[0], 32)
        v[2] = (v[2] + v[3]) & M64
        v[3] = AM._rotl(v[3], 16) ^ v[2]
        v[0] = (v[0] + v[3]) & M64
        v[3] = AM._rotl(v[3], 21) ^ v[0]
        v[2] = (v[2] + v[1]) & M64
        v[1] = AM._rotl(v[1], 17) ^ v[2]
        v[2] = AM._rotl(v[2], 32)

    for block in [w & M64 for w in words] + [((8 * len(words)) & 0xFF) << 56]:
        v[3] ^= block
        rnd()
        v[0] ^= block
    v[2] ^= 0xFF
    rnd()
    rnd()
    rnd()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


@functools.lru_cache(maxsize=1 << 18)
def _sip(words):
    return AM.siphash13_words(words) if len(words) < 32 else _sip_long(words)


def sip(words):
    """The mirror's own siphash13_words wherever it is right (fewer than 32 words: a node of degree
    below 30), this file's beyond; remembered, since most ids stay from one step to the next."""
    return _sip(tuple(words))


def apply_ids(adj, length, wl_iter, half_iter):
    """WLOrbitCodecs::apply (incomplete.rs:193-210) on the prefix's graph `adj` (a set of neighbours
    per position, a loop names its node) with `length` known positions: the id of every position."""
    n = len(adj)
    # hash((n, if i < len { None } else { Some(i) })): () feeds nothing, an Option its discriminant
    hashes = [sip([0]) if i < length else sip([1, i]) for i in range(n)]
    if half_iter:  # half_wl_node_iter (:49-51): h, then the Vec<&()>'s length
        hashes = [sip([hashes[i], len(adj[i])]) for i in range(n)]
    ids = [[h] for h in hashes]
    for _ in range(wl_iter):  # wl_iter (:53-57): h, the Vec's length, the (hash, ()) pairs sorted
        hashes = [sip([hashes[i], len(adj[i])] + sorted(hashes[j] for j in adj[i])) for i in range(n)]
        for id_, h in zip(ids, hashes):
            id_.append(h)
    return [tuple(id_) for id_ in ids]


class WLMixin:
    wl_iter, half_iter = 1, True

    def _orbit_masses(self, adj, length):
        ids = apply_ids(adj, length, self.wl_iter, self.half_iter)[:length]
        present = sorted(set(ids))  # Vec<usize> orders lexicographically; MutCategorical ascending
        return ids, present, [ids.count(i) for i in present]


class ERMirror(WLMixin, AM.Mirror):
    def __init__(self, mass, norm, num_nodes, loops, wl_iter, half_iter):
        AM.Mirror.__init__(self, mass, norm, num_nodes, loops, AM.DEGREE)  # (any setting but NONE)
        self.wl_iter, self.half_iter = wl_iter, half_iter


class PolyaMirror(WLMixin, PM.Mirror):
    def __init__(self, num_nodes, loops, wl_iter, half_iter):
        PM.Mirror.__init__(self, num_nodes, loops, PM.DEGREE)
        self.wl_iter, self.half_iter = wl_iter, half_iter


class Carried:
    """PrefixOrbitCodec<Vec<usize>>'s ids and length under WLOrbitCodecs' incremental updates."""

    def __init__(self, ids, length, wl_iter, half_iter):
        self.ids, self.length, self.wl_iter, self.half_iter = [list(i) for i in ids], length, wl_iter, half_iter

    def swap(self, i, j):  # prefix_orbit.rs:23-39
        self.ids[i], self.ids[j] = self.ids[j], self.ids[i]

    def update_around(self, adj, indices):  # incomplete.rs:97-151
        new_ids_by_distance = [{i: list(self.ids[i]) for i in sorted(indices)}]
        for _ in range(self.wl_iter):  # :103-111
            neighbors_ = {}
            for p in new_ids_by_distance[-1]:
                for i in adj[p]:
                    if all(i not in ids for ids in new_ids_by_distance):
                        neighbors_[i] = list(self.ids[i])
            new_ids_by_distance.append(dict(sorted(neighbors_.items())))
        for i, new_id in new_ids_by_distance[0].items():  # :114-124
            h = sip([0]) if i < self.length else sip([1, i])
            if self.half_iter:
                h = sip([h, len(adj[i])])
            new_id[0] = h
        for it in range(self.wl_iter):  # :127-145
            indices_ = [(u, i) for u, x in enumerate(new_ids_by_distance[:it + 2]) for i in x]

            def prev_hash(i):
                for new_id in new_ids_by_distance:
                    if i in new_id:
                        return new_id[i][it]
                return self.ids[i][it]

            for u, i in indices_:
                neighbor_hashes = sorted(prev_hash(ne) for ne in adj[i])
                new_ids_by_distance[u][i][it + 1] = sip([prev_hash(i), len(adj[i])] + neighbor_hashes)
        touched = 0
        for x in new_ids_by_distance:  # :148-150
            for i, new_id in x.items():
                self.ids[i] = new_id
                touched += 1
        return touched


def _swap_positions(adj, index, last):  # graph.rs:304-331, as arer_mirror's push has it
    adj[index], adj[last] = adj[last], adj[index]
    for v in sorted(set(adj[index]) | set(adj[last]) | {index, last}):
        ei, ej = last in adj[v], index in adj[v]
        adj[v].discard(last)
        adj[v].discard(index)
        if ei:
            adj[v].add(index)
        if ej:
            adj[v].add(last)


def carried_against_apply(n, edges, wl_iter, half_iter, rng):
    """Walks the graph down (a class drawn by rng at every step, its smallest position swapped to
    the end, its slice taken out) and up again (the slices put back), carrying the ids as the
    reference does.  Returns (steps compared, mismatches, the most ids update_around touched)."""
    adj = [set() for _ in range(n)]
    for i, j in edges:
        adj[i].add(j)
        adj[j].add(i)
    car = Carried(apply_ids(adj, n, wl_iter, half_iter), n, wl_iter, half_iter)
    steps = bad = most = 0
    slices = []
    for length in range(n, 0, -1):
        last = length - 1
        known = [tuple(i) for i in car.ids[:length]]
        present = sorted(set(known))
        index = known.index(present[int(rng.integers(len(present)))])  # prefix_orbit.rs:117-119
        if index != last:
            _swap_positions(adj, index, last)
            car.swap(index, last)  # incomplete.rs:233-235
        sl = sorted(j for j in adj[last] if j >= last)
        for j in sl:
            adj[last].discard(j)
            adj[j].discard(last)
        slices.append(sl)
        car.length = last  # pop_id, then update_around_slice (:212-221, 87-95)
        most = max(most, car.update_around(adj, sl + [last]))
        steps += 1
        bad += [tuple(i) for i in car.ids] != apply_ids(adj, last, wl_iter, half_iter)
    assert not any(adj)
    for v in range(n):
        sl = slices.pop()
        for j in sl:
            adj[v].add(j)
            adj[j].add(v)
        car.length = v + 1  # push_id, then update_around_slice (:223-231)
        most = max(most, car.update_around(adj, sl + [v]))
        steps += 1
        bad += [tuple(i) for i in car.ids] != apply_ids(adj, v + 1, wl_iter, half_iter)
    return steps, bad, most


# ---- what the tests share
MASS, NORM = 100, 1000


def all_shapes():
    """Both mirrors' shapes: (list name + shape name, n, edges, loops)."""
    return [("er: " + s[0],) + tuple(s[1:]) for s in AM.shapes()] + [("pu: " + s[0],) + tuple(s[1:]) for s in PM.shapes()]


def mirror_of(model, n, loops, wl_iter, half_iter):
    return ERMirror(MASS, NORM, n, loops, wl_iter, half_iter) if model == "er" else PolyaMirror(n, loops, wl_iter, half_iter)


@functools.lru_cache(maxsize=None)
def expected(model, wl_iter, half_iter, seeds):
    """{(shape, seed name): (bytes after push, perm, pairs as pop returns them, bytes after pop)};
    seeds: a tuple of (name, bytes)."""
    out = {}
    for name, n, edges, loops in all_shapes():
        mirror = mirror_of(model, n, loops, wl_iter, half_iter)
        for sname, seed in seeds:
            pushed, perm = mirror.push_bytes(seed, edges)
            popped, rest = mirror.pop_bytes(pushed)
            out[name, sname] = (pushed, perm, popped, rest)
    return out
