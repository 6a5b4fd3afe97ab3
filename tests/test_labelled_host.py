"""Graph shuffle coding with node and edge labels on the host (include/ans_capi.h section 3:
ans_ar_er_wl_labelled_push / _pop, ans_ar_polya_wl_labelled_push / _pop; ans_amd.AutoregressiveERLabelled,
AutoregressivePolyaLabelled) against the expected-bytes mirror of tests/labelled_mirror.py, the mirror
against wl_mirror without labels and against the reference's incremental form, the new entries against
the unlabelled ones where no mirror is needed, and the label-carrying ids of csrc/ans_wl.hpp (compiled
with g++) against the mirror's."""
import os
import subprocess

import numpy as np
import pytest

import ans_amd as A

import labelled_mirror as LM
import mset_mirror as MM
import wl_mirror as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shuffle-coding_amd", "csrc")

MASS, NORM = LM.MASS, LM.NORM
MODELS = ["er", "pu"]
SETTINGS = LM.SETTINGS


def _seeds():
    """test_wl_host._seeds(): a random seed message, and the same with zero bytes on top."""
    seed = MM.seeds(np.random.default_rng(11), 1, 96)[0]
    return [("seed", seed), ("seed + zeros", seed + b"\x00\x00\x00")]


def _cat(masses):
    return A.Categorical(np.asarray(masses, np.uint64)) if masses is not None else None


def _codec(model, n, loops, wl_iter, half_iter, node_masses, edge_masses):
    if model == "er":
        return A.AutoregressiveERLabelled(A.Bernoulli(MASS, NORM), n, loops, wl_iter, half_iter, _cat(node_masses),
                                          _cat(edge_masses))
    return A.AutoregressivePolyaLabelled(n, loops, wl_iter, half_iter, _cat(node_masses), _cat(edge_masses))


def _symbol(n, node_labels, edges):
    return A.Graph(node_labels if node_labels is not None else [None] * n, edges)


# ---- 1. the mirror without labels is wl_mirror; its carried ids equal apply's
def test_mirror_without_labels_equals_the_wl_mirror():
    seed = _seeds()[0][1]
    for wl_iter, half_iter in SETTINGS:
        for name, n, _, edges, loops, _ in LM.shapes_of(False, False):
            pairs = [e for e, _ in edges]
            for new, old in ((LM.ERMirror(MASS, NORM, n, loops, wl_iter, half_iter, None, None),
                              WM.ERMirror(MASS, NORM, n, loops, wl_iter, half_iter)),
                             (LM.PolyaMirror(n, loops, wl_iter, half_iter, None, None), WM.PolyaMirror(n, loops, wl_iter, half_iter))):
                assert new.push_bytes(seed, None, edges) == old.push_bytes(seed, pairs), (name, wl_iter, half_iter)


@pytest.mark.parametrize("wl_iter", range(4))
def test_carried_ids_equal_apply_at_every_step(wl_iter):
    rng = np.random.default_rng(23 + wl_iter)
    for nl, el in LM.LABELS[:3]:
        for half_iter in (True, False):
            for name, n, node_labels, edges, _, _ in LM.shapes_of(nl, el):
                steps, bad, most = LM.carried_against_apply(n, node_labels, edges, wl_iter, half_iter, rng)
                assert steps == 2 * n and bad == 0, f"{name} wl_iter={wl_iter} half={half_iter} labels={nl, el}: {bad} of {steps}"
                assert most <= n


# ---- 2. the library against the mirror
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("wl_iter,half_iter", SETTINGS)
@pytest.mark.parametrize("nl,el", LM.LABELS)
def test_push_pop_bytes_equal_the_mirror(model, wl_iter, half_iter, nl, el):
    want = LM.expected(model, wl_iter, half_iter, nl, el, tuple(_seeds()))
    rng = np.random.default_rng(5)
    for name, n, node_labels, edges, loops, (node_masses, edge_masses) in LM.shapes_of(nl, el):
        codec = _codec(model, n, loops, wl_iter, half_iter, node_masses, edge_masses)
        for sname, seed in _seeds():
            where = f"{name} from {sname}"
            pushed, perm, popped_nodes, popped_edges, rest = want[name, sname]
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            got_perm = codec.push(m, _symbol(n, node_labels, edges))
            assert m.flatten() == pushed, f"{where}: push"
            assert list(got_perm) == perm, f"{where}: perm"
            m = A.Message.unflatten(pushed, A.GEN_EMPTY)
            got = codec.pop(m)
            assert got.edges == popped_edges, f"{where}: the pairs and their labels as the codec returns them"
            assert list(got.node_labels) == (popped_nodes if nl else [None] * n), f"{where}: the node labels"
            assert m.flatten() == rest, f"{where}: what remains"
            # the popped graph is the input relabelled by perm, labels included; a node's pairs ascend
            want_nodes, want_edges = LM.relabelled(node_labels, edges, perm)
            assert got.edges == want_edges and (not nl or list(got.node_labels) == want_nodes), where
        # the order of the input pairs does not matter
        order = [edges[k] for k in rng.permutation(len(edges))]
        m = A.Message.unflatten(_seeds()[0][1], A.GEN_EMPTY)
        got_perm = codec.push(m, _symbol(n, node_labels, order))
        assert m.flatten() == want[name, "seed"][0] and list(got_perm) == want[name, "seed"][1], name


# ---- 3. without a mirror: no tables give the unlabelled entries' bytes
@pytest.mark.parametrize("wl_iter,half_iter", SETTINGS)
def test_without_tables_the_bytes_are_the_unlabelled_entries(wl_iter, half_iter):
    bern = A.Bernoulli(MASS, NORM)
    for name, n, edges, loops in WM.all_shapes():
        sym = A.Graph([None] * n, [(e, None) for e in edges])
        for new, old in ((A.AutoregressiveERLabelled(bern, n, loops, wl_iter, half_iter), A.AutoregressiveERWL(bern, n, loops, wl_iter, half_iter)),
                         (A.AutoregressivePolyaLabelled(n, loops, wl_iter, half_iter), A.AutoregressivePolyaWL(n, loops, wl_iter, half_iter))):
            for sname, seed in _seeds():
                a, b = A.Message.unflatten(seed, A.GEN_EMPTY), A.Message.unflatten(seed, A.GEN_EMPTY)
                pa, pb = new.push(a, sym), old.push(b, edges)
                assert a.flatten() == b.flatten() and list(pa) == list(pb), f"{name} from {sname}: push"
                ga, eb = new.pop(a), old.pop(b)
                assert a.flatten() == b.flatten(), f"{name} from {sname}: pop"
                # ... and the pairs, once each node's slice is sorted (the labelled pop gives them so)
                assert [e for e, _ in ga.edges] == sorted(eb) and all(l is None for _, l in ga.edges), name


# ---- 4. every error is a status
def _code_of(fn):
    with pytest.raises(A.AnsError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("model", MODELS)
def test_every_error_is_a_status(model):
    seed = _seeds()[0][1]
    nodes, pairs = [0, 1, 0, 3, 6, 1], [((0, 1), 0), ((0, 3), 1), ((2, 3), 3), ((4, 5), 0), ((1, 5), 1)]
    for wl_iter, half_iter in SETTINGS:
        codec = _codec(model, 6, False, wl_iter, half_iter, LM.NODE_MASSES, LM.EDGE_MASSES)

        def push(nodes_, pairs_):
            """The status, and that the message is as it was."""
            m = A.Message.unflatten(seed, A.GEN_EMPTY)
            before = m.flatten()
            code = _code_of(lambda: codec.push(m, A.Graph(nodes_, pairs_)))
            assert m.flatten() == before
            return code
        # a label outside its table, a label of mass 0, a pair given twice
        assert push([0, 1, 0, 3, 7, 1], pairs) == A.ANS_E_SYMBOL
        assert push(nodes, pairs[:2] + [((2, 3), 4)] + pairs[3:]) == A.ANS_E_SYMBOL
        assert push([0, 1, 0, 4, 6, 1], pairs) == A.ANS_E_ZERO_MASS
        assert push(nodes, pairs[:4] + [((1, 5), 2)]) == A.ANS_E_ZERO_MASS
        assert push(nodes, pairs + [((0, 3), 1)]) == A.ANS_E_SYMBOL
        assert push(nodes[:5], pairs) == A.ANS_E_ARG  # five labels for six nodes
        # a pop of a message cut to 2 bytes; a pop with cap one short
        m = A.Message.unflatten(seed, A.GEN_EMPTY)
        codec.push(m, A.Graph(nodes, pairs))
        data = m.flatten()
        assert _code_of(lambda: codec.pop(A.Message.unflatten(data[:2], A.GEN_EMPTY))) == A.ANS_E_EXHAUSTED
        assert _code_of(lambda: codec.pop(A.Message.unflatten(data, A.GEN_EMPTY), cap=len(pairs) - 1)) == A.ANS_E_LEN
        assert len(codec.pop(A.Message.unflatten(data, A.GEN_EMPTY), cap=len(pairs)).edges) == len(pairs)
        assert _code_of(lambda: _codec(model, 3, False, 4, half_iter, LM.NODE_MASSES, None).pop(A.Message.zeros())) == A.ANS_E_ARG


def test_a_table_needs_its_array_and_an_array_its_table():
    lib, m = A.lib(), A.Message.zeros()
    node = A.Categorical(np.asarray(LM.NODE_MASSES, np.uint64))
    pairs, labels, perm = np.zeros((1, 2), np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    pairs[0] = (0, 1)
    count = A.sz(0)
    for table, array in ((node.table, None), (None, A._np_ptr(labels))):
        assert lib.ans_ar_polya_wl_labelled_push(m.h, 2, 0, 1, 1, A._np_ptr(pairs), 1, A._np_ptr(perm), table, None,
                                                 array, None) == A.ANS_E_ARG
        assert lib.ans_ar_polya_wl_labelled_push(m.h, 2, 0, 1, 1, A._np_ptr(pairs), 1, A._np_ptr(perm), None, table,
                                                 None, array) == A.ANS_E_ARG
        assert lib.ans_ar_polya_wl_labelled_pop(m.h, 2, 0, 1, 1, A._np_ptr(pairs), 1, A.ctypes.byref(count), table, None,
                                                array, None) == A.ANS_E_ARG
        bern = A.Bernoulli(MASS, NORM).categorical.table
        assert lib.ans_ar_er_wl_labelled_push(m.h, bern, 2, 0, 1, 1, A._np_ptr(pairs), 1, A._np_ptr(perm), None, table,
                                              None, array) == A.ANS_E_ARG
        assert lib.ans_ar_er_wl_labelled_pop(m.h, bern, 2, 0, 1, 1, A._np_ptr(pairs), 1, A.ctypes.byref(count), table,
                                             None, array, None) == A.ANS_E_ARG


# ---- 5. csrc/ans_wl.hpp with g++ (no HIP): the label-carrying ids of a prefix
CHECKER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ans_wl.hpp"
using namespace shuffle_coding;
struct Acc {
    uint32_t* p;
    uint32_t load(uint32_t i) const { return p[i]; }
    void store(uint32_t i, uint32_t v) { p[i] = v; }
};
struct Ws {
    uint32_t* p;
    Acc at(uint64_t o, uint64_t) const { return Acc{p + o}; }
};
using L = rgraph::Labels<true, true>;
// argv: n, known positions, wl_iter, half_iter, the n node labels, then (i, j, label) per pair; prints
// every level of every position
int main(int argc, char** argv) {
    const uint32_t n = atoi(argv[1]), len = atoi(argv[2]), wl_iter = atoi(argv[3]), half = atoi(argv[4]);
    std::vector<uint32_t> nl, e, el;
    for (uint32_t v = 0; v < n; ++v) nl.push_back(atoi(argv[5 + v]));
    for (int k = 5 + n; k + 2 < argc; k += 3) e.push_back(atoi(argv[k])), e.push_back(atoi(argv[k + 1])), el.push_back(atoi(argv[k + 2]));
    const uint32_t E = el.size();
    std::vector<uint32_t> ws(wl::er_push_entries(n, E, wl_iter, true));
    auto st = wl::ErPush<Acc, L>::make(Ws{ws.data()}, n, E, wl_iter, half != 0);
    st.lab.nl = nl.data();
    if (wl::build_csr(st.off, st.nbr, st.mark, n, true, e.data(), E, [&](uint32_t at, uint32_t k) { st.lab.elab.store(at, el[k]); })) return 1;
    for (uint32_t v = 0; v < n; ++v) st.pos_of.store(v, v), st.node_at.store(v, v);
    st.orb.apply(st.orb.adj_of(st), n, len);
    for (uint32_t p = 0; p < n; ++p)
        for (uint32_t t = 0; t <= wl_iter; ++t) printf("%016llx\n", (unsigned long long)st.orb.id(p, t));
    return 0;
}
"""

# (what, n, known, wl_iter, half_iter, node labels, [((i, j), label)], position, level)
ID_CASES = [
    ("level 0 of a known node of label 3", 3, 2, 0, False, [1, 3, 0], [((0, 1), 0)], 1, 0),
    ("level 0 of an unknown node", 4, 2, 0, False, [1, 3, 0, 0], [((0, 3), 1)], 3, 0),
    ("a half-iteration id with edge labels", 4, 3, 0, True, [0, 0, 1, 0], [((0, 1), 3), ((0, 2), 1), ((0, 3), 1), ((0, 0), 0)], 0, 0),
    ("a level-1 id with pairs", 5, 3, 1, True, [2, 0, 0, 0, 0], [((0, 1), 1), ((0, 2), 0), ((0, 3), 0), ((0, 4), 3), ((1, 2), 1)], 0, 1),
]


def test_the_librarys_ids_are_the_mirrors(tmp_path):
    src, exe = tmp_path / "labelled_ids.cpp", tmp_path / "labelled_ids"
    src.write_text(CHECKER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])
    seen = set()
    for what, n, known, wl_iter, half_iter, nodes, edges, position, level in ID_CASES:
        args = [n, known, wl_iter, int(half_iter)] + nodes + [v for (i, j), l in edges for v in (i, j, l)]
        out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        got = [int(v, 16) for v in out.stdout.split()]
        # the prefix graph: an edge between two unknown positions is absent, an unknown node's label 0
        adj, labels = LM.graph_of(n, nodes, [(e, l) for e, l in edges if e[0] < known or e[1] < known])
        labels = [l if p < known else 0 for p, l in enumerate(labels)]
        want = LM.apply_ids(adj, labels, known, wl_iter, half_iter, True, True)
        assert got == [h for id_ in want for h in id_], what
        seen.add(want[position][level])
    assert len(seen) == len(ID_CASES)
    # the first two by hand: (3, None) feeds 3 and the discriminant 0; (0, Some(3)) feeds 0, 1, 3
    assert LM.apply_ids([{}] * 3, [1, 3, 0], 2, 0, False, True, True)[1] == (WM.sip([3, 0]),)
    assert LM.apply_ids([{}] * 4, [1, 3, 0, 0], 2, 0, False, True, True)[3] == (WM.sip([0, 1, 3]),)
