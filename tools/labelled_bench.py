"""Rate and cost of graph shuffle coding with node and edge labels in bulk on the GPU (DESIGN.md
§3.13): ans_dev_ar_er_wl_labelled_push / _pop and ans_dev_ar_polya_wl_labelled_push / _pop, one graph
per message, at wl_iter 1 with the half iteration (the reference's default), with 7 node labels and 4
edge labels under skewed Categoricals, and in the same run on the same graphs
  * the unlabelled WL kernels (k_ar*_wl_*: the labels dropped), for what the labels cost in time;
  * GpuGraphs, the ordered GraphIID<NodeC, EdgeC, ErdosRenyi> of section 5b with the same tables, for
    the bits the shuffle saves: its stream lengths less that of an empty message's stream (the head
    of Message::zeros()), against the bytes a labelled push adds to its seed.
Two synthetic datasets: molecule-like graphs (n = 18, E = 20) and the n = 32, E = 48 shape of the other
benches; the pairs are uniform over the alphabet, as tools/polya_bench.py draws them.

The slots, the timing (HIP events on the call's stream around each kernel, mean of `reps` passes after
`warm` untimed ones) and the verification of the pairs and the seeds are tools/arpu_bench.py's; the
labels of the last pass are verified here (every position's label is its input node's, every popped
pair carries its input pair's label).  Prints one JSON line per dataset and model; with a path as the
second argument, appends them there.
usage: python tools/labelled_bench.py [graphs=65536] [out.jsonl] [reps=3] [warm=1]
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "shuffle-coding_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ans_amd as A  # noqa: E402
from arpu_bench import Slots  # noqa: E402
from polya_bench import dataset  # noqa: E402

NODE_MASSES = [600, 150, 120, 60, 40, 20, 10]  # seven node labels, one common (a molecule's carbon)
EDGE_MASSES = [700, 200, 80, 20]               # four edge labels


def draw(rng, masses, shape):
    p = np.asarray(masses, np.float64)
    return rng.choice(len(masses), size=shape, p=p / p.sum()).astype(np.uint32)


def entropy_bits(masses):
    p = np.asarray(masses, np.float64) / sum(masses)
    return float(-(p * np.log2(p)).sum())


def time_codec(gpu, codec, labelled, graphs, n, num_edges, edges, nl, el, seed_bytes, reps, warm):
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    s = Slots(graphs, n, num_edges, edges, seed_bytes, codec.slack(n, num_edges) if labelled or codec_is_polya(codec)
              else codec.slack(n), stream)
    if labelled:
        d_nl, d_el = torch.from_numpy(nl.view(np.int32)).cuda(), torch.from_numpy(el.reshape(-1).view(np.int32)).cuda()
        nl_out, el_out = torch.empty_like(d_nl), torch.empty_like(d_el)
        push = lambda: codec.dev_push(graphs, s.d_nn, s.d_edges, s.d_eo, d_nl, d_el, n, num_edges, s.slots, s.cap, s.lens,  # noqa: E731
                                      s.status, stream, d_perm=s.d_perm)
        pop = lambda: codec.dev_pop(graphs, s.d_nn, s.out, s.d_eo, s.d_count, nl_out, el_out, n, num_edges, s.slots, s.cap,  # noqa: E731
                                    s.lens, s.status, stream)
    else:
        push = lambda: codec.dev_push(graphs, s.d_nn, s.d_edges, s.d_eo, n, num_edges, s.slots, s.cap, s.lens, s.status,  # noqa: E731
                                      stream, d_perm=s.d_perm)
        pop = lambda: codec.dev_pop(graphs, s.d_nn, s.out, s.d_eo, s.d_count, n, num_edges, s.slots, s.cap, s.lens,  # noqa: E731
                                    s.status, stream)
    tp, tq, grown, launches, _ = s.time(gpu, push, pop, reps, warm)
    if labelled:
        perm = s.d_perm.to(torch.int64)
        assert torch.equal(nl_out.view(graphs, n), torch.gather(d_nl.view(graphs, n), 1, perm)), "node labels differ"
        pos = torch.argsort(perm, dim=1)
        given = torch.gather(pos, 1, s.d_edges.view(graphs, -1).to(torch.int64)).view(graphs, num_edges, 2).sort(dim=2).values
        weight = torch.tensor([n, 1], device="cuda")
        key = lambda pairs, labels: (((pairs.view(graphs, num_edges, 2).to(torch.int64) * weight).sum(2) << 8)  # noqa: E731
                                     + labels.view(graphs, num_edges).to(torch.int64)).sort(dim=1).values
        assert torch.equal(key(s.out, el_out), key(given, d_el)), "edge labels differ"
    return tp, tq, grown, launches


def codec_is_polya(codec):
    return isinstance(codec, A.GpuAutoregressivePolyaWL)


def run(gpu, model, graphs, n, num_edges, edges, nl, el, bern, iid_bits, reps, warm):
    seed_bytes = int(math.lgamma(n + 1) / math.log(2)) // 8 + num_edges + 32
    node, edge = A.Categorical(np.asarray(NODE_MASSES, np.uint64)), A.Categorical(np.asarray(EDGE_MASSES, np.uint64))
    if model == "er":
        new = A.GpuAutoregressiveERLabelled(gpu, bern, False, 1, True, node, edge)
        old = A.GpuAutoregressiveERWL(gpu, bern, False, 1, True)
    else:
        new = A.GpuAutoregressivePolyaLabelled(gpu, False, 1, True, node, edge)
        old = A.GpuAutoregressivePolyaWL(gpu, False, 1, True)
    tp, tq, grown, launches = time_codec(gpu, new, True, graphs, n, num_edges, edges, nl, el, seed_bytes, reps, warm)
    grid = gpu.last_launch_grid()
    up, uq, ugrown, _ = time_codec(gpu, old, False, graphs, n, num_edges, edges, nl, el, seed_bytes, reps, warm)
    bits = 8 * grown / graphs
    return dict(tool="labelled_bench", model=model, setting="wl1+half", graphs=graphs, nodes=n, edges=num_edges,
                node_labels=len(NODE_MASSES), edge_labels=len(EDGE_MASSES), seed_bytes=seed_bytes,
                push_ms=round(tp, 4), pop_ms=round(tq, 4), push_kgraphs_s=round(graphs / tp, 2),
                pop_kgraphs_s=round(graphs / tq, 2), bits_per_graph=round(bits, 3),
                label_bits_expected=round(n * entropy_bits(NODE_MASSES) + num_edges * entropy_bits(EDGE_MASSES), 3),
                unlabelled_push_ms=round(up, 4), unlabelled_pop_ms=round(uq, 4),
                unlabelled_bits_per_graph=round(8 * ugrown / graphs, 3),
                push_over_unlabelled=round(tp / up, 2), pop_over_unlabelled=round(tq / uq, 2),
                graph_iid_bits_per_graph=round(iid_bits, 3), bits_saved_over_graph_iid=round(iid_bits - bits, 3),
                log2_nfact=round(math.lgamma(n + 1) / math.log(2), 3), launches=launches, grid=grid, reps=reps, warm=warm)


def graph_iid_bits(gpu, bern, n, edges, nl, el):
    """Bits per graph of the ordered codec (GpuGraphs: GraphIID with the Erdős–Rényi indices and the
    same label tables) on the same graphs, less the length of an empty message's stream."""
    node, edge = A.Categorical(np.asarray(NODE_MASSES, np.uint64)), A.Categorical(np.asarray(EDGE_MASSES, np.uint64))
    codec = A.GpuGraphs(gpu, bern, node, edge)
    _, _, lens = codec.encode([(n, nl[g], edges[g], el[g]) for g in range(len(edges))])
    return 8 * (float(lens.astype(np.float64).mean()) - len(A.Message.zeros().flatten()))


def main():
    graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    warm = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    gpu = A.Gpu(0)
    for n, num_edges in ((18, 20), (32, 48)):
        rng = np.random.default_rng(7)
        edges = dataset(rng, graphs, n, num_edges)
        nl, el = draw(rng, NODE_MASSES, (graphs, n)), draw(rng, EDGE_MASSES, (graphs, num_edges))
        bern = A.Bernoulli(num_edges, n * (n - 1) // 2)
        iid_bits = graph_iid_bits(gpu, bern, n, edges, nl, el)
        for model in ("er", "pu"):
            text = json.dumps(run(gpu, model, graphs, n, num_edges, edges, nl, el, bern, iid_bits, reps, warm))
            print(text, flush=True)
            if len(sys.argv) > 2:
                with open(sys.argv[2], "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    main()
