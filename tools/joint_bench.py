"""Rate and cost of joint shuffle coding of graphs in bulk on the GPU:
ans_dev_joint_er_wl_push / _pop and ans_dev_joint_polya_wl_push / _pop, one graph per message, at wl_iter
0 and 1 with the half iteration, for both ordered codecs, and in the same run on the same graphs the
ordered codec alone (the bits the orbits take back are counted from it) and the autoregressive WL kernels
of tools/wl_bench.py at the same settings.

The dataset, the slots, the timing (HIP events on the call's stream around each kernel, mean of `reps`
passes after `warm` untimed ones) and the verification of the last pass (every graph's popped pairs are
its pushed pairs relabelled by the perm the push returned, every slot its seed again) are
tools/arpu_bench.py's.  The seed holds what a joint push pops before it pushes: the order of the nodes
and, under the urn, of the pairs.  The ordered urn alone is k_polya_push on the same slots; the ordered
Erdős–Rényi codec alone costs every graph of one size and edge count the same, E log2(norm / mass) +
(slots - E) log2(norm / (norm - mass)) bits, which is computed, not run.
Prints one JSON line per model and setting; with a path as the fourth argument, appends them there.
usage: python tools/joint_bench.py [graphs=65536] [nodes=32] [edges=48] [out.jsonl] [reps=3] [warm=1]
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
import wl_bench  # noqa: E402
from arpu_bench import Slots  # noqa: E402
from polya_bench import dataset  # noqa: E402


def log2_factorial(k):
    return math.lgamma(k + 1) / math.log(2)


def seed_bytes_of(model, n, num_edges):
    return int(log2_factorial(n) + (log2_factorial(num_edges) if model == "pu" else 0)) // 8 + num_edges + 32


def ordered_bits(gpu, model, graphs, n, num_edges, edges, bern, stream):
    """Bits per graph of the ordered codec alone."""
    if model == "er":
        slots = n * (n - 1) // 2
        return num_edges * math.log2(bern.norm() / bern.pmf(1)) + (slots - num_edges) * math.log2(bern.norm() / bern.pmf(0))
    codec = A.GpuPolyaUrn(gpu, False, False)
    seed_bytes = seed_bytes_of(model, n, num_edges)
    s = Slots(graphs, n, num_edges, edges, seed_bytes, codec.slack(n, num_edges), stream)
    codec.dev_push(graphs, s.d_nn, s.d_edges, s.d_eo, n, num_edges, s.slots, s.cap, s.lens, s.status, stream)
    torch.cuda.synchronize()
    assert gpu.status(s.status, stream) == 0
    return 8 * (int(s.lens.to(torch.int64).sum().item()) - graphs * seed_bytes) / graphs


def run(gpu, model, wl_iter, graphs, n, num_edges, edges, bern, reps, warm):
    seed_bytes = seed_bytes_of(model, n, num_edges)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    codec = A.GpuJointERWL(gpu, bern, False, wl_iter, True) if model == "er" else A.GpuJointPolyaWL(gpu, False, False, wl_iter, True)
    slack = codec.slack(n) if model == "er" else codec.slack(n, num_edges)
    s = Slots(graphs, n, num_edges, edges, seed_bytes, slack, stream)
    tp, tq, grown, launches, _ = s.time(
        gpu,
        lambda: codec.dev_push(graphs, s.d_nn, s.d_edges, s.d_eo, n, num_edges, s.slots, s.cap, s.lens, s.status, stream,
                               d_perm=s.d_perm),
        lambda: codec.dev_pop(graphs, s.d_nn, s.out, s.d_eo, s.d_count, n, num_edges, s.slots, s.cap, s.lens, s.status,
                              stream),
        reps, warm)
    grid = gpu.last_launch_grid()
    del s
    alone = ordered_bits(gpu, model, graphs, n, num_edges, edges, bern, stream)
    ar = wl_bench.run(gpu, model, wl_iter, graphs, n, num_edges, edges, bern, reps, warm)
    bits = 8 * grown / graphs
    return dict(tool="joint_bench", model=model, setting=f"wl{wl_iter}+half", graphs=graphs, nodes=n, edges=num_edges,
                seed_bytes=seed_bytes, push_ms=round(tp, 4), pop_ms=round(tq, 4), push_kgraphs_s=round(graphs / tp, 2),
                pop_kgraphs_s=round(graphs / tq, 2), bits_per_graph=round(bits, 3), ordered_bits_per_graph=round(alone, 3),
                bits_saved=round(alone - bits, 3), log2_nfact=round(log2_factorial(n), 3),
                ar_wl_bits_per_graph=ar["bits_per_graph"], ar_wl_push_ms=ar["push_ms"], ar_wl_pop_ms=ar["pop_ms"],
                push_over_ar_wl=round(tp / ar["push_ms"], 2), pop_over_ar_wl=round(tq / ar["pop_ms"], 2), launches=launches,
                grid=grid, reps=reps, warm=warm)


def main():
    graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    num_edges = int(sys.argv[3]) if len(sys.argv) > 3 else 48
    reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    warm = int(sys.argv[6]) if len(sys.argv) > 6 else 1
    gpu = A.Gpu(0)
    edges = dataset(np.random.default_rng(7), graphs, n, num_edges)
    bern = A.Bernoulli(num_edges, n * (n - 1) // 2)
    for model in ("er", "pu"):
        for wl_iter in (0, 1):
            text = json.dumps(run(gpu, model, wl_iter, graphs, n, num_edges, edges, bern, reps, warm))
            print(text, flush=True)
            if len(sys.argv) > 4:
                with open(sys.argv[4], "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    main()
