"""Rate and cost of graph shuffle coding with Weisfeiler-Lehman orbits in bulk on the GPU (DESIGN.md
§3.12): ans_dev_ar_er_wl_push / _pop and ans_dev_ar_polya_wl_push / _pop, one graph per message, at
wl_iter 0 (the new path), 1 and 2 with the half iteration, for both slice models, and in the same run
the ANS_ORBITS_DEGREE kernels (k_arer_* / k_arpu_*) and the labelled codec (ANS_ORBITS_NONE: the bits
the orbits save are counted from it) on the same graphs.

The dataset, the slots, the timing (HIP events on the call's stream around each kernel, mean of
`reps` passes after `warm` untimed ones) and the verification of the last pass (every graph's popped
pairs are its pushed pairs relabelled by the perm the push returned, every slot its seed again) are
tools/arpu_bench.py's; the Erdős–Rényi slices take the Bernoulli fitted to the dataset's density.
Prints one JSON line per model and setting; with a path as the fourth argument, appends them there.
usage: python tools/wl_bench.py [graphs=65536] [nodes=32] [edges=48] [out.jsonl] [reps=3] [warm=1]
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


def codec_of(gpu, model, bern, setting):
    """setting: "none" / "degree" (the kernels of ans_arer.hip / ans_arpu.hip) or a wl_iter."""
    if setting in ("none", "degree"):
        orbits = A.ORBITS_NONE if setting == "none" else A.ORBITS_DEGREE
        return A.GpuAutoregressiveER(gpu, bern, False, orbits) if model == "er" else A.GpuAutoregressivePolya(gpu, False, orbits)
    return A.GpuAutoregressiveERWL(gpu, bern, False, setting, True) if model == "er" \
        else A.GpuAutoregressivePolyaWL(gpu, False, setting, True)


def run(gpu, model, setting, graphs, n, num_edges, edges, bern, reps, warm):
    seed_bytes = int(math.lgamma(n + 1) / math.log(2)) // 8 + num_edges + 32
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    codec = codec_of(gpu, model, bern, setting)
    slack = codec.slack(n) if model == "er" else codec.slack(n, num_edges)
    s = Slots(graphs, n, num_edges, edges, seed_bytes, slack, stream)
    pop_edges = () if (model == "er" and setting in ("none", "degree")) else (num_edges,)  # (that pop keeps no pairs)
    tp, tq, grown, launches, _ = s.time(
        gpu,
        lambda: codec.dev_push(graphs, s.d_nn, s.d_edges, s.d_eo, n, num_edges, s.slots, s.cap, s.lens, s.status, stream,
                               d_perm=s.d_perm),
        lambda: codec.dev_pop(graphs, s.d_nn, s.out, s.d_eo, s.d_count, n, *pop_edges, s.slots, s.cap, s.lens, s.status,
                              stream),
        reps, warm)
    return dict(tool="wl_bench", model=model, setting=setting if isinstance(setting, str) else f"wl{setting}+half",
                graphs=graphs, nodes=n, edges=num_edges, seed_bytes=seed_bytes, push_ms=round(tp, 4), pop_ms=round(tq, 4),
                push_kgraphs_s=round(graphs / tp, 2), pop_kgraphs_s=round(graphs / tq, 2),
                bits_per_graph=round(8 * grown / graphs, 3), launches=launches, grid=gpu.last_launch_grid(), reps=reps,
                warm=warm)


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
        rows = {}
        for setting in ("none", "degree", 0, 1, 2):
            row = rows[setting] = run(gpu, model, setting, graphs, n, num_edges, edges, bern, reps, warm)
            # against the kernels of the degree classes and the labelled codec of the same run
            row["bits_saved"] = round(rows["none"]["bits_per_graph"] - row["bits_per_graph"], 3)
            row["log2_nfact"] = round(math.lgamma(n + 1) / math.log(2), 3)
            if setting not in ("none", "degree"):
                row["push_over_degree"] = round(row["push_ms"] / rows["degree"]["push_ms"], 2)
                row["pop_over_degree"] = round(row["pop_ms"] / rows["degree"]["pop_ms"], 2)
            text = json.dumps(row)
            print(text, flush=True)
            if len(sys.argv) > 4:
                with open(sys.argv[4], "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    main()
