"""Rate of the Pólya urn edge-index codec in bulk on the GPU: ans_dev_polya_push /
_pop, one graph per message.

Device-resident synthetic dataset: `graphs` simple graphs of `nodes` nodes and `edges` distinct
random edges each, every slot preloaded with random seed bytes (enough for the orbit pops, which
come first).  Both settings the reference's harness runs, (loops, redraws) = (true, true) and
(false, false).  HIP events on the call's stream around each kernel, mean of `reps` passes after
`warm` untimed ones (a pop returns every slot to its seed, so each pass starts from the same bytes);
the last pass is verified: every graph's popped edges are its pushed edge set, every slot its seed
again.  Beside it: the bytes a graph grew by, the launch record, and the library's own
single-thread host codec (ans_polya_push / _pop) on the first 1,024 graphs on this box, the only
other implementation there is.
Prints one JSON line per setting; with a path as the fourth argument, appends them there too.
usage: python tools/polya_bench.py [graphs=65536] [nodes=32] [edges=48] [out.jsonl]
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "shuffle-coding_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ans_amd as A  # noqa: E402


def dataset(rng, graphs, n, num_edges):
    """(graphs, num_edges, 2) u32: per graph num_edges distinct pairs i < j, in random order."""
    jj, ii = np.tril_indices(n, -1)
    pairs = np.stack([ii, jj], axis=1).astype(np.uint32)  # i < j
    out = np.empty((graphs, num_edges, 2), np.uint32)
    for a in range(0, graphs, 4096):
        b = min(graphs, a + 4096)
        pick = np.argpartition(rng.random((b - a, len(pairs)), dtype=np.float32), num_edges - 1, axis=1)[:, :num_edges]
        out[a:b] = pairs[pick]
    return out


def run(gpu, graphs, n, num_edges, edges, loops, redraws, reps=5, warm=2):
    seed_bytes = (int(math.lgamma(num_edges + 1) / math.log(2)) + num_edges) // 8 + 32
    cap = (seed_bytes + A.GpuPolyaUrn.slack(n, num_edges) + 127) // 128 * 128
    codec = A.GpuPolyaUrn(gpu, loops, redraws)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rng = np.random.default_rng(1)
    seeds = rng.integers(0, 256, (graphs, seed_bytes), dtype=np.uint8)
    seeds[:, -1] |= 1  # a nonzero top byte
    d_seeds = torch.from_numpy(seeds).cuda()
    slots = torch.zeros((graphs, cap), dtype=torch.uint8, device="cuda")
    slots[:, :seed_bytes] = d_seeds
    lens = torch.full((graphs,), seed_bytes, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_nn = torch.full((graphs,), n, dtype=torch.int32, device="cuda")
    d_edges = torch.from_numpy(edges.reshape(-1).view(np.int32)).cuda()
    d_eo = torch.arange(0, graphs * num_edges + 1, num_edges, dtype=torch.int64, device="cuda")
    out = torch.empty_like(d_edges)
    launches, pushed_lens = [], None

    def push():
        codec.dev_push(graphs, d_nn, d_edges, d_eo, n, num_edges, slots, cap, lens, status, stream)

    def pop():
        codec.dev_pop(graphs, d_nn, out, d_eo, n, num_edges, slots, cap, lens, status, stream)

    for _ in range(warm):
        push()
        pop()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record(stream)
        push()
        if not launches:
            launches.append(gpu.last_launch())
        e[1].record(stream)
        if e is ev[-1]:
            pushed_lens = lens.clone()
        pop()
        if len(launches) < 2:
            launches.append(gpu.last_launch())
        e[2].record(stream)
    torch.cuda.synchronize()
    assert gpu.status(status, stream) == 0
    assert bool((lens == seed_bytes).all()) and torch.equal(slots[:, :seed_bytes], d_seeds), "slots are not the seeds again"
    key = lambda t: (t.view(graphs, num_edges, 2).to(torch.int64) * torch.tensor([n, 1], device="cuda")).sum(2).sort(dim=1).values  # noqa: E731
    assert torch.equal(key(out), key(d_edges)), "edge sets differ"
    tp = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))
    tq = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))
    grown = int(pushed_lens.to(torch.int64).sum().item()) - graphs * seed_bytes
    # the host codec, single thread, on the first graphs
    hg = min(graphs, 1024)
    host = A.PolyaUrn(n, num_edges, loops, redraws)
    msgs = [A.Message.unflatten(seeds[c].tobytes(), A.GEN_EMPTY) for c in range(hg)]
    t0 = time.perf_counter()
    for c, m in enumerate(msgs):
        host.push(m, edges[c])
    t1 = time.perf_counter()
    host_lens = [len(m.flatten()) for m in msgs]
    t2 = time.perf_counter()
    for m in msgs:
        host.pop(m)
    t3 = time.perf_counter()
    assert host_lens == [int(v) for v in pushed_lens[:hg].cpu().numpy()], "host and GPU lengths differ"
    total_edges = graphs * num_edges
    return dict(tool="polya_bench", graphs=graphs, nodes=n, edges=num_edges, loops=loops, redraws=redraws,
                seed_bytes=seed_bytes, slot_cap=cap, push_ms=round(tp, 4), pop_ms=round(tq, 4),
                push_kgraphs_s=round(graphs / tp, 2), pop_kgraphs_s=round(graphs / tq, 2),
                push_medges_s=round(total_edges / tp / 1e3, 3), pop_medges_s=round(total_edges / tq / 1e3, 3),
                grown_bytes=grown, bits_per_edge=round(8 * grown / max(total_edges, 1), 4),
                launches=launches, reps=reps, warm=warm,
                host=dict(graphs=hg, push_s=round(t1 - t0, 4), pop_s=round(t3 - t2, 4),
                          push_kgraphs_s=round(hg / (t1 - t0) / 1e3, 3), pop_kgraphs_s=round(hg / (t3 - t2) / 1e3, 3)))


def main():
    graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    num_edges = int(sys.argv[3]) if len(sys.argv) > 3 else 48
    gpu = A.Gpu(0)
    edges = dataset(np.random.default_rng(7), graphs, n, num_edges)
    for loops, redraws in ((True, True), (False, False)):
        text = json.dumps(run(gpu, graphs, n, num_edges, edges, loops, redraws))
        print(text, flush=True)
        if len(sys.argv) > 4:
            with open(sys.argv[4], "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
