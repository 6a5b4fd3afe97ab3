"""Rate and cost of the autoregressive Pólya urn graph codecs in bulk on the GPU:
ans_dev_ar_polya_push / _pop, one graph per message, for each `orbits` value.

Device-resident synthetic dataset: `graphs` simple graphs of `nodes` nodes and `edges` distinct
random edges each, every slot preloaded with random seed bytes (enough for the orbit and permutation
pops of a push).  HIP events on the call's stream around each kernel, mean of `reps` passes after
`warm` untimed ones (a pop returns every slot to its seed, so each pass starts from the same bytes);
the last pass is verified: every graph's popped pairs are its pushed pairs relabelled by the perm the
push returned, every slot its seed again.  Beside it, on the same graphs:
  * k_arer_push / k_arer_pop (ans_dev_ar_er_push / _pop) with the Bernoulli fitted to the dataset's
    density, Bernoulli(edges, nodes (nodes - 1) / 2): bits per graph, and one timed pass after one warm;
  * the library's own single-thread host codec (ans_ar_polya_push / _pop) on the first graphs.
Prints one JSON line per orbits value; with a path as the fourth argument, appends them there too.
usage: python tools/arpu_bench.py [graphs=65536] [nodes=32] [edges=48] [out.jsonl]
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "shuffle-coding_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ans_amd as A  # noqa: E402
from polya_bench import dataset  # noqa: E402

ORBITS_NAME = {A.ORBITS_NONE: "none", A.ORBITS_ONE_CLASS: "one_class", A.ORBITS_DEGREE: "degree"}


class Slots:
    """The graphs, their seeded slots and the room for what a pop returns, on the device."""

    def __init__(self, graphs, n, num_edges, edges, seed_bytes, slack, stream):
        self.graphs, self.n, self.num_edges, self.seed_bytes, self.stream = graphs, n, num_edges, seed_bytes, stream
        self.cap = (seed_bytes + slack + 127) // 128 * 128
        rng = np.random.default_rng(1)
        self.seeds = rng.integers(0, 256, (graphs, seed_bytes), dtype=np.uint8)
        self.seeds[:, -1] |= 1  # a nonzero top byte
        self.d_seeds = torch.from_numpy(self.seeds).cuda()
        self.slots = torch.zeros((graphs, self.cap), dtype=torch.uint8, device="cuda")
        self.slots[:, :seed_bytes] = self.d_seeds
        self.lens = torch.full((graphs,), seed_bytes, dtype=torch.int32, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.d_nn = torch.full((graphs,), n, dtype=torch.int32, device="cuda")
        self.d_edges = torch.from_numpy(edges.reshape(-1).view(np.int32)).cuda()
        self.d_eo = torch.arange(0, graphs * num_edges + 1, num_edges, dtype=torch.int64, device="cuda")
        self.d_perm = torch.zeros((graphs, n), dtype=torch.int32, device="cuda")
        self.d_count = torch.zeros(graphs, dtype=torch.int32, device="cuda")
        self.out = torch.empty_like(self.d_edges)

    def time(self, gpu, push, pop, reps, warm):
        """(push ms, pop ms, bytes the push added, kernel names), the last pass verified."""
        for _ in range(warm):
            push()
            pop()
        launches, pushed_lens = [], None
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
        for e in ev:
            e[0].record(self.stream)
            push()
            if not launches:
                launches.append(gpu.last_launch())
            e[1].record(self.stream)
            if e is ev[-1]:
                pushed_lens = self.lens.clone()
            pop()
            if len(launches) < 2:
                launches.append(gpu.last_launch())
            e[2].record(self.stream)
        torch.cuda.synchronize()
        graphs, n, num_edges = self.graphs, self.n, self.num_edges
        assert gpu.status(self.status, self.stream) == 0
        assert bool((self.lens == self.seed_bytes).all()) and torch.equal(self.slots[:, :self.seed_bytes], self.d_seeds), \
            "slots are not the seeds again"
        assert bool((self.d_count == num_edges).all()), "pair counts differ"
        pos = torch.argsort(self.d_perm.to(torch.int64), dim=1)  # the position of every input node
        given = torch.gather(pos, 1, self.d_edges.view(graphs, -1).to(torch.int64)).view(graphs, num_edges, 2)
        given = given.sort(dim=2).values
        weight = torch.tensor([n, 1], device="cuda")
        key = lambda t: (t.view(graphs, num_edges, 2).to(torch.int64) * weight).sum(2).sort(dim=1).values  # noqa: E731
        assert torch.equal(key(self.out), key(given)), "the popped graph is not the input relabelled"
        tp = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))
        tq = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))
        grown = int(pushed_lens.to(torch.int64).sum().item()) - graphs * self.seed_bytes
        return tp, tq, grown, launches, pushed_lens


def run(gpu, graphs, n, num_edges, edges, orbits, reps=5, warm=2):
    seed_bytes = int(math.lgamma(n + 1) / math.log(2)) // 8 + num_edges + 32
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    # ---- the Pólya urn slices
    codec = A.GpuAutoregressivePolya(gpu, False, orbits)
    s = Slots(graphs, n, num_edges, edges, seed_bytes, codec.slack(n, num_edges), stream)
    tp, tq, grown, launches, pushed_lens = s.time(
        gpu,
        lambda: codec.dev_push(graphs, s.d_nn, s.d_edges, s.d_eo, n, num_edges, s.slots, s.cap, s.lens, s.status, stream,
                               d_perm=s.d_perm),
        lambda: codec.dev_pop(graphs, s.d_nn, s.out, s.d_eo, s.d_count, n, num_edges, s.slots, s.cap, s.lens, s.status,
                              stream),
        reps, warm)
    seeds = s.seeds
    del s
    # ---- the Erdős–Rényi slices on the same graphs, the Bernoulli fitted to their density
    bern = A.Bernoulli(num_edges, n * (n - 1) // 2)
    er = A.GpuAutoregressiveER(gpu, bern, False, orbits)
    s = Slots(graphs, n, num_edges, edges, seed_bytes, er.slack(n), stream)
    ep, eq, er_grown, er_launches, _ = s.time(
        gpu,
        lambda: er.dev_push(graphs, s.d_nn, s.d_edges, s.d_eo, n, num_edges, s.slots, s.cap, s.lens, s.status, stream,
                            d_perm=s.d_perm),
        lambda: er.dev_pop(graphs, s.d_nn, s.out, s.d_eo, s.d_count, n, s.slots, s.cap, s.lens, s.status, stream),
        1, 1)
    del s
    # ---- the host codec, single thread, on the first graphs
    hg = min(graphs, 1024 if n <= 64 else 128)
    host = A.AutoregressivePolya(n, False, orbits)
    msgs = [A.Message.unflatten(seeds[c].tobytes(), A.GEN_EMPTY) for c in range(hg)]
    t0 = time.perf_counter()
    for c, m in enumerate(msgs):
        host.push(m, edges[c])
    t1 = time.perf_counter()
    host_lens = [len(m.flatten()) for m in msgs]
    t2 = time.perf_counter()
    for m in msgs:
        host.pop(m, cap=num_edges)
    t3 = time.perf_counter()
    assert host_lens == [int(v) for v in pushed_lens[:hg].cpu().numpy()], "host and GPU lengths differ"
    host_push, host_pop = hg / (t1 - t0), hg / (t3 - t2)
    return dict(tool="arpu_bench", graphs=graphs, nodes=n, edges=num_edges, orbits=ORBITS_NAME[orbits],
                seed_bytes=seed_bytes, push_ms=round(tp, 4), pop_ms=round(tq, 4),
                push_kgraphs_s=round(graphs / tp, 2), pop_kgraphs_s=round(graphs / tq, 2),
                grown_bytes=grown, bits_per_graph=round(8 * grown / graphs, 3), launches=launches, reps=reps, warm=warm,
                arer=dict(mass=num_edges, norm=n * (n - 1) // 2, push_ms=round(ep, 4), pop_ms=round(eq, 4),
                          push_kgraphs_s=round(graphs / ep, 2), pop_kgraphs_s=round(graphs / eq, 2),
                          bits_per_graph=round(8 * er_grown / graphs, 3), launches=er_launches, reps=1, warm=1),
                host=dict(graphs=hg, push_s=round(t1 - t0, 4), pop_s=round(t3 - t2, 4),
                          push_kgraphs_s=round(host_push / 1e3, 3), pop_kgraphs_s=round(host_pop / 1e3, 3),
                          gpu_over_host_push=round(graphs / tp * 1e3 / host_push, 1),
                          gpu_over_host_pop=round(graphs / tq * 1e3 / host_pop, 1)))


def main():
    graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    num_edges = int(sys.argv[3]) if len(sys.argv) > 3 else 48
    gpu = A.Gpu(0)
    edges = dataset(np.random.default_rng(7), graphs, n, num_edges)
    for orbits in (A.ORBITS_NONE, A.ORBITS_ONE_CLASS, A.ORBITS_DEGREE):
        row = run(gpu, graphs, n, num_edges, edges, orbits)
        text = json.dumps(row)
        print(text, flush=True)
        if len(sys.argv) > 4:
            with open(sys.argv[4], "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
