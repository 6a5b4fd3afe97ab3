"""Rate of the autoregressive Erdős–Rényi graph codecs in bulk on the GPU:
ans_dev_ar_er_push / _pop, one graph per message, for each `orbits` value.

Device-resident synthetic dataset: `graphs` simple graphs of `nodes` nodes and `edges` distinct
random edges each, every slot preloaded with random seed bytes (enough for the orbit pops, which
come first); the Bernoulli is the dataset's own, Bernoulli(edges, nodes (nodes - 1) / 2).  HIP events
on the call's stream around each kernel, mean of `reps` passes after `warm` untimed ones (a pop
returns every slot to its seed, so each pass starts from the same bytes); the last pass is verified:
every graph's popped pairs are its pushed pairs relabelled by the perm the push returned, every slot
its seed again.  Beside it, on the same graphs:
  * the same codec through the host-buffer calls (ans_gpu_ar_er_push_graphs / _pop_graphs) and the
    labelled Erdős–Rényi coding of ans_gpu_dense_sets_encode / _decode, which codes the same number
    of indicators with the fast kernels: both synchronous calls with their copies, by the wall clock,
    best of three;
  * the library's own single-thread host codec (ans_ar_er_push / _pop) on the first 1,024 graphs.
Prints one JSON line per orbits value; with a path as the fourth argument, appends them there too.
usage: python tools/arer_bench.py [graphs=65536] [nodes=32] [edges=48] [out.jsonl]
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


def best_of(fn, times=3):
    out, best = None, float("inf")
    for _ in range(times):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t0)
    return out, best * 1e3


def run(gpu, graphs, n, num_edges, edges, bern, orbits, reps=5, warm=2):
    seed_bytes = int(math.lgamma(n + 1) / math.log(2)) // 8 + 32
    codec = A.GpuAutoregressiveER(gpu, bern, False, orbits)
    cap = (seed_bytes + codec.slack(n) + 127) // 128 * 128
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
    d_perm = torch.zeros((graphs, n), dtype=torch.int32, device="cuda")
    d_count = torch.zeros(graphs, dtype=torch.int32, device="cuda")
    out = torch.empty_like(d_edges)
    launches, pushed_lens = [], None

    def push():
        codec.dev_push(graphs, d_nn, d_edges, d_eo, n, num_edges, slots, cap, lens, status, stream, d_perm=d_perm)

    def pop():
        codec.dev_pop(graphs, d_nn, out, d_eo, d_count, n, slots, cap, lens, status, stream)

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
    assert bool((d_count == num_edges).all()), "pair counts differ"
    pos = torch.argsort(d_perm.to(torch.int64), dim=1)  # the position of every input node
    given = torch.gather(pos, 1, d_edges.view(graphs, -1).to(torch.int64)).view(graphs, num_edges, 2).sort(dim=2).values
    key = lambda t: (t.view(graphs, num_edges, 2).to(torch.int64) * torch.tensor([n, 1], device="cuda")).sum(2).sort(dim=1).values  # noqa: E731
    assert torch.equal(key(out), key(given)), "the popped graph is not the input relabelled"
    tp = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))
    tq = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))
    grown = int(pushed_lens.to(torch.int64).sum().item()) - graphs * seed_bytes
    # the host-buffer calls, with their copies
    # (the C entries themselves: the Python wrappers' per-graph list handling is not the library's time)
    P, lib = A._np_ptr, A.lib()
    nn = np.full(graphs, n, np.uint32)
    flat = np.ascontiguousarray(edges.reshape(-1, 2))
    eo = np.arange(graphs + 1, dtype=np.uint64) * np.uint64(num_edges)
    seed_lens = np.full(graphs, seed_bytes, np.uint64)
    seed_offs = np.arange(graphs, dtype=np.uint64) * np.uint64(seed_bytes)
    data = np.ascontiguousarray(seeds.reshape(-1))
    box = [np.empty(graphs * cap, np.uint8), np.zeros(graphs, np.uint64), np.zeros(graphs, np.uint64)]
    rest = [np.empty(graphs * cap, np.uint8), np.zeros(graphs, np.uint64), np.zeros(graphs, np.uint64)]
    perm = np.zeros((graphs, n), np.uint32)
    back, counts, total = np.zeros_like(flat), np.zeros(graphs, np.uint32), A.u64(0)
    _, hb_push = best_of(lambda: A._check(lib.ans_gpu_ar_er_push_graphs(
        codec.table.h, 0, orbits, graphs, P(nn), P(flat), P(eo), P(data), data.size, P(seed_offs), P(seed_lens), P(perm),
        P(box[0]), box[0].size, P(box[1]), P(box[2]), A.ctypes.byref(total)), "ans_gpu_ar_er_push_graphs"))
    pushed_total = total.value
    assert [int(v) for v in box[2]] == [int(v) for v in pushed_lens.cpu().numpy()], "host-buffer and device lengths differ"
    _, hb_pop = best_of(lambda: A._check(lib.ans_gpu_ar_er_pop_graphs(
        codec.table.h, 0, orbits, graphs, P(nn), P(eo), P(box[0]), pushed_total, P(box[1]), P(box[2]), P(back), P(counts),
        P(rest[0]), rest[0].size, P(rest[1]), P(rest[2]), A.ctypes.byref(total)), "ans_gpu_ar_er_pop_graphs"))
    assert bool((counts == num_edges).all()) and bytes(rest[0][:total.value]) == data.tobytes(), "host-buffer round trip"
    # the host codec, single thread, on the first graphs
    hg = min(graphs, 1024)
    host = A.AutoregressiveER(bern, n, False, orbits)
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
    steps = graphs * (n * (n - 1) // 2)
    return dict(tool="arer_bench", graphs=graphs, nodes=n, edges=num_edges, orbits=ORBITS_NAME[orbits],
                mass=int(bern.categorical.masses[1]), norm=bern.norm(), seed_bytes=seed_bytes, slot_cap=cap,
                push_ms=round(tp, 4), pop_ms=round(tq, 4),
                push_kgraphs_s=round(graphs / tp, 2), pop_kgraphs_s=round(graphs / tq, 2),
                push_mindicators_s=round(steps / tp / 1e3, 3), pop_mindicators_s=round(steps / tq / 1e3, 3),
                grown_bytes=grown, bits_per_graph=round(8 * grown / graphs, 3), launches=launches, reps=reps, warm=warm,
                host_buffers=dict(push_ms=round(hb_push, 3), pop_ms=round(hb_pop, 3)),
                host=dict(graphs=hg, push_s=round(t1 - t0, 4), pop_s=round(t3 - t2, 4),
                          push_kgraphs_s=round(hg / (t1 - t0) / 1e3, 3), pop_kgraphs_s=round(hg / (t3 - t2) / 1e3, 3)))


def dense_sets(gpu, graphs, n, edges, bern):
    """The labelled coding of the same graphs: ans_gpu_dense_sets_encode / _decode, host buffers."""
    P, lib = A._np_ptr, A.lib()
    table = A.GpuTable(gpu, bern.categorical)
    num_edges = edges.shape[1]
    nn = np.full(graphs, n, np.uint32)
    flat = np.ascontiguousarray(edges.reshape(-1, 2))
    eo = np.arange(graphs + 1, dtype=np.uint64) * np.uint64(num_edges)
    out = np.empty(graphs * table.slot_capacity(n * (n - 1) // 2), np.uint8)
    offs, lens, total = np.zeros(graphs, np.uint64), np.zeros(graphs, np.uint64), A.u64(0)
    _, enc = best_of(lambda: A._check(lib.ans_gpu_dense_sets_encode(
        table.h, graphs, P(nn), 0, 0, P(flat), P(eo), P(out), out.size, P(offs), P(lens), A.ctypes.byref(total)),
        "ans_gpu_dense_sets_encode"))
    launch = gpu.last_launch()
    back, eo_back = np.zeros_like(flat), np.zeros(graphs + 1, np.uint64)
    _, dec = best_of(lambda: A._check(lib.ans_gpu_dense_sets_decode(
        table.h, graphs, P(nn), 0, 0, P(out), total.value, P(offs), P(lens), P(back), len(back), P(eo_back)),
        "ans_gpu_dense_sets_decode"))
    assert np.array_equal(eo_back, eo), "pair counts differ"
    key = lambda t: np.sort(t.reshape(graphs, num_edges, 2).astype(np.int64) @ np.array([n, 1]), axis=1)  # noqa: E731
    assert np.array_equal(key(back), key(flat)), "edge sets differ"
    return dict(encode_ms=round(enc, 3), decode_ms=round(dec, 3), bytes=int(total.value),
                bits_per_graph=round(8 * int(total.value) / graphs, 3), launches=[launch, gpu.last_launch()])


def main():
    graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    num_edges = int(sys.argv[3]) if len(sys.argv) > 3 else 48
    gpu = A.Gpu(0)
    edges = dataset(np.random.default_rng(7), graphs, n, num_edges)
    bern = A.Bernoulli(num_edges, n * (n - 1) // 2)
    dense = dense_sets(gpu, graphs, n, edges, bern)
    for orbits in (A.ORBITS_NONE, A.ORBITS_ONE_CLASS, A.ORBITS_DEGREE):
        row = run(gpu, graphs, n, num_edges, edges, bern, orbits)
        row["dense_sets"] = dense
        text = json.dumps(row)
        print(text, flush=True)
        if len(sys.argv) > 4:
            with open(sys.argv[4], "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
