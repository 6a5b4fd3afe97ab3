"""Rate of multiset shuffle coding in bulk on the GPU: ans_dev_mset_push / _pop,
one multiset per chunk.

Device-resident: 2^log2n u8 symbols generated in HBM by ans_dev_gen_iid with the C3 table,
chunk_len 4,096 (2^28 symbols: 65,536 multisets), every slot preloaded with 64 random seed bytes.
HIP events on the call's stream around each kernel, mean of `reps` passes after `warm` untimed ones
(a pop returns every slot to its seed, so each pass starts from the same bytes); the last pass is
verified: every chunk's popped values are its pushed multiset, every slot its seed again.
Beside it: the compressed bytes against the ordered ans_dev_independent_encode of the same
symbols, the launch record, and the library's own single-thread host codec (ans_mset_push / _pop)
on the first 2^20 of those symbols on this box, the only other implementation there is.
Prints one JSON line; with a path as the second argument, writes it there too.
usage: python tools/mset_bench.py [log2n=28] [out.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "shuffle-coding_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ans_amd as A  # noqa: E402

L = 4096
SEED_BYTES = 64


def main():
    log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    n = 1 << log2n
    nch = n // L
    reps, warm = 5, 2
    gpu = A.Gpu(0)
    cat = A.Categorical(A.c3_masses())
    ts = A.GpuTableSet(gpu, [cat])
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    d_syms = torch.empty(n, dtype=torch.uint8, device="cuda")
    A.GpuTable(gpu, cat).dev_gen_iid(7, 0, n, d_syms, 1, stream)
    cap = (SEED_BYTES + ts.slot_capacity(L) + ts.mset_pop_slack(L) + 127) // 128 * 128
    rng = np.random.default_rng(1)
    seeds = rng.integers(0, 256, (nch, SEED_BYTES), dtype=np.uint8)
    seeds[:, -1] |= 1  # a nonzero top byte
    d_seeds = torch.from_numpy(seeds).cuda()
    slots = torch.zeros((nch, cap), dtype=torch.uint8, device="cuda")
    slots[:, :SEED_BYTES] = d_seeds
    lens = torch.full((nch,), SEED_BYTES, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty_like(d_syms)
    pushed_lens = None
    launches = []

    def push():
        ts.dev_mset_push(0, d_syms, 1, n, L, slots, cap, lens, status, stream)

    def pop():
        ts.dev_mset_pop(0, slots, cap, lens, n, L, out, 1, status, stream)

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
    assert bool((lens == SEED_BYTES).all()) and torch.equal(slots[:, :SEED_BYTES], d_seeds), "slots are not the seeds again"
    step = max(1, nch // 64)  # sort a chunk in 64 at a time: the multisets must match
    for c0 in range(0, nch, step):
        a, b = c0 * L, min(nch, c0 + step) * L
        assert torch.equal(out[a:b].view(-1, L).sort(dim=1).values, d_syms[a:b].view(-1, L).sort(dim=1).values), "multisets differ"
    tp = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))
    tq = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))
    mset_bytes = int(pushed_lens.to(torch.int64).sum().item()) - nch * SEED_BYTES
    # the ordered coding of the same symbols (Message::zeros() per chunk)
    tids = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ocap = ts.slot_capacity(L)
    oslots = torch.empty(nch * ocap, dtype=torch.uint8, device="cuda")
    olens = torch.zeros(nch, dtype=torch.int32, device="cuda")
    ts.dev_encode(tids, d_syms, 1, n, L, oslots, ocap, olens, status, stream)
    torch.cuda.synchronize()
    assert gpu.status(status, stream) == 0
    ordered_bytes = int(olens.to(torch.int64).sum().item())
    # the host codec, single thread, on the first 2^20 symbols
    hn = min(n, 1 << 20)
    hs = d_syms[:hn].cpu().numpy().astype(np.uint32)
    codec = A.MultisetShuffle(cat, L)
    msgs = [A.Message.unflatten(seeds[c].tobytes(), A.GEN_EMPTY) for c in range(hn // L)]
    t0 = time.perf_counter()
    for c, m in enumerate(msgs):
        codec.push(m, hs[c * L:(c + 1) * L])
    t1 = time.perf_counter()
    host_lens = [len(m.flatten()) for m in msgs]
    t2 = time.perf_counter()
    for m in msgs:
        codec.pop(m)
    t3 = time.perf_counter()
    assert host_lens == [int(v) for v in pushed_lens[:hn // L].cpu().numpy()], "host and GPU lengths differ"
    res = dict(tool="mset_bench", symbols=n, chunk_len=L, chunks=nch, seed_bytes=SEED_BYTES, slot_cap=cap,
               push_ms=round(tp, 4), pop_ms=round(tq, 4),
               push_gsym_s=round(n / (tp * 1e-3) / 1e9, 3), pop_gsym_s=round(n / (tq * 1e-3) / 1e9, 3),
               mset_bytes=mset_bytes, ordered_bytes=ordered_bytes,
               mset_bits_per_symbol=round(8 * mset_bytes / n, 5), ordered_bits_per_symbol=round(8 * ordered_bytes / n, 5),
               launches=launches, reps=reps, warm=warm,
               host=dict(symbols=hn, push_s=round(t1 - t0, 4), pop_s=round(t3 - t2, 4),
                         push_msym_s=round(hn / (t1 - t0) / 1e6, 3), pop_msym_s=round(hn / (t3 - t2) / 1e6, 3)))
    text = json.dumps(res)
    print(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
