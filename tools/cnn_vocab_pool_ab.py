"""Dev tool (GPU): the vocabulary path's pool kernel (hsg_cnn_vocab_pool, k_vocab_pool) against its
yardstick, hsg_cnn_tok_pool (k_tok_pool) with U = V and the identity slot map on the same table.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o pool -- python tools/cnn_vocab_pool_ab.py run DIST
    python tools/cnn_vocab_pool_ab.py summarise DIST DIR/.../pool_kernel_trace.csv OUT.json

cfg2's sentence rows: 32 documents of 35 sentences (synth.make_batch_docs), n = 1,120, L = 100, over
a table of V = 50,000 words and 101 positions (271 MB).  DIST is one of the two token distributions
of tools/model_view_ab.py: ``own`` -- every document draws its own words from the whole vocabulary
-- and ``vocab5000`` -- all documents draw from 5,000 ids, so they share tokens.  After a warm-up
the two kernels alternate ROUNDS times, LAUNCHES launches each, on one stream.  ``run`` also prints
event-clock times; the figures that count are the kernels' own durations in the trace, which
``summarise`` reduces to one median per kernel and alternation."""
import csv
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

ROUNDS, LAUNCHES, WARMUP = 3, 20, 5
KERNELS = ("k_tok_pool", "k_vocab_pool")
DISTS = {"own": {}, "vocab5000": dict(vocab_size=5000)}


def run(dist):
    import numpy as np
    import torch
    from hetersumgraph_amd import _lib, cnn, synth
    from hetersumgraph_amd.module.PositionEmbedding import get_sinusoid_encoding_table
    V, D, L = 50000, 300, 100
    dev = torch.device("cuda", 0)
    docs = synth.make_batch_docs("cfg2", seed=0, n_docs=synth.CONFIGS["cfg2"][1], **DISTS[dist])
    ids = torch.from_numpy(np.concatenate([d.words for d in docs], 0)).to(dev)
    n = ids.shape[0]
    assert tuple(ids.shape) == (1120, L) and int(ids.max()) < V
    torch.manual_seed(1)
    E = torch.nn.Embedding(V, D, padding_idx=0).weight.detach().to(dev)
    P = get_sinusoid_encoding_table(L + 1, D, padding_idx=0).to(dev)
    cw = [(torch.randn(50, 1, h, D) * (6.0 / (h * D + 50 * h * D)) ** 0.5).to(dev) for h in cnn.HEIGHTS]
    cb = [torch.zeros(50, device=dev) for _ in cnn.HEIGHTS]
    table = cnn.VocabTable().get(E, P, cw)
    _, rowoff, rows = cnn._layout(ids)
    slot = torch.arange(V, dtype=torch.int32, device=dev)
    bptr = (ctypes.c_void_p * 6)(*[b.data_ptr() for b in cb])
    lib, ptr, st = _lib.load(), _lib.ptr, _lib.stream_of(E)
    out = {k: (torch.empty(n, 300, device=dev), torch.empty(n, 300, dtype=torch.int32, device=dev)) for k in KERNELS}

    def launch(k):
        f, a = out[k]
        if k == "k_tok_pool":
            rc = lib.hsg_cnn_tok_pool(n, L, V, V, ptr(ids), ptr(rowoff), ptr(slot), ptr(table.TW), table.TW.stride(0), bptr,
                                      ptr(f), ptr(a), st)
        else:
            rc = lib.hsg_cnn_vocab_pool(n, L, V, ptr(ids), ptr(rowoff), ptr(table.TW), table.TW.stride(0), bptr, ptr(f),
                                        ptr(a), st)
        _lib.check(rc, k)

    for k in KERNELS:
        for _ in range(WARMUP):
            launch(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in KERNELS}
    for _ in range(ROUNDS):
        for k in KERNELS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                launch(k)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    same = all(torch.equal(a, b) for a, b in zip(*out.values()))
    print(json.dumps({"dist": dist, "n": n, "L": L, "V": V, "gather_rows": int(rows), "distinct_tokens": int(ids.unique().numel()),
                      "table_bytes": table.nbytes(), "event_us_per_launch": {k: [round(x, 1) for x in v] for k, v in ms.items()},
                      "same_bits": same, "device": torch.cuda.get_device_name(0)}))
    if not same:
        raise SystemExit("the two kernels disagree")


def summarise(dist, trace, dest):
    """The kernels' own durations, in launch order: WARMUP of each, then ROUNDS x (LAUNCHES, LAUNCHES)."""
    rows = [r for r in csv.DictReader(open(trace)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == 2 * WARMUP + 2 * ROUNDS * LAUNCHES, len(rows)
    rows = rows[2 * WARMUP:]
    med = {k: [] for k in KERNELS}
    for rnd in range(ROUNDS):
        for j, k in enumerate(KERNELS):
            part = rows[(2 * rnd + j) * LAUNCHES:(2 * rnd + j + 1) * LAUNCHES]
            assert all(k in r["Kernel_Name"] for r in part), (rnd, k)
            med[k].append(round(statistics.median(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in part) / 1e3, 1))
    rec = {"dist": dist, "launches_per_alternation": LAUNCHES, "median_us_per_alternation": med,
           "vocab_not_slower_in_any_alternation": all(b <= a for a, b in zip(med["k_tok_pool"], med["k_vocab_pool"]))}
    print(json.dumps(rec))
    with open(dest, "w") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run" and sys.argv[2] in DISTS:
        run(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "summarise":
        summarise(*sys.argv[2:])
    else:
        raise SystemExit(__doc__)
