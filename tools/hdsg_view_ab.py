"""Dev tool (GPU): what the doc view of a resident batch (include/hsg_resident_hdsg.h) and the
work lists sized on the host give a whole eager HSumDocGraph training iteration fed by
``ResidentLoader(shuffle=True)``.

    python tools/hdsg_view_ab.py [--store N] [--cnn dw]

cfg4: a store of N (default 256) HDSG examples (synth.make_batch_docs).  One HSumDocGraph
(train.py's defaults: frozen embedding), every native path on (HSG_SENT_LSTM="2",
HSG_MODEL_GLUE, HSG_WORD_EMBED, HSG_SENT_CNN, loss.sentence_loss, optim.Adam with the clip).
Three legs -- ``model_view=False``; the model view with ``doc_view=False``; ``doc_view=True``
-- are alternated three times, one epoch (N / 32 iterations, 8 at the default) each, on the
same batches, after a warm-up epoch of each.  One JSON line per leg and alternation: the
synchronised wall time of every iteration (ms, ``store.batch`` included) with its median, min
and max, and the host's share (until ``adam.step()`` returns, before the synchronise) with the
share of ``store.batch`` in it.  Run it under ``rocprofv3 --kernel-trace --stats`` for the
kernel times (k_res_hdsg, k_rel_work)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from hetersumgraph_amd import HiGraph, _lib, synth  # noqa: E402
from hetersumgraph_amd import loss as hloss  # noqa: E402
from hetersumgraph_amd import optim as hoptim  # noqa: E402
from hetersumgraph_amd.resident import DocumentStore, ResidentLoader  # noqa: E402

ARGS = sys.argv[1:]
opt = lambda name, default: ARGS[ARGS.index(name) + 1] if name in ARGS else default
N_STORE = int(opt("--store", "256"))
CNN = opt("--cnn", "dw")
CFG = "cfg4"
DEV = torch.device("cuda", 0)
REPS = 3
LEGS = (("model_view_off", dict(model_view=False, doc_view=False)),
        ("doc_view_off", dict(model_view=True, doc_view=False)),
        ("doc_view_on", dict(model_view=True, doc_view=True)))


def line(**kw):
    print(json.dumps(kw), flush=True)


def main():
    B = synth.CONFIGS[CFG][1]
    docs = synth.make_batch_docs(CFG, seed=0, n_docs=N_STORE)
    store = DocumentStore.from_doc_arrays(docs, DEV)
    assert store.model_view and store.doc_view, (store.model_view_reason, store.doc_view_reason)
    hps = bench._HPS(2)
    torch.manual_seed(1)
    embed = torch.nn.Embedding(hps.vocab_size, 300, padding_idx=0)
    embed.weight.requires_grad = False
    model = HiGraph.HSumDocGraph(hps, embed).to(DEV).train()
    adam = hoptim.Adam([p for p in model.parameters() if p.requires_grad], lr=hps.lr, max_grad_norm=1.0)

    def epoch(kw, seed):
        wall, host, asm, lists = [], [], [], 0
        loader = ResidentLoader(store, B, shuffle=True, generator=torch.Generator().manual_seed(seed),
                                drop_last=True, **kw)
        torch.cuda.synchronize()
        batches = iter(loader)
        while True:
            t0 = time.perf_counter()                      # the batch's assembly is part of the iteration
            G = next(batches, (None,))[0]
            if G is None:
                break
            ta = time.perf_counter()
            logits = model(G)
            loss = hloss.sentence_loss(G, logits)
            adam.zero_grad()
            loss.backward()
            adam.step()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            wall.append(round((t2 - t0) * 1e3, 3))
            host.append(round((t1 - t0) * 1e3, 3))
            asm.append(round((ta - t0) * 1e3, 3))
            lists += sum(G.resident_work_lists.values())
        return wall, host, asm, lists

    line(config=CFG, store_docs=len(store), nbytes_per_doc=round(store.nbytes / len(store)), cnn=CNN,
         doc_view_default=DocumentStore.DOC_VIEW)
    with _lib.path_options(HSG_SENT_LSTM="2", HSG_MODEL_GLUE="1", HSG_WORD_EMBED="1", HSG_SENT_CNN=CNN):
        for _, kw in LEGS:
            epoch(kw, 3)
        for rep in range(REPS):
            for leg, kw in LEGS:
                wall, host, asm, lists = epoch(kw, 11 + rep)                # every leg sees the same batches
                line(config=CFG, leg=leg, rep=rep, iterations=len(wall), iteration_ms=wall,
                     median_ms=round(statistics.median(wall), 3), min_ms=min(wall), max_ms=max(wall),
                     median_host_ms=round(statistics.median(host), 3), median_batch_ms=round(statistics.median(asm), 3),
                     relations_with_work_lists=lists)


main()
