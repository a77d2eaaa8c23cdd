"""Dev tool (GPU): what the model view of a resident batch (include/hsg_resident_model.h) gives
a whole eager training iteration fed by ``ResidentLoader(shuffle=True)``.

    python tools/model_view_ab.py [--store N] [--configs cfg2,cfg5] [--cnn 0,dw,tokens] [--vocab V]

Per configuration a store of N (default 256) documents (synth.make_batch_docs; ``--vocab V``
draws every document's words from a vocabulary of V ids, so documents share tokens; the default
gives every document its own words).  One model (train.py's defaults: frozen embedding), every
native path on (HSG_SENT_LSTM="2", HSG_MODEL_GLUE, HSG_WORD_EMBED, loss.sentence_loss,
optim.Adam with the clip).  Per value of HSG_SENT_CNN the legs ``model_view=False`` and
``model_view=True`` are alternated three times, one epoch (N / 32 iterations, 8 at the default)
each, on the same batches, after a warm-up epoch of each.  One JSON line per leg and
alternation: the synchronised wall time of every iteration (ms, ``store.batch`` included) with
its median, min and max, the host's share (until ``adam.step()`` returns, before the
synchronise) and, with the view, the median of its bound on the batch's distinct tokens.  Run
it under ``rocprofv3 --kernel-trace --stats`` for the kernel times."""
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
CONFIGS = opt("--configs", "cfg2,cfg5").split(",")
CNN = opt("--cnn", "0,dw,tokens").split(",")
VOCAB = int(opt("--vocab", "0"))
DEV = torch.device("cuda", 0)
REPS = 3


def line(**kw):
    print(json.dumps(kw), flush=True)


def legs(cfg):
    B = synth.CONFIGS[cfg][1]
    over = dict(vocab_size=VOCAB) if VOCAB else {}
    docs = synth.make_batch_docs(cfg, seed=0, n_docs=N_STORE, **over)
    store = DocumentStore.from_doc_arrays(docs, DEV)
    assert store.model_view, store.model_view_reason
    hps = bench._HPS(2, doc_max_timesteps=80 if cfg == "cfg5" else 50)
    torch.manual_seed(1)
    embed = torch.nn.Embedding(hps.vocab_size, 300, padding_idx=0)
    embed.weight.requires_grad = False
    model = HiGraph.HSumGraph(hps, embed).to(DEV).train()
    adam = hoptim.Adam([p for p in model.parameters() if p.requires_grad], lr=hps.lr, max_grad_norm=1.0)

    def epoch(view, seed):
        wall, host, bound = [], [], []
        loader = ResidentLoader(store, B, shuffle=True, generator=torch.Generator().manual_seed(seed),
                                drop_last=True, model_view=view)
        torch.cuda.synchronize()
        batches = iter(loader)
        while True:
            t0 = time.perf_counter()                      # the batch's assembly is part of the iteration
            G = next(batches, (None,))[0]
            if G is None:
                break
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
            if view:
                bound.append(G.model_inputs.bound)
        return wall, host, bound

    line(config=cfg, vocab=VOCAB or hps.vocab_size, store_docs=len(store), nbytes_per_doc=round(store.nbytes / len(store)),
         distinct_per_doc=round(float(store.distinct.mean()), 1))
    for cnn in CNN:
        with _lib.path_options(HSG_SENT_LSTM="2", HSG_MODEL_GLUE="1", HSG_WORD_EMBED="1", HSG_SENT_CNN=cnn):
            for view in (False, True):
                epoch(view, 3)
            for rep in range(REPS):
                for view in (False, True):
                    wall, host, bound = epoch(view, 11 + rep)            # both legs see the same batches
                    rec = dict(config=cfg, cnn=cnn, rep=rep, model_view=view, iterations=len(wall), iteration_ms=wall,
                               median_ms=round(statistics.median(wall), 3), min_ms=min(wall), max_ms=max(wall),
                               median_host_ms=round(statistics.median(host), 3))
                    if bound:
                        rec["median_bound"] = int(statistics.median(bound))
                    line(**rec)


for cfg in CONFIGS:
    legs(cfg)
