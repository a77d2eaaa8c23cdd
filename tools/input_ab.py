"""Dev tool (GPU): the input path -- what produces a batch on the device -- today and through
the device-resident document store (hetersumgraph_amd.resident), in one process.

    python tools/input_ab.py [--store N] [--batches K] [--configs cfg2,cfg4,cfg5] [--no-iter]

Per configuration the store holds N (default 256) distinct documents of that shape
(synth.make_batch_docs) and every batch is a fresh random pick of the configuration's batch
size (32).  After a warm-up, three alternations of two legs, K (default 20) batches each:

  (a) today's main-process path: ``graph_collate_fn`` over PREBUILT member graphs, then
      ``G.to(device)``.  Tokenisation, the tf-idf mapping and the host builder
      (``ExampleSet.__getitem__``) are left out, so this understates today's cost.
  (b) ``store.batch(pick)``.

One JSON line per leg and alternation: the synchronised wall time of every batch (ms), and
for (b) also the host's time until ``store.batch`` returns.  Nothing is averaged away: the
per-batch lists are printed, with their median for reading.  ``store.nbytes`` per document and
the store's build time are printed per configuration.

Then (unless --no-iter), at cfg2: a whole eager training iteration with every native path on
(HSG_SENT_LSTM, HSG_MODEL_GLUE, HSG_WORD_EMBED, loss.sentence_loss, optim.Adam with the clip),
fed by a single-process ``DataLoader(collate_fn=graph_collate_fn)`` over prebuilt member graphs
and by ``ResidentLoader``, alternated three times; the wall time of every iteration is listed.
Run it under ``rocprofv3 --kernel-trace --stats`` for the kernel times."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from hetersumgraph_amd import HiGraph, _lib, synth  # noqa: E402
from hetersumgraph_amd import graph as hg  # noqa: E402
from hetersumgraph_amd import loss as hloss  # noqa: E402
from hetersumgraph_amd import optim as hoptim  # noqa: E402
from hetersumgraph_amd.module.dataloader import graph_collate_fn  # noqa: E402
from hetersumgraph_amd.resident import DocumentStore, ResidentLoader  # noqa: E402

ARGS = sys.argv[1:]
opt = lambda name, default: ARGS[ARGS.index(name) + 1] if name in ARGS else default
N_STORE, N_BATCH = int(opt("--store", "256")), int(opt("--batches", "20"))
CONFIGS = opt("--configs", "cfg2,cfg4,cfg5").split(",")
DEV = torch.device("cuda", 0)
WARM, REPS = 3, 3


def ms(t0):
    return round((time.perf_counter() - t0) * 1e3, 3)


def line(**kw):
    print(json.dumps(kw), flush=True)


def batch_legs(cfg):
    B = synth.CONFIGS[cfg][1]
    docs = synth.make_batch_docs(cfg, seed=0, n_docs=N_STORE)
    graphs = [synth.to_graph(d, hg.DGLGraph) for d in docs]
    t0 = time.perf_counter()
    store = DocumentStore.from_doc_arrays(docs, DEV)
    line(config=cfg, store_docs=len(store), store_build_ms=ms(t0), store_nbytes=store.nbytes,
         nbytes_per_doc=round(store.nbytes / len(store)))
    rng = np.random.default_rng(1)
    pick = lambda: rng.choice(N_STORE, size=B, replace=False).tolist()

    def leg_a(p):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G, _ = graph_collate_fn([(graphs[i], i) for i in p])
        G.to(DEV)
        torch.cuda.synchronize()
        return ms(t0), None, G

    def leg_b(p):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G, _ = store.batch(p)
        host = ms(t0)
        torch.cuda.synchronize()
        return ms(t0), host, G

    for fn in (leg_a, leg_b):
        for _ in range(WARM):
            fn(pick())
    for rep in range(REPS):
        for name, fn in (("a_collate_to", leg_a), ("b_store_batch", leg_b)):
            runs = [fn(pick()) for _ in range(N_BATCH)]
            rec = dict(config=cfg, rep=rep, leg=name, batch_ms=[r[0] for r in runs],
                       median_ms=round(statistics.median(r[0] for r in runs), 3))
            if runs[0][1] is not None:
                rec.update(host_ms=[r[1] for r in runs], median_host_ms=round(statistics.median(r[1] for r in runs), 3),
                           work_lists=any(runs[-1][2].resident_work_lists.values()))
            line(**rec)


class Prebuilt(torch.utils.data.Dataset):
    """``ExampleSet.__getitem__`` without the tokeniser and the builder: a prebuilt member graph."""

    def __init__(self, graphs):
        self.graphs = graphs

    def __getitem__(self, i):
        return self.graphs[i], i

    def __len__(self):
        return len(self.graphs)


def iteration_legs(cfg="cfg2"):
    B = synth.CONFIGS[cfg][1]
    docs = synth.make_batch_docs(cfg, seed=0, n_docs=N_STORE)
    graphs = [synth.to_graph(d, hg.DGLGraph) for d in docs]
    store = DocumentStore.from_doc_arrays(docs, DEV)
    hps = bench._HPS(2)
    torch.manual_seed(1)
    embed = torch.nn.Embedding(hps.vocab_size, 300, padding_idx=0)
    embed.weight.requires_grad = True
    model = HiGraph.HSumGraph(hps, embed).to(DEV).train()
    params = [p for p in model.parameters() if p.requires_grad]
    adam = hoptim.Adam(params, lr=hps.lr, max_grad_norm=1.0)

    def epoch(loader, limit):
        out = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, (G, _) in enumerate(loader):
            G.to(DEV)
            logits = model(G)
            loss = hloss.sentence_loss(G, logits)
            adam.zero_grad()
            loss.backward()
            adam.step()
            torch.cuda.synchronize()
            out.append(ms(t0))
            t0 = time.perf_counter()
            if i + 1 == limit:
                break
        return out

    gen = lambda: torch.Generator().manual_seed(7)
    loaders = (("dataloader", lambda: torch.utils.data.DataLoader(Prebuilt(graphs), batch_size=B, shuffle=True,
                                                                  generator=gen(), collate_fn=graph_collate_fn)),
               ("resident", lambda: ResidentLoader(store, B, shuffle=True, generator=gen())))
    with _lib.path_options(HSG_SENT_LSTM="1", HSG_MODEL_GLUE="1", HSG_WORD_EMBED="1"):
        for _, mk in loaders:
            epoch(mk(), WARM)
        for rep in range(REPS):
            for name, mk in loaders:
                runs = epoch(mk(), N_STORE // B)
                line(config=cfg, rep=rep, loader=name, iteration_ms=runs, median_ms=round(statistics.median(runs), 3))


for cfg in CONFIGS:
    batch_legs(cfg)
if "--no-iter" not in ARGS:
    iteration_legs()
