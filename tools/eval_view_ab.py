"""Dev tool (GPU): what the eval view of a resident batch (include/hsg_resident_eval.h) gives the
evaluation loop fed by ``ResidentLoader``.

    python tools/eval_view_ab.py [--out profiles/r22_eval_view/eval_view_ab.jsonl] [--store 128] [--passes 100]
                                 [--rounds 3] [--paths all|default]

cfg2: a store of ``--store`` documents of 35 sentences (synth.make_batch_docs) with tools/eval_ab.py's
news-like articles, batches of 32.  One HSumGraph in eval mode with random-init weights (train.py's
defaults), m = 3 with trigram blocking on; ``--paths all`` (the default) turns every native path of
the forward on (HSG_SENT_LSTM="1", HSG_MODEL_GLUE, HSG_WORD_EMBED).  Three legs:

  view_off   HSG_EVAL_SELECT="words", ``eval_view=False``: the ids ride on the graph (``G.eval_words``)
             and SLTester packs, pins and uploads them per batch -- the behaviour before the view, the
             yardstick;
  view_on    HSG_EVAL_SELECT="words", ``eval_view=True``: ``G.eval_pack`` from the store;
  text       HSG_EVAL_SELECT="text" over a store built WITHOUT word ids: nothing prepared.

After a warm-up of every leg the legs alternate ``--rounds`` times.  A run is ``--passes`` passes over
the store on a fresh tester, timed with a host clock from the first ``store.batch`` to the end of the
closing ``getMetric()`` followed by a device synchronise: batch assembly included.  Every run is
printed and written as one JSON line -- none is dropped or picked -- then the medians, whether the
view was shorter in every alternation, and whether all legs selected the same sentences.  Run it under
``rocprofv3 --kernel-trace --stats`` for the kernel's own time (k_res_eval)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_ab  # noqa: E402
from hetersumgraph_amd import HiGraph, _lib, evalsel, synth  # noqa: E402
from hetersumgraph_amd.resident import DocumentStore, ResidentLoader  # noqa: E402
from hetersumgraph_amd.Tester import SLTester  # noqa: E402

LEGS = (("view_off", "words", dict(eval_view=False)), ("view_on", "words", dict(eval_view=True)),
        ("text", "text", dict(eval_view=False)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r22_eval_view", "eval_view_ab.jsonl"))
    ap.add_argument("--store", type=int, default=128)
    ap.add_argument("--passes", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=25, help="warm-up passes of every leg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--paths", choices=("all", "default"), default="all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_view_ab.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda", 0)
    B = synth.CONFIGS["cfg2"][1]
    docs = synth.make_batch_docs("cfg2", seed=0, n_docs=args.store)
    counts = [len(d.sent_nodes) for d in docs]
    data = eval_ab.Dataset(eval_ab.make_articles(np.random.default_rng(0), counts))
    words = [[evalsel.word_ids(e.original_article_sents, c)] for e, c in zip(data.examples, counts)]
    stores = {"words": DocumentStore.from_doc_arrays(docs, dev, eval_words=words),
              "text": DocumentStore.from_doc_arrays(docs, dev)}
    assert stores["words"].eval_view, stores["words"].eval_view_reason
    hps = eval_ab.HPS()
    torch.manual_seed(1)
    embed = torch.nn.Embedding(hps.vocab_size, hps.word_emb_dim, padding_idx=0)
    model = HiGraph.HSumGraph(hps, embed).to(dev).eval()
    paths = dict(HSG_SENT_LSTM="1", HSG_MODEL_GLUE="1", HSG_WORD_EMBED="1") if args.paths == "all" else {}

    def run(leg, passes):
        _, mode, kw = LEGS[leg]
        t = SLTester(model, 3, limited=False, blocking_win=3)
        loader = ResidentLoader(stores[mode], B, **kw)
        evalsel.clear_word_cache()
        n = 0
        with torch.no_grad(), _lib.path_options(HSG_EVAL_SELECT=mode, **paths):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                for G, index in loader:
                    t.evaluation(G, index, data, blocking=True)
                    n += 1
            t.getMetric()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return t, dt / n * 1e3, n

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"config": "cfg2", "store_docs": args.store, "docs_per_batch": B, "sentences_per_batch": sum(counts[:B]),
          "words_per_batch": int(stores["words"].words_of[:B].sum()), "paths": paths,
          "eval_view_bytes_per_doc": round(sum(t.numel() * t.element_size()
                                               for t in stores["words"].views["eval_view"].tensors()) / args.store),
          "eval_view_default": DocumentStore.EVAL_VIEW})
    for leg in range(len(LEGS)):
        run(leg, args.warmup)
    ms, testers = {name: [] for name, _, _ in LEGS}, {}
    for rnd in range(args.rounds):
        for leg, (name, mode, kw) in enumerate(LEGS):
            t, per, n = run(leg, args.passes)
            testers[name] = t
            ms[name].append(per)
            emit({"round": rnd, "leg": name, "mode": mode, "batches": n, "ms_per_batch": round(per, 3), **kw})
    emit({"median_ms_per_batch": {k: round(statistics.median(v), 3) for k, v in ms.items()},
          "view_shorter_in_every_alternation": all(a < b for a, b in zip(ms["view_on"], ms["view_off"])),
          "view_minus_off_ms": [round(a - b, 3) for a, b in zip(ms["view_on"], ms["view_off"])]})
    a = testers["view_off"]
    emit({"same_extracts": all(a.extracts == b.extracts for b in testers.values()), "same_counters": all(
        int(getattr(a, k)) == int(getattr(b, k)) for b in testers.values() for k in ("pred", "true", "match", "match_true")),
          "device": torch.cuda.get_device_name(0), "lib": _lib.version()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
