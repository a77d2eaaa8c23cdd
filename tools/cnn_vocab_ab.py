"""Dev tool (GPU): what the sentence CNN's vocabulary path (path_options(HSG_SENT_CNN_VOCAB="1"),
include/hsg_cnn_vocab.h) gives the evaluation loop fed by ``ResidentLoader``.

    python tools/cnn_vocab_ab.py [--out profiles/r23_cnn_vocab/cnn_vocab_ab.jsonl] [--store 128] [--passes 100]
                                 [--rounds 3]

The set-up is tools/eval_view_ab.py's: cfg2, a store of ``--store`` documents of 35 sentences
(synth.make_batch_docs) with tools/eval_ab.py's news-like articles, batches of 32; one HSumGraph in
eval mode with random-init weights (train.py's defaults, vocab_size = 50000, the word embedding
frozen), m = 3 with trigram blocking on; HSG_EVAL_SELECT="words" with the eval view, HSG_SENT_LSTM="1",
HSG_MODEL_GLUE and HSG_WORD_EMBED on, under torch.no_grad().  Three legs:

  cnn_0       HSG_SENT_CNN="0": gather, GEMM over every row, pool -- the yardstick;
  cnn_tokens  HSG_SENT_CNN="tokens": the GEMM over the batch's distinct tokens;
  cnn_vocab   HSG_SENT_CNN_VOCAB="1": one gather launch on the vocabulary product table, which the
              first batch after model.eval() builds (its bytes and build time are reported).

After a warm-up of every leg the legs alternate ``--rounds`` times.  A run is ``--passes`` passes over
the store on a fresh tester, timed with a host clock from the first ``store.batch`` to the end of the
closing ``getMetric()`` followed by a device synchronise.  Every run is printed and written as one JSON
line -- none is dropped or picked -- then the medians, whether the vocabulary path was shorter in
every alternation, and whether the legs selected the same sentences (reported, not required: the
paths round differently).  Run it under ``rocprofv3 --kernel-trace --stats`` for the kernels' own time."""
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

LEGS = (("cnn_0", dict(HSG_SENT_CNN="0")), ("cnn_tokens", dict(HSG_SENT_CNN="tokens")),
        ("cnn_vocab", dict(HSG_SENT_CNN_VOCAB="1")))
PATHS = dict(HSG_EVAL_SELECT="words", HSG_SENT_LSTM="1", HSG_MODEL_GLUE="1", HSG_WORD_EMBED="1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r23_cnn_vocab", "cnn_vocab_ab.jsonl"))
    ap.add_argument("--store", type=int, default=128)
    ap.add_argument("--passes", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=25, help="warm-up passes of every leg")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cnn_vocab_ab.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda", 0)
    B = synth.CONFIGS["cfg2"][1]
    docs = synth.make_batch_docs("cfg2", seed=0, n_docs=args.store)
    counts = [len(d.sent_nodes) for d in docs]
    data = eval_ab.Dataset(eval_ab.make_articles(np.random.default_rng(0), counts))
    words = [[evalsel.word_ids(e.original_article_sents, c)] for e, c in zip(data.examples, counts)]
    store = DocumentStore.from_doc_arrays(docs, dev, eval_words=words)
    assert store.eval_view, store.eval_view_reason
    hps = eval_ab.HPS()
    torch.manual_seed(1)
    embed = torch.nn.Embedding(hps.vocab_size, hps.word_emb_dim, padding_idx=0)
    embed.weight.requires_grad_(False)                       # train.py's default: embed_train = False
    model = HiGraph.HSumGraph(hps, embed).to(dev).eval()
    table = model.ngram_enc._vocab_table

    def run(leg, passes):
        _, switch = LEGS[leg]
        t = SLTester(model, 3, limited=False, blocking_win=3)
        loader = ResidentLoader(store, B, eval_view=True)
        evalsel.clear_word_cache()
        n = 0
        with torch.no_grad(), _lib.path_options(**PATHS, **switch):
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

    # the table on its own: built once per evaluation pass (model.eval() drops it)
    enc = model.ngram_enc
    build_ms = []
    with torch.no_grad():
        for _ in range(3):
            enc.drop_vocab_table()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table.get(*enc._vocab_args()[:3])
            torch.cuda.synchronize()
            build_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    emit({"config": "cfg2", "store_docs": args.store, "docs_per_batch": B, "sentences_per_batch": sum(counts[:B]),
          "vocab_size": hps.vocab_size, "paths": PATHS, "table_bytes": table.nbytes(), "table_build_ms": build_ms,
          "table_budget_mb": _lib.path_option("HSG_SENT_CNN_VOCAB_MB", "1024")})
    for leg in range(len(LEGS)):
        run(leg, args.warmup)
    ms, testers = {name: [] for name, _ in LEGS}, {}
    for rnd in range(args.rounds):
        for leg, (name, switch) in enumerate(LEGS):
            builds = table.builds
            t, per, n = run(leg, args.passes)
            testers[name] = t
            ms[name].append(per)
            emit({"round": rnd, "leg": name, "batches": n, "ms_per_batch": round(per, 3), "table_builds": table.builds - builds,
                  **switch})
    emit({"median_ms_per_batch": {k: round(statistics.median(v), 3) for k, v in ms.items()},
          "vocab_shorter_than_cnn_0_in_every_alternation": all(a < b for a, b in zip(ms["cnn_vocab"], ms["cnn_0"])),
          "vocab_shorter_than_tokens_in_every_alternation": all(a < b for a, b in zip(ms["cnn_vocab"], ms["cnn_tokens"])),
          "vocab_minus_cnn_0_ms": [round(a - b, 3) for a, b in zip(ms["cnn_vocab"], ms["cnn_0"])],
          "vocab_minus_tokens_ms": [round(a - b, 3) for a, b in zip(ms["cnn_vocab"], ms["cnn_tokens"])]})
    a = testers["cnn_0"]
    emit({"same_extracts": {k: a.extracts == b.extracts for k, b in testers.items()},
          "same_counters": {k: all(int(getattr(a, c)) == int(getattr(b, c)) for c in ("pred", "true", "match", "match_true"))
                            for k, b in testers.items()},
          "device": torch.cuda.get_device_name(0), "lib": _lib.version()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
