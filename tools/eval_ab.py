"""A/B of the evaluation loop (GPU): SLTester.evaluation as it is by default (leg 0) against
the native evaluation step, ``path_options(HSG_EVAL_SELECT="1")`` (leg 1), and against the
native step on word ids, ``path_options(HSG_EVAL_SELECT="words")``, in the three states its
host side can be in: nothing prepared, the per-example cache cleared before every batch so
that every batch splits and interns its texts (leg 2); the ids attached to the graph, as
``ExampleSet(eval_words=True)`` attaches them in the DataLoader workers (leg 3); the
per-example cache warm, filled before the clock starts (leg 4).  Leg 5 is the native step with
the word ids made on the device from the sentences' bytes,
``path_options(HSG_EVAL_SELECT="text")``, with nothing prepared and the cache cleared before
every batch, as leg 2.  Leg 0 is the yardstick.

    python tools/eval_ab.py [--out profiles/r14_eval_text/eval_ab.jsonl] [--batches 20] [--rounds 3]

One process, one device.  A cfg2-shaped batch (32 documents of 35 sentences), the real
HSumGraph forward in eval mode with random-init weights, synthetic article texts, m = 3 with
n-gram blocking on.  After a warm-up of both legs the legs alternate ``--rounds`` times;
each run is ``--batches`` evaluation calls on a fresh tester and is timed with a host clock
from the first call to the end of the closing ``getMetric()`` (which, on leg 1, is the final
``sync()``) followed by a device synchronise.  Every run is printed and written as one JSON
line -- none is dropped or picked -- followed by lines with the host cost of the operand
packing alone (n-gram ids; word ids made from the texts; word ids already made; the texts'
bytes) and one that states whether all legs selected the same sentences.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hetersumgraph_amd import HiGraph, _lib, evalsel, synth  # noqa: E402
from hetersumgraph_amd import graph as hg  # noqa: E402
from hetersumgraph_amd.Tester import SLTester  # noqa: E402


class HPS:
    """train.py's argparse defaults (train.py:279-309)."""

    def __init__(self):
        self.__dict__.update(dict(
            vocab_size=50000, n_iter=1, word_emb_dim=300, embed_train=False, feat_embed_size=50,
            lstm_hidden_state=128, lstm_layers=2, bidirectional=True, n_feature_size=128, hidden_size=64,
            ffn_inner_hidden_size=512, n_head=8, recurrent_dropout_prob=0.1, atten_dropout_prob=0.1,
            ffn_dropout_prob=0.1, sent_max_len=100, doc_max_timesteps=50, lr=0.0005, cuda=True))


class Example:
    def __init__(self, sents):
        self.original_article_sents = sents
        self.original_abstract = " ".join(sents[:2])


class Dataset:
    def __init__(self, articles):
        self.examples = [Example(s) for s in articles]

    def get_example(self, i):
        return self.examples[i]


def make_articles(rng, counts, vocab=3000, phrases=40):
    """News-like articles: sentences of 12 to 35 words over a Zipf-ish vocabulary, with stock
    phrases of 4 words that recur inside an article (what trigram blocking acts on)."""
    words = [f"w{i}" for i in range(vocab)]
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    out = []
    for n in counts:
        stock = [" ".join(words[j] for j in rng.choice(vocab, 4, p=p)) for _ in range(phrases)]
        sents = []
        for _ in range(n):
            toks = [words[j] for j in rng.choice(vocab, int(rng.integers(12, 36)), p=p)]
            if rng.random() < 0.4:
                toks.insert(int(rng.integers(0, len(toks))), stock[int(rng.integers(0, phrases))])
            sents.append(" ".join(toks))
        out.append(sents)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r14_eval_text", "eval_ab.jsonl"))
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_ab.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda", 0)
    docs = synth.make_batch_docs("cfg2", seed=0)
    G = hg.batch([synth.to_graph(d, hg.DGLGraph) for d in docs])
    G.to(dev)
    counts = list(HiGraph.sentence_counts(G))
    rng = np.random.default_rng(0)
    data = Dataset(make_articles(rng, counts))
    index = list(range(len(counts)))
    hps = HPS()
    torch.manual_seed(1)
    embed = torch.nn.Embedding(hps.vocab_size, hps.word_emb_dim, padding_idx=0)
    model = HiGraph.HSumGraph(hps, embed).to(dev).eval()

    sents = [e.original_article_sents for e in data.examples]
    attached = [evalsel.word_ids(s, c) for s, c in zip(sents, counts)]
    LEGS = {0: ("0", "default"), 1: ("1", "HSG_EVAL_SELECT=1"),
            2: ("words", "HSG_EVAL_SELECT=words, nothing prepared (cache cleared before every batch)"),
            3: ("words", "HSG_EVAL_SELECT=words, G.eval_words attached"),
            4: ("words", "HSG_EVAL_SELECT=words, warm per-example cache"),
            5: ("text", "HSG_EVAL_SELECT=text, nothing prepared (cache cleared before every batch)")}

    def run(leg, batches):
        t = SLTester(model, 3, limited=False, blocking_win=3)
        if leg == 3:
            G.eval_words = attached
        elif hasattr(G, "eval_words"):
            del G.eval_words
        evalsel.clear_word_cache()
        if leg == 4:                                       # warm: filled before the clock starts
            for j, c in zip(index, counts):
                evalsel.words_for(data, j, data.get_example(j).original_article_sents, c)
        with torch.no_grad(), _lib.path_options(HSG_EVAL_SELECT=LEGS[leg][0]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(batches):
                if leg in (2, 5):
                    evalsel.clear_word_cache()
                t.evaluation(G, index, data, blocking=True)
            t.getMetric()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return t, dt

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for leg in LEGS:
        run(leg, args.warmup)
    testers = {}
    for rnd in range(args.rounds):
        for leg in LEGS:
            t, dt = run(leg, args.batches)
            testers[leg] = t
            emit({"round": rnd, "leg": leg, "path": LEGS[leg][1],
                  "batches": args.batches, "docs_per_batch": len(counts), "sentences_per_batch": sum(counts),
                  "ms_per_batch": round(dt / args.batches * 1e3, 3)})
    t0 = time.perf_counter()
    for _ in range(args.batches):
        pack = evalsel.pack_batch(sents, counts, 3)
    emit({"host_only": "evalsel.pack_batch", "ms_per_batch": round((time.perf_counter() - t0) / args.batches * 1e3, 3),
          "ngram_ids_per_batch": pack.T, "gram_max": pack.gram_max})
    t0 = time.perf_counter()
    for _ in range(args.batches):
        words = evalsel.pack_words([evalsel.word_ids(s, c) for s, c in zip(sents, counts)], counts)
    emit({"host_only": "evalsel.word_ids + pack_words", "words_per_batch": words.W, "tab_cap": words.tab_cap(3, 3),
          "ms_per_batch": round((time.perf_counter() - t0) / args.batches * 1e3, 3)})
    t0 = time.perf_counter()
    for _ in range(args.batches):
        words = evalsel.pack_words(attached, counts)
        words.tab_cap(3, 3)
    emit({"host_only": "evalsel.pack_words + tab_cap (ids already made)",
          "ms_per_batch": round((time.perf_counter() - t0) / args.batches * 1e3, 3)})
    t0 = time.perf_counter()
    for _ in range(args.batches):
        text = evalsel.pack_text(sents, counts)
        text.tab_cap(3, 3)
    emit({"host_only": "evalsel.pack_text + tab_cap", "bytes_per_batch": text.nbytes, "tab_cap": text.tab_cap(3, 3),
          "word_bound": int(text.word_bound().sum()),
          "ms_per_batch": round((time.perf_counter() - t0) / args.batches * 1e3, 3)})
    a = testers[0]
    emit({"same_extracts": all(a.extracts == b.extracts for b in testers.values()), "same_counters": all(
        int(getattr(a, k)) == int(getattr(b, k)) for b in testers.values() for k in ("pred", "true", "match", "match_true")),
          "running_loss": [float(b.running_loss) for b in testers.values()],
          "device": torch.cuda.get_device_name(0), "lib": _lib.version()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
