"""Golden outputs of the reference's evaluation-time selection for the word-id blocking path
(include/hsg_eval_words.h): n-gram windows 1, 2 and 5, m in {0, 1, 3, 5}, blocking on and off.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_words_golden.py --ref <reference checkout>

Like make_eval_golden.py this runs the reference's Tester.py (read-only, at generation time
only) over the test-only DGL-0.4 shim with seeded logits from a stand-in model, and writes
recorded results only: eval_words.json holds, per window, the inputs (texts, logits, labels,
sentence counts) and, per case, the reference SLTester's accumulated state.  The full
hypotheses are left out to keep the file small: they are the article sentences named by the
recorded ``extracts`` (the length-limited ones, cut to the short abstracts, are recorded).

Where eval_select.json holds short hand-built sentences, these are four documents of 6 to 12
sentences of 30 to 90 tokens drawn uniformly from a small vocabulary (3000 / 60 / 5 words for
windows 1 / 2 / 5): many sentences have more than 64 windows (more than one stride of the
wave), two sentences share a window about as often as not, so blocking decides most walks,
and a document's chosen sentences store several hundred windows.

The generator asserts that no two scores inside a document are equal, and -- so that the
fixture cannot be vacuous -- for each window, over the (document, m in {3, 5}) blocking cases:
at least half choose a sentence after having skipped one, at least one ends with fewer than k
sentences, at least one ends with exactly k.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import dgl_shim  # noqa: E402
from hetersumgraph_amd import synth  # noqa: E402
from make_tester_golden import _Model, _Set, state  # noqa: E402

N_WINS = (1, 2, 5)
VOCAB = {1: 3000, 2: 60, 5: 5}
MS = (0, 1, 3, 5)
SHAPES = [(12, 40, 5), (9, 30, 4), (8, 30, 4), (6, 20, 3)]          # sentence nodes, word nodes, edges per sentence
SEED = 5


def make_texts(rng, w, counts):
    V = VOCAB[w]
    out = []
    for n in counts:
        sents = [" ".join(f"v{j}" for j in rng.integers(0, V, int(rng.integers(30, 91)))) for _ in range(n)]
        out.append({"sents": sents, "abstract": " ".join(sents[0].split()[:6]) + " summary"})
    return out


def make_case(w):
    """Docs, logits, article texts for window w (deterministic: the tests rebuild them)."""
    rng = np.random.default_rng(SEED + w)
    docs = [synth.make_hsg_doc(rng, N=n, W=wd, k=k, vocab_size=500) for n, wd, k in SHAPES]
    counts = [int((d.ndtype == 1).sum()) for d in docs]
    logits = rng.standard_normal((sum(counts), 2)).astype(np.float32)
    texts = make_texts(rng, w, counts)
    o = 0
    for n in counts:                                                   # no ties inside a document
        assert len(set(logits[o:o + n, 1].tolist())) == n and not np.isnan(logits[o:o + n]).any()
        assert (logits[o:o + n, 0] != logits[o:o + n, 1]).all()
        o += n
    return docs, logits, texts


def walk_facts(cases, inputs):
    """Per window, over the (document, m in {3, 5}) blocking cases: how many chose a sentence
    after having skipped one, ended short of k, ended with exactly k; and how many there are."""
    facts = {}
    for c in cases:
        if not (c["blocking"] and c["m"] in (3, 5)):
            continue
        inp = inputs[str(c["n_win"])]
        f = facts.setdefault(c["n_win"], dict(skipped=0, short=0, full=0, n=0))
        o = 0
        for n, ext in zip(inp["counts"], c["state"]["extracts"]):
            order = np.argsort(-np.asarray(inp["logits"], np.float32)[o:o + n, 1], kind="stable").tolist()
            k = min(c["m"], n)
            f["n"] += 1
            f["skipped"] += ext != order[:len(ext)]
            f["short"] += len(ext) < k
            f["full"] += len(ext) == k
            o += n
    return facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    shim = types.ModuleType("dgl")
    for k in ("DGLGraph", "batch", "unbatch", "sum_nodes", "init"):
        setattr(shim, k, getattr(dgl_shim, k))
    sys.modules["dgl"] = shim
    sys.modules["rouge"] = types.ModuleType("rouge")
    sys.modules["rouge"].Rouge = None
    import Tester  # noqa: E402  (reference)

    out = {"inputs": {}, "cases": []}
    for w in N_WINS:
        docs, logits, texts = make_case(w)
        G = dgl_shim.batch([synth.to_graph(d, dgl_shim.DGLGraph) for d in docs])
        snode = G.filter_nodes(lambda nodes: nodes.data["dtype"] == 1)
        labels = G.ndata["label"][snode].sum(-1).tolist()
        out["inputs"][str(w)] = {"logits": logits.tolist(), "texts": texts, "labels": labels,
                                 "counts": [len(t["sents"]) for t in texts]}
        for m in MS:
            for blocking in (False, True):
                G = dgl_shim.batch([synth.to_graph(d, dgl_shim.DGLGraph) for d in docs])
                t = Tester.SLTester(_Model(logits), m, limited=True, blocking_win=w)
                t.evaluation(G, list(range(len(docs))), _Set(texts), blocking=blocking)
                t.getMetric()
                st = state(t)
                del st["refer"], st["hyps"]                            # the inputs' abstracts; the extracts' sentences
                out["cases"].append({"n_win": w, "m": m, "blocking": blocking, "state": st})
    facts = walk_facts(out["cases"], out["inputs"])
    for w in N_WINS:
        f = facts[w]
        assert 2 * f["skipped"] >= f["n"] and f["short"] >= 1 and f["full"] >= 1, (w, f)
    path = os.path.join(HERE, "eval_words.json")
    with open(path, "w") as f:
        json.dump(out, f)
    assert os.path.getsize(path) < 100 * 1024, os.path.getsize(path)
    print(len(out["cases"]), "cases,", os.path.getsize(path), "bytes,", facts)


if __name__ == "__main__":
    main()
