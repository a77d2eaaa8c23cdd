"""Golden outputs of the reference's evaluation-time selection for the word ids made from
article bytes (include/hsg_eval_text.h): n-gram windows 2 and 3, m in {0, 1, 3, 5}, blocking on
and off, over texts whose words are separated by EVERY whitespace code point of str.split().

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_text_golden.py --ref <reference checkout>

Like make_eval_words_golden.py this runs the reference's Tester.py (read-only, at generation
time only) over the test-only DGL-0.4 shim with seeded logits from a stand-in model, and writes
recorded results only: eval_text.json holds, per window, the inputs (texts, logits, labels,
sentence counts) and, per case, the reference SLTester's accumulated state.  The full
hypotheses are left out to keep the file small: they are the article sentences named by the
recorded ``extracts``; so are the length-limited ones, which here -- a plain space is rare in
these texts -- are nearly as long (the tests cut the hypotheses by TestPipLine.hyps' rule).

Four documents of 6 to 12 sentences of 12 to 40 words from a small vocabulary (40 / 12 words
for windows 2 / 3; a fifth of it non-ASCII).  Between two words stands a run of one or two
separators drawn uniformly from all 29 whitespace code points -- so only about one gap in
twenty is a plain space -- and a third of the sentences begin, a third end with such a run.

The generator asserts that no two scores inside a document are equal, that every one of the
29 code points occurs as a separator, and -- so that the fixture cannot be vacuous -- for each
window: for at least half of the (document, m in {3, 5}) blocking cases the reference's
extracts differ from those of the same walk over pieces split at 0x20 alone; at least one case
ends with fewer than k sentences, at least one with exactly k.
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

N_WINS = (2, 3)
VOCAB = {2: 40, 3: 12}
MS = (0, 1, 3, 5)
SHAPES = [(12, 40, 5), (9, 30, 4), (8, 30, 4), (6, 20, 3)]          # sentence nodes, word nodes, edges per sentence
SEED = 11
SPACES = [chr(c) for c in range(0x3001) if chr(c).isspace()]       # the 29 code points of str.split()
NON_ASCII = ["é", "ß", "Жук", "中文", "あ", "€5", "naïve", "😀"]


def word(j):
    return NON_ASCII[j // 5 % len(NON_ASCII)] if j % 5 == 4 else f"v{j}"


def make_texts(rng, w, counts):
    V = VOCAB[w]

    def run():
        return "".join(SPACES[j] for j in rng.integers(0, len(SPACES), int(rng.integers(1, 3))))
    out = []
    for n in counts:
        sents = []
        for _ in range(n):
            toks = [word(int(j)) for j in rng.integers(0, V, int(rng.integers(12, 41)))]
            s = toks[0] + "".join(run() + t for t in toks[1:])
            u = rng.random(2)
            sents.append((run() if u[0] < 1 / 3 else "") + s + (run() if u[1] < 1 / 3 else ""))
        out.append({"sents": sents, "abstract": " ".join(sents[0].split()[:6]) + " summary"})
    return out


def make_case(w):
    """Docs, logits, article texts for window w (deterministic: the tests rebuild them)."""
    assert len(SPACES) == 29
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


def walk(pieces, order, n_win, k):
    """The reference's walk (Tester.py:155-184) over given pieces."""
    seen, chosen = set(), []
    for i in order:
        grams = [" ".join(pieces[i][t:t + n_win]) for t in range(len(pieces[i]) - n_win)]
        if any(g in seen for g in grams):
            continue
        chosen.append(i)
        seen.update(grams)
        if len(chosen) >= k:
            break
    return chosen


def walk_facts(cases, inputs):
    """Per window, over the (document, m in {3, 5}) blocking cases: how many differ from the walk
    of a splitter that knows only 0x20, ended short of k, ended with exactly k; how many there are."""
    facts = {}
    for c in cases:
        if not (c["blocking"] and c["m"] in (3, 5)):
            continue
        inp = inputs[str(c["n_win"])]
        f = facts.setdefault(c["n_win"], dict(differs=0, short=0, full=0, n=0))
        o = 0
        for n, ext, t in zip(inp["counts"], c["state"]["extracts"], inp["texts"]):
            order = np.argsort(-np.asarray(inp["logits"], np.float32)[o:o + n, 1], kind="stable").tolist()
            k = min(c["m"], n)
            assert ext == walk([s.split() for s in t["sents"]], order, c["n_win"], k)
            naive = walk([[p for p in s.split(" ") if p] for s in t["sents"]], order, c["n_win"], k)
            f["n"] += 1
            f["differs"] += ext != naive
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
        used = {ch for t in texts for s in t["sents"] for ch in s if ch.isspace()}
        assert used == set(SPACES), sorted(set(SPACES) - used)
        assert any(not s.isascii() for t in texts for s in t["sents"])
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
                del st["refer"], st["hyps"], st["hyps_limited"]        # the inputs' abstracts; the extracts' sentences
                out["cases"].append({"n_win": w, "m": m, "blocking": blocking, "state": st})
    facts = walk_facts(out["cases"], out["inputs"])
    for w in N_WINS:
        f = facts[w]
        assert 2 * f["differs"] >= f["n"] and f["short"] >= 1 and f["full"] >= 1, (w, f)
    path = os.path.join(HERE, "eval_text.json")
    with open(path, "w") as f:
        json.dump(out, f)
    assert os.path.getsize(path) < 100 * 1024, os.path.getsize(path)
    print(len(out["cases"]), "cases,", os.path.getsize(path), "bytes,", facts)


if __name__ == "__main__":
    main()
