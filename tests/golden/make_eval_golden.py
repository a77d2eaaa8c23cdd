"""Golden outputs of the reference's evaluation-time selection for the native evaluation
step (include/hsg_eval.h): n-gram windows 2, 3 and 4, m in {0, 1, 3, 5}, blocking on and off.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_golden.py --ref <reference checkout>

Like make_tester_golden.py this runs the reference's Tester.py (read-only, at generation
time only) over the test-only DGL-0.4 shim with seeded logits from a stand-in model, and
writes recorded results only: eval_select.json holds, per window, the inputs (texts, logits,
labels, sentence counts) and, per case, the reference SLTester's accumulated state.

The texts are built to contain what n-gram blocking can get wrong: sentences of at most
n_win tokens (no n-gram at all), an n-gram repeated inside one sentence, two sentences that
share only their LAST n-gram (which the reference never uses, so they must not block each
other), tabs, double spaces and U+00A0 between words, a one-sentence document, m > N, and a
document where everything after the first pick is blocked.

The generator asserts that no two scores inside a document are equal, so the reference's
unspecified order among equal scores never enters the fixture.
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
from make_tester_golden import WORDS, _Model, _Set, state  # noqa: E402

N_WINS = (2, 3, 4)
MS = (0, 1, 3, 5)
SHAPES = [(7, 30, 5), (5, 20, 4), (5, 22, 4), (2, 9, 3), (1, 5, 2)]
SEED = 77


def make_texts(rng, w):
    """Article texts of the five documents for window w."""
    tail = lambda lo=w + 2, hi=w + 7: " ".join(WORDS[j] for j in rng.integers(0, len(WORDS), int(rng.integers(lo, hi))))
    common = " ".join(f"end{i}" for i in range(w))                    # the shared LAST n-gram
    rep = " ".join(f"rep{i}" for i in range(w))
    a = [tail(),
         " ".join(f"tiny{i}" for i in range(w)),                       # exactly w tokens: no n-gram
         f"{rep} {rep} {rep} stop here",                               # its own n-grams repeat
         f"left alpha beta gamma {common}",                            # these two share only the last n-gram
         f"right delta kappa omega {common}",
         "the\tcat  sat\u00a0on the   mat\tquietly " + tail(),    # same words as the next one after split()
         "the cat sat on the mat loudly " + tail()]
    b = [f"every one of these starts the same way {i} " + tail() for i in range(5)]   # one survivor
    c = [("the dog ran far away today " + tail()) if i % 3 else tail() for i in range(5)]
    d = ["short", tail()]                                              # one token; m > N for m in {3, 5}
    e = [tail()]                                                       # a one-sentence document
    return [{"sents": s, "abstract": s[0] + " summary"} for s in (a, b, c, d, e)]


def make_case(w):
    """Docs, logits, article texts for window w (deterministic: the tests rebuild them)."""
    rng = np.random.default_rng(SEED + w)
    docs = [synth.make_hsg_doc(rng, N=n, W=wd, k=k, vocab_size=500) for n, wd, k in SHAPES]
    counts = [int((d.ndtype == 1).sum()) for d in docs]
    logits = rng.standard_normal((sum(counts), 2)).astype(np.float32)
    texts = make_texts(rng, w)
    assert [len(t["sents"]) for t in texts] == counts
    o = 0
    for n in counts:                                                   # no ties inside a document
        assert len(set(logits[o:o + n, 1].tolist())) == n and not np.isnan(logits[o:o + n]).any()
        assert (logits[o:o + n, 0] != logits[o:o + n, 1]).all()
        o += n
    return docs, logits, texts


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
                del st["refer"]                                        # the inputs' abstracts, verbatim
                out["cases"].append({"n_win": w, "m": m, "blocking": blocking, "state": st})
    # the property the texts are built for: with blocking, document 1 keeps one sentence only
    for c in out["cases"]:
        if c["blocking"] and c["m"] >= 3:
            assert len(c["state"]["extracts"][1]) == 1, c["state"]["extracts"]
    path = os.path.join(HERE, "eval_select.json")
    with open(path, "w") as f:
        json.dump(out, f)
    assert os.path.getsize(path) < 100 * 1024, os.path.getsize(path)
    print(len(out["cases"]), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
