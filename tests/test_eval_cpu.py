"""The selection contract of include/hsg_eval.h on the CPU: its numpy restatement
(tests/eval_ref.py) reproduces the reference SLTester's recorded results -- every
``extracts`` entry and all four counters of tests/golden/tester.json and of
tests/golden/eval_select.json (windows 2, 3, 4; m in {0, 1, 3, 5}; blocking on and off) --
from document-local integer ids and a seen set; ``evalsel.ngram_ids`` / ``pack_batch`` name
the same n-gram classes as the reference's joined strings; and the order rules the
reference leaves open (ties, +-0, NaN) are what the header says.  No GPU needed."""
import json
import os

import numpy as np
import pytest
import torch

import eval_ref as R
import make_eval_golden as MG
import make_tester_golden as MT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def graph_labels(docs):
    """(per-sentence labels int64 [n], sentence counts) of the batched synthetic graph."""
    from hetersumgraph_amd import graph as hg
    from hetersumgraph_amd import synth
    from hetersumgraph_amd.HiGraph import node_ids, sentence_counts
    G = hg.batch([synth.to_graph(d, hg.DGLGraph) for d in docs])
    return G.ndata["label"][node_ids(G, "dtype", 1.0)].sum(-1).numpy(), list(sentence_counts(G))


def ref_state(logits, labels, counts, texts, m, blocking, n_win, ids_from):
    """(extracts, [pred, true, match_true, match]) from the restatement."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    kw = {}
    if blocking:
        if ids_from == "strings":
            per = [R.string_ids(t["sents"][:c], n_win) for t, c in zip(texts, counts)]
            flat = [ids for doc, _ in per for ids in doc]
            kw = dict(gram_ptr=np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int32),
                      gram_ids=np.asarray([g for x in flat for g in x], np.int32),
                      gram_cnt=np.asarray([c for _, c in per], np.int32))
        else:
            from hetersumgraph_amd import evalsel
            pack = evalsel.pack_batch([t["sents"] for t in texts], counts, n_win, pin=False)
            gp, gi, gc = (v.numpy() for v in pack.views())
            kw = dict(gram_ptr=gp, gram_ids=gi, gram_cnt=gc)
        kw["gram_max"] = int(max(kw["gram_cnt"]))
    n_max = max(counts)
    sel, nsel, cnts, tot = R.select_ref(logits, labels, off, m, n_max, n_max, **kw)
    assert (nsel >= 0).all() and (cnts.sum(0) == tot).all()
    return [sel[d, :nsel[d]].tolist() for d in range(len(counts))], tot.tolist()


def check_state(got, ref):
    extracts, tot = got
    assert extracts == ref["extracts"]
    assert tot == [ref["pred"], ref["true"], ref["match_true"], ref["match"]]


def no_ties(logits, counts):
    o = 0
    for n in counts:
        assert len(set(np.asarray(logits, np.float32)[o:o + n, 1].tolist())) == n
        o += n


@pytest.mark.parametrize("ids_from", ["strings", "evalsel"])
@pytest.mark.parametrize("case", _load("tester.json")["cases"],
                         ids=lambda c: f"seed{c['seed']}-m{c['m']}-block{int(c['blocking'])}")
def test_restatement_reproduces_tester_golden(case, ids_from):
    docs, logits, texts = MT.make_case(case["seed"])
    labels, counts = graph_labels(docs)
    no_ties(logits, counts)                    # the reference's tie order never enters this fixture
    check_state(ref_state(logits, labels, counts, texts, case["m"], case["blocking"], 3, ids_from), case["state"])


EVAL = _load("eval_select.json")


def test_eval_golden_covers_the_stated_cases():
    got = sorted((c["n_win"], c["m"], c["blocking"]) for c in EVAL["cases"])
    assert got == sorted((w, m, b) for w in (2, 3, 4) for m in (0, 1, 3, 5) for b in (False, True))
    assert os.path.getsize(os.path.join(GOLDEN, "eval_select.json")) < 100 * 1024
    for w in (2, 3, 4):
        docs, logits, texts = MG.make_case(w)
        inp = EVAL["inputs"][str(w)]
        np.testing.assert_array_equal(logits, np.asarray(inp["logits"], np.float32))
        assert texts == inp["texts"]
        labels, counts = graph_labels(docs)
        assert labels.tolist() == inp["labels"] and counts == inp["counts"]
        no_ties(logits, counts)
        # what the texts are built to contain
        a = texts[0]["sents"]
        grams = R.string_grams(a, w)
        assert grams[1] == [] and len(a[1].split()) == w                           # at most n_win tokens
        assert len(set(grams[2])) < len(grams[2])                                  # a repeat inside one sentence
        assert a[3].split()[-w:] == a[4].split()[-w:] and not set(grams[3]) & set(grams[4])   # only the last one shared
        assert "\t" in a[5] and "  " in a[5] and "\u00a0" in a[5] and set(grams[5]) & set(grams[6])
        assert counts[-1] == 1 and counts[-2] == 2                                 # one sentence; m > N
    for c in EVAL["cases"]:                                                        # all but the first pick blocked
        if c["blocking"] and c["m"] >= 3:
            assert len(c["state"]["extracts"][1]) == 1
        if c["m"] == 5 and not c["blocking"]:
            assert [len(e) for e in c["state"]["extracts"]] == [5, 5, 5, 2, 1]


@pytest.mark.parametrize("ids_from", ["strings", "evalsel"])
@pytest.mark.parametrize("case", EVAL["cases"], ids=lambda c: f"w{c['n_win']}-m{c['m']}-block{int(c['blocking'])}")
def test_restatement_reproduces_eval_golden(case, ids_from):
    inp = EVAL["inputs"][str(case["n_win"])]
    got = ref_state(np.asarray(inp["logits"], np.float32), np.asarray(inp["labels"]), inp["counts"], inp["texts"],
                    case["m"], case["blocking"], case["n_win"], ids_from)
    check_state(got, case["state"])


@pytest.mark.parametrize("w", [1, 2, 3, 4, 6])
def test_ngram_ids_name_the_reference_strings_classes(w):
    from hetersumgraph_amd import evalsel
    docs = [t["sents"] for ww in (2, 3, 4) for t in EVAL["inputs"][str(ww)]["texts"]]
    docs += [t["sents"] for t in _load("tester.json")["cases"][0]["texts"]]
    docs += [[], [""], ["   "], ["a\u2003b\u00a0c d e f a b c", "a b c\nd e f"]]
    for sents in docs:
        ptr, ids, nd = evalsel.ngram_ids(sents, w)
        want, want_nd = R.string_ids(sents, w)
        assert ptr.dtype == np.int32 and ids.dtype == np.int32 and ptr.shape == (len(sents) + 1,)
        got = [ids[ptr[i]:ptr[i + 1]].tolist() for i in range(len(sents))]
        assert nd == want_nd and R.same_partition(got, want)
        assert ids.size == 0 or (ids.min() >= 0 and ids.max() == nd - 1 and len(set(ids.tolist())) == nd)
        # more sentence nodes than article sentences: the extra rows get no ids; fewer: the rest is not looked at
        p2, i2, nd2 = evalsel.ngram_ids(sents, w, len(sents) + 2)
        assert p2.tolist() == ptr.tolist() + [ptr[-1]] * 2 and i2.tolist() == ids.tolist() and nd2 == nd
        if len(sents) > 1:
            p3, i3, nd3 = evalsel.ngram_ids(sents, w, len(sents) - 1)
            w3, wn3 = R.string_ids(sents[:-1], w)
            assert nd3 == wn3 and R.same_partition([i3[p3[i]:p3[i + 1]].tolist() for i in range(len(sents) - 1)], w3)


def test_pack_batch_layout():
    from hetersumgraph_amd import evalsel
    texts = EVAL["inputs"]["3"]["texts"]
    counts = EVAL["inputs"]["3"]["counts"]
    pack = evalsel.pack_batch([t["sents"] for t in texts], counts, 3, pin=False)
    gp, gi, gc = (v.numpy() for v in pack.views())
    assert pack.buf.dtype == torch.int32 and pack.n == sum(counts) and pack.B == len(counts)
    assert gp.shape == (pack.n + 1,) and gc.shape == (pack.B,) and gp[0] == 0 and gp[-1] == pack.T
    assert gi.shape == (max(pack.T, 1),) and pack.gram_max == gc.max()
    o = 0
    for d, (t, c) in enumerate(zip(texts, counts)):
        ptr, ids, nd = evalsel.ngram_ids(t["sents"], 3, c)
        assert (gp[o:o + c + 1] - gp[o]).tolist() == ptr.tolist() and gc[d] == nd
        assert gi[gp[o]:gp[o + c]].tolist() == ids.tolist()
        o += c
    empty = evalsel.pack_batch([["a b"], []], [1, 0], 3, pin=False)       # no ids at all: the ids view is not empty
    assert empty.T == 0 and empty.views()[1].numel() == 1 and empty.gram_max == 0


def test_order_rules():
    f = np.float32
    nan, inf = f("nan"), f("inf")
    assert R.candidate_order([f(1), f(1), f(1)]) == [0, 1, 2]                     # ties: ascending index
    assert R.candidate_order([f(0.5), f(2), f(0.5), f(2), f(-1), f(0.5)]) == [1, 3, 0, 2, 5, 4]
    assert R.candidate_order([f(-0.0), f(0.0), f(-0.0), f(1e-30), f(-1e-30)]) == [3, 0, 1, 2, 4]   # -0.0 == 0.0
    assert R.candidate_order([f(1), nan, inf, nan, -inf]) == [1, 3, 2, 0, 4]       # NaN above everything, NaNs tie
    # where the order is not a tie, it is torch's descending sort (NaN first there too)
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 7, 40):
        x = torch.randn(n, generator=g)
        if n > 2:
            x[1] = float("nan")
            x[2] = float("inf")
        assert R.candidate_order([f(v) for v in x.tolist()]) == x.sort(descending=True, stable=True)[1].tolist()
    p = np.asarray([[0, 1], [0, 3], [0, 2], [0, 3]], np.float32)
    assert R.select_doc(p, 2) == [1, 3] and R.select_doc(p, 9) == [1, 3, 2, 0]
    # blocking: a skipped sentence adds no ids; own repeats do not block; no ids -> never blocked
    p = np.asarray([[0, 5], [0, 4], [0, 3], [0, 2], [0, 1]], np.float32)
    grams = [[0, 0, 1], [1, 2], [2], [], [0]]
    assert R.select_doc(p, 5, grams) == [0, 2, 3]          # 1 is skipped, so its id 2 does not block sentence 2
    assert R.select_doc(p, 2, grams) == [0, 2]


def test_m0_rule_is_torch_argmax():
    vals = [0.0, -0.0, 1.0, -1.0, float("nan"), float("inf"), float("-inf")]
    p = np.asarray([[a, b] for a in vals for b in vals], np.float32)
    want = torch.arange(len(p))[torch.from_numpy(p).max(1)[1] != 0].tolist()
    assert R.select_doc(p, 0) == want
    assert R.counts_doc(want, np.ones(len(p), np.int64)) == [len(want), len(p), len(want), len(want)]
