"""The word-id blocking path on the CPU (include/hsg_eval_words.h, evalsel.word_ids and
friends, ExampleSet(eval_words=True)): the plain-Python restatement (tests/eval_words_ref.py)
reproduces the reference SLTester's recorded ``extracts`` of every blocking case of
tests/golden/eval_select.json and tests/golden/eval_words.json from word ids alone; the host
side builds the operands the header documents; the per-example cache and the dataset keyword
behave as INTEGRATION.md says.  No GPU needed."""
import gc
import json
import os
import pickle

import numpy as np
import pytest
import torch

import eval_words_ref as W
import make_eval_words_golden as MW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


EVAL = _load("eval_select.json")
WORDS = _load("eval_words.json")
BLOCKING = [(name, c) for name, g in (("select", EVAL), ("words", WORDS)) for c in g["cases"] if c["blocking"]]


@pytest.mark.parametrize("name,case", BLOCKING, ids=lambda x: x if isinstance(x, str) else f"w{x['n_win']}-m{x['m']}")
def test_restatement_reproduces_the_recorded_extracts(name, case):
    inp = (EVAL if name == "select" else WORDS)["inputs"][str(case["n_win"])]
    logits = np.asarray(inp["logits"], np.float32)
    got, o = [], 0
    for t, c in zip(inp["texts"], inp["counts"]):
        got.append(W.select_doc_words(logits[o:o + c], case["m"], W.split_ids(t["sents"][:c]), case["n_win"]))
        o += c
    assert got == case["state"]["extracts"]


def test_words_golden_covers_the_stated_cases():
    got = sorted((c["n_win"], c["m"], c["blocking"]) for c in WORDS["cases"])
    assert got == sorted((w, m, b) for w in (1, 2, 5) for m in (0, 1, 3, 5) for b in (False, True))
    assert os.path.getsize(os.path.join(GOLDEN, "eval_words.json")) < 100 * 1024
    for w in (1, 2, 5):
        docs, logits, texts = MW.make_case(w)
        inp = WORDS["inputs"][str(w)]
        np.testing.assert_array_equal(logits, np.asarray(inp["logits"], np.float32))
        assert texts == inp["texts"] and len(texts) == 4
        lens = [len(s.split()) for t in texts for s in t["sents"]]
        assert all(6 <= c <= 12 for c in inp["counts"]) and min(lens) >= 30 and max(lens) <= 90
        assert sum(n - w > 64 for n in lens) >= 4                      # more windows than one stride of the wave
        o = 0
        for n in inp["counts"]:                                        # no ties inside a document
            assert len(set(logits[o:o + n, 1].tolist())) == n
            o += n
    # what the generator asserted, from the recorded results alone
    for w, f in MW.walk_facts(WORDS["cases"], WORDS["inputs"]).items():
        assert f["n"] == 8 and 2 * f["skipped"] >= f["n"] and f["short"] >= 1 and f["full"] >= 1, (w, f)


def test_refusal_rule_counts_windows_with_repeats():
    p = np.asarray([[0, 5], [0, 4], [0, 3]], np.float32)
    sents = [[7] * 40, [7] * 5, list(range(100, 130))]                # 37 equal windows | blocked | 27 windows
    assert W.select_doc_words(p, 3, sents, 3, 64) == [0, 2]           # 37 + 27 = 64: accepted
    assert W.select_doc_words(p, 3, sents, 3, 63) is None             # the third sentence would make 64 > 63
    assert W.select_doc_words(p, 1, sents, 3, 37) == [0]              # never reached: not refused
    assert W.select_doc_words(p, 3, [[7] * 40, [7] * 5, [1, 2, 3]], 3, 37) == [0, 2]   # a sentence without windows
    assert W.windows([1, 2, 3, 4], 3) == [(1, 2, 3)] and W.windows([1, 2, 3], 3) == [] and W.windows([], 1) == []


# ---- evalsel.word_ids / pack_words ------------------------------------------------------------

DOCS = [t["sents"] for w in ("2", "3", "4") for t in EVAL["inputs"][w]["texts"]] + \
       [[], [""], ["   "], ["a b c d e f a b c", "a\tb  c\nd e f", "A a"]]


def test_word_ids_equal_id_iff_equal_piece():
    from hetersumgraph_amd import evalsel
    for sents in DOCS:
        ptr, ids = evalsel.word_ids(sents)
        assert ptr.dtype == np.int32 and ids.dtype == np.int32 and ptr.shape == (len(sents) + 1,)
        pieces = [p for s in sents for p in s.split()]                 # tabs, double spaces, U+00A0: str.split's rule
        assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(s.split()) for s in sents])]).tolist()
        assert len(ids) == len(pieces)
        for a in range(len(pieces)):
            for b in range(a + 1, min(a + 40, len(pieces))):
                assert (ids[a] == ids[b]) == (pieces[a] == pieces[b])
        assert len(set(ids.tolist())) == len(set(pieces))
        # first-appearance order, as the restatement's own dict
        assert [ids[ptr[i]:ptr[i + 1]].tolist() for i in range(len(sents))] == W.split_ids(sents)
        # more sentence nodes than article sentences: the extra rows are empty; fewer: the rest is not looked at
        p2, i2 = evalsel.word_ids(sents, len(sents) + 2)
        assert p2.tolist() == ptr.tolist() + [ptr[-1]] * 2 and i2.tolist() == ids.tolist()
        if len(sents) > 1:
            p3, i3 = evalsel.word_ids(sents, len(sents) - 1)
            assert p3.tolist() == ptr[:-1].tolist() and i3.tolist() == ids[:ptr[-2]].tolist()
            assert [i3[p3[i]:p3[i + 1]].tolist() for i in range(len(sents) - 1)] == W.split_ids(sents[:-1])
    ptr, ids = evalsel.word_ids(["the\tcat  sat on", "the cat sat on"])
    assert ids[:4].tolist() == ids[4:].tolist() == [0, 1, 2, 3]


def test_pack_words_layout_and_tab_cap():
    from hetersumgraph_amd import evalsel
    texts, counts = WORDS["inputs"]["2"]["texts"], WORDS["inputs"]["2"]["counts"]
    counts = [counts[0] + 1, counts[1] - 2] + counts[2:]              # one row beyond the article, two cut off
    parts = [evalsel.word_ids(t["sents"], c) for t, c in zip(texts, counts)]
    pack = evalsel.pack_words(parts, counts, pin=False)
    wp, wi = (v.numpy() for v in pack.views())
    n = sum(counts)
    assert pack.buf.dtype == torch.int32 and pack.buf.dim() == 1 and pack.n == n and pack.B == len(counts)
    assert wp.shape == (n + 1,) and wp[0] == 0 and wp[-1] == pack.W and wi.shape == (pack.W,)
    assert pack.buf.numel() == n + 1 + pack.W
    o = 0
    for (p, ids), c in zip(parts, counts):
        assert (wp[o:o + c + 1] - wp[o]).tolist() == p.tolist() and wi[wp[o]:wp[o + c]].tolist() == ids.tolist()
        o += c
    # tab_cap: max(64, next_pow2(2 * win_need)), win_need the largest sum of the min(m, N_d) largest window counts
    lens = np.diff(wp)
    for n_win in (1, 2, 5, 8):
        for m in (0, 1, 3, 5, 100):
            need, o = 0, 0
            for c in counts:
                win = sorted(max(int(x) - n_win, 0) for x in lens[o:o + c])
                need = max(need, sum(win[len(win) - min(m, c):]) if m else 0)
                o += c
            cap = 64
            while cap < 2 * need:
                cap *= 2
            assert pack.win_need(n_win, m) == need and pack.tab_cap(n_win, m) == cap, (n_win, m)
    assert pack.tab_cap(2, 3) >= 512 and pack.tab_cap(2, 0) == 64
    same = pack.to(torch.device("cpu"))
    assert same.tab_cap(2, 3) == pack.tab_cap(2, 3) and torch.equal(same.buf, pack.buf)
    empty = evalsel.pack_words([evalsel.word_ids([], 1), evalsel.word_ids([], 0)], [1, 0], pin=False)
    assert empty.W == 0 and empty.views()[1].numel() == 1 and empty.views()[0].tolist() == [0, 0]
    assert empty.tab_cap(3, 3) == 64
    for w, want in ((31, 64), (32, 64), (33, 128), (4096, 8192), (4097, 16384)):
        one = evalsel.pack_words([(np.asarray([0, w + 1], np.int32), np.zeros(w + 1, np.int32))], [1], pin=False)
        assert one.win_need(1, 3) == w and one.tab_cap(1, 3) == want
    with pytest.raises(RuntimeError, match="different batches"):
        evalsel.pack_words(parts, counts[::-1], pin=False)


def test_select_words_refuses_cpu_tensors():
    from hetersumgraph_amd import evalsel
    logits, labels = torch.zeros(3, 2), torch.zeros(3, dtype=torch.int64)
    off, totals = torch.tensor([0, 3], dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        evalsel.select_words(logits, labels, off, 3, 3, 3, totals)
    with pytest.raises(RuntimeError, match="ROCm device"):
        evalsel.select_words(logits.double(), labels, off, 3, 3, 3, totals)


# ---- the per-example cache -----------------------------------------------------------------------

class _Data:
    pass


def test_word_cache():
    from hetersumgraph_amd import evalsel
    evalsel.clear_word_cache()
    ds, other = _Data(), _Data()
    sents = ["a b c d", "b c d e f", "a a"]
    a = evalsel.words_for(ds, 4, sents, 3)
    assert a[0].tolist() == [0, 4, 9, 11] and a[1].tolist() == [0, 1, 2, 3, 1, 2, 3, 4, 5, 0, 0]
    b = evalsel.words_for(ds, 4, ["never looked at"], 3)               # a hit: the same arrays, the texts not read
    assert b[0] is a[0] and b[1] is a[1]
    cut = evalsel.words_for(ds, 4, sents, 2)                           # the entry holds the whole article
    assert cut[0].tolist() == [0, 4, 9] and cut[1].tolist() == a[1][:9].tolist() and np.shares_memory(cut[1], a[1])
    more = evalsel.words_for(ds, 4, sents, 5)
    assert more[0].tolist() == [0, 4, 9, 11, 11, 11] and more[1] is a[1]
    assert evalsel.words_for(ds, 4, sents, 3)[0] is a[0]               # cutting left the entry alone
    assert evalsel.words_for(ds, 5, ["x y"], 1)[1].tolist() == [0, 1]  # another example
    assert evalsel.words_for(other, 4, ["x y z"], 1)[1].tolist() == [0, 1, 2]   # another dataset
    assert len(evalsel._WORD_CACHE) == 2 and sorted(evalsel._WORD_CACHE[ds]) == [4, 5]
    del other
    gc.collect()
    assert len(evalsel._WORD_CACHE) == 1                               # the entry goes with its dataset
    evalsel.clear_word_cache()
    assert len(evalsel._WORD_CACHE) == 0
    c = evalsel.words_for(ds, 4, ["p q"], 1)
    assert c[1].tolist() == [0, 1]                                     # rebuilt from the texts given now
    assert evalsel.words_for([1, 2], 0, ["p q p"], 1)[1].tolist() == [0, 1, 0]   # not weakly referenceable: uncached
    evalsel.clear_word_cache()


# ---- dataset and graph ------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def host_lib():
    from hetersumgraph_amd import build
    build.build_host(verbose=False)


def _dataset(tmp_path, kind, seed, **kw):
    from graph_data import STOPWORDS, make_files
    from hetersumgraph_amd.module.dataloader import ExampleSet, MultiExampleSet
    d = str(tmp_path / f"{kind}{seed}")
    vocab = make_files(d, seed=seed, n_examples=6, multi=kind == "hdsg")
    args = [os.path.join(d, "data.jsonl"), vocab, 7, 12, os.path.join(d, "filter_word.txt"), os.path.join(d, "w2s.jsonl")]
    if kind == "hdsg":
        return MultiExampleSet(*args, os.path.join(d, "w2d.jsonl"), stopwords=STOPWORDS, **kw)
    return ExampleSet(*args, stopwords=STOPWORDS, **kw)


def _same_graph(a, b):
    assert a.number_of_nodes() == b.number_of_nodes() and a.number_of_edges() == b.number_of_edges()
    for k in a.ndata.keys():
        assert torch.equal(a.ndata[k], b.ndata[k]), k
    for k in a.edata.keys():
        assert torch.equal(a.edata[k], b.edata[k]), k
    assert all(torch.equal(x, y) for x, y in zip(a.all_edges(), b.all_edges()))


@pytest.mark.parametrize("kind,seed", [("hsg", 7), ("hdsg", 11)])
def test_dataset_keyword_attaches_word_ids(tmp_path, kind, seed):
    from hetersumgraph_amd import evalsel
    from hetersumgraph_amd import graph as hg
    from hetersumgraph_amd.HiGraph import sentence_counts
    from hetersumgraph_amd.module.dataloader import graph_collate_fn
    ds, plain = _dataset(tmp_path, kind, seed, eval_words=True), _dataset(tmp_path, kind, seed)
    samples, cut = [], 0
    for i in range(len(ds)):
        G, idx = ds[i]
        P, _ = plain[i]
        assert idx == i and not hasattr(P, "eval_words")              # without the keyword: today's graph
        _same_graph(G, P)
        assert {k for k in vars(G) if k not in vars(P)} == {"eval_words"}
        rows = list(sentence_counts(G))[0]
        sents = ds.get_example(i).original_article_sents
        cut += rows < len(sents)
        (ptr, ids), = G.eval_words
        want = evalsel.word_ids(sents, rows)
        assert ptr.dtype == np.int32 and ids.dtype == np.int32 and len(ptr) == rows + 1
        assert ptr.tolist() == want[0].tolist() and ids.tolist() == want[1].tolist()
        G2 = pickle.loads(pickle.dumps(G))                             # as from a DataLoader worker
        assert G2.eval_words[0][0].tolist() == ptr.tolist() and G2.eval_words[0][1].tolist() == ids.tolist()
        samples.append((G2, idx))
    assert cut >= 1                                                    # an article longer than doc_max_timesteps
    # graph_collate_fn reorders by sentence count: the list follows the members
    bg, index = graph_collate_fn(samples[::-1])
    counts = list(sentence_counts(bg))
    assert counts == sorted(counts, reverse=True) and len(set(counts)) > 1 and len(bg.eval_words) == len(index)
    for j, i in enumerate(index):
        want = evalsel.word_ids(ds.get_example(i).original_article_sents, counts[j])
        assert bg.eval_words[j][0].tolist() == want[0].tolist() and bg.eval_words[j][1].tolist() == want[1].tolist()
    evalsel.pack_words(bg.eval_words, counts, pin=False)               # the operands of exactly this batch
    # mixed members: no attribute; no keyword: no attribute
    assert not hasattr(hg.batch([samples[0][0], plain[1][0]]), "eval_words")
    assert not hasattr(graph_collate_fn([plain[0], plain[1]])[0], "eval_words")
