"""SLTester.evaluation with the native evaluation step on word ids
(``path_options(HSG_EVAL_SELECT="words")``: hsg_doc_ce + hsg_eval_select_words, device
accumulators, pipelined read-back) over DEVICE logits: its accumulated state equals the
reference SLTester's recorded outputs exactly (tests/golden/eval_select.json and
tests/golden/eval_words.json; the running loss to test_gpu_tester.py's 1e-6 relative) and a
switch-off tester's state on the same input -- with the word ids taken from
``evalsel.words_for``'s per-example cache, and with the ids the dataset would attach to the
graph (``G.eval_words``) -- keeps document order over several batches, and drains correctly
when an accessor is read between batches."""
import json
import os

import pytest
import torch

import make_eval_golden as MG
import make_eval_words_golden as MW
from make_tester_golden import _Set, make_case
from test_gpu_eval_tester import _DeviceModel, assert_golden, assert_same_state, graph_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def run(batches, m, blocking, n_win, mode, attach=False, between=None, sets=None):
    """A tester after ``evaluation`` over every (docs, logits, texts) batch in turn.  attach:
    the graphs carry ``eval_words`` as ExampleSet(eval_words=True) graphs do after batching."""
    from hetersumgraph_amd import _lib, evalsel
    from hetersumgraph_amd.HiGraph import sentence_counts
    from hetersumgraph_amd.Tester import SLTester
    t = SLTester(_DeviceModel(*[b[1] for b in batches]), m, limited=True, blocking_win=n_win)
    sets = [_Set(b[2]) for b in batches] if sets is None else sets
    with _lib.path_options(HSG_EVAL_SELECT=mode):
        for (docs, _, texts), data in zip(batches, sets):
            G = graph_of(docs)
            if attach:
                G.eval_words = [evalsel.word_ids(x["sents"], c) for x, c in zip(texts, sentence_counts(G))]
            t.evaluation(G, list(range(len(docs))), data, blocking=blocking)
            if between is not None:
                between(t)
        t.getMetric()
    return t


GOLDENS = {"select": (_load("eval_select.json"), MG), "words": (_load("eval_words.json"), MW)}


@pytest.mark.parametrize("attach", [False, True], ids=["cache", "graph"])
@pytest.mark.parametrize("name,case", [(n, c) for n, (g, _) in GOLDENS.items() for c in g["cases"]],
                         ids=lambda x: x if isinstance(x, str) else f"w{x['n_win']}-m{x['m']}-block{int(x['blocking'])}")
def test_words_step_matches_the_goldens(name, case, attach):
    from hetersumgraph_amd import evalsel
    gold, gen = GOLDENS[name]
    w = case["n_win"]
    batch = gen.make_case(w)
    texts = gold["inputs"][str(w)]["texts"]
    assert batch[2] == texts
    evalsel.clear_word_cache()
    data = _Set(texts)
    t = run([batch], case["m"], case["blocking"], w, "words", attach=attach, sets=[data])
    # the word ids came from where they should: the graph's are used as they are, else one cache entry per example
    used_cache = case["blocking"] and case["m"] != 0 and not attach
    assert len(evalsel._WORD_CACHE) == int(used_cache)
    if used_cache:
        assert sorted(evalsel._WORD_CACHE[data]) == list(range(len(texts)))
    ref = dict(case["state"])
    ref.setdefault("hyps", ["\n".join(x["sents"][i] for i in e) for x, e in zip(texts, ref["extracts"])])
    assert_golden(t, ref, [x["abstract"] for x in texts])
    assert_same_state(t, run([batch], case["m"], case["blocking"], w, "0"))
    evalsel.clear_word_cache()


@pytest.mark.parametrize("attach", [False, True], ids=["cache", "graph"])
@pytest.mark.parametrize("m,blocking", [(3, True), (3, False), (0, False)])
def test_three_batches_keep_document_order(m, blocking, attach):
    batches = [make_case(31), MW.make_case(2), MG.make_case(3), make_case(32)]
    t = run(batches, m, blocking, 2, "words", attach=attach)
    singles = [run([b], m, blocking, 2, "words", attach=attach) for b in batches]
    assert t.extracts == [e for s in singles for e in s.extracts]
    assert t._hyps == [h for s in singles for h in s._hyps]
    assert t.batch_number == 4 and t.example_num == 19
    assert_same_state(t, run(batches, m, blocking, 2, "0"))


def test_a_warm_cache_is_not_rebuilt():
    """A second tester over the same dataset (train.py makes one per epoch) finds the ids
    made by the first: the texts are not split again."""
    from hetersumgraph_amd import evalsel
    evalsel.clear_word_cache()
    batch = MW.make_case(2)
    data = _Set(batch[2])
    a = run([batch], 3, True, 2, "words", sets=[data])
    entries = dict(evalsel._WORD_CACHE[data])
    calls = []
    real = evalsel.word_ids
    evalsel.word_ids = lambda *args: calls.append(args) or real(*args)
    try:
        b = run([batch], 3, True, 5, "words", sets=[data])             # another window: the same ids serve
    finally:
        evalsel.word_ids = real
    assert calls == [] and all(evalsel._WORD_CACHE[data][i][1] is entries[i][1] for i in entries)
    assert a.extracts == run([batch], 3, True, 2, "0").extracts and b.extracts == run([batch], 3, True, 5, "0").extracts
    evalsel.clear_word_cache()


def test_reading_hyps_between_batches_drains():
    batches = [make_case(31), MW.make_case(2), make_case(32)]
    seen = []

    def between(t):
        assert t._pending is not None                      # the batch just issued is still in flight
        seen.append((len(t.hyps), t.rougePairNum, len(t.extractLabel), int(t.pred)))
        assert t._pending is None
    t = run(batches, 3, True, 2, "words", between=between)
    assert [s[:3] for s in seen] == [(5, 5, 5), (9, 9, 9), (14, 14, 14)]
    assert [s[3] for s in seen] == sorted(s[3] for s in seen) and seen[-1][3] == int(t.pred)
    assert_same_state(t, run(batches, 3, True, 2, "0"))


def test_errors_name_the_switch_value():
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.Tester import SLTester
    docs, logits, texts = make_case(31)

    class _Cpu:
        def forward(self, G):
            return torch.from_numpy(logits)
    with _lib.path_options(HSG_EVAL_SELECT="words"):
        with pytest.raises(RuntimeError, match="HSG_EVAL_SELECT=words.*ROCm device"):
            SLTester(_Cpu(), 3).evaluation(graph_of(docs), list(range(len(docs))), _Set(texts))
        # word ids of another batch on the graph: refused on the host, nothing is launched with them
        G = graph_of(docs)
        G.eval_words = [(torch.zeros(2, dtype=torch.int32).numpy(), torch.zeros(0, dtype=torch.int32).numpy())] * len(docs)
        with pytest.raises(RuntimeError, match="different batches"):
            SLTester(_DeviceModel(logits), 3).evaluation(G, list(range(len(docs))), _Set(texts), blocking=True)
    with _lib.path_options(HSG_EVAL_SELECT="1"):
        with pytest.raises(RuntimeError, match="HSG_EVAL_SELECT=1.*ROCm device"):
            SLTester(_Cpu(), 3).evaluation(graph_of(docs), list(range(len(docs))), _Set(texts))
