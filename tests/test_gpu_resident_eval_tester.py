"""SLTester.evaluation over resident batches that carry the eval view (``G.eval_pack``,
include/hsg_resident_eval.h) with ``path_options(HSG_EVAL_SELECT="words")`` and ``"text"``: the
blocking operand is the pack assembled on the device, so nothing is packed or uploaded on the
host and the dataset is first read in ``_drain``.  Its accumulated state equals the reference
SLTester's recorded outputs (tests/golden/eval_select.json and tests/golden/eval_words.json:
exactly; the running loss to test_gpu_tester.py's 1e-6 relative) for every recorded
(n_win, m, blocking) case, and the state of the same run without the view; document order holds
over the batches of a ``ResidentLoader``; an accessor read between batches drains.

``store.batch`` sorts by sentence count, so the fixtures' logit blocks are permuted into the
batch's document order and the recorded per-document results are compared by ``index``."""
import json
import os

import numpy as np
import pytest
import torch

import make_eval_golden as MG
import make_eval_words_golden as MW
from make_tester_golden import _Set, make_case
from test_gpu_eval_tester import assert_golden, assert_same_state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


GOLDENS = {"select": (_load("eval_select.json"), MG), "words": (_load("eval_words.json"), MW)}
_stores = {}


def store_of(key, docs, texts):
    """A store of the fixture's documents with the word ids of its texts (one build per fixture)."""
    from hetersumgraph_amd.evalsel import word_ids
    from hetersumgraph_amd.resident import DocumentStore
    if key not in _stores:
        words = [[word_ids(t["sents"], len(d.sent_nodes))] for d, t in zip(docs, texts)]
        _stores[key] = DocumentStore.from_doc_arrays(docs, DEV, chunk=3, eval_words=words)
        assert _stores[key].eval_view, _stores[key].eval_view_reason
    return _stores[key]


def blocks(docs, logits):
    """The fixture's logits per document (its rows are the documents' sentences in order)."""
    ends = np.cumsum([len(d.sent_nodes) for d in docs])
    return np.split(np.asarray(logits, np.float32), ends[:-1])


class _BlockModel:
    """Returns the logit blocks of the batch's documents, in the batch's order."""

    def __init__(self, per_doc):
        self.per_doc, self.index = per_doc, None

    def forward(self, G):
        assert G.ndata["label"].is_cuda
        return torch.from_numpy(np.concatenate([self.per_doc[i] for i in self.index])).cuda()


class _CountingSet(_Set):
    """Records, per ``get_example`` call, whether the tester was draining."""

    def __init__(self, texts):
        super().__init__(texts)
        self.calls, self.draining = [], False

    def get_example(self, i):
        self.calls.append((i, self.draining))
        return super().get_example(i)


def run(store, per_doc, texts, picks, m, blocking, n_win, mode, eval_view, between=None, data=None):
    """A tester after ``evaluation`` over ``store.batch(pick)`` for every pick in turn; returns it
    with the dataset indices in the order the documents went through."""
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.Tester import SLTester
    model = _BlockModel(per_doc)
    t = SLTester(model, m, limited=True, blocking_win=n_win)
    data = _Set(texts) if data is None else data
    order = []
    with _lib.path_options(HSG_EVAL_SELECT=mode):
        for pick in picks:
            G, index = store.batch(pick, eval_view=eval_view)
            assert hasattr(G, "eval_pack") == bool(eval_view)
            model.index = index
            order += index
            t.evaluation(G, index, data, blocking=blocking)
            if between is not None:
                between(t)
        t.getMetric()
    return t, order


@pytest.fixture
def no_host_packing(monkeypatch):
    """``pack_words``, ``pack_text`` and ``words_for`` raise: the view must not reach them."""
    from hetersumgraph_amd import evalsel

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"evalsel.{name} was reached with the eval view on the graph")
        return f
    for name in ("pack_words", "pack_text", "words_for"):
        monkeypatch.setattr(evalsel, name, refuse(name))


CASES = [(n, c) for n, (g, _) in GOLDENS.items() for c in g["cases"]]


@pytest.mark.parametrize("name,case", CASES,
                         ids=lambda x: x if isinstance(x, str) else f"w{x['n_win']}-m{x['m']}-block{int(x['blocking'])}")
def test_view_matches_the_goldens_through_the_store(name, case):
    gold, gen = GOLDENS[name]
    w = case["n_win"]
    docs, logits, texts = gen.make_case(w)
    assert texts == gold["inputs"][str(w)]["texts"]
    store, per_doc = store_of((name, w), docs, texts), blocks(docs, logits)
    pick = list(range(len(docs)))
    t, order = run(store, per_doc, texts, [pick], case["m"], case["blocking"], w, "words", True)
    assert sorted(order) == pick
    ref = dict(case["state"])
    ref.setdefault("hyps", ["\n".join(x["sents"][i] for i in e) for x, e in zip(texts, ref["extracts"])])
    for k in ("extracts", "hyps", "hyps_limited"):                   # recorded per document: into the batch's order
        ref[k] = [ref[k][i] for i in order]
    assert_golden(t, ref, [texts[i]["abstract"] for i in order])
    off, order_off = run(store, per_doc, texts, [pick], case["m"], case["blocking"], w, "words", False)
    assert order_off == order
    assert_same_state(t, off)


def test_text_mode_takes_the_view_too(no_host_packing):
    docs, logits, texts = MW.make_case(2)
    store, per_doc = store_of(("words", 2), docs, texts), blocks(docs, logits)
    t, order = run(store, per_doc, texts, [[2, 0, 3, 1]], 3, True, 2, "text", True)
    assert order == [0, 1, 2, 3]                                     # 12, 9, 8 and 6 sentences
    case = next(c for c in GOLDENS["words"][0]["cases"] if (c["n_win"], c["m"], c["blocking"]) == (2, 3, True))
    assert t.extracts == [case["state"]["extracts"][i] for i in order]


def test_text_mode_equals_the_run_without_the_view():
    docs, logits, texts = MW.make_case(2)
    store, per_doc = store_of(("words", 2), docs, texts), blocks(docs, logits)
    pick = [2, 0, 3, 1]
    on, order = run(store, per_doc, texts, [pick], 3, True, 2, "text", True)
    off, order_off = run(store, per_doc, texts, [pick], 3, True, 2, "text", False)
    assert order == order_off
    assert_same_state(on, off)


def test_host_packing_is_not_used_and_the_dataset_is_read_in_drain(no_host_packing, monkeypatch):
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.Tester import SLTester
    docs, logits, texts = MW.make_case(5)
    store, per_doc = store_of(("words", 5), docs, texts), blocks(docs, logits)
    data = _CountingSet(texts)
    real = SLTester._drain

    def drain(self, pending):
        data.draining = True
        try:
            return real(self, pending)
        finally:
            data.draining = False
    monkeypatch.setattr(SLTester, "_drain", drain)
    model = _BlockModel(per_doc)
    t = SLTester(model, 3, limited=True, blocking_win=5)
    with _lib.path_options(HSG_EVAL_SELECT="words"):
        G, index = store.batch([1, 3, 0, 2], eval_view=True)
        model.index = index
        t.evaluation(G, index, data, blocking=True)
        assert data.calls == [] and t._pending is not None          # launched; the dataset was not touched
        t.sync()
    assert data.calls == [(i, True) for i in index]
    case = next(c for c in GOLDENS["words"][0]["cases"] if (c["n_win"], c["m"], c["blocking"]) == (5, 3, True))
    assert t.extracts == [case["state"]["extracts"][i] for i in index]
    # without the view the same batch packs on the host: the refusal above is not vacuous
    with _lib.path_options(HSG_EVAL_SELECT="words"):
        G, index = store.batch([1, 3, 0, 2], eval_view=False)
        with pytest.raises(AssertionError, match="pack_words was reached"):
            SLTester(model, 3, limited=True, blocking_win=5).evaluation(G, index, _Set(texts), blocking=True)


def _loader_case():
    docs, logits, texts = make_case(31)
    return docs, texts, blocks(docs, logits), store_of(("tester", 31), docs, texts)


@pytest.mark.parametrize("m,blocking", [(3, True), (3, False), (0, False)])
def test_three_loader_batches_keep_document_order(m, blocking):
    from hetersumgraph_amd.resident import ResidentLoader
    docs, texts, per_doc, store = _loader_case()
    picks = ResidentLoader(store, 2, eval_view=True).batches()
    assert len(picks) == 3
    t, order = run(store, per_doc, texts, picks, m, blocking, 3, "words", True)
    singles = [run(store, per_doc, texts, [p], m, blocking, 3, "words", True)[0] for p in picks]
    assert t.extracts == [e for s in singles for e in s.extracts]
    assert t._hyps == [h for s in singles for h in s._hyps]
    assert t._refer == [texts[i]["abstract"] for i in order]
    assert t.batch_number == 3 and t.example_num == 5
    assert_same_state(t, run(store, per_doc, texts, picks, m, blocking, 3, "words", False)[0])


def test_reading_hyps_between_batches_drains():
    from hetersumgraph_amd.resident import ResidentLoader
    docs, texts, per_doc, store = _loader_case()
    picks = ResidentLoader(store, 2, eval_view=True).batches()
    seen = []

    def between(t):
        assert t._pending is not None                      # the batch just issued is still in flight
        seen.append((len(t.hyps), t.rougePairNum, len(t.extractLabel), int(t.pred)))
        assert t._pending is None
    t, _ = run(store, per_doc, texts, picks, 3, True, 3, "words", True, between=between)
    assert [s[:3] for s in seen] == [(2, 2, 2), (4, 4, 4), (5, 5, 5)]
    assert [s[3] for s in seen] == sorted(s[3] for s in seen) and seen[-1][3] == int(t.pred)
    assert_same_state(t, run(store, per_doc, texts, picks, 3, True, 3, "words", False)[0])


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_one_batch_under_the_sync_check():
    """The batch with its eval view is assembled, and the evaluation step issued, with torch's
    synchronisation check set to raise: no device-to-host copy into pageable memory, no
    ``.item()``, no synchronise before the launches."""
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.Tester import SLTester
    docs, logits, texts = MW.make_case(2)
    store, per_doc = store_of(("words", 2), docs, texts), blocks(docs, logits)
    pick = [0, 1, 2, 3]
    warm, _ = run(store, per_doc, texts, [pick], 3, True, 2, "words", True)        # first use: module load, pinned pool
    torch.cuda.synchronize()

    class _Ready:                                            # the logits are on the device before the check is armed
        def __init__(self, x):
            self.x = x

        def forward(self, G):
            return self.x
    order = store.batch(pick, eval_view=True)[1]
    model = _Ready(torch.from_numpy(np.concatenate([per_doc[i] for i in order])).cuda())
    t = SLTester(model, 3, limited=True, blocking_win=2)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with _lib.path_options(HSG_EVAL_SELECT="words"):
            G, index = store.batch(pick, eval_view=True)
            t.evaluation(G, index, _Set(texts), blocking=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    t.getMetric()
    assert index == order and t.extracts == warm.extracts
