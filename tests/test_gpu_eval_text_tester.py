"""SLTester.evaluation with the word ids made on the device
(``path_options(HSG_EVAL_SELECT="text")``: evalsel.pack_text -> hsg_eval_text_words ->
hsg_eval_select_words) over DEVICE logits: its accumulated state -- extracts, hyps, refer, the
four counters, the loss, the length-limited hypotheses -- equals the reference SLTester's
recorded outputs (tests/golden/eval_select.json, eval_words.json and eval_text.json) and a
switch-off tester's state on the same input; with ``G.eval_words`` attached it equals mode
"words"; it still passes with ``SLTester.ngram_blocking`` patched to raise, which shows that the
device path ran; it neither reads nor fills the per-example cache; and with m == 0 or without
blocking it touches no text."""
import json
import os

import pytest
import torch

import make_eval_golden as MG
import make_eval_text_golden as MT
import make_eval_words_golden as MW
from make_tester_golden import _Set, make_case
from test_gpu_eval_tester import _DeviceModel, assert_golden, assert_same_state, graph_of
from test_gpu_eval_words_tester import run

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


GOLDENS = {"select": (_load("eval_select.json"), MG), "words": (_load("eval_words.json"), MW),
           "text": (_load("eval_text.json"), MT)}


@pytest.fixture
def no_host_blocking(monkeypatch):
    """The default loop's host blocking raises: whoever passes did not go through it."""
    from hetersumgraph_amd.Tester import SLTester

    def boom(*a, **k):
        raise AssertionError("SLTester.ngram_blocking was called: the default loop ran")
    monkeypatch.setattr(SLTester, "ngram_blocking", boom)


@pytest.mark.parametrize("name,case", [(n, c) for n, (g, _) in GOLDENS.items() for c in g["cases"]],
                         ids=lambda x: x if isinstance(x, str) else f"w{x['n_win']}-m{x['m']}-block{int(x['blocking'])}")
def test_text_step_matches_the_goldens(name, case):
    from hetersumgraph_amd import evalsel
    gold, gen = GOLDENS[name]
    w = case["n_win"]
    batch = gen.make_case(w)
    texts = gold["inputs"][str(w)]["texts"]
    assert batch[2] == texts
    evalsel.clear_word_cache()
    t = run([batch], case["m"], case["blocking"], w, "text")
    assert len(evalsel._WORD_CACHE) == 0                                   # the per-example cache is not filled
    refer = [x["abstract"] for x in texts]
    ref = dict(case["state"])
    ref.setdefault("hyps", ["\n".join(x["sents"][i] for i in e) for x, e in zip(texts, ref["extracts"])])
    # TestPipLine.hyps' rule, where the fixture leaves the cut hypotheses out
    ref.setdefault("hyps_limited", [" ".join(h.split(" ")[:len(r.split(" "))]) for h, r in zip(ref["hyps"], refer)])
    assert_golden(t, ref, refer)
    assert_same_state(t, run([batch], case["m"], case["blocking"], w, "0"))
    # with the ids attached to the graph the batch is mode "words"'s
    assert_same_state(run([batch], case["m"], case["blocking"], w, "text", attach=True),
                      run([batch], case["m"], case["blocking"], w, "words", attach=True))
    assert len(evalsel._WORD_CACHE) == 0


@pytest.mark.parametrize("m,blocking", [(3, True), (5, True), (3, False), (0, True)])
def test_several_random_batches_keep_document_order(m, blocking):
    batches = [make_case(31), MT.make_case(2), MW.make_case(2), MG.make_case(3), make_case(32)]
    t = run(batches, m, blocking, 2, "text")
    singles = [run([b], m, blocking, 2, "text") for b in batches]
    assert t.extracts == [e for s in singles for e in s.extracts]
    assert t._hyps == [h for s in singles for h in s._hyps]
    assert t.batch_number == 5
    assert_same_state(t, run(batches, m, blocking, 2, "0"))


def test_the_device_path_ran(no_host_blocking):
    """With the default loop's host blocking patched to raise, "text" still passes and gives
    the recorded extracts; the default loop itself does raise."""
    gold, _ = GOLDENS["text"]
    for w, m in ((2, 3), (3, 5)):
        batch = MT.make_case(w)
        t = run([batch], m, True, w, "text")
        case = [c for c in gold["cases"] if (c["n_win"], c["m"], c["blocking"]) == (w, m, True)][0]
        assert t.extracts == case["state"]["extracts"]
    with pytest.raises(AssertionError, match="the default loop ran"):
        run([MT.make_case(2)], 3, True, 2, "0")


def test_the_attached_ids_are_used_as_they_are(monkeypatch):
    from hetersumgraph_amd import evalsel
    monkeypatch.setattr(evalsel, "pack_text", lambda *a, **k: pytest.fail("pack_text was called"))
    batch = MT.make_case(3)
    assert run([batch], 3, True, 3, "text", attach=True).extracts == run([batch], 3, True, 3, "words").extracts


@pytest.mark.parametrize("m,blocking", [(0, True), (0, False), (3, False)])
def test_no_text_is_touched_without_blocking_or_with_m_zero(monkeypatch, m, blocking):
    from hetersumgraph_amd import evalsel
    for name in ("pack_text", "text_words", "pack_words", "words_for", "pack_batch"):
        monkeypatch.setattr(evalsel, name, lambda *a, _n=name, **k: pytest.fail(f"evalsel.{_n} was called"))
    batch = MT.make_case(2)
    t = run([batch], m, blocking, 2, "text")
    monkeypatch.undo()
    assert_same_state(t, run([batch], m, blocking, 2, "0"))


def test_errors_name_the_switch_value():
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.Tester import SLTester
    docs, logits, texts = make_case(31)

    class _Cpu:
        def forward(self, G):
            return torch.from_numpy(logits)
    with _lib.path_options(HSG_EVAL_SELECT="text"):
        with pytest.raises(RuntimeError, match="HSG_EVAL_SELECT=text.*ROCm device"):
            SLTester(_Cpu(), 3).evaluation(graph_of(docs), list(range(len(docs))), _Set(texts), blocking=True)
        # a document whose chosen sentences store more windows than the largest table: refused by the kernel,
        # reported when its batch is drained
        long = [dict(t, sents=[" ".join(f"u{i}x{j}" for j in range(6000)) for i in range(len(t["sents"]))]) for t in texts]
        t = SLTester(_DeviceModel(logits), 3, blocking_win=3)
        t.evaluation(graph_of(docs), list(range(len(docs))), _Set(long), blocking=True)
        with pytest.raises(RuntimeError, match="HSG_EVAL_SELECT=text.*document 0.*hsg_eval_select_words's limits"):
            t.sync()
