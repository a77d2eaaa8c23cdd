"""The model view of a resident batch without a GPU (include/hsg_resident_model.h): the numpy
restatement (tests/resident_model_ref.py) equals, for any pick list, what today's code builds
on ``graph.batch`` of the same members -- ``node_ids``, ``sentence_counts``, ``lstm.DocLayout``,
``cnn._layout``'s length / rowoff / rows computed with torch on the CPU, and the ``torch.where``
of ``register_tfidf_table``; the word node list is the W2S relation's source list; the store's
build-time validation names the document it declines; refusals return HSG_EINVAL before any
launch; and every writing entry point of the header has a guard-band case."""
import ctypes

import numpy as np
import pytest

import abi
import resident_model_ref as MR
import resident_ref as R

HEADER = "hsg_resident_model.h"
CASES = [  # documents, pick lists (positions into the documents, in batch order)
    ("jitter", [[0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3], [1, 1, 4, 1]]),
    ("extremes", [[0], [1, 0, 5, 3, 2, 4, 0], [3, 4]]),
    ("cfg4", [[1, 2, 0], [2]]),
    ("model", [[2, 1, 4, 0, 3], [3], [1, 1]]),
    ("model_hdsg", [[1, 0, 2]]),
]


def docs_of(name):
    return MR.model_docs("hdsg" if name == "model_hdsg" else "hsg") if name.startswith("model") else R.case_docs(name)


@pytest.mark.parametrize("name,picks", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_todays_constructions(name, picks):
    docs = docs_of(name)
    for pick in picks:
        got = MR.model_view(docs, pick)
        G = R.todays_batch([docs[s] for s in pick])
        want = MR.todays(G)
        for k in MR.OUTPUTS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (pick, k, got[k].shape, want[k].shape)
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{pick} {k}")
        rows, bound, top, glen = MR.host_facts(docs, pick)
        assert rows == want["rows"] == int(got["rowoff"][-1]) and glen == want["glen"]
        ids = want["sent_ids"]
        assert bound >= len(np.unique(np.concatenate([ids.reshape(-1), [0]]))) and top >= ids.max(initial=0)
        # the word nodes are the W2S relation's sources, in its order
        np.testing.assert_array_equal(R.batch_relation("W2S", [docs[s] for s in pick])["src_nodes"], want["word_nodes"])


def test_a_pick_outside_the_documents_is_an_empty_document():
    docs = docs_of("model")
    a, b = MR.model_view(docs, [1, 9, -1, 3]), MR.model_view(docs, [1, 3])
    for k in MR.OUTPUTS:
        if k != "doc_off":
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["doc_off"].tolist() == [0, 5, 5, 5, 6] and b["doc_off"].tolist() == [0, 5, 6]


def test_the_toy_documents_hold_the_edge_cases():
    docs = docs_of("model")
    length = MR.doc_lengths(docs[1])[0]
    assert length[0] == MR.SMALL["sent_max_len"] and length[2] == 0 and len(docs[3].sent_nodes) == 1
    assert any((d.ndtype == 2).any() for d in docs_of("model_hdsg"))


def test_the_stores_layout_rule_is_the_restatements():
    from hetersumgraph_amd.resident import sentence_layout, view_refusal
    for name in ("jitter", "model", "model_hdsg", "cfg4"):
        for no, d in enumerate(docs_of(name)):
            length, pre, rows, inner = sentence_layout(d.words)
            want = MR.doc_lengths(d)
            assert np.array_equal(length, want[0]) and np.array_equal(pre, want[1]) and rows == MR.doc_rows(d)
            assert not inner and view_refusal(d, no) is None


@pytest.mark.parametrize("how,word", [("inner_pad", "PAD"), ("negative", "negative"), ("order", "ascending")])
def test_validation_declines_naming_the_document(how, word):
    from hetersumgraph_amd.resident import view_refusal
    reason = view_refusal(MR.broken(docs_of("model")[2], how), 17)
    assert reason is not None and reason.startswith("document 17:") and word in reason


def test_supported_limits():
    from hetersumgraph_amd import _lib
    lib, top = _lib.load(), 2 ** 31 - 1
    for args, want in (((1, 0, 0, 0), 1), ((1 << 20, top, top, top), 1), ((0, 1, 1, 1), 0), (((1 << 20) + 1, 1, 1, 1), 0),
                       ((1, top + 1, 0, 0), 0), ((1, 0, top + 1, 0), 0), ((1, 0, 0, top + 1), 0), ((1, -1, 0, 0), 0),
                       ((1, 0, -1, 0), 0), ((1, 0, 0, -1), 0), ((32, 1120, 159040, 40000), 1)):
        assert bool(lib.hsg_res_model_supported(*args)) == bool(want), args


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands for
    a non-NULL device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p, top = _lib.load(), _lib.HSG_EINVAL, 16, 2 ** 31 - 1

    def store(**kw):
        f = dict(n_docs=4, starts=p, bases=p, sent_len=8, label_len=5, sent_rank=p, words=p, tffrac=p, edtype=p)
        f.update(kw)
        return ctypes.byref(_lib.HsgResStore(**f))

    def model(st=None, tok=(p, p), B=2, pick=p, offs=p, rowbase=p, ns=5, E=7, outs=None):
        outs = [p] * 8 if outs is None else outs
        return lib.hsg_res_model(store() if st is None else st, *tok, B, pick, offs, rowbase, ns, E, *outs, None)
    drop = lambda i: [None if j == i else p for j in range(8)]
    assert lib.hsg_res_model(None, p, p, 2, p, p, p, 5, 7, *[p] * 8, None) == EINVAL
    for kw in [dict(B=0), dict(B=-1), dict(B=(1 << 20) + 1), dict(pick=None), dict(offs=None), dict(rowbase=None),
               dict(ns=-1), dict(E=-1), dict(ns=top + 1), dict(E=top + 1), dict(tok=(None, p)), dict(tok=(p, None)),
               dict(st=store(sent_len=0)), dict(st=store(starts=None)), dict(st=store(bases=None)),
               dict(st=store(n_docs=0)), dict(st=store(n_docs=top + 1)), dict(st=store(sent_rank=None)),
               dict(st=store(words=None)), dict(st=store(tffrac=None)), dict(st=store(edtype=None))] + \
              [dict(outs=drop(i)) for i in range(8)]:
        assert model(**kw) == EINVAL, kw
    # rowoff and doc_off hold elements even when the batch has no sentence and no edge
    assert model(ns=0, E=0, outs=drop(4)) == EINVAL and model(ns=0, E=0, outs=drop(5)) == EINVAL


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_resident_model_guard import CASES as GUARD
    w = abi.writable_entry_points([HEADER])
    assert list(w) == ["hsg_res_model"] and len(w["hsg_res_model"]) == 8
    for prm in ("int64_t *sent_nodes", "int64_t *sent_ids", "int32_t *rowoff", "int32_t *doc_off", "int64_t *prev",
                "int64_t *tfidf_index"):
        assert prm in w["hsg_res_model"], prm
    missing = sorted(n for n in w if n not in GUARD)
    assert not missing, f"no guard-band case: {missing}"
    assert set(GUARD) <= set(w) and all(GUARD.values())


def test_the_registry_lists_the_header():
    from hetersumgraph_amd import _lib
    assert _lib.exports(HEADER) == ("hsg_res_model_supported", "hsg_res_model")
