"""The eval view of a resident batch on the GPU (include/hsg_resident_eval.h,
``DocumentStore.batch(eval_view=True)``): ``G.eval_pack.buf`` is bit-equal to
``evalsel.pack_words(G.eval_words, counts).buf`` -- what ``SLTester`` packs and uploads per batch
without the view -- with equal ``n``, ``B``, ``W`` and ``tab_cap(n_win, m)`` for every window of
1..8 words and m of 0..6; with and without the model view; for a ``MultiExampleSet`` store; and
the batch without the view, or of a store that declined it, is today's batch.  The documents
and their word lists are tests/resident_eval_ref.py's."""
import os

import numpy as np
import pytest
import torch

import resident_eval_ref as ER
import resident_ref as R
from hetersumgraph_amd import graph as hg
from test_gpu_resident import assert_same_batch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# dataset indices in the order given to batch(): 3,000 words in 5 rows beside a single word; batches
# of one document (no word at all: W == 0; one row); a repeated index; every document, shuffled
# (the sort by sentence count reorders them); two wordless documents (W == 0)
PICKS = ([6, 4], [0], [5], [1, 1, 4, 1], [4, 6, 2, 0, 5, 3, 1], [0, 0])
_made = {}


def made():
    from hetersumgraph_amd.resident import DocumentStore
    if not _made:
        docs = ER.eval_docs()
        words = ER.word_lists(docs)
        store = DocumentStore.from_doc_arrays(docs, DEV, chunk=2, eval_words=[[w] for w in words])
        _made.update(docs=docs, words=words, store=store)
    return _made["docs"], _made["words"], _made["store"]


def assert_pack(G, counts):
    """The contract on ``G.eval_pack``."""
    from hetersumgraph_amd.evalsel import WordPack, pack_words
    want = pack_words(G.eval_words, counts, pin=False)
    got = G.eval_pack
    assert isinstance(got, WordPack) and got.buf.device == DEV and got.buf.dtype == torch.int32
    assert (got.n, got.B, got.W, list(got.counts)) == (want.n, want.B, want.W, list(want.counts))
    assert got.buf.shape == want.buf.shape and torch.equal(got.buf.cpu(), want.buf)
    for a, b in zip(got.views(), want.views()):
        assert torch.equal(a.cpu(), b)
    for n_win in range(1, 9):
        for m in range(0, 7):
            assert got.tab_cap(n_win, m) == want.tab_cap(n_win, m), (n_win, m)
    assert got.to(DEV) is got
    return want


@pytest.mark.parametrize("model_view", [None, False], ids=["views", "no_model_view"])
@pytest.mark.parametrize("pick", PICKS, ids=lambda p: "-".join(map(str, p)))
def test_eval_pack_is_pack_words(pick, model_view):
    docs, words, store = made()
    assert store.eval_view and store.eval_view_reason is None
    G, index = store.batch(pick, model_view=model_view, eval_view=True)
    n_sent = [len(docs[i].sent_nodes) for i in pick]
    assert index == [pick[j] for j in np.argsort(-np.asarray(n_sent), kind="stable")]
    assert all(a[0] is words[i][0] and a[1] is words[i][1] for a, i in zip(G.eval_words, index))     # as today
    want = assert_pack(G, [len(docs[i].sent_nodes) for i in index])
    if pick in ([0], [0, 0]):
        assert want.W == 0 and G.eval_pack.buf.numel() == want.n + 2 and int(G.eval_pack.buf[-1]) == 0
    if pick == [6, 4]:
        assert index == [6, 4] and want.W == 3001
    if pick == [4, 6, 2, 0, 5, 3, 1]:
        assert index != pick and sorted(index) == sorted(pick)
    assert model_view is None or G.model_inputs is None


def test_without_the_view_the_batch_is_todays():
    docs, words, store = made()
    from hetersumgraph_amd.resident import DocumentStore
    assert DocumentStore.EVAL_VIEW is True                      # the measured default
    G, index = store.batch([4, 6, 2, 0, 5, 3, 1], eval_view=False)
    assert not hasattr(G, "eval_pack")
    assert_same_batch(G, R.todays_batch([docs[i] for i in index]).to(DEV))
    assert all(a[0] is words[i][0] for a, i in zip(G.eval_words, index))
    for kw in (dict(eval_view=True), {}):                       # the view changes nothing else of the batch
        H, index2 = store.batch([4, 6, 2, 0, 5, 3, 1], **kw)
        assert index2 == index and hasattr(H, "eval_pack")
        assert_same_batch(H, R.todays_batch([docs[i] for i in index]).to(DEV))
    try:                                                        # None follows the class default
        DocumentStore.EVAL_VIEW = False
        assert not hasattr(store.batch([3, 1])[0], "eval_pack") and hasattr(store.batch([3, 1], eval_view=True)[0], "eval_pack")
    finally:
        DocumentStore.EVAL_VIEW = True


def test_a_store_with_other_eval_words_declines_the_view():
    from hetersumgraph_amd.resident import DocumentStore, ResidentLoader
    docs, words, _ = made()
    fake = [[[i, i + 1]] for i in range(len(docs))]
    store = DocumentStore.from_doc_arrays(docs, DEV, chunk=3, eval_words=fake)
    assert store.eval_view is False and store.eval_view_reason.startswith("document 0:")
    for G, index in ResidentLoader(store, 4, eval_view=True):
        assert not hasattr(G, "eval_pack") and G.eval_words == [fake[i][0] for i in index]
        assert_same_batch(G, R.todays_batch([docs[i] for i in index]).to(DEV))
    with pytest.raises(RuntimeError, match="declined the eval view"):
        store.seen_need(3, 3)
    late = [[w] for w in words[:4]] + [[words[4], words[4]]] + [[w] for w in words[5:]]
    store = DocumentStore.from_doc_arrays(docs, DEV, chunk=3, eval_words=late)
    assert store.eval_view is False and store.eval_view_reason.startswith("document 4:") and "2 parts" in store.eval_view_reason
    none = DocumentStore.from_doc_arrays(docs[:2], DEV)
    assert none.eval_view is False and "without eval_words" in none.eval_view_reason
    assert not hasattr(none.batch([0, 1], eval_view=True)[0], "eval_pack")


def test_from_a_multi_example_set(tmp_path):
    """``from_dataset`` over a MultiExampleSet made with ``eval_words=True``: the store accepts the
    ids the dataset makes, and every batch of a loader carries their pack."""
    from graph_data import STOPWORDS, make_files
    from hetersumgraph_amd import build
    from hetersumgraph_amd.HiGraph import sentence_counts
    from hetersumgraph_amd.evalsel import pack_words
    from hetersumgraph_amd.module.dataloader import MultiExampleSet
    from hetersumgraph_amd.resident import DocumentStore, ResidentLoader
    build.build_host(verbose=False)
    d = str(tmp_path / "hdsg")
    vocab = make_files(d, seed=11, n_examples=6, multi=True)
    ds = MultiExampleSet(os.path.join(d, "data.jsonl"), vocab, 7, 12, os.path.join(d, "filter_word.txt"),
                         os.path.join(d, "w2s.jsonl"), os.path.join(d, "w2d.jsonl"), stopwords=STOPWORDS, eval_words=True)
    store = DocumentStore.from_dataset(ds, DEV, indices=[4, 0, 5, 2, 1, 3], chunk=2)
    assert store.eval_view, store.eval_view_reason
    seen = []
    for G, index in ResidentLoader(store, 4, eval_view=True):
        seen += index
        T = hg.batch([ds[i][0] for i in index]).to(DEV)
        assert_same_batch(G, T)
        counts = list(sentence_counts(T))
        assert_pack(G, counts)
        assert torch.equal(G.eval_pack.buf.cpu(), pack_words(T.eval_words, counts, pin=False).buf)
    assert sorted(seen) == list(range(6))
