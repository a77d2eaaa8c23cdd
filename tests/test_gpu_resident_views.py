"""All eight ``(model_view, doc_view, eval_view)`` combinations of ``DocumentStore.batch`` on one
store that can carry all three views: every view that should be present is bit-equal to its numpy
restatement (tests/resident_model_ref.py, resident_hdsg_ref.py, resident_eval_ref.py) -- so each
view read its own running offsets out of the one pinned copy, whichever other views rode in it --
every view that should be absent is absent, and the graph and both relations are those of the
batch without any view.  The store is the seven toy HDSG examples in chunks of two (non-zero
stored bases) with word lists that hold a row of 0 words and a row of 1 word; the pick repeats a
document, is reordered by the length sort and holds document 5, which needs a work list."""
import itertools

import numpy as np
import pytest
import torch

import resident_eval_ref as ER
import resident_hdsg_ref as HR
import resident_model_ref as MR
import resident_ref as R
from hetersumgraph_amd.relation import HOT_KINDS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KEYS = [("hdsg_layout", str(DEV)), ("hdsg_head_layout", str(DEV))]
CHUNK, PICK = 2, [2, 2, 1, 5, 0]
_made = {}


def word_lists(docs):
    """Per document its ``(ptr int32 [N + 1], ids int32 [W])`` as tests/resident_eval_ref.py draws
    them: 0 .. 12 words per row, the first row of 0 words and the last of 1."""
    rng = np.random.default_rng(29)
    out = []
    for d in docs:
        N = len(d.sent_nodes)
        lens = rng.integers(0, 13, N).astype(np.int64)
        lens[0], lens[-1] = 0, 1
        ptr = np.zeros(N + 1, np.int32)
        np.cumsum(lens, out=ptr[1:])
        W = int(ptr[-1])
        out.append((ptr, rng.integers(0, max(W // 2, 1), W).astype(np.int32)))
    return out


def made():
    """The store, and the expected value of every view for PICK (computed once, never changed)."""
    from hetersumgraph_amd.resident import DocumentStore, batch_order
    if not _made:
        docs = HR.hdsg_docs()
        words = word_lists(docs)
        assert any((np.diff(p) == 0).any() for p, _ in words) and any((np.diff(p) == 1).any() for p, _ in words)
        store = DocumentStore.from_doc_arrays(docs, DEV, chunk=CHUNK, eval_words=[[w] for w in words])
        n_sent = [len(docs[i].sent_nodes) for i in PICK]
        index = [PICK[j] for j in batch_order(n_sent)]
        assert index != PICK and len(set(index)) < len(index)            # reordered, with a repeat
        _made.update(docs=docs, words=words, store=store, index=index, model=MR.model_view(docs, index),
                     facts=MR.host_facts(docs, index), doc=HR.doc_view(docs, index),
                     pack=ER.eval_pack(R.build_store(docs, CHUNK), words, index))
    return _made


def same(a, b, what):
    """Equal dtype, shape and bits."""
    b = torch.as_tensor(b)
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8)), what


def doc_view_of(G):
    """The eighteen outputs of the doc view as the batch carries them, named as the header names them."""
    lay, hl = G._rel_cache[KEYS[0]], G._rel_cache[KEYS[1]]
    out = {k: lay[k.replace("64", "")] for k in HR.DICT}
    out.update({k: getattr(hl, k) for k in HR.HEAD}, inv_cnt=lay["inv_cnt"])
    assert hl.inv_cnt is lay["inv_cnt"]
    return out


def graph_and_relations(G):
    out = {("ndata", k): G.ndata[k] for k in G.ndata.keys()}
    out.update({("edata", k): G.edata[k] for k in G.edata.keys()})
    out["src"], out["dst"] = G._src_t(), G._dst_t()
    for kind in HOT_KINDS:
        out.update({(kind, k): v for k, v in G.relation(kind).dev.items()})
    return out


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_every_combination_of_the_three_views():
    from hetersumgraph_amd.evalsel import pack_words
    m = made()
    docs, store, index = m["docs"], m["store"], m["index"]
    assert store.model_view and store.doc_view and store.eval_view
    G0, index0 = store.batch(PICK, model_view=False, doc_view=False, eval_view=False)
    assert index0 == index and any(G0.resident_work_lists.values())
    base = graph_and_relations(G0)
    assert any(k[1] in ("dwork", "swork") for k in base)
    for mv, dv, ev in itertools.product((False, True), repeat=3):
        flags = dict(model_view=mv, doc_view=dv, eval_view=ev)
        if mv and dv and ev:
            store.batch(PICK, **flags)                          # warm-up: the allocator's blocks
            torch.cuda.synchronize()
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                G, got_index = store.batch(PICK, **flags)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
        else:
            G, got_index = store.batch(PICK, **flags)
        assert got_index == index, flags
        # the model view
        view = G.model_inputs
        if mv:
            assert view is not None, flags
            for k in MR.OUTPUTS:
                same(getattr(view, k), m["model"][k], (flags, k))
            assert (view.rows, view.bound, view.max_token, list(view.glen)) == m["facts"], flags
            same(G._rel_cache[("sent_doc_off", str(DEV))], m["model"]["doc_off"], (flags, "sent_doc_off"))
        else:
            assert view is None and ("sent_doc_off", str(DEV)) not in G._rel_cache, flags
        # the doc view: only with the model view
        if mv and dv:
            got = doc_view_of(G)
            for k in HR.OUTPUTS:
                same(got[k], m["doc"][k], (flags, k))
        else:
            assert not any(k in G._rel_cache for k in KEYS), flags
        # the eval view
        if ev:
            pack = G.eval_pack
            counts = [len(docs[i].sent_nodes) for i in index]
            want = pack_words(G.eval_words, counts, pin=False)
            same(pack.buf, m["pack"], (flags, "restatement"))
            same(pack.buf, want.buf, (flags, "pack_words"))
            assert (pack.n, pack.B, pack.W, list(pack.counts)) == (want.n, want.B, want.W, counts), flags
        else:
            assert not hasattr(G, "eval_pack"), flags
        # the graph and both relations are the all-off batch's, work lists included
        assert G.resident_work_lists == G0.resident_work_lists, flags
        got = graph_and_relations(G)
        assert set(got) == set(base), (flags, sorted(set(got) ^ set(base), key=str))
        for k, v in base.items():
            same(got[k], v, (flags, k))
