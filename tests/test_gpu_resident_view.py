"""The model view of a resident batch on the GPU (include/hsg_resident_model.h,
hetersumgraph_amd/resident.py): every output bit-equal to the numpy restatement
(tests/resident_model_ref.py) and to what today's code caches on today's batch of the same
members; a declined store's batches carry no view; a training step on a fresh batch with the
view performs no host wait (and does without it); the model's results are bitwise unchanged;
and a write to the graph's columns drops the view."""
import numpy as np
import pytest
import torch

import resident_model_ref as MR
import resident_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = [  # id, documents, build chunk, pick lists (dataset indices, in the order given to batch())
    ("one_sentence", "model", 2, [[3]]),                       # B = 1, a one-sentence document
    ("pads", "model", 5, [[1], [1, 0]]),                       # a sentence without PAD, an all-PAD sentence
    ("repeat", "model", 2, [[1, 1, 4, 1]]),
    ("reordered", "model", 2, [[3, 0, 2, 1, 4]]),              # the length sort reorders the pick
    ("chunk2", "model", 2, [[0, 1, 2, 3, 4], [4, 2]]),         # stored bases are non-zero
    ("jitter", "jitter", 2, [[4, 2, 0, 3, 1]]),
    ("hdsg", "model_hdsg", 2, [[1, 0, 2], [2]]),               # doc nodes: sent_nodes excludes them
    ("cfg4", "cfg4", 2, [[1, 2, 0]]),
]
_stores = {}


def docs_of(name):
    if name.startswith("model"):
        return MR.model_docs("hdsg" if name == "model_hdsg" else "hsg")
    return R.case_docs(name)


def store_of(name, chunk):
    from hetersumgraph_amd.resident import DocumentStore
    if (name, chunk) not in _stores:
        docs = docs_of(name)
        _stores[name, chunk] = (docs, DocumentStore.from_doc_arrays(docs, DEV, chunk=chunk))
    return _stores[name, chunk]


def same(a, b, what):
    b = torch.as_tensor(b)
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a.cpu(), b.cpu()), what


@pytest.mark.parametrize("cid,name,chunk,picks", CASES, ids=[c[0] for c in CASES])
def test_view_is_the_restatement_and_todays_caches(cid, name, chunk, picks):
    from hetersumgraph_amd import HiGraph, loss as hloss
    docs, store = store_of(name, chunk)
    assert store.model_view and store.model_view_reason is None
    for pick in picks:
        G, index = store.batch(pick, model_view=True)
        view = G.model_inputs
        assert view is not None
        want = MR.model_view(docs, index)
        T = R.todays_batch([docs[i] for i in index]).to(DEV)
        today = MR.todays(T)
        for k in MR.OUTPUTS:
            same(getattr(view, k), want[k], (cid, pick, k, "restatement"))
            same(getattr(view, k), today[k], (cid, pick, k, "today"))
        rows, bound, top, glen = MR.host_facts(docs, index)
        assert (view.rows, view.bound, view.max_token, list(view.glen)) == (rows, bound, top, glen)
        assert view.rows == today["rows"]
        # what the model's accessors now return, against today's on today's batch
        same(HiGraph.node_ids(G, "unit", 0.0), HiGraph.node_ids(T, "unit", 0.0), "word nodes")
        same(HiGraph.node_ids(G, "dtype", 1.0), HiGraph.node_ids(T, "dtype", 1.0), "sentence nodes")
        assert HiGraph.sentence_counts(G) == HiGraph.sentence_counts(T)
        for a, b in zip(hloss.sentence_loss_inputs(G), hloss.sentence_loss_inputs(T)):
            same(a, b, "sentence_loss_inputs")
        for g in (G, T):
            HiGraph.register_tfidf_table(g, torch.zeros(10, 4, device=DEV))
        same(G._eframe().cols["tfidfembed"].index, T._eframe().cols["tfidfembed"].index, "tfidf_index")
        lay, tl = view.doc_layout, __import__("hetersumgraph_amd.lstm", fromlist=["x"]).DocLayout(tuple(glen), DEV)
        assert (lay.glen, lay.n_docs, lay.n_rows) == (tl.glen, tl.n_docs, tl.n_rows)
        same(lay.doc_off, tl.doc_off, "doc_off")
        same(lay.prev, tl.prev, "prev")
        # and the batch itself is the batch without the view
        G0, index0 = store.batch(pick, model_view=False)
        assert index0 == index and G0.model_inputs is None
        assert not any(k[0] in ("sent_counts", "tfidf_index", "sent_doc_off") or k[0][0] == "nodes" for k in G0._rel_cache)
        for k in ("words", "position", "label", "id", "unit", "dtype"):
            assert torch.equal(G.ndata[k], G0.ndata[k]), k


@pytest.mark.parametrize("how", ["inner_pad", "negative", "order"])
def test_a_declined_store_yields_batches_without_a_view(how):
    from hetersumgraph_amd.resident import DocumentStore
    docs = MR.model_docs()
    docs[2] = MR.broken(docs[2], how)
    store = DocumentStore.from_doc_arrays(docs, DEV, chunk=2)          # builds, as it does today
    assert store.model_view is False and store.model_view_reason.startswith("document 2:")
    for flag in (None, True, False):
        G, index = store.batch([0, 1], model_view=flag)
        assert G.model_inputs is None and ("sent_doc_off", str(DEV)) not in G._rel_cache
    T = R.todays_batch([docs[i] for i in index]).to(DEV)
    assert torch.equal(G.ndata["words"], T.ndata["words"])


# ---- the models on the toy documents of tests/test_gpu_resident_model.py ------------------------
def model_store(cls):
    from hetersumgraph_amd.resident import DocumentStore
    from test_gpu_resident_model import documents
    if cls not in _stores:
        docs = documents(cls)
        _stores[cls] = (docs, DocumentStore.from_doc_arrays(docs, DEV, chunk=2))
    return _stores[cls]


def make_model(cls, embed_train):
    """tests/test_gpu_resident_model.py's seeded model, in train mode; the embedding frozen
    where the token paths of the sentence CNN are to run."""
    import model_ref as M
    from test_gpu_resident_model import CASES as SEEDS
    model = M.make_model(cls, dict(SEEDS)[cls], {"vocab_size": 500, "n_iter": 2, "doc_max_timesteps": 50})
    model._embed.weight.requires_grad = embed_train
    return model.to(DEV).train()


def switches(lstm, embed, cnn):
    return dict(HSG_SENT_LSTM=lstm, HSG_MODEL_GLUE="1", HSG_WORD_EMBED=embed, HSG_SENT_CNN=cnn)


def step(model, adam, G):
    from hetersumgraph_amd import loss as hloss
    logits = model(G)
    loss = hloss.sentence_loss(G, logits)
    loss.backward()
    adam.step()
    return logits, loss


# HSG_SENT_CNN="tokens" is left out: sizing its token table by the view's bound of the distinct
# tokens measured slower than their exact count, so it keeps its single read-back
COMBOS = [(lstm, embed, cnn) for lstm in ("1", "2") for embed in ("0", "1") for cnn in ("0", "dw")]


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
@pytest.mark.parametrize("lstm,embed,cnn", COMBOS, ids=["lstm%s-embed%s-cnn_%s" % c for c in COMBOS])
def test_a_step_on_a_fresh_batch_waits_for_nothing(lstm, embed, cnn):
    """With the view: batch assembly, forward, loss, backward and the optimizer step complete
    under torch's synchronisation check.  Without it the same sequence raises: the check sees
    the waits this removes."""
    from hetersumgraph_amd import optim, rng
    from hetersumgraph_amd._lib import path_options
    docs, store = model_store("HSumGraph")
    model = make_model("HSumGraph", embed == "1")
    adam = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-4, max_grad_norm=1.0)
    rng.manual_seed(5)
    with path_options(**switches(lstm, embed, cnn)):
        for view in (True, False):
            G, _ = store.batch([0, 2, 4], model_view=view)                 # warm-up on another pick
            step(model, adam, G)
            adam.zero_grad()
            torch.cuda.synchronize()
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                if view:
                    G, _ = store.batch([3, 1, 2, 0], model_view=True)
                    assert G.model_inputs is not None
                    logits, loss = step(model, adam, G)
                else:
                    with pytest.raises(RuntimeError):
                        G, _ = store.batch([3, 1, 2, 0], model_view=False)
                        step(model, adam, G)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
            adam.zero_grad()
            torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def run_once(cls, docs, make_batch, opts, embed_train, disturb=None):
    """One forward / loss / backward of a freshly seeded model on ``make_batch()``: logits, loss
    and every parameter gradient."""
    from hetersumgraph_amd import loss as hloss, rng
    from hetersumgraph_amd._lib import path_options
    model = make_model(cls, embed_train)
    rng.manual_seed(9)
    with path_options(**opts):
        G = make_batch()
        if disturb is not None:
            disturb(G)
        logits = model(G)
        loss = hloss.sentence_loss(G, logits)
        loss.backward()
    return dict(logits=logits.detach(), loss=loss.detach().view(1),
                **{"grad:" + n: p.grad for n, p in model.named_parameters() if p.grad is not None})


def assert_bitwise(a, b, what):
    assert a.keys() == b.keys() and len(a) > 10, what
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


RESULT_CASES = [("HSumGraph", c) for c in (("1", "0", "0"), ("2", "0", "dw"), ("2", "0", "tokens"), ("2", "1", "0"))] + \
               [("HSumDocGraph", c) for c in (("2", "0", "dw"), ("1", "1", "0"))]


@pytest.mark.parametrize("cls,combo", RESULT_CASES, ids=["-".join((c[0],) + c[1]) for c in RESULT_CASES])
def test_results_are_unchanged(cls, combo):
    """View on against view off, and against today's batch of the same members: logits, loss
    and every parameter gradient, bitwise."""
    docs, store = model_store(cls)
    pick = [2, 0, 1]
    opts, train = switches(*combo), combo[1] == "1"
    index = store.batch(pick)[1]
    on = run_once(cls, docs, lambda: store.batch(pick, model_view=True)[0], opts, train)
    off = run_once(cls, docs, lambda: store.batch(pick, model_view=False)[0], opts, train)
    today = run_once(cls, docs, lambda: R.todays_batch([docs[i] for i in index]).to(DEV), opts, train)
    assert_bitwise(on, off, "view on / off")
    assert_bitwise(on, today, "view on / today's batch")
    assert bool(on["logits"].abs().sum() > 0)


def test_a_write_to_the_token_rows_drops_the_view():
    """A changed token after assembly, by assignment and in place: the forward uses the new
    tokens and equals today's batch given the same write; the untouched batch differs."""
    docs, store = model_store("HSumGraph")
    pick, opts = [2, 0, 1], switches("2", "0", "dw")
    index = store.batch(pick)[1]

    def assign(G):
        w = G.ndata["words"].clone()
        w[G.ndata["dtype"] == 1, 0] = 11
        G.ndata["words"] = w

    def in_place(G):
        G.ndata["words"][G.ndata["dtype"] == 1, 0] = 11

    resident = lambda: store.batch(pick, model_view=True)[0]
    today = run_once("HSumGraph", docs, lambda: R.todays_batch([docs[i] for i in index]).to(DEV), opts, False, assign)
    plain = run_once("HSumGraph", docs, resident, opts, False)
    assert not torch.equal(plain["logits"], today["logits"])
    for write in (assign, in_place):
        assert_bitwise(run_once("HSumGraph", docs, resident, opts, False, write), today, write.__name__)
    G = resident()
    assert G.model_inputs is not None and ("sent_doc_off", str(DEV)) in G._rel_cache
    assign(G)
    assert G.model_inputs is None and ("sent_doc_off", str(DEV)) not in G._rel_cache
    assert ("rel", "W2S", str(DEV)) in G._rel_cache            # the relations stay: no structural column was written
    G = resident()
    G.ndata["unit"] = G.ndata["unit"].clone()
    assert G.model_inputs is None and not G._rel_cache


@pytest.mark.parametrize("mode", ["dw", "tokens"])
def test_token_paths_on_the_views_layout_give_todays_bits(mode):
    """``cnn.sent_cnn_tokens`` on the view's token rows: feat, and the weight and bias gradients
    that arg routes, on the view's layout and on the layout computed (and read back) from the
    ids -- bitwise equal; the vocabulary range check, made on the host, raises today's error."""
    from hetersumgraph_amd import cnn
    docs, store = store_of("model", 2)
    G, _ = store.batch([2, 1, 4, 0, 3], model_view=True)
    view = G.model_inputs
    assert len(torch.unique(view.sent_ids)) <= view.bound < 500 and view.max_token == int(view.sent_ids.max())
    torch.manual_seed(2)
    E, P = torch.randn(500, 300, device=DEV), torch.randn(13, 300, device=DEV)
    Ws = [torch.randn(50, 1, h, 300, device=DEV).mul_(0.05) for h in cnn.HEIGHTS]
    bs = [torch.randn(50, device=DEV) for _ in cnn.HEIGHTS]
    up = torch.randn(view.sent_ids.shape[0], 300, device=DEV)
    runs = []
    for layout in (None, view.layout):
        ws, b = [w.clone().requires_grad_() for w in Ws], [x.clone().requires_grad_() for x in bs]
        feat = cnn.sent_cnn_tokens(view.sent_ids, E, P, ws, b, mode=mode, layout=layout)
        (feat * up).sum().backward()
        runs.append([feat.detach()] + [w.grad for w in ws] + [x.grad for x in b])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))
    assert bool(runs[0][0].any())
    with pytest.raises(ValueError, match="outside the vocabulary"):          # the range check, on the host
        cnn.sent_cnn_tokens(view.sent_ids, E[:view.max_token], P, Ws, bs, mode=mode, layout=view.layout)
