"""The doc view of a resident batch on the GPU (include/hsg_resident_hdsg.h,
hetersumgraph_amd/resident.py): every output bit-equal to the numpy restatement
(tests/resident_hdsg_ref.py) and to what today's code builds on today's batch of the same
members; work lists sized on the host equal today's, with no read-back; a training step of
``HSumDocGraph`` on a fresh batch that needs work lists performs no host wait (and does without
the doc view); the model's results are bitwise unchanged; a declined store's batches run today's
code with today's errors; and a write to the graph's columns drops the doc view."""
import numpy as np
import pytest
import torch

import resident_hdsg_ref as HR
import resident_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KEYS = [("hdsg_layout", str(DEV)), ("hdsg_head_layout", str(DEV))]
CASES = [(name, "toy", chunk, pick) for name, (chunk, pick) in HR.PICKS.items()] + [("cfg4", "cfg4", 2, [1, 2, 0])]
_stores = {}


def store_of(name, chunk):
    from hetersumgraph_amd.resident import DocumentStore
    if (name, chunk) not in _stores:
        docs = {"toy": HR.hdsg_docs, "work": HR.work_docs}[name]() if name != "cfg4" else R.case_docs(name)
        _stores[name, chunk] = (docs, DocumentStore.from_doc_arrays(docs, DEV, chunk=chunk))
    return _stores[name, chunk]


def same(a, b, what):
    b = torch.as_tensor(b)
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8)), what


def view_of(G):
    """The eighteen outputs as the batch carries them, named as the header names them."""
    lay, hl = G._rel_cache[KEYS[0]], G._rel_cache[KEYS[1]]
    out = {k: lay[k.replace("64", "")] for k in HR.DICT}
    out.update({k: getattr(hl, k) for k in HR.HEAD}, inv_cnt=lay["inv_cnt"])
    assert hl.inv_cnt is lay["inv_cnt"]
    return out, lay, hl


@pytest.mark.parametrize("cid,name,chunk,pick", CASES, ids=[c[0] for c in CASES])
def test_doc_view_is_the_restatement_and_todays(cid, name, chunk, pick):
    from hetersumgraph_amd import HiGraph
    docs, store = store_of(name, chunk)
    assert store.doc_view and store.doc_view_reason is None and store.model_view
    G, index = store.batch(pick, doc_view=True)
    got, lay, hl = view_of(G)
    want = HR.doc_view(docs, index)
    T = R.todays_batch([docs[i] for i in index]).to(DEV)
    today = HR.todays(T)
    for k in HR.OUTPUTS:
        same(got[k], want[k], (cid, k, "restatement"))
        same(got[k], today[k], (cid, k, "today"))
    tl = HiGraph._hdsg_head_layout(T)
    assert lay["n_docs"] == today["n_docs"] and hl.ok and today["ok"]
    assert (hl.n_s, hl.n_docs, hl.n_super) == (tl.n_s, tl.n_docs, tl.n_super)
    assert set(vars(hl)) == set(vars(tl))
    # what the model's accessors now return
    assert HiGraph._hdsg_layout(G) is lay and HiGraph._hdsg_head_layout(G) is hl
    # and the batch itself is the batch without the doc view
    for flag in (False, None):                              # None: the store's default
        G0, index0 = store.batch(pick, doc_view=flag)
        on = flag is None and store.DOC_VIEW
        assert index0 == index and G0.model_inputs is not None and all((k in G0._rel_cache) == on for k in KEYS)
        for k in ("words", "position", "label", "id", "unit", "dtype"):
            assert torch.equal(G.ndata[k], G0.ndata[k]), k
    G0, _ = store.batch(pick, model_view=False, doc_view=True)       # the doc view rides on the model view
    assert G0.model_inputs is None and not any(k in G0._rel_cache for k in KEYS)


def test_the_loader_passes_the_switch_on():
    from hetersumgraph_amd.resident import ResidentLoader
    docs, store = store_of("toy", 4)
    for flag in (True, False):
        G, _ = next(iter(ResidentLoader(store, 3, doc_view=flag)))
        assert all((k in G._rel_cache) == flag for k in KEYS)


# ---- work lists sized on the host ---------------------------------------------------------------------
WORK_PICKS = {  # name -> (pick, per kind the sides that carry a list)
    "pmin": ([0], {"W2S": ["dwork"], "S2W": ["swork"]}),                  # a doc node of 40 word edges, P = 32
    "mean": ([1], {"W2S": ["dwork"], "S2W": ["swork"]}),                  # destinations of 40 and 100: P = 70
    "both": ([0, 1], {"W2S": ["dwork"], "S2W": ["swork"]}),               # the same store, P = 32: the 40 splits too
    "multiple": ([2, 3], {"W2S": ["dwork"], "S2W": ["swork"]}),           # 64 = 2 * P
    "none": ([3, 4], {"W2S": [], "S2W": []}),
}


def sync_error(fn):
    """``fn()`` under torch's synchronisation check: its result, or the RuntimeError of the first host wait."""
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn(), None
    except RuntimeError as e:
        return None, e
    finally:
        torch.cuda.set_sync_debug_mode(mode)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
@pytest.mark.parametrize("name", sorted(WORK_PICKS))
def test_work_lists_are_todays_without_the_read_back(name):
    docs, store = store_of("work", 4)
    pick, sides = WORK_PICKS[name]
    store.batch(pick, doc_view=True)                         # warm-up: the allocator's blocks
    (G, index), err = sync_error(lambda: store.batch(pick, doc_view=True))
    assert err is None
    G0, _ = store.batch(pick, doc_view=False)                # today's path, with its read-back
    T = R.todays_batch([docs[i] for i in index]).to(DEV)
    assert G.resident_work_lists == G0.resident_work_lists == {k: bool(v) for k, v in sides.items()}
    for kind, have in sides.items():
        d, d0, dt = (g._rel_cache[("rel", kind, str(DEV))].dev for g in (G, G0, T))
        for key, ptr in (("dwork", "indptr"), ("swork", "cindptr")):
            assert (key in d) == (key in d0) == (key in dt) == (key in have), (kind, key)
            if key not in have:
                continue
            same(d[key], d0[key], (kind, key, "doc view off"))
            same(d[key], dt[key], (kind, key, "today's batch"))
            items, count = HR.rel_work(np.diff(d[ptr].cpu().numpy()), 32, 1)
            w = d[key].cpu().numpy()
            assert count > 0 and w.shape == (5 * count,) and np.array_equal(w[:4 * count].reshape(-1, 4), items)
            assert not w[4 * count:].any()                   # the arrival counters
    if name != "none":
        _, err = sync_error(lambda: store.batch(pick, doc_view=False))
        assert err is not None                               # the check sees the read-back this removes


def test_two_picks_of_one_store_have_different_piece_lengths():
    docs, store = store_of("work", 4)
    n_items = {}
    for name in ("mean", "both"):
        G, _ = store.batch(WORK_PICKS[name][0], doc_view=True)
        rel = G._rel_cache[("rel", "W2S", str(DEV))]
        n_items[name] = (rel.dev["dwork"].numel() // 5, rel.n_dst)
    assert n_items["mean"] == (3, 2)                         # P = 70: only the 100 splits, in two
    assert n_items["both"] == (9 + 1 + 1 + 1 + 3, 9)         # P = 32: three of 40 -> 2 each, 100 -> 4


# ---- the models on the examples that need work lists --------------------------------------------------
def make_model(embed_train=False):
    from test_gpu_resident_view import make_model as mk
    return mk("HSumDocGraph", embed_train)


COMBOS = [(lstm, cnn) for lstm in ("1", "2") for cnn in ("0", "dw")]


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
@pytest.mark.parametrize("lstm,cnn", COMBOS, ids=["lstm%s-cnn_%s" % c for c in COMBOS])
def test_a_step_on_a_fresh_hdsg_batch_waits_for_nothing(lstm, cnn):
    """With the doc view: batch assembly (work lists included), forward, loss, backward and the
    optimizer step of HSumDocGraph complete under torch's synchronisation check.  Without it the
    same sequence raises: the check sees the waits this removes."""
    from hetersumgraph_amd import optim, rng
    from hetersumgraph_amd._lib import path_options
    from test_gpu_resident_view import step, switches
    docs, store = store_of("work", 2)
    model = make_model()
    adam = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-4, max_grad_norm=1.0)
    rng.manual_seed(5)
    fresh = [0, 1, 3]

    def run(view):
        G, _ = store.batch(fresh, doc_view=view)
        assert any(G.resident_work_lists.values()) and all((k in G._rel_cache) == view for k in KEYS)
        return step(model, adam, G)

    with path_options(**switches(lstm, "0", cnn)):
        for view in (True, False):
            G, _ = store.batch([2, 3, 4], doc_view=view)                  # warm-up on another pick
            step(model, adam, G)
            adam.zero_grad()
            out, err = sync_error(lambda: run(view))
            if view:
                assert err is None, err
                logits, loss = out
            else:
                assert err is not None
            adam.zero_grad()
            torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss))


GLUE_OFF = dict(HSG_SENT_LSTM="1", HSG_MODEL_GLUE="0", HSG_WORD_EMBED="0", HSG_SENT_CNN="0")
# glue off is the torch path reading the int64 dict: its index_add accumulates with atomics, so
# that pick holds doc nodes of at most two sentences (a + b is b + a; a third term has an order)
RESULT_CASES = [("glue_on", None, [0, 1, 2]), ("glue_off", GLUE_OFF, [1, 2, 3, 4])]


@pytest.mark.parametrize("cid,opts,pick", RESULT_CASES, ids=[c[0] for c in RESULT_CASES])
def test_results_are_unchanged(cid, opts, pick):
    """Doc view on against off, and against today's batch of the same members: logits, loss and
    every parameter gradient, bitwise."""
    from test_gpu_resident_view import assert_bitwise, run_once, switches
    docs, store = store_of("work", 2)
    opts = switches("2", "0", "dw") if opts is None else opts
    index = store.batch(pick)[1]
    assert max(np.bincount(HR.local(docs[i])["pair_d"]).max() for i in index) <= (2 if cid == "glue_off" else 3)
    on = run_once("HSumDocGraph", docs, lambda: store.batch(pick, doc_view=True)[0], opts, False)
    off = run_once("HSumDocGraph", docs, lambda: store.batch(pick, doc_view=False)[0], opts, False)
    today = run_once("HSumDocGraph", docs, lambda: R.todays_batch([docs[i] for i in index]).to(DEV), opts, False)
    assert_bitwise(on, off, "doc view on / off")
    assert_bitwise(on, today, "doc view on / today's batch")
    assert bool(on["logits"].abs().sum() > 0)


@pytest.mark.parametrize("how", sorted(HR.REFUSALS))
def test_a_declined_store_runs_todays_code_with_todays_errors(how):
    from hetersumgraph_amd._lib import path_options
    from hetersumgraph_amd.resident import DocumentStore
    from test_gpu_resident_view import switches
    docs = HR.hdsg_docs()[:4]
    docs[3] = HR.broken(docs[3], how)
    store = DocumentStore.from_doc_arrays(docs, DEV, chunk=2)          # builds, as it does today
    assert store.doc_view is False and store.doc_view_reason.startswith("document 3:")
    assert HR.REFUSALS[how] in store.doc_view_reason and store.model_view
    # the fallback is the torch path, whose index_add accumulates with atomics: the pick holds doc
    # nodes of at most two sentences, as test_results_are_unchanged's glue-off case does
    for flag in (None, True, False):
        G, index = store.batch([0, 3], doc_view=flag)
        assert G.model_inputs is not None and not any(k in G._rel_cache for k in KEYS)
    T = R.todays_batch([docs[i] for i in index]).to(DEV)
    model = make_model().eval()
    outcome = []
    with path_options(**switches("2", "0", "dw")), torch.no_grad():
        for g in (T, G):
            try:
                outcome.append(model(g))
            except (AssertionError, KeyError) as e:
                outcome.append((type(e), e.args))
    if torch.is_tensor(outcome[0]):
        assert how == "supernodes" and torch.equal(outcome[0].view(torch.int32), outcome[1].view(torch.int32))
    else:
        assert how != "supernodes" and outcome[0] == outcome[1]


def test_a_write_to_the_unit_column_drops_the_doc_view():
    from test_gpu_resident_view import assert_bitwise, run_once, switches
    docs, store = store_of("work", 2)
    pick, opts = [0, 2, 3], switches("2", "0", "dw")
    index = store.batch(pick)[1]

    def write(G):
        G.ndata["unit"] = G.ndata["unit"].clone()

    G, _ = store.batch(pick, doc_view=True)
    assert all(k in G._rel_cache for k in KEYS)
    write(G)
    assert not any(k in G._rel_cache for k in KEYS) and G.model_inputs is None
    G, _ = store.batch(pick, doc_view=True)
    G.ndata["words"] = G.ndata["words"].clone()             # the doc view goes with the rest of the view
    assert not any(k in G._rel_cache for k in KEYS) and ("rel", "W2S", str(DEV)) in G._rel_cache
    got = run_once("HSumDocGraph", docs, lambda: store.batch(pick, doc_view=True)[0], opts, False, write)
    today = run_once("HSumDocGraph", docs, lambda: R.todays_batch([docs[i] for i in index]).to(DEV), opts, False, write)
    assert_bitwise(got, today, "after the write")
