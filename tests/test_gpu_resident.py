"""``DocumentStore.batch`` against today's path -- ``graph.batch`` of the same members in the
returned order, then ``.to(device)`` -- bit for bit: every ndata / edata column, the edge
lists, every array of both relations, the sizes, and whether a work list is attached.  Then
the graph API on the resident batch, the host views, the no-host-wait property (asserted by
construction: the batch is assembled under torch's synchronisation check and carries no work
list), the loader and the refusals."""
import numpy as np
import pytest
import torch

import resident_ref as R
from hetersumgraph_amd import graph as hg
from hetersumgraph_amd import synth
from hetersumgraph_amd.relation import HOT_KINDS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = [  # documents, build chunk, pick lists (dataset indices, in the order given to batch())
    ("jitter", 2, [[0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3], [1, 1, 4, 1]]),
    ("extremes", 4, [[0, 1, 2, 3, 4, 5], [3], [4], [1, 0, 5, 3, 2, 4, 0]]),
    ("cfg1", 2, [[2, 0, 1]]),
    ("cfg4", 2, [[1, 2, 0], [2]]),
    ("cfg5", 3, [[0, 2, 1]]),
    ("tiny257", 100, [list(range(257))]),
]
_stores = {}


def store_of(name, chunk):
    from hetersumgraph_amd.resident import DocumentStore
    if (name, chunk) not in _stores:
        docs = R.case_docs(name)
        _stores[name, chunk] = (docs, DocumentStore.from_doc_arrays(docs, DEV, chunk=chunk))
    return _stores[name, chunk]


def todays(docs, index):
    return R.todays_batch([docs[i] for i in index]).to(DEV)


def assert_same_batch(G, T):
    assert isinstance(G, hg.BatchedDGLGraph) and G.device == T.device
    assert G.number_of_nodes() == T.number_of_nodes() and G.number_of_edges() == T.number_of_edges()
    assert (G.batch_size, list(G.batch_num_nodes), list(G.batch_num_edges)) == \
        (T.batch_size, list(T.batch_num_nodes), list(T.batch_num_edges))
    for view in ("ndata", "edata"):
        g, t = getattr(G, view), getattr(T, view)
        assert set(g.keys()) == set(t.keys())
        for k in t.keys():
            assert g[k].dtype == t[k].dtype and g[k].shape == t[k].shape and g[k].device == t[k].device, (view, k)
            assert torch.equal(g[k], t[k]), (view, k)
    assert torch.equal(G._src_t(), T._src_t()) and torch.equal(G._dst_t(), T._dst_t())
    assert G._src_t().dtype == torch.int64
    for kind in HOT_KINDS:
        a, b = G.relation(kind), T.relation(kind)
        assert (a.n_src, a.n_dst, a.n_typed, a.n_edges_total) == (b.n_src, b.n_dst, b.n_typed, b.n_edges_total), kind
        assert a.host is None and a.device == b.device
        assert set(a.dev) == set(b.dev), (kind, sorted(a.dev), sorted(b.dev))         # dwork / swork too
        assert G.resident_work_lists[kind] == ("dwork" in b.dev or "swork" in b.dev), kind
        for k, v in b.dev.items():
            assert a.dev[k].dtype == v.dtype and a.dev[k].shape == v.shape, (kind, k)
            assert torch.equal(a.dev[k], v), (kind, k)
        ca, cb = a.cstruct(), b.cstruct()
        assert (ca.n_src, ca.n_dst, ca.n_edges, ca.n_dwork, ca.n_swork) == \
            (cb.n_src, cb.n_dst, cb.n_edges, cb.n_dwork, cb.n_swork)


@pytest.mark.parametrize("name,chunk,picks", CASES, ids=[c[0] for c in CASES])
def test_batch_is_todays_batch(name, chunk, picks):
    docs, store = store_of(name, chunk)
    assert len(store) == len(docs) and store.nbytes > 0
    for pick in picks:
        G, index = store.batch(pick)
        n_sent = [len(docs[i].sent_nodes) for i in pick]
        want = [pick[j] for j in np.argsort(-np.asarray(n_sent), kind="stable")]
        assert index == want, "descending sentence count, ties in the order given"
        assert_same_batch(G, todays(docs, index))


def test_work_list_only_where_todays_path_has_one():
    for name, chunk, want in (("cfg4", 2, True), ("cfg5", 3, False), ("cfg1", 2, False)):
        docs, store = store_of(name, chunk)
        G, index = store.batch([0, 1, 2])
        T = todays(docs, index)
        has = any(k in T.relation(kind).dev for kind in HOT_KINDS for k in ("dwork", "swork"))
        assert has == want == any(G.resident_work_lists.values()), name


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_no_host_wait_at_cfg2_and_cfg5_shapes():
    """By construction: the batch is assembled with torch's synchronisation check set to raise
    (a device-to-host copy, a pageable host-to-device copy, an .item() or a synchronise would),
    its relations carry no work list (the one read-back that remains is attach_work_lists'),
    and the pick list went through pinned memory.  Torch's check sees torch's own calls; the
    four C entry points in between only launch (include/hsg_resident.h: no synchronisation)."""
    from hetersumgraph_amd.resident import DocumentStore
    for cfg in ("cfg2", "cfg5"):
        docs = synth.make_batch_docs(cfg, seed=4, n_docs=4)
        store = DocumentStore.from_doc_arrays(docs, DEV, chunk=3)
        store.batch([0, 1])                                     # first use: pinned pool, module load
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            G, index = store.batch([2, 0, 3, 1])
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert G.resident_work_lists == {"W2S": False, "S2W": False}
        for kind in HOT_KINDS:
            assert "dwork" not in G.relation(kind).dev and "swork" not in G.relation(kind).dev
        assert G.to(DEV) is G and G.to("cuda") is G           # already there: nothing moves
        assert_same_batch(G, todays(docs, index))


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_sync_check_sees_todays_path():
    """The check above is not vacuous: today's path trips it."""
    docs = R.case_docs("jitter")
    T = R.todays_batch(docs[:2])
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            T.to(DEV)
    finally:
        torch.cuda.set_sync_debug_mode(mode)


def test_graph_api_on_the_resident_batch():
    for name, chunk, pick in (("jitter", 2, [4, 2, 0, 3, 1]), ("cfg4", 2, [1, 2, 0])):
        docs, store = store_of(name, chunk)
        G, index = store.batch(pick)
        T = todays(docs, index)
        for key in ("unit", "ndtype", "tffrac", "edtype"):
            a, b = G.host_column(key), T.host_column(key)
            assert a.dtype == b.dtype and np.array_equal(a, b), key
        assert np.array_equal(G._src, T._src) and np.array_equal(G._dst, T._dst) and G._src.dtype == np.int64
        snode = lambda g: g.filter_nodes(lambda nodes: nodes.data["dtype"] == 1)
        assert torch.equal(snode(G), snode(T))
        wsedge = lambda g: g.filter_edges(lambda e: (e.src["unit"] == 0) & (e.dst["unit"] == 1))
        assert torch.equal(wsedge(G), wsedge(T))
        for v in (int(snode(T)[0]), int(snode(T)[-1]), 0):
            assert torch.equal(G.predecessors(v), T.predecessors(v))
            assert torch.equal(G.in_edges(v, form="eid"), T.in_edges(v, form="eid"))
        assert torch.equal(G.in_degrees(), T.in_degrees())
        G.ndata["x"] = T.ndata["x"] = torch.arange(G.number_of_nodes(), device=DEV, dtype=torch.float32)[:, None]
        assert torch.equal(hg.sum_nodes(G, "x"), hg.sum_nodes(T, "x"))
        gs, ts = hg.unbatch(G), hg.unbatch(T)
        assert len(gs) == len(ts) == len(pick)
        for a, b in zip(gs, ts):
            assert a.number_of_nodes() == b.number_of_nodes() and np.array_equal(a._src, b._src)
            assert np.array_equal(a._dst, b._dst)
            for k in b.ndata.keys():
                assert torch.equal(a.ndata[k], b.ndata[k]), k
            for k in b.edata.keys():
                assert torch.equal(a.edata[k], b.edata[k]), k


def test_a_structural_write_falls_back_to_the_graphs_own_columns():
    docs, store = store_of("jitter", 2)
    G, index = store.batch([0, 1])
    T = todays(docs, index)
    for g in (G, T):
        unit = g.ndata["unit"].clone()
        unit[0] = 1.0
        g.ndata["unit"] = unit
    assert np.array_equal(G.host_column("unit"), T.host_column("unit")) and G.host_column("unit")[0] == 1.0
    assert np.array_equal(G._src, T._src)
    for kind in HOT_KINDS:                                      # rebuilt by today's builder
        for k, v in T.relation(kind).dev.items():
            assert torch.equal(G.relation(kind).dev[k], v), (kind, k)


def test_loader_iterates_like_the_dataloader():
    from hetersumgraph_amd.resident import DocumentStore, ResidentLoader
    docs = R.case_docs("jitter")
    store = DocumentStore.from_doc_arrays(docs, DEV, chunk=2, indices=[10, 11, 12, 13, 14],
                                          eval_words=[[[i, i + 1]] for i in range(5)])
    by_index = {10 + i: d for i, d in enumerate(docs)}
    seen = []
    for G, index in ResidentLoader(store, 2, shuffle=True, generator=torch.Generator().manual_seed(3)):
        seen += index
        members = [synth.to_graph(by_index[i], hg.DGLGraph) for i in index]
        for m, i in zip(members, index):
            m.eval_words = [[i - 10, i - 9]]
        T = hg.batch(members).to(DEV)
        assert_same_batch(G, T)
        assert G.eval_words == T.eval_words
    assert sorted(seen) == [10, 11, 12, 13, 14]


@pytest.mark.parametrize("kind,seed", [("hsg", 7), ("hdsg", 11)])
def test_from_dataset(tmp_path, kind, seed):
    """``from_dataset`` over an ExampleSet / MultiExampleSet made with ``eval_words=True``: a
    subset of the dataset in another order, built in chunks of 2; every batch equals
    ``graph.batch`` of the dataset's own items, ``G.eval_words`` included."""
    import os

    from graph_data import STOPWORDS, make_files
    from hetersumgraph_amd import build
    from hetersumgraph_amd.module.dataloader import ExampleSet, MultiExampleSet
    from hetersumgraph_amd.resident import DocumentStore, ResidentLoader
    build.build_host(verbose=False)
    d = str(tmp_path / kind)
    vocab = make_files(d, seed=seed, n_examples=6, multi=kind == "hdsg")
    args = [os.path.join(d, "data.jsonl"), vocab, 7, 12, os.path.join(d, "filter_word.txt"), os.path.join(d, "w2s.jsonl")]
    if kind == "hdsg":
        ds = MultiExampleSet(*args, os.path.join(d, "w2d.jsonl"), stopwords=STOPWORDS, eval_words=True)
    else:
        ds = ExampleSet(*args, stopwords=STOPWORDS, eval_words=True)
    store = DocumentStore.from_dataset(ds, DEV, indices=[4, 0, 5, 2, 1], chunk=2)
    assert len(store) == 5 and store.indices == [4, 0, 5, 2, 1]
    seen = []
    for G, index in ResidentLoader(store, 3):
        seen += index
        T = hg.batch([ds[i][0] for i in index]).to(DEV)
        assert_same_batch(G, T)
        assert len(G.eval_words) == len(T.eval_words) == len(index)
        for a, b in zip(G.eval_words, T.eval_words):
            assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    assert sorted(seen) == [0, 1, 2, 4, 5]
    with pytest.raises(IndexError, match="not in the store"):
        store.batch([3])


def test_refusals():
    docs, store = store_of("jitter", 2)
    with pytest.raises(IndexError, match="not in the store"):
        store.batch([0, 5])
    with pytest.raises(IndexError, match="not in the store"):
        store.batch([-1])
    with pytest.raises(ValueError):
        store.batch([])
    from hetersumgraph_amd.resident import DocumentStore
    with pytest.raises(RuntimeError, match="ROCm device"):
        DocumentStore.from_doc_arrays(docs, "cpu")
    import dataclasses
    wide = dataclasses.replace(docs[0], tffrac=docs[0].tffrac + 300)
    with pytest.raises(ValueError, match="does not fit uint8"):
        DocumentStore.from_doc_arrays([wide], DEV)
    moved = dataclasses.replace(docs[0], position=docs[0].position + 1)
    with pytest.raises(ValueError, match="position"):
        DocumentStore.from_doc_arrays([moved], DEV)


def test_a_batch_beyond_supported_is_refused():
    """More than 2^31 - 1 nodes in one batch: refused on the host counts, before any launch
    (the counts are raised for the test; no such batch is assembled)."""
    docs, store = store_of("jitter", 2)
    saved = store.counts.copy()
    try:
        store.counts[:, R.NODE] = 2 ** 30
        with pytest.raises(RuntimeError, match="hsg_res_supported"):
            store.batch([0, 1])
    finally:
        store.counts[:] = saved
    G, index = store.batch([0, 1])
    assert_same_batch(G, todays(docs, index))
