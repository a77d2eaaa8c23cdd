"""The resident store's assembly without a GPU: the numpy restatement (tests/resident_ref.py,
written from include/hsg_resident.h) gives, for any pick list, exactly ``graph.batch`` of the
``to_graph`` members and exactly the relation of the concatenated batch -- the check that
per-document relations, kept chunk-relative with their bases, concatenate to the batch's.
Also the host restatement of the work-list rule, the batch order and ResidentLoader's index
bookkeeping."""
import numpy as np
import pytest
import torch

import resident_ref as ref

CASES = [  # documents, build chunk, pick lists (store slots in batch order)
    ("jitter", 2, [[0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3], [1, 1, 4, 1]]),
    ("extremes", 4, [[0, 1, 2, 3, 4, 5], [3, 4], [4], [1, 0, 5, 3, 2, 4, 0]]),
    ("cfg1", 2, [[2, 0, 1]]),
    ("cfg4", 2, [[1, 2, 0], [2]]),
    ("cfg5", 3, [[0, 2]]),
]

_stores = {}


def store_of(name, chunk):
    if (name, chunk) not in _stores:
        docs = ref.case_docs(name)
        _stores[name, chunk] = (docs, ref.build_store(docs, chunk))
    return _stores[name, chunk]


@pytest.mark.parametrize("name,chunk,picks", CASES, ids=[c[0] for c in CASES])
def test_graph_columns_equal_graph_batch(name, chunk, picks):
    docs, store = store_of(name, chunk)
    for pick in picks:
        got = ref.graph(store, pick)
        g = ref.todays_batch([docs[s] for s in pick])
        assert set(g.ndata.keys()) == {"unit", "dtype", "id", "words", "position", "label"}
        assert set(g.edata.keys()) == {"tffrac", "dtype"}
        for k, col in (("unit", g.ndata["unit"]), ("ndtype", g.ndata["dtype"]), ("id", g.ndata["id"]),
                       ("words", g.ndata["words"]), ("position", g.ndata["position"]), ("label", g.ndata["label"]),
                       ("tffrac", g.edata["tffrac"]), ("edtype", g.edata["dtype"])):
            want = col.numpy()
            assert got[k].dtype == want.dtype and got[k].shape == want.shape, (pick, k)
            np.testing.assert_array_equal(got[k], want, err_msg=f"{pick} {k}")
        np.testing.assert_array_equal(got["src"], g._src, err_msg=str(pick))
        np.testing.assert_array_equal(got["dst"], g._dst, err_msg=str(pick))


@pytest.mark.parametrize("name,chunk,picks", CASES, ids=[c[0] for c in CASES])
def test_relations_concatenate_to_the_batch_relation(name, chunk, picks):
    docs, store = store_of(name, chunk)
    for pick in picks:
        for q, kind in enumerate(ref.KINDS):
            got = ref.relation(store, q, pick)
            want = ref.batch_relation(kind, [docs[s] for s in pick])
            for k in ref.REL_ARRAYS:
                assert got[k].shape == want[k].shape, (pick, kind, k)
                np.testing.assert_array_equal(got[k].astype(np.int64), np.asarray(want[k]).astype(np.int64),
                                              err_msg=f"{pick} {kind} {k}")


def test_tiny_documents_across_a_scan_tile():
    docs, store = store_of("tiny257", 100)
    pick = list(range(257))
    got = ref.relation(store, 0, pick)
    want = ref.batch_relation("W2S", docs)
    for k in ref.REL_ARRAYS:
        np.testing.assert_array_equal(got[k].astype(np.int64), np.asarray(want[k]).astype(np.int64), err_msg=k)
    offs = ref.offsets(store, pick)
    assert offs.shape == (ref.NFAM, 258) and (offs[:, 0] == 0).all()
    np.testing.assert_array_equal(offs[ref.NODE, 1:], np.cumsum([d.n_nodes for d in docs]))


def test_a_pick_outside_the_store_is_an_empty_document():
    docs, store = store_of("jitter", 2)
    a, b = ref.offsets(store, [1, 7, -1, 3]), ref.offsets(store, [1, 3])
    np.testing.assert_array_equal(a[:, [0, 1, 4]], b)
    np.testing.assert_array_equal(a[:, 1], a[:, 2])
    np.testing.assert_array_equal(a[:, 1], a[:, 3])


def test_work_list_rule():
    from hetersumgraph_amd.resident import needs_work_list
    # P = max(32, 1 * ceil(n_typed / n)): split only a segment LONGER than P
    assert not needs_work_list(10, 100, 32, 32, 1) and needs_work_list(10, 100, 33, 32, 1)
    assert not needs_work_list(2, 100, 50, 32, 1) and needs_work_list(2, 100, 51, 32, 1)
    assert not needs_work_list(2, 101, 51, 32, 1) and needs_work_list(2, 101, 52, 32, 1)      # ceil
    assert needs_work_list(3, 90, 61, 32, 2) and not needs_work_list(3, 90, 60, 32, 2)
    assert not needs_work_list(0, 0, 0, 32, 1) and not needs_work_list(5, 1000, 900, 0, 1)   # no nodes / lists off
    # the defaults are relation.py's
    from hetersumgraph_amd import relation
    assert needs_work_list(4, 8, relation.PIECE_MIN + 1) and not needs_work_list(4, 8, relation.PIECE_MIN)


def test_work_list_rule_on_the_configurations():
    """cfg2 / cfg5 documents have no segment to split; cfg4's doc supernodes have (relation.py)."""
    from hetersumgraph_amd import synth
    from hetersumgraph_amd.resident import doc_counts, needs_work_list
    for cfg, want in (("cfg2", False), ("cfg5", False), ("cfg4", True)):
        docs = synth.make_batch_docs(cfg, seed=2, n_docs=3)
        cl = [doc_counts(d) for d in docs]
        tot = sum(c for c, _ in cl)
        lng = np.max([l for _, l in cl], 0)
        need = False
        for q in range(2):
            need |= needs_work_list(tot[ref.DST(q)], tot[ref.TYP(q)], lng[q, 0])
            need |= needs_work_list(tot[ref.SRC(q)], tot[ref.TYP(q)], lng[q, 1])
            np.testing.assert_array_equal(cl[0][0], ref.counts_of(docs[0]))
            r = ref.batch_relation(ref.KINDS[q], docs)
            assert lng[q, 0] == np.diff(r["indptr"]).max() and lng[q, 1] == np.diff(r["cindptr"]).max()
        assert need == want, cfg


def test_batch_order_is_stable_descending():
    from hetersumgraph_amd.resident import batch_order
    assert batch_order([3, 5, 3, 5, 1, 3]).tolist() == [1, 3, 0, 2, 5, 4]
    assert batch_order([2]).tolist() == [0]


class _FakeStore:
    def __init__(self, indices):
        self.indices = list(indices)
        self.seen = []

    def __len__(self):
        return len(self.indices)

    def batch(self, idx):
        self.seen.append(list(idx))
        return "G", list(idx)


def test_loader_index_bookkeeping():
    from hetersumgraph_amd.resident import ResidentLoader
    st = _FakeStore([10, 11, 12, 13, 14, 15, 16])
    assert [ix for _, ix in ResidentLoader(st, 3)] == [[10, 11, 12], [13, 14, 15], [16]]
    assert len(ResidentLoader(st, 3)) == 3 and len(ResidentLoader(st, 3, drop_last=True)) == 2
    assert [ix for _, ix in ResidentLoader(st, 3, drop_last=True)] == [[10, 11, 12], [13, 14, 15]]
    assert len(ResidentLoader(st, 7, drop_last=True)) == 1 and len(ResidentLoader(st, 8, drop_last=True)) == 0
    assert list(ResidentLoader(st, 8, drop_last=True)) == []
    # shuffled: the permutation is the generator's, every document once, dataset indices
    g = torch.Generator().manual_seed(5)
    got = [ix for _, ix in ResidentLoader(st, 2, shuffle=True, generator=g)]
    perm = torch.randperm(7, generator=torch.Generator().manual_seed(5)).tolist()
    assert [i for b in got for i in b] == [10 + s for s in perm] and [len(b) for b in got] == [2, 2, 2, 1]
    again = [ix for _, ix in ResidentLoader(st, 2, shuffle=True, generator=g)]
    assert sorted(i for b in again for i in b) == st.indices
    with pytest.raises(ValueError):
        ResidentLoader(st, 0)


def test_a_cpu_device_is_refused():
    from hetersumgraph_amd import synth
    from hetersumgraph_amd.resident import DocumentStore
    with pytest.raises(RuntimeError, match="ROCm device"):
        DocumentStore.from_doc_arrays(synth.make_batch_docs("cfg1", n_docs=1), torch.device("cpu"))


def test_narrowing_is_checked():
    from hetersumgraph_amd.resident import _narrow
    assert _narrow(np.array([0.0, 2.0], np.float32), np.uint8, "unit", 0).dtype == np.uint8
    for bad, dt in ((np.array([0.5], np.float32), np.uint8), (np.array([256]), np.uint8), (np.array([-1]), np.uint8),
                    (np.array([2 ** 31]), np.int32)):
        with pytest.raises(ValueError, match="does not fit"):
            _narrow(bad, dt, "x", 3)
