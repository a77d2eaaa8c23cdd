"""The doc view of a resident batch without a GPU (include/hsg_resident_hdsg.h): the numpy
restatement (tests/resident_hdsg_ref.py) equals, for any pick list, what today's code builds on
``graph.batch`` of the same members -- ``HiGraph._hdsg_layout`` and ``head.HeadLayout``; the
store's per-document columns are the restatement's; the host's work-list count rule equals a
restatement of ``k_rel_work``; the build-time validation names the document it declines;
refusals return HSG_EINVAL before any launch; the struct mirror equals the header; and every
writing entry point of the header has a guard-band case."""
import ctypes

import numpy as np
import pytest

import abi
import resident_hdsg_ref as HR
import resident_ref as R

HEADER = "hsg_resident_hdsg.h"
CASES = [("toy", [p for _, p in HR.PICKS.values()]), ("cfg4", [[1, 2, 0], [2]])]


def docs_of(name):
    return HR.hdsg_docs() if name == "toy" else R.case_docs(name)


@pytest.mark.parametrize("name,picks", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_todays_constructions(name, picks):
    docs = docs_of(name)
    for pick in picks:
        got = HR.doc_view(docs, pick)
        want = HR.todays(R.todays_batch([docs[s] for s in pick]))
        assert want["ok"] and want["n_docs"] == len(got["inv_cnt"]) > 0
        for k in HR.OUTPUTS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (pick, k, got[k].shape, want[k].shape)
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{pick} {k}")
        assert np.array_equal(got["inv_cnt"].view(np.int32), want["inv_cnt"].view(np.int32))
        base = HR.bases(docs, pick)
        assert base[0, -1] == len(got["inv_cnt"]) and base[1, -1] == len(got["pair_s"])


def test_a_pick_outside_the_documents_is_an_empty_document():
    docs = docs_of("toy")
    a, b = HR.doc_view(docs, [1, 9, -1, 3]), HR.doc_view(docs, [1, 3])
    for k in HR.OUTPUTS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert HR.bases(docs, [1, 9, -1, 3])[0].tolist() == [0, 3, 3, 3, 6] and HR.bases(docs, [1, 3])[0].tolist() == [0, 3, 6]


def test_the_toy_documents_hold_the_edge_cases():
    docs = docs_of("toy")
    assert HR.counts(docs[0]) == (1, 2, 1, 1)
    c = HR.local(docs[1])
    assert np.diff(np.append(c["doc_ptr"], len(c["doc_sent"]))).tolist() == [4, 1, 2]
    c = HR.local(docs[2])                                   # a sentence of two docs, a pair listed twice
    assert len(c["pair_s"]) == 5 + 4 and np.diff(np.append(c["sent_ptr"], len(c["sent_doc"]))).tolist() == [2, 2, 1, 1, 3]
    assert c["doc_super"][0] == c["doc_row"][1] and c["doc_super"][4] == c["doc_row"][1]      # the last pair wins


def test_the_stores_columns_are_the_restatements():
    from hetersumgraph_amd.resident import HDSG_COLUMNS, doc_view_local
    assert sorted(k for fam in HDSG_COLUMNS.values() for k in fam) == sorted(HR.COLUMNS)
    for name in ("toy", "cfg4"):
        for no, d in enumerate(docs_of(name)):
            reason, got = doc_view_local(d, no)
            want = HR.local(d)
            assert reason is None and got.keys() == want.keys()
            for k in want:
                assert got[k].dtype == want[k].dtype, k
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} {no} {k}")


@pytest.mark.parametrize("how", sorted(HR.REFUSALS))
def test_validation_declines_naming_the_document(how):
    from hetersumgraph_amd.resident import doc_view_local
    reason, cols = doc_view_local(HR.broken(docs_of("toy")[3], how), 17)
    assert cols is None and reason.startswith("document 17:") and HR.REFUSALS[how] in reason


# ---- the work lists' size on the host -------------------------------------------------------------------
def long_of(deg, above=32):
    deg = np.asarray(deg, np.int64)
    return deg[deg > above]


DEGREES = {  # name -> (segment lengths, the piece length they give with PIECE_MIN 32, PIECE_MULT 1)
    "none_long": ([5, 32, 7, 0, 31], 32),
    "pmin": ([40, 5, 5, 5, 5, 5, 33], 32),                  # P equal to PIECE_MIN
    "mean": ([40, 100], 70),                                # P equal to the mean: only the 100 splits
    "multiple": ([64, 96, 3, 3, 3, 3, 3, 3], 32),           # degrees that are exact multiples of P
    "multiple_of_mean": ([140, 70, 0], 70),
    "just_above": ([33, 1, 1], 32),
    "empty": ([], 32),
}


@pytest.mark.parametrize("name", sorted(DEGREES))
def test_the_host_count_is_k_rel_works(name):
    from hetersumgraph_amd.resident import needs_work_list, work_items
    deg, P = DEGREES[name]
    n, E = len(deg), int(sum(deg))
    assert n == 0 or max(32, -(-E // n)) == P
    items, count = HR.rel_work(deg, 32, 1)
    assert work_items(n, E, long_of(deg), 32, 1) == count
    assert (count > 0) == needs_work_list(n, E, max(deg, default=0), 32, 1)
    assert count <= n + 2 * E // 32 + 1                      # today's capacity
    if name == "mean":
        assert count == 3 and items[:, 0].tolist() == [0, -2, -2] and items[1:, 1:3].tolist() == [[40, 90], [90, 140]]
    if name == "multiple":
        assert count == 8 + 1 + 2
    if name in ("none_long", "empty"):
        assert count == 0


def test_the_host_count_over_random_degree_lists():
    from hetersumgraph_amd.resident import work_items
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(300):
        n = int(rng.integers(1, 40))
        deg = rng.integers(0, int(rng.choice([8, 40, 200, 600])), size=n)
        if rng.random() < 0.3:
            deg[rng.integers(0, n)] = int(rng.integers(100, 2000))
        for pmin, mult in ((32, 1), (32, 2), (48, 1), (64, 3)):
            count = HR.rel_work(deg, pmin, mult)[1]
            assert work_items(n, int(deg.sum()), long_of(deg), pmin, mult) == count, (deg.tolist(), pmin, mult)
            assert count <= n + 2 * int(deg.sum()) // pmin + 1
            seen.add(count > 0)
    assert seen == {True, False}
    assert work_items(5, 1000, [900], 0, 1) == 0 and work_items(0, 0, [], 32, 1) == 0        # lists off / no nodes
    with pytest.raises(ValueError, match="kept threshold"):
        work_items(5, 1000, [900], 16, 1)                    # segments of 17 .. 32 were not kept


def test_the_kept_lengths_are_the_documents_long_segments():
    from hetersumgraph_amd.relation import PIECE_MIN
    from hetersumgraph_amd.resident import doc_counts, long_segments
    docs = HR.work_docs()
    for d in docs:
        lng, kept = doc_counts(d)[1], long_segments(d)
        for q in range(2):
            for side in range(2):
                assert (kept[q][side] > PIECE_MIN).all()
                assert kept[q][side].max(initial=0) == (lng[q, side] if lng[q, side] > PIECE_MIN else 0)
    assert sorted(long_segments(docs[1])[0][0].tolist()) == [40, 100] and not len(long_segments(docs[3])[0][0])
    assert long_segments(docs[2])[0][0].tolist() == [64, 64] and long_segments(docs[2])[1][1].tolist() == [64, 64]


# ---- the C ABI --------------------------------------------------------------------------------------
def test_supported_limits():
    from hetersumgraph_amd import _lib
    lib, top = _lib.load(), 2 ** 31 - 1
    for args, want in (((1, 0, 0, 0, 0), 1), ((1 << 20, top, top, top, top), 1), ((0, 1, 1, 1, 1), 0),
                       (((1 << 20) + 1, 1, 1, 1, 1), 0), ((1, top + 1, 0, 0, 0), 0), ((1, 0, top + 1, 0, 0), 0),
                       ((1, 0, 0, top + 1, 0), 0), ((1, 0, 0, 0, top + 1), 0), ((1, -1, 0, 0, 0), 0), ((1, 0, -1, 0, 0), 0),
                       ((1, 0, 0, -1, 0), 0), ((1, 0, 0, 0, -1), 0), ((32, 1440, 96, 1440, 1536), 1)):
        assert bool(lib.hsg_res_hdsg_supported(*args)) == bool(want), args


N_OUT = len(HR.OUTPUTS)
ALWAYS = [HR.OUTPUTS.index(k) for k in ("doc_ptr", "sent_ptr", "sup_ptr")]


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands for
    a non-NULL device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p, top = _lib.load(), _lib.HSG_EINVAL, 16, 2 ** 31 - 1
    names = [f[0] for f in _lib.HsgResHdsgCols._fields_]

    def store(**kw):
        f = dict(n_docs=4, starts=p, bases=p, sent_len=8, label_len=5)
        f.update(kw)
        return ctypes.byref(_lib.HsgResStore(**f))

    def cols(**kw):
        return ctypes.byref(_lib.HsgResHdsgCols(**dict({k: p for k in names}, **kw)))

    def view(st=None, c=None, B=2, pick=p, offs=p, docbase=p, pairbase=p, n=(5, 2, 5, 7), outs=None):
        outs = [p] * N_OUT if outs is None else outs
        return lib.hsg_res_hdsg(store() if st is None else st, cols() if c is None else c, B, pick, offs, docbase,
                                pairbase, *n, *outs, None)
    drop = lambda i: [None if j == i else p for j in range(N_OUT)]
    assert lib.hsg_res_hdsg(None, cols(), 2, p, p, p, p, 5, 2, 5, 7, *[p] * N_OUT, None) == EINVAL
    for kw in [dict(B=0), dict(B=-1), dict(B=(1 << 20) + 1), dict(pick=None), dict(offs=None), dict(docbase=None),
               dict(pairbase=None), dict(st=store(starts=None)), dict(st=store(bases=None)),
               dict(st=store(n_docs=0)), dict(st=store(n_docs=top + 1))] + \
              [dict(n=tuple(bad if j == i else v for j, v in enumerate((5, 2, 5, 7)))) for i in range(4) for bad in (-1, top + 1)] + \
              [dict(c=cols(**{k: None})) for k in names] + [dict(outs=drop(i)) for i in range(N_OUT)]:
        assert view(**kw) == EINVAL, kw
    assert lib.hsg_res_hdsg(store(), None, 2, p, p, p, p, 5, 2, 5, 7, *[p] * N_OUT, None) == EINVAL
    # the three pointer arrays hold their closing element even in a batch of nothing
    for i in ALWAYS:
        assert view(n=(0, 0, 0, 0), outs=drop(i)) == EINVAL


def test_the_struct_mirror_equals_the_header():
    from hetersumgraph_amd import _lib
    assert list(_lib.HsgResHdsgCols._fields_) == abi.mirror_fields(HEADER, "hsg_res_hdsg_cols")
    assert [f[0] for f in _lib.HsgResHdsgCols._fields_] == ["dstart", "pstart"] + list(HR.COLUMNS)


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_resident_hdsg_guard import CASES as GUARD
    w = abi.writable_entry_points([HEADER])
    assert list(w) == ["hsg_res_hdsg"] and len(w["hsg_res_hdsg"]) == N_OUT == 18
    declared = [prm.split("*")[1] for prm in w["hsg_res_hdsg"]]
    assert declared == list(HR.OUTPUTS)                      # the restatement names every output, in order
    missing = sorted(n for n in w if n not in GUARD)
    assert not missing, f"no guard-band case: {missing}"
    assert set(GUARD) <= set(w) and all(GUARD.values())


def test_the_registry_lists_the_header():
    from hetersumgraph_amd import _lib
    assert _lib.exports(HEADER) == ("hsg_res_hdsg_supported", "hsg_res_hdsg")


# ---- head.HeadLayout.prebuilt ---------------------------------------------------------------------------
def test_a_prebuilt_head_layout_is_the_constructed_one():
    import torch
    from hetersumgraph_amd import HiGraph, head
    docs = docs_of("toy")
    G = R.todays_batch([docs[s] for s in (2, 1, 0)])
    want = HiGraph._hdsg_head_layout(G)
    lists = {k: getattr(want, k) for k in head.HeadLayout.INT_LISTS}
    got = head.HeadLayout.prebuilt(want.n_s, want.n_docs, want.n_super, want.inv_cnt, **lists)
    assert (got.n_s, got.n_docs, got.n_super, got.ok) == (want.n_s, want.n_docs, want.n_super, True) and want.ok
    assert set(vars(got)) == set(vars(want))
    for k in lists:
        assert getattr(got, k) is lists[k]
    for bad in (dict(doc_ptr=lists["doc_ptr"][:-1]), dict(sent_doc=lists["sent_doc"].long()),
                dict(sup_list=lists["sup_list"][:-1])):
        with pytest.raises(ValueError):
            head.HeadLayout.prebuilt(want.n_s, want.n_docs, want.n_super, want.inv_cnt, **dict(lists, **bad))
    with pytest.raises(ValueError):
        head.HeadLayout.prebuilt(want.n_s, want.n_docs, want.n_super + 1, want.inv_cnt, **lists)
    with pytest.raises(ValueError):
        head.HeadLayout.prebuilt(want.n_s, want.n_docs, want.n_super, want.inv_cnt.double(), **lists)
    with pytest.raises(ValueError):
        head.HeadLayout.prebuilt(want.n_s, want.n_docs, want.n_super, want.inv_cnt, **{k: v for k, v in lists.items() if k != "sup_ptr"})
    assert torch.equal(got.inv_cnt, want.inv_cnt)
