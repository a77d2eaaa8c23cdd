"""The eval view of a resident batch without a GPU (include/hsg_resident_eval.h): the header's
declarations are the registry's and its struct the ctypes mirror's; refusals return HSG_EINVAL
before any launch; the numpy restatement (tests/resident_eval_ref.py) equals
``evalsel.pack_words`` of the picked documents; ``eval_view_local`` accepts ``word_ids``'
output and names why it declines anything else; the store's cached seen-set rule equals
``pack_words(...).tab_cap``; and the writing entry point has a guard-band case."""
import ctypes
import types

import numpy as np
import pytest

import abi
import resident_eval_ref as ER
import resident_ref as R

HEADER = "hsg_resident_eval.h"
PICKS = ([6, 4], [0], [3], [1, 1, 4, 1], [4, 6, 2, 0, 5, 3, 1], [0, 0])


# ---- the C ABI --------------------------------------------------------------------------------------
def test_the_registry_lists_the_header():
    from hetersumgraph_amd import _lib
    assert _lib.exports(HEADER) == ("hsg_res_eval_supported", "hsg_res_eval")
    assert set(abi.declared_functions(HEADER)) == set(abi.declarations(HEADER)) == set(_lib.ABI[HEADER])
    for name, args in _lib.ABI[HEADER].items():
        restype, argtypes = abi.signature(HEADER, name)
        assert args == argtypes and _lib.RESTYPE.get(name, ctypes.c_int) == restype == ctypes.c_int, name
    lib = _lib.load()
    assert lib.hsg_res_eval.argtypes == _lib.ABI[HEADER]["hsg_res_eval"]


def test_the_struct_mirror_equals_the_header():
    from hetersumgraph_amd import _lib
    assert list(_lib.HsgResEvalCols._fields_) == abi.mirror_fields(HEADER, "hsg_res_eval_cols")
    assert [f[0] for f in _lib.HsgResEvalCols._fields_] == list(ER.COLUMNS)


def test_supported_limits():
    from hetersumgraph_amd import _lib
    lib, top = _lib.load(), 2 ** 31 - 1
    for args, want in (((1, 0, 0), 1), ((1 << 20, 5, 7), 1), ((0, 1, 1), 0), (((1 << 20) + 1, 1, 1), 0), ((-1, 1, 1), 0),
                       ((1, -1, 0), 0), ((1, 0, -1), 0), ((32, 1440, 32000), 1),
                       # the pack's n_sent + 1 + max(n_words, 1) elements
                       ((1, top - 2, 0), 1), ((1, top - 2, 1), 1), ((1, top - 1, 0), 0), ((1, top - 1, 1), 0),
                       ((1, 0, top - 1), 1), ((1, 0, top), 0), ((1, 1, top - 2), 1), ((1, 1, top - 1), 0),
                       ((1, top, 0), 0), ((1, top + 1, 0), 0), ((1, 0, top + 1), 0), ((1, 2 ** 62, 2 ** 62), 0)):
        assert bool(lib.hsg_res_eval_supported(*args)) == bool(want), args


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands for
    a non-NULL device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p, top = _lib.load(), _lib.HSG_EINVAL, 16, 2 ** 31 - 1

    def store(**kw):
        f = dict(n_docs=4, starts=p, bases=p, sent_len=8, label_len=5)
        f.update(kw)
        return ctypes.byref(_lib.HsgResStore(**f))

    def cols(**kw):
        return ctypes.byref(_lib.HsgResEvalCols(**dict({k: p for k in ER.COLUMNS}, **kw)))

    def view(st=None, c=None, B=2, pick=p, offs=p, wordbase=p, n=(5, 9), pack=p):
        return lib.hsg_res_eval(store() if st is None else st, cols() if c is None else c, B, pick, offs, wordbase, *n,
                                pack, None)
    assert lib.hsg_res_eval(None, cols(), 2, p, p, p, 5, 9, p, None) == EINVAL
    assert lib.hsg_res_eval(store(), None, 2, p, p, p, 5, 9, p, None) == EINVAL
    for kw in [dict(B=0), dict(B=-1), dict(B=(1 << 20) + 1), dict(pick=None), dict(offs=None), dict(wordbase=None),
               dict(pack=None), dict(st=store(starts=None)), dict(st=store(bases=None)), dict(st=store(n_docs=0)),
               dict(st=store(n_docs=top + 1)), dict(n=(-1, 9)), dict(n=(5, -1)), dict(n=(top - 1, 1)), dict(n=(0, top)),
               dict(n=(top + 1, 0)), dict(c=cols(wstart=None)), dict(c=cols(wend=None)), dict(c=cols(wid=None)),
               dict(c=cols(wstart=None), n=(0, 0)), dict(c=cols(wend=None), n=(1, 0)), dict(c=cols(wid=None), n=(0, 1))]:
        assert view(**kw) == EINVAL, kw


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_resident_eval_guard import CASES as GUARD
    w = abi.writable_entry_points([HEADER])
    assert w == {"hsg_res_eval": ["int32_t *pack"]}
    assert set(GUARD) == set(w) and all(GUARD.values())


# ---- the restatement ------------------------------------------------------------------------------------
def test_the_word_lists_hold_the_edge_cases():
    docs = ER.eval_docs()
    words = ER.word_lists(docs)
    lens = [np.diff(p) for p, _ in words]
    assert [len(x) for x in lens] == [1, 40, 3, 4, 2, 1, 5] == [len(d.sent_nodes) for d in docs]
    assert len(words[0][1]) == 0 and len(words[4][1]) == 1 and len(words[6][1]) == 3000
    assert {0, 1} <= set(lens[1].tolist()) and lens[1].max() > 1


@pytest.mark.parametrize("pick", PICKS, ids=lambda p: "-".join(map(str, p)))
def test_restatement_equals_pack_words(pick):
    from hetersumgraph_amd.evalsel import pack_words
    docs = ER.eval_docs()
    words, store = ER.word_lists(docs), R.build_store(docs, 2)
    counts = [len(docs[s].sent_nodes) for s in pick]
    want = pack_words([words[s] for s in pick], counts, pin=False)
    got = ER.eval_pack(store, words, pick)
    assert got.dtype == np.int32 and np.array_equal(got, want.buf.numpy())
    assert len(got) == want.n + 1 + max(want.W, 1) and ER.wordbase(words, pick)[-1] == want.W
    if pick in ([0], [0, 0]):
        assert want.W == 0 and len(got) == want.n + 2 and got[-1] == 0


def test_a_pick_outside_the_documents_is_an_empty_document():
    docs = ER.eval_docs()
    words, store = ER.word_lists(docs), R.build_store(docs, 2)
    assert np.array_equal(ER.eval_pack(store, words, [2, 7, -1, 5]), ER.eval_pack(store, words, [2, 5]))
    assert ER.wordbase(words, [2, 7, -1, 5]).tolist() == [0, 8, 8, 8, 12]


# ---- the build-time validation ----------------------------------------------------------------------
def test_eval_view_local_accepts_word_ids():
    from hetersumgraph_amd.evalsel import word_ids
    from hetersumgraph_amd.resident import eval_view_local
    sents = ["a b c a", "", "c  d", "e"]
    for n in (4, 6, 2, 0):                                   # as given, rows beyond the article, an article cut at n
        ptr, ids = word_ids(sents, n)
        got = eval_view_local([(ptr, ids)], n)
        assert isinstance(got, dict) and sorted(got) == ["lens", "wend", "wid"]
        assert got["wend"].dtype == got["wid"].dtype == np.int32 and got["lens"].dtype == np.int64
        assert got["wend"].tolist() == ptr[1:].tolist() and got["wid"].tolist() == ids.tolist()
        assert got["lens"].tolist() == np.diff(ptr).tolist()
    assert eval_view_local([word_ids(sents, 6)], 6)["lens"].tolist() == [4, 0, 2, 1, 0, 0]
    assert eval_view_local([word_ids(sents, 2)], 2)["wid"].tolist() == [0, 1, 2, 0]
    assert isinstance(eval_view_local([[[0, 2], [5, 5]]], 1), dict)                   # plain lists of ints serve


def test_eval_view_local_names_the_reason():
    from hetersumgraph_amd.evalsel import word_ids
    from hetersumgraph_amd.resident import eval_view_local
    ptr, ids = word_ids(["a b", "c"], 2)
    i32 = lambda *a: np.asarray(a, np.int32)
    for entry, n, why in (([[3, 4]], 2, "one-dimensional integer arrays"),            # a fake entry
                          ([(ptr, ids), (ptr, ids)], 2, "2 parts"),
                          ([], 2, "0 parts"),
                          ((ptr, ids), 2, "2 parts"),                                # the pair itself, not a list of one
                          ([(ptr, ids)], 3, "3 elements for 3 sentence rows"),       # a wrong row count
                          ([(ptr, ids)], 1, "3 elements for 1 sentence rows"),
                          ([(i32(0, 3, 2, 3), i32(0, 1, 2))], 3, "decreases"),
                          ([(i32(0, 2, 2), i32(0, 1, 2))], 2, "ends at 2 for 3 word ids"),
                          ([(i32(1, 2, 3), i32(0, 1, 2))], 2, "begins at 1"),
                          ([(ptr.astype(np.float32), ids)], 2, "integer arrays"),
                          ([(ptr, ids.astype(np.float64))], 2, "integer arrays"),
                          ([(i32(0, 1), np.asarray([2 ** 31]))], 1, "does not fit int32"),
                          ([(ptr, ids, ids)], 2, "not a (ptr, ids) pair"),
                          (None, 2, "NoneType")):
        got = eval_view_local(entry, n)
        assert isinstance(got, str) and why in got, (entry, got)


# ---- the seen set's size ------------------------------------------------------------------------------
def test_the_cached_rule_is_pack_words_tab_cap():
    from hetersumgraph_amd.evalsel import pack_words
    from hetersumgraph_amd.resident import ResidentWordPack, seen_columns, seen_need
    rng = np.random.default_rng(3)
    n_docs = 9
    lens = [rng.integers(0, 40, int(rng.integers(1, 12))) for _ in range(n_docs)]
    lens[2][:] = 0
    lens.append(np.asarray([0, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0]))                    # exactly n_win words, for every n_win
    lens.append(np.zeros(0, np.int64))                                              # a document without a row
    n_docs = len(lens)
    parts = [(np.concatenate([[0], np.cumsum(x)]).astype(np.int32), np.zeros(int(np.sum(x)), np.int32)) for x in lens]
    cols, calls = seen_columns(lens), []
    cache = {}

    def need(n_win, m):
        if (n_win, m) not in cache:
            calls.append((n_win, m))
            cache[n_win, m] = seen_need(*cols, n_docs, n_win, m)
        return cache[n_win, m]
    store = types.SimpleNamespace(seen_need=need)
    seen = set()
    for pick in ([0], [9], [10], [2, 2], [9, 3, 10], list(range(n_docs)), [5, 1, 5, 8]):
        counts = [len(lens[s]) for s in pick]
        want = pack_words([parts[s] for s in pick], counts, pin=False)
        got = ResidentWordPack(None, want.n, want.B, want.W, counts, store, np.asarray(pick))
        for n_win in range(1, 9):
            for m in range(0, 7):
                assert got.win_need(n_win, m) == want.win_need(n_win, m), (pick, n_win, m)
                assert got.tab_cap(n_win, m) == want.tab_cap(n_win, m), (pick, n_win, m)
                seen.add(want.tab_cap(n_win, m))
    assert len(calls) == 8 * 7 and len(seen) > 2 and 64 in seen                   # once per pair over the whole store
