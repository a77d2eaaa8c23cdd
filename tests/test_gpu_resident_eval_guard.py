"""Guard bands and poison around the buffer the eval view's entry point writes
(include/hsg_resident_eval.h), with the machinery of tests/test_gpu_guard_bands.py as
tests/test_gpu_resident_hdsg_guard.py uses it: each case runs once on a ``guard.guarded`` pack
of EXACTLY the documented size and once on a plain tensor, and the shared body asserts the bands
intact, every documented element written, the two runs bitwise equal and the values exactly
those of the contract's numpy restatement (tests/resident_eval_ref.py).  The store is
tests/resident_ref.py's, uploaded, with the eval view's columns beside it: these cases do not go
through hetersumgraph_amd/resident.py.

CASES is this header's table (tests/test_resident_eval_cpu.py checks that the writing entry
point has a case).  The pick lists: one document without a word (n_words == 0: the padding
element); one of a single row; 3,000 words in 5 rows beside a single word; a repeated slot; every
document in another order; slots of -1 and n_docs (empty documents), alone and among others."""
import ctypes

import numpy as np
import pytest
import torch

import resident_eval_ref as ER
import resident_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`
from test_gpu_resident_guard import exact

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
PICKS = {  # name -> (build chunk, pick list)
    "noword": (4, [0]),
    "one": (4, [5]),
    "long_and_single": (2, [6, 4]),
    "repeat": (2, [1, 1, 4, 1]),
    "shuffled": (2, [4, 6, 2, 0, 5, 3, 1]),
    "outside": (2, [2, 7, -1, 5]),
    "all_outside": (2, [7, -1]),
    "nowords_twice": (4, [0, 0]),
}
_stores = {}


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


def operands(mk, pick):
    from hetersumgraph_amd import _lib
    chunk, slots = PICKS[pick]
    if chunk not in _stores:
        docs = ER.eval_docs()
        _stores[chunk] = (R.build_store(docs, chunk), ER.word_lists(docs))
    store, words = _stores[chunk]
    cs, keep = R.upload(store, "cuda")
    mk.keep.append(keep)
    ints = lambda a: mk.ints(torch.from_numpy(np.ascontiguousarray(a)))
    dcols = {k: ints(v) for k, v in ER.store_columns(words).items()}
    cstruct = _lib.HsgResEvalCols(**{k: P(v) for k, v in dcols.items()})
    mk.keep.append(cstruct)
    return (store, words, cs, cstruct, slots, ints(np.asarray(slots, np.int32)), ints(R.offsets(store, slots)),
            ints(ER.wordbase(words, slots)))


@case("hsg_res_eval", *[dict(pick=k) for k in PICKS])
def c_res_eval(lib, mk, pick):
    store, words, cs, cols, slots, dpick, offs, wordbase = operands(mk, pick)
    want = ER.eval_pack(store, words, slots)
    n_sent, n_words = int(R.offsets(store, slots)[R.SENT, -1]), int(ER.wordbase(words, slots)[-1])
    assert len(want) == n_sent + 1 + max(n_words, 1)
    pack = mk.out("pack", 1, len(want), torch.int32)
    call(lib, "hsg_res_eval", ctypes.byref(cs), ctypes.byref(cols), len(slots), P(dpick), P(offs), P(wordbase), n_sent,
         n_words, P(pack))
    if pick in ("noword", "nowords_twice"):
        assert n_words == 0 and n_sent == len(slots) and want.tolist() == [0] * (n_sent + 2)
    if pick == "all_outside":
        assert (n_sent, n_words) == (0, 0) and want.tolist() == [0, 0]
    if pick == "long_and_single":
        assert n_words == 3001
    return {"pack": (exact(want), 0, 0)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_resident_eval_guard_bands(fn, kw):
    run_case(fn, kw)
