"""Guard bands and poison around every buffer the doc view's entry point writes
(include/hsg_resident_hdsg.h), with the machinery of tests/test_gpu_guard_bands.py as
tests/test_gpu_resident_guard.py uses it: each case runs once on ``guard.guarded`` outputs of
EXACTLY the documented size and once on plain tensors, and the shared body asserts the bands
intact, every documented element written, the two runs bitwise equal and the values exactly
those of the contract's numpy restatement (tests/resident_hdsg_ref.py).  The store is
tests/resident_ref.py's, uploaded, with the doc view's columns beside it: these cases do not go
through hetersumgraph_amd/resident.py.

CASES is this header's table (tests/test_resident_hdsg_cpu.py checks that every writing entry
point has a case).  The pick lists: one example of one doc node and one sentence; three doc
nodes of unequal sentence counts; a repeated slot; every toy example in another order over build
chunks of 2; slots outside the store (empty documents); the cfg4 examples; and 300 examples,
more than one block per family walks in one stride."""
import ctypes

import numpy as np
import pytest
import torch

import resident_hdsg_ref as HR
import resident_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`
from test_gpu_resident_guard import exact, outputs

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
PICKS = {  # name -> (documents, build chunk, pick list)
    "one": ("toy", 4, [0]),
    "three_docs": ("toy", 4, [1]),
    "repeat": ("toy", 2, [2, 2, 1, 2]),
    "shuffled": ("toy", 2, [4, 6, 2, 0, 5, 3, 1]),
    "outside": ("toy", 2, [1, 9, -1, 3]),
    "all_outside": ("toy", 2, [7, -2]),
    "cfg4": ("cfg4", 2, [1, 2, 0]),
    "many300": ("toy", 4, [i % 7 for i in range(300)]),
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
    name, chunk, slots = PICKS[pick]
    if (name, chunk) not in _stores:
        docs = HR.hdsg_docs() if name == "toy" else R.case_docs(name)
        _stores[name, chunk] = (docs, R.build_store(docs, chunk), HR.store_columns(docs))
    docs, store, cols = _stores[name, chunk]
    cs, keep = R.upload(store, "cuda")
    mk.keep.append(keep)
    ints = lambda a: mk.ints(torch.from_numpy(np.ascontiguousarray(a)))
    dcols = {k: ints(v) for k, v in cols.items()}
    cstruct = _lib.HsgResHdsgCols(**{k: P(v) for k, v in dcols.items()})
    mk.keep.append(cstruct)
    base = HR.bases(docs, slots)
    return (docs, cs, cstruct, slots, ints(np.asarray(slots, np.int32)), ints(R.offsets(store, slots)), ints(base[0]),
            ints(base[1]))


@case("hsg_res_hdsg", *[dict(pick=k) for k in PICKS])
def c_res_hdsg(lib, mk, pick):
    docs, cs, cols, slots, dpick, offs, docbase, pairbase = operands(mk, pick)
    want = HR.doc_view(docs, slots)
    o = outputs(mk, want, HR.OUTPUTS)
    n = [len(want[k]) for k in ("sent_super", "inv_cnt", "pair_s", "super_pos")]
    call(lib, "hsg_res_hdsg", ctypes.byref(cs), ctypes.byref(cols), len(slots), P(dpick), P(offs), P(docbase),
         P(pairbase), *n, *[P(o[k]) for k in HR.OUTPUTS])
    if pick == "all_outside":
        assert n == [0, 0, 0, 0] and want["doc_ptr"].tolist() == [0]
    return {k: (exact(want[k]), 0, 0) for k in HR.OUTPUTS}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_resident_hdsg_guard_bands(fn, kw):
    run_case(fn, kw)
