"""Guard bands and poison around every buffer the model view's entry point writes
(include/hsg_resident_model.h), with the machinery of tests/test_gpu_guard_bands.py as
tests/test_gpu_resident_guard.py uses it: each case runs once on ``guard.guarded`` outputs of
EXACTLY the documented size and once on plain tensors, and the shared body asserts the bands
intact, every documented element written, the two runs bitwise equal and the values exactly
those of the contract's numpy restatement (tests/resident_model_ref.py).  The store is
tests/resident_ref.py's, uploaded, with the two new columns beside it: these cases do not go
through hetersumgraph_amd/resident.py.

CASES is this header's table (tests/test_resident_model_cpu.py checks that every writing entry
point has a case).  The pick lists: one one-sentence document; every document in another order
over build chunks of 2; a repeated slot; slots outside the store (empty documents); documents
without a word node or a typed edge; an HDSG batch with doc nodes; the toy documents with a
full and an all-PAD sentence; and 257 tiny documents."""
import numpy as np
import pytest
import torch

import resident_model_ref as MR
import resident_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`
from test_gpu_resident_guard import exact, outputs

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
PICKS = {  # name -> (documents, build chunk, pick list)
    "one": ("extremes", 4, [0]),
    "shuffled": ("jitter", 2, [4, 2, 0, 3, 1]),
    "repeat": ("jitter", 2, [1, 1, 4, 1]),
    "outside": ("jitter", 2, [1, 7, -1, 3]),
    "extremes": ("extremes", 4, [1, 0, 5, 3, 2, 4, 0]),
    "nowords": ("extremes", 4, [3]),
    "hdsg": ("cfg4", 2, [1, 2, 0]),
    "pads": ("model", 2, [2, 1, 4, 0, 3]),
    "tiny257": ("tiny257", 100, list(range(257))),
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
    name, chunk, slots = PICKS[pick]
    if (name, chunk) not in _stores:
        docs = MR.model_docs() if name == "model" else R.case_docs(name)
        _stores[name, chunk] = (docs, R.build_store(docs, chunk))
    docs, store = _stores[name, chunk]
    cs, keep = R.upload(store, "cuda")
    mk.keep.append(keep)
    ints = lambda a: mk.ints(torch.from_numpy(np.ascontiguousarray(a)))
    tok_len, tok_row = MR.view_columns(docs)
    return (docs, store, cs, slots, ints(np.asarray(slots, np.int32)), ints(tok_len), ints(tok_row),
            ints(R.offsets(store, slots)), ints(MR.rowbase(docs, slots)))


@case("hsg_res_model", *[dict(pick=k) for k in PICKS])
def c_res_model(lib, mk, pick):
    import ctypes
    docs, store, cs, slots, dpick, tok_len, tok_row, offs, rowbase = operands(mk, pick)
    want = MR.model_view(docs, slots)
    o = outputs(mk, want, MR.OUTPUTS)
    call(lib, "hsg_res_model", ctypes.byref(cs), P(tok_len), P(tok_row), len(slots), P(dpick), P(offs), P(rowbase),
         len(want["sent_nodes"]), len(want["tfidf_index"]), *[P(o[k]) for k in MR.OUTPUTS])
    return {k: (exact(want[k]), 0, 0) for k in MR.OUTPUTS}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_resident_model_guard_bands(fn, kw):
    run_case(fn, kw)
