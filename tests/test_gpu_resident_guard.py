"""Guard bands and poison around every buffer the resident store's entry points write
(include/hsg_resident.h), with the machinery of tests/test_gpu_guard_bands.py: each case runs
once on ``guard.guarded`` outputs of EXACTLY the documented size and once on plain tensors,
and the shared body asserts the bands intact, every documented element written, the two runs
bitwise equal and the values exactly those of the contract's numpy restatement
(tests/resident_ref.py).  The store itself is the restatement's, uploaded: these cases do not
go through hetersumgraph_amd/resident.py.

CASES is this header's table (tests/test_resident_abi.py checks that every writing entry point
has a case).  The pick lists: one document; every document in shuffled order over build chunks
of 2; a repeated slot; slots outside the store (empty documents); documents whose columns are
empty (no word node: no source / destination of one kind; no typed edge at all); and 257 tiny
documents, one past the offsets kernel's scan tile."""
import ctypes

import numpy as np
import pytest
import torch

import resident_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
PICKS = {  # name -> (documents, build chunk, pick list)
    "one": ("jitter", 2, [3]),
    "shuffled": ("jitter", 2, [4, 2, 0, 3, 1]),
    "repeat": ("jitter", 2, [1, 1, 4, 1]),
    "outside": ("jitter", 2, [1, 7, -1, 3]),
    "extremes": ("extremes", 4, [1, 0, 5, 3, 2, 4, 0]),
    "nowords": ("extremes", 4, [3]),
    "notyped": ("extremes", 4, [4]),
    "hdsg": ("cfg4", 2, [1, 2, 0]),
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
        _stores[name, chunk] = R.build_store(R.case_docs(name), chunk)
    store = _stores[name, chunk]
    cs, keep = R.upload(store, "cuda")
    mk.keep.append(keep)
    return store, ctypes.byref(cs), slots, mk.ints(torch.tensor(slots, dtype=torch.int32))


def exact(want):
    def check(got):
        got = got.contiguous().numpy()
        assert got.dtype == want.dtype, (got.dtype, want.dtype)
        assert np.array_equal(got.reshape(want.shape), want)
    return check


TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32,
         np.dtype(np.uint8): torch.uint8}


def outputs(mk, want, names):
    """One guarded output per array of ``want``, exactly its size; 2-D arrays keep their rows."""
    outs = {}
    for k in names:
        w = want[k]
        rows, cols = (w.shape if w.ndim == 2 else (1, w.shape[0]))
        outs[k] = mk.out(k, rows, cols, TORCH[w.dtype])
    return outs


@case("hsg_res_offsets", *[dict(pick=k) for k in ("one", "shuffled", "outside", "extremes", "tiny257")])
def c_res_offsets(lib, mk, pick):
    store, cs, slots, dpick = operands(mk, pick)
    want = R.offsets(store, slots)
    offs = mk.out("offs", R.NFAM, len(slots) + 1, torch.int64)
    call(lib, "hsg_res_offsets", cs, len(slots), P(dpick), P(offs))
    return {"offs": (exact(want), 0, 0)}


GRAPH_OUTS = ("unit", "ndtype", "id", "words", "position", "label", "src", "dst", "tffrac", "edtype")


@case("hsg_res_graph", *[dict(pick=k) for k in PICKS])
def c_res_graph(lib, mk, pick):
    store, cs, slots, dpick = operands(mk, pick)
    want = R.graph(store, slots)
    offs = mk.ints(torch.from_numpy(R.offsets(store, slots)))
    o = outputs(mk, want, GRAPH_OUTS)
    call(lib, "hsg_res_graph", cs, len(slots), P(dpick), P(offs), len(want["unit"]), len(want["src"]),
         *[P(o[k]) for k in GRAPH_OUTS])
    return {k: (exact(want[k]), 0, 0) for k in GRAPH_OUTS}


@case("hsg_res_relation", *[dict(pick=k, kind=q) for k in PICKS for q in (0, 1)])
def c_res_relation(lib, mk, pick, kind):
    store, cs, slots, dpick = operands(mk, pick)
    want = R.relation(store, kind, slots)
    offs = mk.ints(torch.from_numpy(R.offsets(store, slots)))
    o = outputs(mk, want, R.REL_ARRAYS)
    call(lib, "hsg_res_relation", cs, kind, len(slots), P(dpick), P(offs), len(want["src_nodes"]),
         len(want["dst_nodes"]), len(want["src"]), *[P(o[k]) for k in R.REL_ARRAYS])
    if pick == "notyped":
        assert len(want["src"]) == 0 and len(want["indptr"]) >= 1
    if pick == "nowords":
        assert len(want["src_nodes" if kind == 0 else "dst_nodes"]) == 0
    return {k: (exact(want[k]), 0, 0) for k in R.REL_ARRAYS}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_resident_guard_bands(fn, kw):
    run_case(fn, kw)
