"""Guard bands and poison around every buffer the model-glue entry points write
(include/hsg_model.h), with the machinery of tests/test_gpu_guard_bands.py: each case runs
once on ``guard.guarded`` outputs of EXACTLY the documented size (row pitches larger than
the widths) with ``guard.poisoned_input`` inputs, once on plain tensors, and the shared
body asserts the bands intact, the inputs bitwise unchanged, every documented element
written, the pad columns untouched, nothing NaN, the two runs bitwise equal and the values
against the fp64 restatement (tests/head_ref.py).

CASES is this header's table (tests/test_model_abi.py checks that every writing entry
point has a case).  Shapes: 9 rows -- not a multiple of the 4 rows of a block -- with L a
strided view, both LSTM widths; the HDSG layouts with docs of 1, 2 and 7 sentences and
with a doc whose sentences interleave with another's.
"""
import pytest
import torch

import head_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


TOL = (2e-5, 2e-5)                           # atol, rtol: a value check; tests/test_gpu_head.py holds the tight bound
N = 9
PAD = 8


def _dims(Lw):
    return (300, 128, Lw, 64)


@case("hsg_sentfeat_fwd", dict(Lw=256), dict(Lw=128))
def c_sentfeat_fwd(lib, mk, Lw):
    E, Fn, _, Hs = dims = _dims(Lw)
    c = R.sent_case(N, dims)
    assert N % lib.hsg_sentfeat_rows() != 0
    ngram, L = mk.inp(c["ngram"], pitch=E + PAD), mk.inp(c["L"].contiguous(), pitch=Lw + 24, plain_pitch=Lw + 4)
    X, F, S = mk.out("X", N, E, pitch=E + PAD), mk.out("F", N, 2 * Fn, pitch=2 * Fn + PAD), mk.out("S", N, Hs, pitch=Hs + PAD)
    call(lib, "hsg_sentfeat_fwd", N, E, Fn, Lw, Hs, R.N_POS, P(ngram), ngram.stride(0), P(mk.ints(c["pos"])),
         P(mk.inp(c["P"])), P(L), L.stride(0), P(mk.inp(c["Wc"])), P(mk.inp(c["bc"])), P(mk.inp(c["Wl"])),
         P(mk.inp(c["bl"])), P(mk.inp(c["Wn"])), P(X), X.stride(0), P(F), F.stride(0), P(S), S.stride(0))
    r = R.sent_features(c, torch.float64)
    return {"X": (r["x"], *TOL), "F": (r["F"], *TOL), "S": (r["S"], *TOL)}


@case("hsg_sentfeat_bwd", dict(Lw=256), dict(Lw=128))
def c_sentfeat_bwd(lib, mk, Lw):
    E, Fn, _, Hs = dims = _dims(Lw)
    c = R.sent_case(N, dims)
    dS = mk.inp(c["dS"], pitch=Hs + PAD)
    dF, dng, dL = (mk.out("dF", N, 2 * Fn, pitch=2 * Fn + PAD), mk.out("dngram", N, E, pitch=E + PAD),
                   mk.out("dL", N, Lw, pitch=Lw + PAD))
    call(lib, "hsg_sentfeat_bwd", N, E, Fn, Lw, Hs, P(dS), dS.stride(0), P(mk.inp(c["Wc"])), P(mk.inp(c["Wl"])),
         P(mk.inp(c["Wn"])), P(dF), dF.stride(0), P(dng), dng.stride(0), P(dL), dL.stride(0))
    r = R.sent_features(c, torch.float64)
    return {"dF": (r["dF"], *TOL), "dngram": (r["dngram"], *TOL), "dL": (r["dL"], *TOL)}


def _head_layout(lay):
    from hetersumgraph_amd.head import HeadLayout
    h = HeadLayout(lay["pair_s"], lay["pair_d"], lay["n_s"], lay["n_docs"], lay["super_pos"], lay["sent_super"],
                   lay["doc_super"], lay["inv_cnt"], "cuda")
    assert h.ok
    return h


HDSG = (dict(layout="docs_1_2_7"), dict(layout="interleaved"), dict(layout="doc_after_sentences"))


@case("hsg_docinit_fwd", *HDSG)
def c_docinit_fwd(lib, mk, layout):
    lay = R.LAYOUTS[layout]
    h, c, Hs = _head_layout(lay), R.doc_case(lay), 64
    S = mk.inp(c["S"], pitch=Hs + PAD)
    mean, init = mk.out("mean", h.n_docs, Hs), mk.out("init", h.n_super, Hs, pitch=Hs + PAD)
    call(lib, "hsg_docinit_fwd", h.n_s, h.n_docs, h.n_super, Hs, P(S), S.stride(0), P(h.super_src), P(h.doc_ptr),
         P(h.doc_sent), P(mk.inp(torch.from_numpy(lay["inv_cnt"]))), P(mk.inp(c["Wd"])), P(mean), P(init), init.stride(0))
    r = R.doc_init(c, lay, torch.float64)
    return {"mean": (r["mean"], *TOL), "init": (r["init"], *TOL)}


@case("hsg_docinit_bwd", *HDSG)
def c_docinit_bwd(lib, mk, layout):
    lay = R.LAYOUTS[layout]
    h, c, Hs = _head_layout(lay), R.doc_case(lay), 64
    r = R.doc_init(c, lay, torch.float64)
    dInit = mk.inp(c["dInit"], pitch=Hs + PAD)
    dS, dWd = mk.out("dS", h.n_s, Hs, pitch=Hs + PAD), mk.out("dWd", Hs, Hs)
    call(lib, "hsg_docinit_bwd", h.n_s, h.n_docs, h.n_super, Hs, P(dInit), dInit.stride(0), P(h.sent_row), P(h.doc_row),
         P(h.sent_ptr), P(h.sent_doc), P(mk.inp(torch.from_numpy(lay["inv_cnt"]))), P(mk.inp(c["Wd"])),
         P(mk.inp(r["mean"].float())), P(dS), dS.stride(0), P(dWd))
    return {"dS": (r["dS"], *TOL), "dWd": (r["dWd"], *TOL)}


LOGITS = (dict(layout="hsg"),) + HDSG


def _logit_case(layout):
    if layout == "hsg":
        return None, None, R.hsg_case(70)
    lay = R.LAYOUTS[layout]
    return lay, _head_layout(lay), R.doc_case(lay)


@case("hsg_logits_fwd", *LOGITS)
def c_logits_fwd(lib, mk, layout):
    lay, h, c = _logit_case(layout)
    n_super, Hs = c["state"].shape
    n = h.n_s if h else n_super
    state = mk.inp(c["state"], pitch=Hs + PAD)
    out = mk.out("logits", 1, 2 * n)
    call(lib, "hsg_logits_fwd", n, Hs, n_super, P(state), state.stride(0), P(h.sent_super) if h else None,
         P(h.doc_super) if h else None, P(mk.inp(c["Wh"])), P(mk.inp(c["bh"])), P(out))
    return {"logits": (R.logits(c, lay, torch.float64)["logits"].reshape(1, -1), *TOL)}


@case("hsg_logits_bwd", *LOGITS)
def c_logits_bwd(lib, mk, layout):
    lay, h, c = _logit_case(layout)
    n_super, Hs = c["state"].shape
    n = h.n_s if h else n_super
    W = c["Wh"].shape[1]
    state = mk.inp(c["state"], pitch=Hs + PAD)
    nb = lib.hsg_logits_bwd_blocks(n)
    assert nb == -(-n // 64)
    dstate, ws = mk.out("dstate", n_super, Hs, pitch=Hs + PAD), mk.scratch("ws", nb * (2 * W + 2))
    dWh, dbh = mk.out("dWh", 1, 2 * W), mk.out("dbh", 1, 2)
    call(lib, "hsg_logits_bwd", n, Hs, n_super, P(mk.inp(c["dlogits"].reshape(1, -1))), P(state), state.stride(0),
         P(h.sent_super) if h else None, P(h.doc_super) if h else None, P(h.sup_sent) if h else None,
         P(h.sup_ptr) if h else None, P(h.sup_list) if h else None, P(mk.inp(c["Wh"])), P(dstate), dstate.stride(0), P(ws),
         P(dWh), P(dbh))
    r = R.logits(c, lay, torch.float64)
    return {"dstate": (r["dstate"], *TOL), "dWh": (r["dWhb"][:2 * W].reshape(1, -1), *TOL),
            "dbh": (r["dWhb"][2 * W:].reshape(1, -1), *TOL)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_model_guard_bands(fn, kw):
    run_case(fn, kw)
