"""Guard bands and poison around every buffer the word-embedding entry points write
(include/hsg_embed.h), with the machinery of tests/test_gpu_guard_bands.py: each case runs
once on ``guard.guarded`` outputs of EXACTLY the documented size -- dE [V, D], the workspace
at exactly ``hsg_embed_ws_floats``, Xw with a row pitch larger than D -- with
``guard.poisoned_input`` source matrices of wider pitch, once on plain tensors, and the
shared body asserts the bands intact, the inputs bitwise unchanged, every documented
element written, the pad columns untouched, nothing NaN and the two runs bitwise equal.
The values are checked bit for bit against the order contract's numpy restatement and
against fp64 within the derived bound (tests/embed_ref.py).

CASES is this header's table (tests/test_embed_abi.py checks that every writing entry point
has a case).
"""
import numpy as np
import pytest
import torch

import embed_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
V = R.V_CASE
PAD = 8


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


@case("hsg_embed_rows", dict(D=4), dict(D=300))
def c_embed_rows(lib, mk, D):
    g = torch.Generator().manual_seed(5)
    E = torch.randn(V, D, generator=g)
    wid = torch.tensor([3, V - 1, 0, 3, 11, 36, 1, 20, 20], dtype=torch.int64)
    Ed = mk.inp(E)
    Xw = mk.out("Xw", len(wid), D, pitch=D + PAD)
    call(lib, "hsg_embed_rows", len(wid), V, D, P(mk.ints(wid)), P(Ed), P(Xw), Xw.stride(0))

    def bitwise(got):
        assert torch.equal(got.contiguous().view(torch.int32), E[wid].view(torch.int32))
    return {"Xw": (bitwise, 0, 0)}


@case("hsg_embed_keys", dict(pad=0), dict(pad=None), dict(pad=0, words=0), dict(pad=0, sents=0))
def c_embed_keys(lib, mk, pad, words=1, sents=1):
    L = 9
    ids = torch.tensor([[5, 6, 7, 8, 0, 0, 0, 0, 0], [9, 0, 0, 0, 0, 0, 0, 0, 0], [3, 3, 4, 5, 6, 7, 8, 36, 2],
                        [6, 6, 6, 6, 6, 6, 0, 0, 0]], dtype=torch.int64)[:4 * sents]
    wid = torch.tensor([2, 3, 0, 5, 6, 36, 8, 9, 36, 11, 6], dtype=torch.int64)[:11 * words]
    n, n_w = ids.shape[0], wid.shape[0]
    rowoff = torch.zeros(n + 1, dtype=torch.int32)
    rowoff[1:] = torch.cumsum((ids != 0).sum(1) + 1, 0)
    rows = int(rowoff[-1])
    out = mk.out("keys", 1, n_w + rows, dtype=torch.int64)
    call(lib, "hsg_embed_keys", n_w, n, L, rows, P(mk.ints(wid)) if n_w else None, P(mk.ints(ids)) if n else None,
         P(mk.ints(rowoff)), -1 if pad is None else pad, P(out))
    want = R.keys_unsorted(np.concatenate([wid.numpy(), R.cnn_tokens(ids.numpy())]), pad)

    def check(got):
        assert np.array_equal(got.contiguous().numpy().reshape(-1), want)
    return {"keys": (check, 0, 0)}


@case("hsg_embed_grad", dict(kind="mixed", D=4), dict(kind="mixed", D=300), dict(kind="heavy", D=4),
      dict(kind="no_words", D=4), dict(kind="no_rows", D=4), dict(kind="empty", D=4))
def c_embed_grad(lib, mk, kind, D):
    Pc = lib.hsg_embed_piece_rows()
    c = R.grad_case(Pc, kind, D, padding_idx=0)
    n_w, rows = len(c["tok_w"]), len(c["tok_c"])
    keys = R.keys_of(np.concatenate([c["tok_w"], c["tok_c"]]), 0)
    n_occ = len(keys)
    dW = mk.inp(torch.from_numpy(c["dW"]), pitch=D + PAD) if n_w else None
    dX = mk.inp(torch.from_numpy(c["dX"]), pitch=D + 2 * PAD, plain_pitch=D + 4) if rows else None
    dE = mk.out("dE", V, D)
    n_ws = lib.hsg_embed_ws_floats(n_occ, D)
    assert n_ws == 2 * D * -(-n_occ // Pc)
    ws = mk.scratch("ws", n_ws)
    call(lib, "hsg_embed_grad", V, D, n_occ, P(mk.ints(torch.from_numpy(keys))) if n_occ else None, n_w, P(dW),
         dW.stride(0) if n_w else 0, rows, P(dX), dX.stride(0) if rows else 0, P(dE), P(ws))
    want, ref, bound = R.case_reference(c, Pc, 0)

    def check(got):
        got = got.contiguous().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    return {"dE": (check, 0, 0)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_embed_guard_bands(fn, kw):
    run_case(fn, kw)
