"""Guard bands and poison around every buffer the token-path entry points write
(include/hsg_cnn_tokens.h), with the machinery of tests/test_gpu_guard_bands.py: each case runs
once on ``guard.guarded`` outputs of EXACTLY the documented size -- present [V], Tb [U + L + 1,
D], feat / arg [n, 300], dbias [300], the workspace at exactly ``hsg_cnn_tok_dw_ws_floats``,
dWall and Tb with a row pitch larger than D -- with ``guard.poisoned_input`` operands of wider
pitch (TW among them), once on plain tensors, and the shared body asserts the bands intact, the
inputs bitwise unchanged, every documented element written, the pad columns untouched, nothing
NaN and the two runs bitwise equal.  The values are checked bit for bit against the contracts'
numpy restatements (tests/cnn_tokens_ref.py).

CASES is this header's table (tests/test_cnn_tokens_abi.py checks that every writing entry
point has a case).
"""
import ctypes

import numpy as np
import pytest
import torch

import cnn_tokens_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
V = 37
PAD = 8
SHAPES = (dict(D=4, L=7), dict(D=300, L=20))


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


def batch(D, L, n=70):
    """ids [n, L] (lengths 0, 1, 6, L, a repeated token; V - 1 present) and float32 parameters."""
    ids = R.small_ids(n, L, V, 11)
    if n > 5:
        ids[5, 0] = V - 1
    E, Pm, cw, cb = R.params(V, D, L, 12)
    f = np.float32
    return ids, f(E), f(Pm), [f(w) for w in cw], [f(b) for b in cb]


def rowoff_of(ids):
    r = np.zeros(ids.shape[0] + 1, np.int32)
    r[1:] = np.cumsum(R.lengths(ids) + 1)
    return torch.from_numpy(r)


def bits_equal(want):
    want = np.ascontiguousarray(want)

    def check(got):
        got = got.contiguous().numpy().reshape(want.shape)
        assert got.dtype == want.dtype
        iv = {4: np.int32, 8: np.int64}[want.itemsize]
        assert np.array_equal(got.view(iv), want.view(iv))
    return check


@case("hsg_cnn_tok_mark", dict(L=7), dict(L=20), dict(L=7, n=0), dict(L=7, bad=V), dict(L=7, bad=-1))
def c_mark(lib, mk, L, n=70, bad=None):
    ids = R.small_ids(n, L, V, 11)
    if bad is not None:
        ids[3, 2] = bad
    present = mk.out("present", 1, V, dtype=torch.int32, init=torch.zeros(1, V, dtype=torch.int32))
    flag = mk.out("bad", 1, 1, dtype=torch.int32, init=torch.zeros(1, 1, dtype=torch.int32))
    call(lib, "hsg_cnn_tok_mark", n, L, V, P(mk.ints(torch.from_numpy(ids))) if n else None, P(present), P(flag))
    ok = ids.copy()
    if bad is not None:
        ok[3, 2] = 0
    want, _, _ = R.slot_map(ok, V)
    return {"present": (bits_equal(want), 0, 0), "bad": (bits_equal(np.array([int(bad is not None)], np.int32)), 0, 0)}


@case("hsg_cnn_tok_table", *SHAPES, dict(D=4, L=7, n=0))
def c_table(lib, mk, D, L, n=70):
    ids, E, Pm, _, _ = batch(D, L, n)
    present, slot, U = R.slot_map(ids, V)
    Tb = mk.out("Tb", U + L + 1, D, pitch=D + PAD)
    call(lib, "hsg_cnn_tok_table", V, D, U, L, P(mk.ints(torch.from_numpy(present))), P(mk.ints(torch.from_numpy(slot))),
         P(mk.inp(torch.from_numpy(E))), P(mk.inp(torch.from_numpy(Pm))), P(Tb), Tb.stride(0))
    want, U2 = R.table(ids, V, E, Pm)
    assert U2 == U and (n or U == 1)
    return {"Tb": (bits_equal(want), 0, 0)}


@case("hsg_cnn_tok_pool", *SHAPES)
def c_pool(lib, mk, D, L, n=70):
    ids, E, Pm, cw, cb = batch(D, L, n)
    _, slot, U = R.slot_map(ids, V)
    Tb, _ = R.table(ids, V, E, Pm)
    TW = (Tb.astype(np.float64) @ R.stack_taps(cw).astype(np.float64).T).astype(np.float32)
    TWd = mk.inp(torch.from_numpy(TW), pitch=R.NY + 2 + PAD, plain_pitch=R.NY + 2)
    bias = [mk.inp(torch.from_numpy(b)) for b in cb]
    bptr = (ctypes.c_void_p * 6)(*[P(b) for b in bias])
    feat = mk.out("feat", n, R.NF)
    arg = mk.out("arg", n, R.NF, dtype=torch.int32)
    call(lib, "hsg_cnn_tok_pool", n, L, V, U, P(mk.ints(torch.from_numpy(ids))), P(mk.ints(rowoff_of(ids))),
         P(mk.ints(torch.from_numpy(slot))), P(TWd), TWd.stride(0), bptr, P(feat), P(arg))
    wf, wa = R.pool(ids, slot, U, TW, cb)
    return {"feat": (bits_equal(wf), 0, 0), "arg": (bits_equal(wa), 0, 0)}


@case("hsg_cnn_tok_dw", *SHAPES, dict(D=4, L=7, n=0), dict(D=4, L=7, n=64), dict(D=4, L=7, n=129))
def c_dw(lib, mk, D, L, n=70):
    C = lib.hsg_cnn_tok_chunk()
    ids, E, Pm, cw, cb = batch(D, L, max(n, 1))
    ids = ids[:n]
    feat, arg = R.conv_tokens64(ids, V, E, Pm, cw, cb) if n else (np.zeros((0, R.NF)), np.zeros((0, R.NF), np.int32))
    feat = feat.astype(np.float32)
    dfeat = np.random.default_rng(13).standard_normal(feat.shape).astype(np.float32)
    nws = lib.hsg_cnn_tok_dw_ws_floats(n, D)
    assert nws == -(-n // C) * (R.NY * D + R.NF)
    ws = mk.scratch("ws", nws)
    dWall = mk.out("dWall", R.NY, D, pitch=D + PAD)
    dbias = mk.out("dbias", 1, R.NF)
    dev = lambda a: P(mk.ints(torch.from_numpy(np.ascontiguousarray(a)))) if n else None
    call(lib, "hsg_cnn_tok_dw", n, L, V, D, dev(ids), P(mk.ints(rowoff_of(ids))), P(mk.inp(torch.from_numpy(E))),
         P(mk.inp(torch.from_numpy(Pm))), P(mk.inp(torch.from_numpy(feat))) if n else None, dev(arg),
         P(mk.inp(torch.from_numpy(dfeat))) if n else None, P(ws), P(dWall), dWall.stride(0), P(dbias))
    ww, wb = R.dw(ids, E, Pm, feat, arg, dfeat, C)
    if n == 0:
        assert not ww.any() and not np.signbit(ww).any()
    return {"dWall": (bits_equal(ww), 0, 0), "dbias": (bits_equal(wb), 0, 0)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_cnn_tokens_guard_bands(fn, kw):
    run_case(fn, kw)
