"""Guard bands and poison around every buffer the LSTM training-path entry points write
(include/hsg_lstm_train.h), with the machinery of tests/test_gpu_guard_bands.py: each case
runs once on ``guard.guarded`` outputs of EXACTLY the documented size -- the pack buffer at
``hsg_lstm_pack_floats``, dW_ih [M, in], dW_hh [ndir, G, hid], db [M] and the workspace at
exactly ``hsg_lstm_dw_ws_floats`` -- with ``guard.poisoned_input`` operands (x and h with a
row pitch wider than their rows, NaN in the pad and around every input), once on plain
tensors, and the shared body asserts the bands intact, the inputs bitwise unchanged, every
documented element written, nothing NaN and the two runs bitwise equal.  h_prev is read in
place, so a read of the row before the first or after the last row of h would bring the
poison in.  Values: hsg_lstm_pack bit for bit against tests/lstm_train_ref.py, hsg_lstm_dw
under the rule of tests/test_gpu_lstm_train.py (4 x the fp32 CPU error on the same inputs).

CASES is this header's table (tests/test_lstm_train_abi.py checks that every writing entry
point has a case).
"""
import ctypes

import numpy as np
import pytest
import torch

import lstm_train_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
PAD = 8


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


def bits_equal(want):
    want = np.ascontiguousarray(want)

    def check(got):
        got = got.contiguous().numpy().reshape(want.shape)
        assert got.dtype == want.dtype
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    return check


@case("hsg_lstm_pack", dict(layers=2, ndir=2, inp=300), dict(layers=1, ndir=1, inp=4), dict(layers=4, ndir=2, inp=256))
def c_pack(lib, mk, layers, ndir, inp):
    rng = np.random.default_rng(21)
    shapes = []
    for layer in range(layers):
        in_l = inp if layer == 0 else ndir * R.HID
        shapes += [(R.G, in_l), (R.G, R.HID), (R.G,), (R.G,)] * ndir
    params = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    dev = [mk.inp(torch.from_numpy(q)) for q in params]
    n = lib.hsg_lstm_pack_floats(layers, R.HID, ndir, inp)
    out = mk.out("out", 1, n)
    call(lib, "hsg_lstm_pack", layers, R.HID, ndir, inp, (ctypes.c_void_p * len(dev))(*[P(q) for q in dev]), P(out))
    return {"out": (bits_equal(R.pack_ref(params, layers, ndir, inp)), 0, 0)}


@case("hsg_lstm_dw", *[dict(name=k) for k in R.CASES], dict(name="one_doc_one_step", rows=0),
      dict(name="unidirectional", docs=0))
def c_dw(lib, mk, name, rows=None, docs=None):
    lens, inp, ndir = R.CASES[name]
    dg, x, h = R.random_operands(name)
    if rows == 0:
        lens, dg, x, h = [0], dg[:0], x[:0], h[:0]
    n, M = sum(lens), ndir * R.G
    n_docs = len(lens) if docs is None else docs
    nws = lib.hsg_lstm_dw_ws_floats(n, ndir, inp)
    assert nws == R.ws_floats(n, ndir, inp)
    ws = mk.scratch("ws", nws)
    dwih, dwhh, db = mk.out("dW_ih", M, inp), mk.out("dW_hh", M, R.HID), mk.out("db", 1, M)
    off = mk.ints(torch.from_numpy(R.doc_offsets(lens).astype(np.int32)))
    t = torch.from_numpy
    xd = mk.inp(t(x), pitch=inp + PAD) if n else None
    hd = mk.inp(t(h), pitch=ndir * R.HID + PAD) if n else None
    call(lib, "hsg_lstm_dw", n_docs, n, R.HID, ndir, inp, P(off), P(mk.inp(t(dg))) if n else None, P(xd),
         xd.stride(0) if n else inp, P(hd), hd.stride(0) if n else ndir * R.HID, P(ws), P(dwih), P(dwhh), P(db))
    if docs == 0:                                        # no document: nothing is summed
        dg = np.zeros_like(dg)
    r64, r32 = R.dw_ref(dg, x, h, lens, ndir), R.dw_f32(dg, x, h, lens, ndir)

    def check(i, nm):
        def fn(got):
            R.within_yardstick(f"{name} {nm}", got.numpy(), r64[i], r32[i])
            if n == 0 or docs == 0:
                assert not got.numpy().any() and not np.signbit(got.numpy()).any()
        return fn
    return {"dW_ih": (check(0, "dW_ih"), 0, 0), "dW_hh": (check(1, "dW_hh"), 0, 0), "db": (check(2, "db"), 0, 0)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_lstm_train_guard_bands(fn, kw):
    run_case(fn, kw)
