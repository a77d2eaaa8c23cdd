"""Guard bands and poison around the buffers the vocabulary path's entry point writes
(include/hsg_cnn_vocab.h), with the machinery of tests/test_gpu_guard_bands.py as
tests/test_gpu_cnn_tokens_guard.py uses it: each case runs once on ``guard.guarded`` outputs of
EXACTLY the documented size -- feat / arg [n, 300] -- with a ``guard.poisoned_input`` TW of wider
pitch (the kernel reads whole rows as 16-byte vectors: the poison in the pad columns must not
reach a value), once on plain tensors, and the shared body asserts the bands intact, the inputs
bitwise unchanged, every documented element written, nothing NaN and the two runs bitwise equal.
The values are checked bit for bit against the contract's numpy restatement
(tests/cnn_tokens_ref.py, with U = V and the identity slot map).

CASES is this header's table (tests/test_cnn_vocab_abi.py checks that every writing entry point
has a case).
"""
import ctypes

import numpy as np
import pytest
import torch

import cnn_tokens_ref as R
from test_gpu_cnn_tokens_guard import PAD, V, batch, bits_equal, rowoff_of
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


@case("hsg_cnn_vocab_pool", dict(D=4, L=7), dict(D=300, L=20), dict(D=4, L=7, n=0))
def c_pool(lib, mk, D, L, n=70):
    ids, E, Pm, cw, cb = batch(D, L, max(n, 1))
    ids = ids[:n]
    Tb = np.concatenate([E, Pm[:L + 1]], 0)
    TW = (Tb.astype(np.float64) @ R.stack_taps(cw).astype(np.float64).T).astype(np.float32)
    TWd = mk.inp(torch.from_numpy(TW), pitch=R.NY + 2 + PAD, plain_pitch=R.NY + 2)
    bias = [mk.inp(torch.from_numpy(b)) for b in cb]
    bptr = (ctypes.c_void_p * 6)(*[P(b) for b in bias])
    feat = mk.out("feat", n, R.NF)
    arg = mk.out("arg", n, R.NF, dtype=torch.int32)
    call(lib, "hsg_cnn_vocab_pool", n, L, V, P(mk.ints(torch.from_numpy(ids))) if n else None, P(mk.ints(rowoff_of(ids))),
         P(TWd), TWd.stride(0), bptr, P(feat), P(arg))      # n = 0: real pointers, nothing written
    wf, wa = R.pool(ids, np.arange(V, dtype=np.int32), V, TW, cb)
    return {"feat": (bits_equal(wf), 0, 0), "arg": (bits_equal(wa), 0, 0)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_cnn_vocab_guard_bands(fn, kw):
    run_case(fn, kw)
