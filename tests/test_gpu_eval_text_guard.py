"""Guard bands around every buffer hsg_eval_text_words writes (include/hsg_eval_text.h), with
the machinery of tests/test_gpu_guard_bands.py and the pattern of
tests/test_gpu_eval_words_guard.py: each case runs once on ``guard.guarded`` buffers of EXACTLY
the documented size -- word_ptr [n + 1], word_ids [word_cap] with word_cap the bound and the
bound + 1, ws [hsg_eval_text_workspace_bytes] -- and once on plain tensors, and the shared body
asserts the bands intact, every documented element written, nothing of word_ids at or beyond
word_ptr[n] written, the two runs bitwise equal and the values exactly those of the contract's
restatement (tests/eval_text_ref.py).

The text is read-only; it sits between hostile neighbours: the first row begins with the
continuation bytes of a whitespace sequence and the last one ends with the first bytes of one,
and the bytes before and after the text would complete them -- a read outside [0, nbytes)
changes the split, which is compared with the restatement's.  The ``ptr`` variants hand the
kernel a byte_ptr of negative, oversized and descending values, and one whose rows overlap so
that there are more words than the bound (they are capped there), ``doc`` a doc_off of any
content.

CASES is this header's table (tests/test_eval_text_abi.py checks that every writing entry point
has a case)."""
import numpy as np
import pytest
import torch

import eval_text_ref as R
from test_eval_text_cpu import hand_batch, random_rows
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


@case("hsg_eval_text_words", dict(batch="hand", extra=0), dict(batch="hand", extra=1), dict(batch="random", extra=0),
      dict(batch="random", extra=1), dict(batch="random", extra=0, ptr="wild"), dict(batch="random", extra=0, ptr="overlap"),
      dict(batch="random", extra=1, ptr="overlap"),
      dict(batch="random", extra=0, ptr="descending"), dict(batch="hand", extra=0, doc="wild"),
      dict(batch="full", extra=0))
def c_eval_text_words(lib, mk, batch, extra, ptr=None, doc=None):
    rng = np.random.default_rng(17)
    if batch == "hand":
        rows, off = hand_batch()
    elif batch == "random":
        rows, off = random_rows(rng, 5, 40)
    else:
        rows, off = [b"a", b"b", b"c"], np.asarray([0, 2, 3], np.int32)   # one-byte rows: as many words as the bound
    if batch != "full":
        rows = [b"\x80\xa0x"] + rows + [b"y\xe2\x80"]                      # cut sequences at both ends of the text
        off = np.concatenate([[0], off[1:] + 1, [off[-1] + 2]]).astype(np.int32)
    text, bp = R.pack_rows(rows)
    n, B, nbytes = len(rows), len(off) - 1, len(text)
    if ptr == "wild":
        bp = rng.choice(np.asarray([-2 ** 31, -1, 0, 2, nbytes // 3, nbytes // 2, nbytes - 1, nbytes, nbytes + 1, 2 ** 31 - 1]),
                        n + 1).astype(np.int32)
    elif ptr == "overlap":                                                # every other row is the whole text
        bp = np.where(np.arange(n + 1) % 2 == 0, -5, nbytes + 1).astype(np.int32)
    elif ptr == "descending":
        bp = bp[::-1].copy()
    if doc == "wild":
        off = rng.choice(np.asarray([-2 ** 31, -3, 0, 1, n // 2, n - 1, n, n + 1, 2 ** 31 - 1]), B + 1).astype(np.int32)
    bound = int(lib.hsg_eval_text_word_bound(n, nbytes))
    assert bound == R.word_bound(n, nbytes)
    cap = bound + extra
    w_ptr, w_ids = R.text_words_ref(text, bp, off)
    W = int(w_ptr[-1])
    if ptr is None:
        assert 0 < W <= bound and (W == bound) == (batch == "full")
    elif ptr == "overlap":
        assert W == bound                                                 # more words than the bound: capped
    # the text between bytes that would complete its first and last rows' cut sequences
    hostile = torch.from_numpy(np.frombuffer(b"\xe2\x80" * 64 + text + b"\x80\xa8" * 64, np.uint8).copy())
    t_dev = mk.ints(hostile)[128:128 + nbytes]
    word_ptr = mk.out("word_ptr", 1, n + 1, torch.int32)
    mask = torch.zeros(1, cap, dtype=torch.bool)
    mask[0, :W] = True
    word_ids = mk.out("word_ids", 1, cap, torch.int32, mask=mask, rest="untouched")
    ws = mk.scratch("ws", int(lib.hsg_eval_text_workspace_bytes(n, B, nbytes)), torch.uint8)
    call(lib, "hsg_eval_text_words", n, B, P(t_dev), nbytes, P(mk.ints(torch.from_numpy(bp))),
         P(mk.ints(torch.from_numpy(off))), cap, P(word_ptr), P(word_ids), P(ws))

    def exact(want):
        def check(got):
            assert np.array_equal(got.contiguous().numpy().reshape(-1)[:len(want)], want)
        return check
    return {"word_ptr": (exact(w_ptr), 0, 0), "word_ids": (exact(w_ids), 0, 0)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_eval_text_guard_bands(fn, kw):
    run_case(fn, kw)
