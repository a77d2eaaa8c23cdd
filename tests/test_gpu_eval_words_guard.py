"""Guard bands and poison around every buffer hsg_eval_select_words writes
(include/hsg_eval_words.h), with the machinery of tests/test_gpu_guard_bands.py and the
pattern of tests/test_gpu_eval_guard.py: each case runs once on ``guard.guarded`` outputs of
EXACTLY the documented size -- sel [B, sel_ld], nsel [B], doc_counts [B, 4], totals [4] -- with
a ``guard.poisoned_input`` logits matrix, once on plain tensors, and the shared body asserts
the bands intact, the inputs bitwise unchanged, every documented element written, the two runs
bitwise equal and the values exactly those of the contract's restatement
(tests/eval_words_ref.py).  ``totals`` is updated in place, so it starts from values of its
own, not from the guard pattern, and "written" is shown by its value.

``word_ids`` is a guarded buffer of exactly word_ptr[n] elements too (declared as an output
that must come back with the values it went in with): the ``ptr`` variants hand the kernel a
word_ptr of descending, negative and oversized values, under which nothing outside word_ids
may be read -- a read of the bands would change the selection, which is compared with the
restatement's under the header's clamping rule -- and nothing at all may be written.

CASES is this header's table (tests/test_eval_words_abi.py checks that every writing entry
point has a case); the shapes are the smallest at which the kernel can go wrong: documents of
0, 1, 2 and 65 rows (one past a wave's stride), an empty document first and last, a refused
document in the middle (its rows, or the windows of its chosen sentences), m of 0, 3 and above
N, blocking on and off, a sentence of more windows than two strides of the wave.
"""
import numpy as np
import pytest
import torch

import eval_words_ref as W
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
ROWS = [0, 1, 65, 6, 2, 0]
REFUSED = 3                                  # the 6-row document, when n_max or tab_cap says so
TOTALS0 = [7, 11, 13, 17]
N_WIN = 2


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


@case("hsg_eval_select_words", dict(m=0, block=0), dict(m=3, block=0), dict(m=3, block=1), dict(m=3, block=1, bad="cap"),
      dict(m=3, block=0, bad="rows"), dict(m=0, block=0, bad="rows"), dict(m=3, block=1, bad="rows"),
      dict(m=100, block=1), dict(m=3, block=1, ptr="descending"), dict(m=100, block=1, ptr="wild"),
      dict(m=0, block=1, ptr="wild"))
def c_eval_select_words(lib, mk, m, block, bad=None, ptr=None):
    rng = np.random.default_rng(21)
    rows = [5 if (bad == "rows" and r == 65) else r for r in ROWS]
    n, B = sum(rows), len(rows)
    n_max = 5 if bad == "rows" else 65                    # "rows": the 6-row document is over n_max
    tab_cap = 1024
    logits = rng.standard_normal((n, 2)).astype(np.float32)
    labels = rng.integers(0, 2, n)
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    kw, dev = {}, {}
    if block:
        vocab = [1, 3, 12, 40, 5, 1]
        words = [rng.integers(0, vocab[d], int(rng.integers(0, 9))).tolist() for d in range(B) for _ in range(rows[d])]
        words[off[2] + 7] = rng.integers(100, 4000, 132).tolist()        # 130 windows: more than two strides of the wave
        if bad == "cap":                                                 # 400 + 400 + 400 distinct windows: the third does not fit
            for i in range(6):
                words[off[REFUSED] + i] = list(range(1000 * i, 1000 * i + 402))
        wp = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32)
        ids = np.asarray([x for w in words for x in w], np.int32)
        if ptr == "descending":
            wp[:-1] = wp[-2::-1].copy()
        elif ptr == "wild":
            wp[:-1] = rng.choice(np.asarray([-2 ** 31, -1, 0, 3, len(ids) // 2, len(ids), len(ids) + 1, 2 ** 31 - 1]), n)
        kw = dict(word_ptr=wp, word_ids=ids)
        dev["word_ptr"] = mk.ints(torch.from_numpy(wp))
        dev["word_ids"] = mk.out("word_ids", 1, len(ids), torch.int32, init=torch.from_numpy(ids)[None])
    sel_ld = n_max if m == 0 else min(m, n_max)
    sel = mk.out("sel", B, sel_ld, torch.int32)
    nsel = mk.out("nsel", 1, B, torch.int32)
    cnts = mk.out("doc_counts", B, 4, torch.int32)
    totals = mk.out("totals", 1, 4, torch.int64, init=torch.tensor([TOTALS0]))
    call(lib, "hsg_eval_select_words", n, B, P(mk.inp(torch.from_numpy(logits))), P(mk.ints(torch.from_numpy(labels))),
         P(mk.ints(torch.from_numpy(off))), m, n_max, N_WIN, P(dev.get("word_ptr")), P(dev.get("word_ids")), tab_cap,
         P(sel), sel_ld, P(nsel), P(cnts), P(totals))
    w_sel, w_nsel, w_cnts, w_tot = W.select_words_ref(logits, labels, off, m, n_max, sel_ld, N_WIN, tab_cap=tab_cap, **kw)
    if ptr is None:
        assert (w_nsel[REFUSED] == -1) == (bad is not None) and (np.delete(w_nsel, REFUSED) >= 0).all()

    def exact(want):
        def check(got):
            assert np.array_equal(got.contiguous().numpy().reshape(want.shape), want)
        return check
    refs = {"sel": (exact(w_sel), 0, 0), "nsel": (exact(w_nsel), 0, 0), "doc_counts": (exact(w_cnts), 0, 0),
            "totals": (exact(w_tot + np.asarray(TOTALS0)), 0, 0)}
    if block:
        refs["word_ids"] = (exact(kw["word_ids"]), 0, 0)                # read-only: back as it went in
    return refs


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_eval_words_guard_bands(fn, kw):
    run_case(fn, kw)
