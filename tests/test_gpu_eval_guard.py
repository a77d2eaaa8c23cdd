"""Guard bands and poison around every buffer hsg_eval_select writes (include/hsg_eval.h),
with the machinery of tests/test_gpu_guard_bands.py: each case runs once on ``guard.guarded``
outputs of EXACTLY the documented size -- sel [B, sel_ld], nsel [B], doc_counts [B, 4],
totals [4] -- with a ``guard.poisoned_input`` logits matrix, once on plain tensors, and the
shared body asserts the bands intact, the inputs bitwise unchanged, every documented element
written, the two runs bitwise equal and the values exactly those of the contract's numpy
restatement (tests/eval_ref.py).  ``totals`` is updated in place, so it starts from values
of its own, not from the guard pattern, and "written" is shown by its value.

CASES is this header's table (tests/test_eval_abi.py checks that every writing entry point
has a case); the shapes are the smallest at which the kernel can go wrong: documents of 0,
1, 2 and 65 rows (one past a wave's stride), an empty document first and last, a refused
document in the middle, m of 0 and 3, blocking on and off.
"""
import numpy as np
import pytest
import torch

import eval_ref as R
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]
ROWS = [0, 1, 65, 6, 2, 0]
REFUSED = 3                                  # the 6-row document, when n_max or an id says so
TOTALS0 = [7, 11, 13, 17]


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


@case("hsg_eval_select", dict(m=0, block=0), dict(m=3, block=0), dict(m=3, block=1), dict(m=3, block=1, bad="id"),
      dict(m=3, block=0, bad="rows"), dict(m=0, block=0, bad="rows"), dict(m=100, block=1))
def c_eval_select(lib, mk, m, block, bad=None):
    rng = np.random.default_rng(21)
    rows = [5 if (bad == "rows" and r == 65) else r for r in ROWS]
    n, B = sum(rows), len(rows)
    n_max = 5 if bad == "rows" else 65                    # "rows": the 6-row document is over n_max
    logits = rng.standard_normal((n, 2)).astype(np.float32)
    labels = rng.integers(0, 2, n)
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    kw, gram_max = {}, 0
    if block:
        cnt = np.asarray([0, 1, 65, 33, 32, 0], np.int32)
        grams = [rng.integers(0, cnt[d], int(rng.integers(0, 4))).tolist() for d in range(B) for _ in range(rows[d])]
        grams[off[2] + 7] = rng.integers(0, 65, 130).tolist()            # more ids than two strides of the wave
        if bad == "id":
            grams[off[REFUSED] + 2] = [1, 33]
        kw = dict(gram_ptr=np.concatenate([[0], np.cumsum([len(g) for g in grams])]).astype(np.int32),
                  gram_ids=np.asarray([x for g in grams for x in g], np.int32), gram_cnt=cnt)
        gram_max = 65
    sel_ld = n_max if m == 0 else min(m, n_max)
    dev = {k: mk.ints(torch.from_numpy(v)) for k, v in kw.items()}
    sel = mk.out("sel", B, sel_ld, torch.int32)
    nsel = mk.out("nsel", 1, B, torch.int32)
    cnts = mk.out("doc_counts", B, 4, torch.int32)
    totals = mk.out("totals", 1, 4, torch.int64, init=torch.tensor([TOTALS0]))
    call(lib, "hsg_eval_select", n, B, P(mk.inp(torch.from_numpy(logits))), P(mk.ints(torch.from_numpy(labels))),
         P(mk.ints(torch.from_numpy(off))), m, n_max, P(dev.get("gram_ptr")), P(dev.get("gram_ids")),
         P(dev.get("gram_cnt")), gram_max, P(sel), sel_ld, P(nsel), P(cnts), P(totals))
    w_sel, w_nsel, w_cnts, w_tot = R.select_ref(logits, labels, off, m, n_max, sel_ld, gram_max=gram_max, **kw)
    assert (w_nsel[REFUSED] == -1) == (bad is not None) and (np.delete(w_nsel, REFUSED) >= 0).all()

    def exact(want):
        def check(got):
            assert np.array_equal(got.contiguous().numpy().reshape(want.shape), want)
        return check
    return {"sel": (exact(w_sel), 0, 0), "nsel": (exact(w_nsel), 0, 0), "doc_counts": (exact(w_cnts), 0, 0),
            "totals": (exact(w_tot + np.asarray(TOTALS0)), 0, 0)}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_eval_guard_bands(fn, kw):
    run_case(fn, kw)
