"""hsg_eval_select (include/hsg_eval.h) on the GPU against the contract's numpy restatement
(tests/eval_ref.py): every output must be EXACTLY equal -- the selection is integers and an
order, there is nothing to tolerate.

Shapes are the smallest at which the one-wave-per-document kernel can go wrong: documents of
0, 1, 2, 63, 64, 65 and 130 rows (below, at and above one wave's stride, and a third pass),
an empty document first and last, m of 0, 1, 3 and above N, sentences with 0, 1, 64, 65 and
130 ids (the lanes' stride over a candidate's ids), ids at bits 31, 32, 63 and 64 (the
bitmap's word boundaries), gram_cnt of 0, 1, 32, 33 and the limit 262144.
"""
import numpy as np
import pytest
import torch

import eval_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(DEV)


class Batch:
    """Host arrays of one call and their device copies."""

    def __init__(self, logits, labels, rows, grams=None, cnt=None):
        self.logits = np.asarray(logits, np.float32).reshape(-1, 2)
        self.labels = np.asarray(labels, np.int64)
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
        self.n, self.B = len(self.logits), len(rows)
        assert self.off[-1] == self.n == len(self.labels)
        self.kw = {}
        if grams is not None:                              # grams: one id list per row
            assert len(grams) == self.n and len(cnt) == self.B
            self.kw = dict(gram_ptr=np.concatenate([[0], np.cumsum([len(g) for g in grams])]).astype(np.int32),
                           gram_ids=np.asarray([x for g in grams for x in g] or [0], np.int32),
                           gram_cnt=np.asarray(cnt, np.int32))
        self.d = dict(logits=dev(self.logits, np.float32), labels=dev(self.labels, np.int64), off=dev(self.off, np.int32),
                      **{k: dev(v, np.int32) for k, v in self.kw.items()})

    def outputs(self, sel_ld, totals0=(0, 0, 0, 0)):
        return (torch.full((self.B, sel_ld), 77, dtype=torch.int32, device=DEV),
                torch.full((self.B,), 77, dtype=torch.int32, device=DEV),
                torch.full((self.B, 4), 77, dtype=torch.int32, device=DEV),
                torch.tensor(totals0, dtype=torch.int64, device=DEV))

    def launch(self, m, n_max, sel_ld, gram_max, outs):
        from hetersumgraph_amd._lib import check, load, ptr
        d = self.d
        sel, nsel, cnts, totals = outs
        check(load().hsg_eval_select(self.n, self.B, ptr(d["logits"]) if self.n else None,
                                     ptr(d["labels"]) if self.n else None, ptr(d["off"]), m, n_max,
                                     ptr(d.get("gram_ptr")), ptr(d.get("gram_ids")), ptr(d.get("gram_cnt")), gram_max,
                                     ptr(sel), sel_ld, ptr(nsel), ptr(cnts), ptr(totals),
                                     torch.cuda.current_stream().cuda_stream), "hsg_eval_select")

    def reference(self, m, n_max, sel_ld, gram_max):
        return R.select_ref(self.logits, self.labels, self.off, m, n_max, sel_ld, gram_max=gram_max, **self.kw)

    def check(self, m, n_max=None, sel_ld=None, gram_max=None, totals0=(3, 1, 4, 1)):
        """One launch against the restatement, exactly; returns the device outputs."""
        rows = np.diff(self.off)
        n_max = int(max(rows.max(), 1)) if n_max is None else n_max
        sel_ld = (n_max if m == 0 else min(m, n_max)) if sel_ld is None else sel_ld
        gram_max = int(self.kw["gram_cnt"].max()) if gram_max is None and self.kw else (gram_max or 0)
        outs = self.outputs(sel_ld, totals0)
        self.launch(m, n_max, sel_ld, gram_max, outs)
        torch.cuda.synchronize()
        sel, nsel, cnts, tot = self.reference(m, n_max, sel_ld, gram_max)
        assert outs[1].cpu().numpy().tolist() == nsel.tolist()
        assert np.array_equal(outs[0].cpu().numpy(), sel)
        assert np.array_equal(outs[2].cpu().numpy(), cnts)
        assert outs[3].cpu().numpy().tolist() == (tot + np.asarray(totals0)).tolist()
        return outs, (sel, nsel, cnts, tot)


ROWS = [0, 1, 2, 63, 64, 65, 130, 0]
CNTS = [0, 1, 32, 33, 65, 200, 3000, 0]
ID_LENS = [0, 1, 64, 65, 130, 2, 3, 0, 1, 5]


def shapes_batch(seed, blocking):
    rng = np.random.default_rng(seed)
    n = sum(ROWS)
    logits = rng.standard_normal((n, 2)).astype(np.float32)
    labels = rng.integers(0, 2, n)
    if not blocking:
        return Batch(logits, labels, ROWS)
    grams, r = [], 0
    for rows, cnt in zip(ROWS, CNTS):
        for _ in range(rows):
            k = ID_LENS[r % len(ID_LENS)] if cnt else 0
            # documents with many ids draw short lists too, so that more than one candidate survives
            k = k if cnt < 3000 else [0, 1, 2, 3, 64, 65, 130, 1, 2, 3][r % 10]
            grams.append(rng.integers(0, cnt, k).tolist() if cnt else [])
            r += 1
    return Batch(logits, labels, ROWS, grams, CNTS)


BATCHES = {}


def shared(blocking):
    if blocking not in BATCHES:
        BATCHES[blocking] = shapes_batch(11 + blocking, blocking)
    return BATCHES[blocking]


@pytest.mark.parametrize("blocking", [False, True], ids=["plain", "blocking"])
@pytest.mark.parametrize("m", [0, 1, 3, 200])
def test_shapes_exact(m, blocking):
    b = shared(blocking)
    _, (_, nsel, _, _) = b.check(m)
    assert nsel[0] == 0 and nsel[-1] == 0                  # the empty documents
    if m == 200 and not blocking:
        assert nsel.tolist() == ROWS                       # m above N: every row, in candidate order
    if m == 3 and blocking:
        assert (nsel >= 0).all() and nsel[2] >= 1 and nsel[6] >= 2


def test_larger_n_max_gram_max_and_sel_ld_change_nothing():
    b = shared(True)
    a, _ = b.check(3)
    c, _ = b.check(3, n_max=1024, sel_ld=7, gram_max=262144)
    assert torch.equal(a[0], c[0][:, :3]) and bool((c[0][:, 3:] == -1).all()) and torch.equal(a[2], c[2])


def test_bitmap_word_boundaries():
    ids = [[31], [32], [63], [64], [31, 64], [30], [33], [62], [0], [32, 0]]
    n = len(ids)
    logits = np.stack([np.zeros(n), -np.arange(n)], 1)      # candidate order = index order
    b = Batch(logits, np.ones(n), [n], ids, [65])
    _, (sel, nsel, _, _) = b.check(n)
    assert sel[0, :nsel[0]].tolist() == [0, 1, 2, 3, 5, 6, 7, 8]
    for cnt in (32, 33):                                   # the last bit of a word / the first of the next
        b = Batch(logits[:3], np.ones(3), [3], [[cnt - 1], [0, cnt - 1], [cnt - 2]], [cnt])
        assert b.check(3)[1][0][0].tolist() == [0, 2, -1]


def test_gram_cnt_at_the_limit():
    top = 262144
    ids = [[top - 1], [0], [top - 1, 5], [131072], [0], [131071, 131073]]
    logits = np.stack([np.zeros(6), -np.arange(6)], 1)
    b = Batch(logits, [1, 0, 1, 0, 1, 1], [0, 6, 0], ids, [0, top, top])
    _, (sel, nsel, _, _) = b.check(6)
    assert sel[1, :nsel[1]].tolist() == [0, 1, 3, 5]


def test_ties_signed_zero_and_nan():
    f = np.float32
    nan = f("nan")
    equal = np.full(70, 0.25, np.float32)
    special = np.asarray([0.0, -0.0, nan, 1.0, -0.0, np.inf, nan, -np.inf, 0.0, 1.0], np.float32)
    p1 = np.concatenate([equal, special])
    p0 = np.concatenate([np.zeros(70, np.float32), np.asarray([nan, 0.0, 0.0, nan, -0.0, 1.0, nan, 0.0, -0.0, 1.0], f)])
    b = Batch(np.stack([p0, p1], 1), np.ones(80), [70, 10])
    _, (sel, nsel, _, _) = b.check(80)
    assert sel[0, :70].tolist() == list(range(70))         # all equal: ascending index
    assert sel[1, :10].tolist() == [2, 6, 5, 3, 9, 0, 1, 4, 8, 7]
    _, (sel, _, _, _) = b.check(3)
    assert sel.tolist() == [[0, 1, 2], [2, 6, 5]]
    _, (sel, nsel, _, _) = b.check(0)                      # torch's argmax NaN rule
    want = torch.from_numpy(np.stack([p0, p1], 1)[70:]).max(1)[1].ne(0).nonzero().view(-1).tolist()
    assert sel[1, :nsel[1]].tolist() == want and nsel[0] == 70
    # blocking walks the same order: with one shared id only the first candidate of each document survives
    b = Batch(np.stack([p0, p1], 1), np.ones(80), [70, 10], [[0]] * 80, [1, 1])
    _, (sel, nsel, _, _) = b.check(5)
    assert nsel.tolist() == [1, 1] and sel[:, 0].tolist() == [0, 2]


def test_refused_documents_leave_their_neighbours_alone():
    rng = np.random.default_rng(5)
    rows = [3, 5, 4]
    n = sum(rows)
    logits, labels = rng.standard_normal((n, 2)), rng.integers(0, 2, n)
    grams = [[int(x) for x in rng.integers(0, 9, 2)] for _ in range(n)]
    # a document over n_max
    for m in (0, 2):
        _, (sel, nsel, cnts, _) = Batch(logits, labels, rows, grams, [9, 9, 9]).check(m, n_max=4)
        assert nsel[1] == -1 and nsel[0] >= 0 and nsel[2] >= 0 and (sel[1] == -1).all() and (cnts[1] == 0).all()
    # an id outside [0, gram_cnt), negative or too large; a gram_cnt over gram_max
    for bad in (9, -1, 2 ** 31 - 1, -2 ** 31):
        g = [list(x) for x in grams]
        g[5][1] = bad
        _, (_, nsel, _, _) = Batch(logits, labels, rows, g, [9, 9, 9]).check(2)
        assert nsel[1] == -1 and nsel[0] >= 1 and nsel[2] >= 1
    _, (_, nsel, _, _) = Batch(logits, labels, rows, grams, [9, 40, 9]).check(2, gram_max=39)
    assert nsel.tolist()[1] == -1 and nsel[0] >= 1
    # with m == 0 blocking is ignored: the same operands are not even read
    g = [list(x) for x in grams]
    g[5][1] = 2 ** 31 - 1
    _, (_, nsel, _, _) = Batch(logits, labels, rows, g, [9, 9, 9]).check(0)
    assert (nsel >= 0).all()


def test_n_zero_still_writes_the_outputs():
    b = Batch(np.zeros((0, 2)), [], [0, 0, 0])
    _, (sel, nsel, cnts, _) = b.check(3, n_max=4)
    assert nsel.tolist() == [0, 0, 0] and (sel == -1).all() and (cnts == 0).all()
    b.check(0, n_max=4)


def test_offsets_are_clamped():
    rng = np.random.default_rng(6)
    b = Batch(rng.standard_normal((6, 2)), rng.integers(0, 2, 6), [2, 4])
    b.off = np.asarray([-3, 2, 9], np.int32)               # -> [0, 2, 6]
    b.d["off"] = dev(b.off, np.int32)
    _, (_, nsel, _, _) = b.check(5)
    assert nsel.tolist() == [2, 4]


def test_totals_accumulate_and_runs_are_bitwise_equal():
    b = shared(True)
    n_max, sel_ld, gram_max = max(ROWS), 3, max(CNTS)
    _, _, _, delta = b.reference(3, n_max, sel_ld, gram_max)
    o1 = b.outputs(sel_ld)
    b.launch(3, n_max, sel_ld, gram_max, o1)
    b.launch(3, n_max, sel_ld, gram_max, o1)
    o2 = b.outputs(sel_ld)
    b.launch(3, n_max, sel_ld, gram_max, o2)
    torch.cuda.synchronize()
    assert o1[3].tolist() == (2 * delta).tolist() and o2[3].tolist() == delta.tolist()
    for a, c in zip(o1[:3], o2[:3]):
        assert torch.equal(a, c)


def test_graph_capture_replays():
    """One single-stream capture replayed twice: sel unchanged, totals added twice.  A call
    that synchronised or allocated could not be captured at all."""
    b = shared(True)
    n_max, sel_ld, gram_max = max(ROWS), 3, max(CNTS)
    sel, nsel, cnts, delta = b.reference(3, n_max, sel_ld, gram_max)
    outs = b.outputs(sel_ld)
    b.launch(3, n_max, sel_ld, gram_max, outs)             # warm-up outside the capture
    torch.cuda.synchronize()
    outs[3].zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.launch(3, n_max, sel_ld, gram_max, outs)
    torch.cuda.synchronize()
    assert outs[3].tolist() == [0, 0, 0, 0]                # capturing ran nothing
    for k in (1, 2):
        outs[0].fill_(77)
        g.replay()
        torch.cuda.synchronize()
        assert outs[3].tolist() == (k * delta).tolist()
        assert np.array_equal(outs[0].cpu().numpy(), sel) and outs[1].cpu().numpy().tolist() == nsel.tolist()
        assert np.array_equal(outs[2].cpu().numpy(), cnts)


def test_python_wrapper_matches_and_refuses():
    from hetersumgraph_amd import evalsel
    texts = [["a b c d e", "a b c d x", "q r s t u v", "a b"], ["q r s t", "z"]]
    counts = [4, 2]
    pack = evalsel.pack_batch(texts, counts, 2)
    rng = np.random.default_rng(9)
    logits = rng.standard_normal((6, 2)).astype(np.float32)
    labels = rng.integers(0, 2, 6)
    off = np.asarray([0, 4, 6], np.int32)
    totals = torch.zeros(4, dtype=torch.int64, device=DEV)
    sel, nsel, cnts = evalsel.select(dev(logits, np.float32), dev(labels, np.int64), dev(off, np.int32), 3, 4, totals,
                                     pack.to(torch.device(DEV)))
    gp, gi, gc = (v.numpy() for v in pack.views())
    want = R.select_ref(logits, labels, off, 3, 4, 3, gp, gi, gc, pack.gram_max)
    assert np.array_equal(sel.cpu().numpy(), want[0]) and nsel.cpu().numpy().tolist() == want[1].tolist()
    assert np.array_equal(cnts.cpu().numpy(), want[2]) and totals.tolist() == want[3].tolist()
    with pytest.raises(RuntimeError, match="hsg_eval_select_supported"):
        evalsel.select(dev(logits, np.float32), dev(labels, np.int64), dev(off, np.int32), 3, 1025, totals)
    with pytest.raises(RuntimeError, match="int64"):
        evalsel.select(dev(logits, np.float32), dev(labels, np.int32), dev(off, np.int32), 3, 4, totals)
