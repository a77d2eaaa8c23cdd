"""hsg_eval_select_words (include/hsg_eval_words.h) on the GPU against the contract's
plain-Python restatement (tests/eval_words_ref.py): every output must be EXACTLY equal -- the
selection is integers and an order, there is nothing to tolerate.

Shapes are the smallest at which the one-wave-per-document kernel can go wrong: B of 1 and 33,
documents of 0, 1, 2, 63, 64, 65 and 130 rows (below, at and above one wave's stride, and a
third pass), an empty document first and last, m of 0, 1, 3 and above N, N at n_max and one
above, windows of 1, 3 and 8 words, sentences of n_win, n_win + 1, n_win + 64 and n_win + 65
words (no window, one, one stride of the wave, one more), one 600-word sentence of a single
repeated word (equal windows only), ids that differ only above bit 12 and ids from {0, 1}
(whatever the hash does with them, membership is decided by the ids), the table filled to
exactly tab_cap and one above, tied and NaN scores.
"""
import json
import os

import numpy as np
import pytest
import torch

import eval_ref as R
import eval_words_ref as W

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(DEV)


class Batch:
    """Host arrays of one call and their device copies.  words: one id list per row, or None."""

    def __init__(self, logits, labels, rows, words=None):
        self.logits = np.asarray(logits, np.float32).reshape(-1, 2)
        self.labels = np.asarray(labels, np.int64)
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
        self.n, self.B = len(self.logits), len(rows)
        assert self.off[-1] == self.n == len(self.labels)
        self.kw = {}
        if words is not None:
            assert len(words) == self.n
            self.kw = dict(word_ptr=np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32),
                           word_ids=np.asarray([x for w in words for x in w] or [0], np.int32))
        self.upload()

    def upload(self):
        self.d = dict(logits=dev(self.logits, np.float32), labels=dev(self.labels, np.int64), off=dev(self.off, np.int32),
                      **{k: dev(v, np.int32) for k, v in self.kw.items()})

    def outputs(self, sel_ld, totals0=(0, 0, 0, 0)):
        return (torch.full((self.B, sel_ld), 77, dtype=torch.int32, device=DEV),
                torch.full((self.B,), 77, dtype=torch.int32, device=DEV),
                torch.full((self.B, 4), 77, dtype=torch.int32, device=DEV),
                torch.tensor(totals0, dtype=torch.int64, device=DEV))

    def launch(self, m, n_max, sel_ld, n_win, tab_cap, outs):
        from hetersumgraph_amd._lib import check, load, ptr
        d = self.d
        sel, nsel, cnts, totals = outs
        check(load().hsg_eval_select_words(self.n, self.B, ptr(d["logits"]) if self.n else None,
                                           ptr(d["labels"]) if self.n else None, ptr(d["off"]), m, n_max, n_win,
                                           ptr(d.get("word_ptr")), ptr(d.get("word_ids")), tab_cap,
                                           ptr(sel), sel_ld, ptr(nsel), ptr(cnts), ptr(totals),
                                           torch.cuda.current_stream().cuda_stream), "hsg_eval_select_words")

    def reference(self, m, n_max, sel_ld, n_win, tab_cap):
        return W.select_words_ref(self.logits, self.labels, self.off, m, n_max, sel_ld, n_win, tab_cap=tab_cap, **self.kw)

    def check(self, m, n_win=3, tab_cap=8192, n_max=None, sel_ld=None, totals0=(3, 1, 4, 1)):
        """One launch against the restatement, exactly; returns the device outputs and the reference."""
        rows = np.diff(self.off)
        n_max = int(max(rows.max(), 1)) if n_max is None else n_max
        sel_ld = (n_max if m == 0 else min(m, n_max)) if sel_ld is None else sel_ld
        outs = self.outputs(sel_ld, totals0)
        self.launch(m, n_max, sel_ld, n_win, tab_cap, outs)
        torch.cuda.synchronize()
        sel, nsel, cnts, tot = self.reference(m, n_max, sel_ld, n_win, tab_cap)
        assert outs[1].cpu().numpy().tolist() == nsel.tolist()
        assert np.array_equal(outs[0].cpu().numpy(), sel)
        assert np.array_equal(outs[2].cpu().numpy(), cnts)
        assert outs[3].cpu().numpy().tolist() == (tot + np.asarray(totals0)).tolist()
        return outs, (sel, nsel, cnts, tot)


def walked_past_a_blocked_one(b, sel, nsel):
    """Documents whose choice is not a prefix of the candidate order: a sentence was skipped
    and a later one chosen."""
    out = []
    for d in range(b.B):
        o, e = b.off[d], b.off[d + 1]
        order = R.candidate_order([np.float32(v) for v in b.logits[o:e, 1]])
        out.append(nsel[d] > 0 and sel[d, :nsel[d]].tolist() != order[:nsel[d]])
    return out


# ---- the goldens through the Python wrapper -------------------------------------------------------

def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


GOLDENS = {"select": _load("eval_select.json"), "words": _load("eval_words.json")}


@pytest.mark.parametrize("name,case", [(n, c) for n, g in GOLDENS.items() for c in g["cases"]],
                         ids=lambda x: x if isinstance(x, str) else f"w{x['n_win']}-m{x['m']}-block{int(x['blocking'])}")
def test_goldens_through_select_words(name, case):
    from hetersumgraph_amd import evalsel
    w, m = case["n_win"], case["m"]
    inp = GOLDENS[name]["inputs"][str(w)]
    counts = inp["counts"]
    logits, labels = np.asarray(inp["logits"], np.float32), np.asarray(inp["labels"], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pack = None
    if case["blocking"]:
        pack = evalsel.pack_words([evalsel.word_ids(t["sents"], c) for t, c in zip(inp["texts"], counts)], counts)
        if name == "words" and m >= 3:
            assert pack.tab_cap(w, m) >= 512                        # several hundred windows stored
    totals = torch.zeros(4, dtype=torch.int64, device=DEV)
    n_max = max(counts)
    sel, nsel, cnts = evalsel.select_words(dev(logits, np.float32), dev(labels, np.int64), dev(off, np.int32), m, n_max,
                                           w, totals, None if pack is None else pack.to(torch.device(DEV)))
    sel, nsel = sel.cpu().numpy(), nsel.cpu().numpy()
    st = case["state"]
    assert [sel[d, :nsel[d]].tolist() for d in range(len(counts))] == st["extracts"]      # the reference's choice
    assert totals.tolist() == [st["pred"], st["true"], st["match_true"], st["match"]]
    kw = {}
    if pack is not None:
        kw = dict(word_ptr=pack.views()[0].numpy(), word_ids=pack.views()[1].numpy(), tab_cap=pack.tab_cap(w, m))
    want = W.select_words_ref(logits, labels, off, m, n_max, sel.shape[1], w, **kw)
    assert np.array_equal(sel, want[0]) and nsel.tolist() == want[1].tolist()
    assert np.array_equal(cnts.cpu().numpy(), want[2]) and totals.tolist() == want[3].tolist()


# ---- shapes ----------------------------------------------------------------------------------------

ROWS = [0, 1, 2, 63, 64, 65, 130, 0] + [1 + i % 9 for i in range(24)] + [0]          # B = 33
VOCABS = {1: (40, 400, 4000), 3: (3, 6, 40), 8: (2, 3, 5)}      # per window: blocks nearly always / often / rarely


def shapes_batch(seed, n_win, blocking):
    rng = np.random.default_rng(seed)
    n = sum(ROWS)
    logits = rng.standard_normal((n, 2)).astype(np.float32)
    labels = rng.integers(0, 2, n)
    if not blocking:
        return Batch(logits, labels, ROWS)
    lens = [n_win, n_win + 1, n_win + 64, n_win + 65, 0, 1, n_win + 7, n_win + 20, n_win - 1, n_win + 2]
    words, r = [], 0
    for d, rows in enumerate(ROWS):
        for _ in range(rows):
            words.append(rng.integers(0, VOCABS[n_win][d % 3], lens[r % len(lens)]).tolist())
            r += 1
    return Batch(logits, labels, ROWS, words)


BATCHES = {}


def shared(n_win, blocking):
    key = (n_win if blocking else 0, blocking)
    if key not in BATCHES:
        BATCHES[key] = shapes_batch(11 + n_win, n_win, blocking)
    return BATCHES[key]


@pytest.mark.parametrize("n_win", [1, 3, 8])
@pytest.mark.parametrize("m", [0, 1, 3, 200])
def test_shapes_exact_blocking(m, n_win):
    b = shared(n_win, True)
    assert b.B == 33
    _, (sel, nsel, _, _) = b.check(m, n_win)
    assert nsel[0] == 0 and nsel[-1] == 0 and (nsel >= 0).all()      # the empty documents; nothing refused
    if m in (3, 200):
        skipped = walked_past_a_blocked_one(b, sel, nsel)
        assert sum(skipped) >= 3                                     # blocking decided, and the walk went on
        k = np.minimum(m, np.diff(b.off))
        assert ((nsel == k) & (k > 1)).any()                         # some walks fill up ...
        assert m == 3 or (nsel < k).any()                            # ... and with m above N some run out


@pytest.mark.parametrize("m", [0, 1, 3, 200])
def test_shapes_exact_plain(m):
    b = shared(3, False)
    _, (_, nsel, _, _) = b.check(m, 3, tab_cap=64)
    if m == 200:
        assert nsel.tolist() == ROWS                                 # m above N: every row, in candidate order


def test_one_document_of_one_row():
    for words in ([[4, 4, 4, 4, 4]], [[]], None):
        b = Batch([[0.5, -0.5]], [1], [1], words)                    # B = 1, N = 1, m > N
        _, (sel, nsel, cnts, _) = b.check(3, 3, tab_cap=64)
        assert sel.tolist() == [[0]] and nsel.tolist() == [1] and cnts.tolist() == [[1, 1, 1, 1]]
        b.check(0, 3, tab_cap=64)


def test_larger_limits_change_nothing():
    b = shared(3, True)
    a, _ = b.check(3, 3, tab_cap=1024)
    c, _ = b.check(3, 3, tab_cap=8192, n_max=1024, sel_ld=7)
    assert torch.equal(a[0], c[0][:, :3]) and bool((c[0][:, 3:] == -1).all()) and torch.equal(a[2], c[2])


def test_n_max_and_one_above():
    rng = np.random.default_rng(5)
    rows = [3, 6, 5]
    n = sum(rows)
    words = [rng.integers(0, 9, 6).tolist() for _ in range(n)]
    for m in (0, 2):
        for w in (words, None):
            b = Batch(rng.standard_normal((n, 2)), rng.integers(0, 2, n), rows, w)
            _, (sel, nsel, cnts, _) = b.check(m, 2, tab_cap=64, n_max=5)
            assert nsel[1] == -1 and (sel[1] == -1).all() and (cnts[1] == 0).all()       # 6 rows: refused
            assert nsel[0] >= 0 and nsel[2] >= (1 if m else 0)                            # 5 rows = n_max: served
            _, (_, nsel, _, _) = b.check(m, 2, tab_cap=64, n_max=6)
            assert (nsel >= 0).all()


def test_one_long_sentence_of_one_word():
    """600 equal words: 597 equal windows, all in one slot; the count that the refusal rule
    uses is still 597."""
    words = [[9] * 600, [9] * 4, [1, 2, 3, 4, 5], [9] * 3, [9, 9, 1, 2, 3, 9, 9]]
    n = len(words)
    logits = np.stack([np.zeros(n), -np.arange(n)], 1)              # candidate order = index order
    b = Batch(logits, np.ones(n), [n], words)
    _, (sel, nsel, _, _) = b.check(5, 3, tab_cap=1024)
    assert sel[0, :nsel[0]].tolist() == [0, 2, 3]                    # [9]*4 blocked, [9]*3 has no window, (1,2,3) blocked
    _, (_, nsel, _, _) = b.check(5, 3, tab_cap=512)                  # 597 windows do not fit 512: refused
    assert nsel.tolist() == [-1]
    _, (sel, nsel, _, _) = b.check(5, 1, tab_cap=1024)               # unigrams: 599 x (9,), then everything with a 9 blocked
    assert sel[0, :nsel[0]].tolist() == [0, 2]
    b = Batch(logits[::-1].copy(), np.ones(n), [n], words)           # reverse order: the long one comes last and is blocked
    _, (sel, nsel, _, _) = b.check(5, 3, tab_cap=1024)
    assert sel[0, :nsel[0]].tolist() == [4, 3, 1]                    # (1,2,3) of row 2 is blocked by row 4


@pytest.mark.parametrize("n_win", [1, 3, 8])
def test_ids_are_only_compared(n_win):
    """Ids that are all multiples of 4096, negative and extreme ids: the same choice as with
    the small ids they stand for.  Ids from {0, 1}: long runs of equal and near-equal windows."""
    b = shared(n_win, True)
    _, (sel, nsel, _, _) = b.check(3, n_win)
    table = (np.arange(4000, dtype=np.int64) * 4096 - 2 ** 23).astype(np.int32)          # multiples of 4096, both signs
    table[-4:] = [-2 ** 31, 2 ** 31 - 1, -1, 1]                       # the largest vocabulary also meets the extremes
    assert len(set(table.tolist())) == len(table)
    c = Batch(b.logits, b.labels, ROWS, [table[w].tolist() for w in
                                         [b.kw["word_ids"][b.kw["word_ptr"][i]:b.kw["word_ptr"][i + 1]] for i in range(b.n)]])
    assert n_win == 1 or (c.kw["word_ids"] % 4096 == 0).all()
    _, (sel2, nsel2, _, _) = c.check(3, n_win)
    assert np.array_equal(sel, sel2) and np.array_equal(nsel, nsel2)
    rng = np.random.default_rng(8)
    rows = [6, 9, 1, 12]
    n = sum(rows)
    words = [rng.integers(0, 2, int(rng.integers(0, 30))).tolist() for _ in range(n)]
    z = Batch(rng.standard_normal((n, 2)), rng.integers(0, 2, n), rows, words)
    _, (sel, nsel, _, _) = z.check(4, n_win, tab_cap=128)
    assert (nsel >= 1).all()


def test_table_filled_to_exactly_tab_cap():
    """tab_cap = 64: chosen sentences with 30 + 34 = 64 windows are accepted, 30 + 35 refuse
    the document -- its neighbours are served and totals goes without it."""
    rng = np.random.default_rng(3)
    rows = [3, 3, 2]
    n = sum(rows)
    logits = np.stack([np.zeros(n), -np.arange(n, dtype=np.float32)], 1)
    labels = np.ones(n)
    for last, want in ((37, 2), (38, -1)):
        ids = iter(range(10 ** 6))
        take = lambda k: [next(ids) for _ in range(k)]                # all ids distinct: nothing blocks
        words = [take(5), take(9), take(4)] + [take(33), take(last), take(50)] + [take(20), take(47)]
        b = Batch(logits, labels, rows, words)
        _, (sel, nsel, cnts, tot) = b.check(2, 3, tab_cap=64)
        assert nsel.tolist() == [2, want, 2]
        assert tot.tolist() == cnts[[0, 2]].sum(0).tolist() if want < 0 else tot[0] == 6
        if want < 0:
            assert (sel[1] == -1).all() and (cnts[1] == 0).all()
    # a blocked sentence does not count: 30 + (blocked 40) + 34 = 64
    ids = iter(range(10 ** 6))
    first = take(33)
    b = Batch(logits[:3], labels[:3], [3], [first, first[:3] + take(40), take(37)])
    _, (sel, nsel, _, _) = b.check(2, 3, tab_cap=64)
    assert sel.tolist() == [[0, 2]]


def test_ties_signed_zero_and_nan():
    f = np.float32
    nan = f("nan")
    equal = np.full(70, 0.25, np.float32)
    special = np.asarray([0.0, -0.0, nan, 1.0, -0.0, np.inf, nan, -np.inf, 0.0, 1.0], np.float32)
    p1 = np.concatenate([equal, special])
    p0 = np.concatenate([np.zeros(70, np.float32), np.asarray([nan, 0.0, 0.0, nan, -0.0, 1.0, nan, 0.0, -0.0, 1.0], f)])
    b = Batch(np.stack([p0, p1], 1), np.ones(80), [70, 10])
    _, (sel, nsel, _, _) = b.check(80, tab_cap=64)
    assert sel[0, :70].tolist() == list(range(70))         # all equal: ascending index
    assert sel[1, :10].tolist() == [2, 6, 5, 3, 9, 0, 1, 4, 8, 7]
    _, (sel, nsel, _, _) = b.check(0, tab_cap=64)          # torch's argmax NaN rule
    want = torch.from_numpy(np.stack([p0, p1], 1)[70:]).max(1)[1].ne(0).nonzero().view(-1).tolist()
    assert sel[1, :nsel[1]].tolist() == want and nsel[0] == 70
    # blocking walks the same order: with one shared window only the first candidate of each document survives
    b = Batch(np.stack([p0, p1], 1), np.ones(80), [70, 10], [[5, 6, 7, 8]] * 80)
    _, (sel, nsel, _, _) = b.check(5, 3, tab_cap=64)
    assert nsel.tolist() == [1, 1] and sel[:, 0].tolist() == [0, 2]
    # ... and sentences that share only their LAST n-gram do not block each other
    b = Batch(np.stack([p0, p1], 1), np.ones(80), [70, 10], [[i, 5, 6, 7] for i in range(80)])
    _, (sel, nsel, _, _) = b.check(5, 3, tab_cap=64)
    assert nsel.tolist() == [5, 5] and sel[0].tolist() == [0, 1, 2, 3, 4]


def test_m0_never_reads_the_word_operands():
    b = shared(3, False)
    want, _ = b.check(0, 3, tab_cap=64)
    p = Batch(b.logits, b.labels, ROWS, [[1, 2, 3, 4, 5]] * b.n)
    # poison: pointers far outside a one-element id buffer (clamping would keep even a read in range)
    p.kw = dict(word_ptr=np.concatenate([np.full(b.n, 2 ** 30, np.int32), [1]]).astype(np.int32),
                word_ids=np.asarray([-2 ** 31], np.int32))
    p.upload()
    got, _ = p.check(0, 3, tab_cap=64)
    for a, c in zip(want[:3], got[:3]):
        assert torch.equal(a, c)


def test_word_ptr_is_clamped():
    rng = np.random.default_rng(6)
    rows = [4, 5]
    words = [rng.integers(0, 4, 12).tolist() for _ in range(9)]
    b = Batch(rng.standard_normal((9, 2)), rng.integers(0, 2, 9), rows, words)
    W_ = int(b.kw["word_ptr"][-1])
    for bad in ([W_, 90, 70, 50, 30, 10, 0, -5, 40, W_],                                 # descending, negative
                [0, 2 ** 31 - 1, 12, -2 ** 31, 36, 2 ** 31 - 1, 2 ** 31 - 1, 80, 0, W_],       # oversized
                [-1] * 9 + [W_], [5] * 9 + [W_], [0, 12, 24, 36, 48, 60, 72, 84, 96, 0], [7] * 9 + [-3]):
        b.kw["word_ptr"] = np.asarray(bad, np.int32)
        b.upload()
        b.check(3, 3, tab_cap=128)
        b.check(9, 1, tab_cap=128)


def test_n_zero_still_writes_the_outputs():
    b = Batch(np.zeros((0, 2)), [], [0, 0, 0], [])
    _, (sel, nsel, cnts, _) = b.check(3, 3, tab_cap=64, n_max=4)
    assert nsel.tolist() == [0, 0, 0] and (sel == -1).all() and (cnts == 0).all()
    b.check(0, 3, tab_cap=64, n_max=4)


def test_offsets_are_clamped():
    rng = np.random.default_rng(6)
    b = Batch(rng.standard_normal((6, 2)), rng.integers(0, 2, 6), [2, 4], [[i, i + 1] for i in range(6)])
    b.off = np.asarray([-3, 2, 9], np.int32)               # -> [0, 2, 6]
    b.upload()
    _, (_, nsel, _, _) = b.check(5, 1, tab_cap=64)
    assert nsel.tolist() == [2, 4]


def test_totals_accumulate_and_runs_are_bitwise_equal():
    b = shared(3, True)
    n_max, sel_ld = max(ROWS), 3
    _, _, _, delta = b.reference(3, n_max, sel_ld, 3, 2048)
    o1 = b.outputs(sel_ld)
    b.launch(3, n_max, sel_ld, 3, 2048, o1)
    b.launch(3, n_max, sel_ld, 3, 2048, o1)
    o2 = b.outputs(sel_ld)
    b.launch(3, n_max, sel_ld, 3, 2048, o2)
    torch.cuda.synchronize()
    assert o1[3].tolist() == (2 * delta).tolist() and o2[3].tolist() == delta.tolist()
    for a, c in zip(o1[:3], o2[:3]):
        assert torch.equal(a, c)


def test_graph_capture_replays():
    """One single-stream capture replayed twice: sel unchanged, totals added twice.  A call
    that synchronised or allocated could not be captured at all."""
    b = shared(3, True)
    n_max, sel_ld = max(ROWS), 3
    sel, nsel, cnts, delta = b.reference(3, n_max, sel_ld, 3, 2048)
    outs = b.outputs(sel_ld)
    b.launch(3, n_max, sel_ld, 3, 2048, outs)              # warm-up outside the capture
    torch.cuda.synchronize()
    outs[3].zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.launch(3, n_max, sel_ld, 3, 2048, outs)
    torch.cuda.synchronize()
    assert outs[3].tolist() == [0, 0, 0, 0]                # capturing ran nothing
    for k in (1, 2):
        outs[0].fill_(77)
        g.replay()
        torch.cuda.synchronize()
        assert outs[3].tolist() == (k * delta).tolist()
        assert np.array_equal(outs[0].cpu().numpy(), sel) and outs[1].cpu().numpy().tolist() == nsel.tolist()
        assert np.array_equal(outs[2].cpu().numpy(), cnts)


# ---- against the dense-id entry point -------------------------------------------------------------------

@pytest.mark.parametrize("n_win,vocab", [(1, 300), (2, 30), (3, 8), (4, 4)])
def test_same_selection_as_hsg_eval_select(n_win, vocab):
    """Random texts: hsg_eval_select on evalsel.pack_batch's dense n-gram ids and
    hsg_eval_select_words on evalsel.pack_words' word ids choose the same sentences."""
    from hetersumgraph_amd import evalsel
    rng = np.random.default_rng(40 + n_win)
    counts = [int(c) for c in rng.integers(1, 14, 9)] + [1]
    texts = [[" ".join(f"t{j}" for j in rng.integers(0, vocab, int(rng.integers(0, 40)))) for _ in range(c + d % 2)]
             for d, c in enumerate(counts)]                            # every other article is longer than its rows
    n = sum(counts)
    logits, labels = dev(rng.standard_normal((n, 2)), np.float32), dev(rng.integers(0, 2, n), np.int64)
    off = dev(np.concatenate([[0], np.cumsum(counts)]), np.int32)
    device = torch.device(DEV)
    for m in (1, 3, 20):
        ta, tb = (torch.zeros(4, dtype=torch.int64, device=DEV) for _ in range(2))
        a = evalsel.select(logits, labels, off, m, max(counts), ta, evalsel.pack_batch(texts, counts, n_win).to(device))
        words = evalsel.pack_words([evalsel.word_ids(t, c) for t, c in zip(texts, counts)], counts)
        b = evalsel.select_words(logits, labels, off, m, max(counts), n_win, tb, words.to(device))
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert ta.tolist() == tb.tolist() and int(b[1].min()) >= 1
    assert (a[1].cpu().numpy() < np.minimum(20, counts)).any()          # blocking decided something


def test_python_wrapper_refuses():
    from hetersumgraph_amd import evalsel
    rng = np.random.default_rng(9)
    logits, labels = dev(rng.standard_normal((6, 2)), np.float32), dev(rng.integers(0, 2, 6), np.int64)
    off, totals = dev([0, 4, 6], np.int32), torch.zeros(4, dtype=torch.int64, device=DEV)
    texts = [["a b c d e", "a b c d x", "q r s t u v", "a b"], ["q r s t", "z"]]
    pack = evalsel.pack_words([evalsel.word_ids(t) for t in texts], [4, 2]).to(torch.device(DEV))
    for kw in (dict(n_max=1025), dict(n_win=9), dict(n_win=0), dict(tab_cap=96), dict(tab_cap=16384)):
        args = dict(n_max=4, n_win=2, tab_cap=None)
        args.update(kw)
        with pytest.raises(RuntimeError, match="hsg_eval_words_supported"):
            evalsel.select_words(logits, labels, off, 3, args["n_max"], args["n_win"], totals, pack, args["tab_cap"])
    long = evalsel.pack_words([evalsel.word_ids(["w " * 5000] * 4), evalsel.word_ids(["x", "y"])], [4, 2])
    assert long.tab_cap(2, 3) == 32768                                   # beyond the 8192 slots: declined, no fallback
    with pytest.raises(RuntimeError, match="hsg_eval_words_supported"):
        evalsel.select_words(logits, labels, off, 3, 4, 2, totals, long.to(torch.device(DEV)))
    with pytest.raises(RuntimeError, match="int64"):
        evalsel.select_words(logits, dev(rng.integers(0, 2, 6), np.int32), off, 3, 4, 2, totals, pack)
    with pytest.raises(RuntimeError, match="another batch"):
        evalsel.select_words(logits[:5], labels[:5], dev([0, 4, 5], np.int32), 3, 4, 2, totals, pack)
    assert totals.tolist() == [0, 0, 0, 0]
