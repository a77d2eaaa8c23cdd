"""hsg_eval_text_words (include/hsg_eval_text.h) on the GPU against the contract's plain-Python
restatement (tests/eval_text_ref.py): word_ptr and the written part of word_ids must be
BIT-EQUAL -- they are counts and positions, there is nothing to tolerate -- and the selection
on the device-made ids must be the selection on ``evalsel.word_ids``'s.

Shapes are the smallest at which the kernels can go wrong: the hand-built raw-byte batch
(sequences cut by a row's end, stray continuation bytes, near misses of every sequence, a
document of 0 rows, empty and whitespace-only rows, words of 65, 300 and 365 bytes -- beyond
one stride of the wave -- words that differ only in the last byte, prefixes, the same word in
two documents), n = 0, nbytes = 0, seeded random batches of 1, 4 and 32 documents over
vocabularies of 5, 60 and 3000 words (every word repeated many times; hardly any repeated),
and one document of more than 5000 words with more than 2000 distinct ones (more than one
word per thread of its block, probing far beyond one wave's stride)."""
import json
import os

import numpy as np
import pytest
import torch

import eval_text_ref as R
from test_eval_text_cpu import big_document, hand_batch, random_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(DEV)


def pack_raw(rows, off, byte_ptr=None):
    """A host TextPack of raw byte rows (evalsel.pack_text takes str only)."""
    from hetersumgraph_amd import evalsel
    text, ptr = R.pack_rows(rows)
    ptr = ptr if byte_ptr is None else np.asarray(byte_ptr, np.int32)
    n = len(ptr) - 1
    buf = torch.from_numpy(np.concatenate([ptr.view(np.uint8), np.frombuffer(text, np.uint8)]).copy())
    return evalsel.TextPack(buf, n, len(off) - 1, len(text), np.diff(ptr).astype(np.int64), np.diff(off).tolist()), text, ptr


def device_words(rows, off, doc_off=None, byte_ptr=None):
    """(word_ptr, the whole word_ids buffer, the restatement's pair) of one call."""
    from hetersumgraph_amd import evalsel
    pack, text, ptr = pack_raw(rows, off, byte_ptr)
    doc_off = off if doc_off is None else doc_off
    words = evalsel.text_words(pack.to(torch.device(DEV)), dev(doc_off, np.int32))
    torch.cuda.synchronize()
    assert words.lens is None and words.n == pack.n and words.B == pack.B and words.buf.dtype == torch.int32
    wp, ids = (x.cpu().numpy() for x in words.views())
    return wp, ids, R.text_words_ref(text, ptr, doc_off)


def check(rows, off, **kw):
    wp, ids, (rp, ri) = device_words(rows, off, **kw)
    assert wp.dtype == np.int32 and np.array_equal(wp, rp)
    assert np.array_equal(ids[:rp[-1]], ri)
    return rp, ri


def test_hand_built_raw_bytes():
    rows, off = hand_batch()
    wp, ids = check(rows, off)
    assert wp[-1] >= 90 and (np.diff(wp) == 0).sum() >= 4 and len(set(ids.tolist())) < len(ids)


def test_no_rows_and_no_bytes():
    wp, ids, (rp, _) = device_words([], np.asarray([0, 0], np.int32))                 # n = 0
    assert wp.tolist() == rp.tolist() == [0]
    wp, ids, (rp, _) = device_words([], np.asarray([0, 0, 0, 0], np.int32))           # n = 0, three empty documents
    assert wp.tolist() == [0]
    check([b"", b"", b""], np.asarray([0, 2, 3], np.int32))                            # nbytes = 0, a bound of 1
    check([b""], np.asarray([0, 1], np.int32))                                         # nbytes = 0, a bound of 0
    check([b"x"], np.asarray([0, 1], np.int32))                                        # one byte, one word


@pytest.mark.parametrize("vocab", [5, 60, 3000])
@pytest.mark.parametrize("B", [1, 4, 32])
def test_random_batches(B, vocab):
    rows, off = random_rows(np.random.default_rng(100 * B + vocab), B, vocab)
    wp, ids = check(rows, off)
    assert wp[-1] > 0


def test_one_large_document_and_reproducibility():
    rows, off = big_document(np.random.default_rng(3))
    wp, ids = check(rows, off)
    assert wp[-1] >= 5000 and len(set(ids.tolist())) >= 2000
    a = device_words(rows, off)
    b = device_words(rows, off)
    assert a[0].tobytes() == b[0].tobytes() and a[1][:wp[-1]].tobytes() == b[1][:wp[-1]].tobytes()


def test_doc_off_and_byte_ptr_of_any_content():
    rows, off = random_rows(np.random.default_rng(5), 6, 12)
    n = len(rows)
    for doc_off in ([3, 1, 4, 1, 5, 9, 2], [0, -7, 2 ** 31 - 1, 3, 3, n, n], [n, n, 0, 0, 2, 2, -2 ** 31]):
        check(rows, off, doc_off=np.asarray(doc_off, np.int64).astype(np.int32))
    text, ptr = R.pack_rows(rows)
    rng = np.random.default_rng(6)
    wild = rng.choice(np.asarray([-2 ** 31, -1, 0, 1, len(text) // 3, len(text) // 2, len(text), len(text) + 1, 2 ** 31 - 1]), n + 1)
    check(rows, off, byte_ptr=wild)                                                    # overlapping rows: capped at the bound
    check(rows, off, byte_ptr=ptr[::-1].copy())                                        # descending: every row empty


def test_words_beyond_the_bound_are_dropped():
    rows = [b"a b c d e f g h"]
    wp, ids = check(rows * 1, np.asarray([0, 6], np.int32), byte_ptr=[0, 15, 0, 15, -7, 99, 0])
    assert wp.tolist() == [0, 8, 8, 10, 10, 10, 10] and ids.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]


def test_wrapper_refuses_what_the_kernel_would():
    from hetersumgraph_amd import evalsel
    pack, _, _ = pack_raw([b"a b"], np.asarray([0, 1], np.int32))
    with pytest.raises(RuntimeError, match="ROCm device"):
        evalsel.text_words(pack)
    with pytest.raises(RuntimeError, match="doc_off"):
        evalsel.text_words(pack.to(torch.device(DEV)), dev([0, 1, 1], np.int32))
    words = evalsel.text_words(pack.to(torch.device(DEV)))                             # doc_off from the pack's counts
    assert words.views()[0].tolist() == [0, 2]
    with pytest.raises(RuntimeError, match="tab_cap"):
        words.tab_cap(3, 3)


# ---- the selection on device-made ids ------------------------------------------------------------

def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


GOLDENS = {"select": _load("eval_select.json"), "words": _load("eval_words.json"), "text": _load("eval_text.json")}


@pytest.mark.parametrize("name,case", [(n, c) for n, g in GOLDENS.items() for c in g["cases"] if c["blocking"]],
                         ids=lambda x: x if isinstance(x, str) else f"w{x['n_win']}-m{x['m']}")
def test_selection_on_device_ids_is_selection_on_host_ids(name, case):
    from hetersumgraph_amd import evalsel
    w, m = case["n_win"], case["m"]
    inp = GOLDENS[name]["inputs"][str(w)]
    counts = inp["counts"]
    sents = [t["sents"] for t in inp["texts"]]
    logits, labels = dev(inp["logits"], np.float32), dev(inp["labels"], np.int64)
    off = dev(np.concatenate([[0], np.cumsum(counts)]), np.int32)
    n_max = max(counts)
    host = evalsel.pack_words([evalsel.word_ids(s, c) for s, c in zip(sents, counts)], counts)
    text = evalsel.pack_text(sents, counts)
    assert text.tab_cap(w, max(m, 1)) >= host.tab_cap(w, max(m, 1))
    made = evalsel.text_words(text.to(torch.device(DEV)), off)
    assert np.array_equal(made.views()[0].cpu().numpy(), host.views()[0].numpy())      # the same words per row
    outs = []
    for words, cap in ((made, text.tab_cap(w, m)), (host.to(torch.device(DEV)), None)):
        totals = torch.zeros(4, dtype=torch.int64, device=DEV)
        sel, nsel, cnts = evalsel.select_words(logits, labels, off, m, n_max, w, totals, words, cap)
        outs.append((sel.cpu().numpy(), nsel.cpu().numpy(), cnts.cpu().numpy(), totals.tolist()))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    st = case["state"]
    assert [a[0][d, :a[1][d]].tolist() for d in range(len(counts))] == st["extracts"]   # the reference's choice
    assert a[3] == [st["pred"], st["true"], st["match_true"], st["match"]]
