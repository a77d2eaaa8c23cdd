"""The word ids from article bytes on the CPU (include/hsg_eval_text.h, evalsel.pack_text): the
contract's restatement (tests/eval_text_ref.py) is pinned against Python itself -- its
whitespace table against ``str.isspace`` over every code point, its split against
``str.split`` -- and against the header's raw-byte rules; its ids are ``evalsel.word_ids``'s
partition and obey the smallest-position rule; ``pack_text`` has the documented layout and
bounds.  The batch builders here are shared with the GPU tests.  No GPU needed."""
import json
import os

import numpy as np
import pytest
import torch

import eval_text_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_text.json")

WS = sorted(R.whitespace_code_points())
ALPHABET = ([chr(c) for c in WS] * 2 + list("abcdefgh.,-'") + ["é", "ß", "Ж", "中", "あ", "€", "​", "﻿",
            "😀", "𐍈", "\ud800", "\udfff", "\x00", "\x7f", "\x1b", "\u0084", "\u0086", "\u009f", "¡"])


# ---- builders shared with tests/test_gpu_eval_text*.py ----------------------------------------

def hand_batch():
    """(rows, doc_off): the raw-byte cases of the header, one hazard per row."""
    w65, w300 = bytes(range(0x30, 0x30 + 65)), bytes(0x41 + (i * 7) % 26 for i in range(300))
    docs = [
        # sequences cut by a row's end must not join with the next row's continuation bytes
        [b"ab\xc2", b"\x85cd \xa0", b"x\xe2\x80", b"\x80y\xe2\x80", b"\xa8", b"q\xe3\x80", b"\x80 \xe3", b"\x80\x80",
         b"\xe1\x9a", b"\x80", b"\xe2\x81", b"\x9f\xe2"],
        [],                                                                        # a document of 0 rows
        # stray continuation bytes are not whitespace; near misses of every multi-byte sequence
        [b"a\x85b \xa0c \x85 \xa0", b"\xc2\x84 \xc2\x86 \xc2\x9f \xc2\xa1 \xc3\x85", b"\xe1\x9a\x81 \xe1\x9b\x80 \xe0\x9a\x80",
         b"\xe2\x80\x7f \xe2\x80\x8b \xe2\x80\xa7 \xe2\x80\xaa \xe2\x80\xae \xe2\x80\xb0", b"\xe2\x81\x9e \xe2\x82\x9f \xe3\x80\x81 \xe3\x81\x80",
         b"\x08 \x0e \x1b \x21 \x7f \x00"],
        # empty and whitespace-only rows
        [b"", b" \t\n\x0b\x0c\r\x1c\x1d\x1e\x1f", R.enc(" 　\u0085      "), b"", b" "],
        # long words, words that differ only in the last byte, prefixes
        [w65 + b" " + w300, w300[:-1] + b"B " + w300 + b" " + w300[:-1] + b"C", w65[:64] + b"\t" + w65 + b"\n" + w65[:-1] + b"!",
         b"ab abc abcd a abc ab", w300 + w65 + b" " + w300[:299], b"abcd"],
        # the same words again in another document, every whitespace sequence as a separator
        [b"abc ab " + w65, b"".join(s + b"w%d" % (i % 5) for i, s in enumerate(R.WS_SEQS)) + b" ", b"cd y q x"],
    ]
    rows = [r for d in docs for r in d]
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int32)
    return rows, off


def random_rows(rng, B, vocab, rows_per_doc=(0, 9), words_per_row=(0, 30)):
    """(rows, doc_off): B documents over a vocabulary of ``vocab`` byte strings of 1..20 bytes
    (ASCII and multi-byte, none containing whitespace), joined by runs of 1..3 whitespace
    sequences, sometimes leading and trailing."""
    letters = [R.enc(c) for c in "abcdefghijklmnopqrstuvwxyz0123456789éßЖ中😀"] + [b"\x85", b"\xa0", b"\xc2", b"\xe2\x80"]
    words = set()
    while len(words) < vocab:
        w = b"".join(letters[j] for j in rng.integers(0, len(letters), int(rng.integers(1, 6))))
        if len(R.split_bytes(w)) == 1 and R.split_bytes(w)[0] == w:
            words.add(w)
    words = sorted(words)
    rows, counts = [], []

    def sep():
        return b"".join(R.WS_SEQS[j] for j in rng.integers(0, len(R.WS_SEQS), int(rng.integers(1, 4))))
    for _ in range(B):
        c = int(rng.integers(*rows_per_doc))
        counts.append(c)
        for _ in range(c):
            ws = [words[j] for j in rng.integers(0, vocab, int(rng.integers(*words_per_row)))]
            parts = [sep()] if rng.random() < 0.3 else []                            # leading whitespace
            for w in ws:
                parts += [w, sep()]
            if ws and rng.random() < 0.5:
                parts.pop()                                                          # no trailing whitespace
            row = b"".join(parts)
            rows.append(row)
    return rows, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def big_document(rng):
    """One document of at least 5000 words with at least 2000 distinct ones."""
    rows, off = random_rows(rng, 1, 2600, rows_per_doc=(120, 121), words_per_row=(40, 56))
    return rows, off


# ---- the whitespace table and the split, against Python ---------------------------------------

def test_whitespace_table_is_str_isspace():
    assert R.whitespace_code_points() == {c for c in range(0x110000) if chr(c).isspace()}
    assert len(R.WS_SEQS) == 29 and all(R.enc(chr(c)) in R.WS_SEQS for c in WS)


def check_split(s):
    got = [t.decode("utf-8", "surrogatepass") for t in R.split_bytes(R.enc(s))]
    assert got == s.split(), (s, got)


def test_split_is_str_split_around_every_whitespace_code_point():
    for c in WS:
        for ch in (chr(c - 1), chr(c), chr(c + 1)):
            for s in (f"ab{ch}cd", f"{ch}ab", f"ab{ch}", ch, ch + ch, f"a{ch}{ch}b{ch}", f" {ch} x {ch}", f"é{ch}中{ch}😀"):
                check_split(s)


def test_split_is_str_split_at_every_one_byte_character():
    for c in range(128):
        for s in (f"ab{chr(c)}cd", chr(c), f"{chr(c)}x", f"x{chr(c)}"):
            check_split(s)


def test_split_is_str_split_on_random_strings():
    rng = np.random.default_rng(7)
    for _ in range(600):
        check_split("".join(ALPHABET[j] for j in rng.integers(0, len(ALPHABET), int(rng.integers(0, 40)))))


def test_raw_byte_rules():
    # a truncated sequence at a row's end is a word byte and never joins with the next row
    for head, tail in ((b"\xc2", b"\x85"), (b"\xc2", b"\xa0"), (b"\xe2\x80", b"\x80"), (b"\xe2", b"\x80\xa8"),
                       (b"\xe3\x80", b"\x80"), (b"\xe3", b"\x80\x80"), (b"\xe1\x9a", b"\x80"), (b"\xe2\x81", b"\x9f")):
        assert R.split_bytes(b"ab" + head) == [b"ab" + head]
        assert R.split_bytes(tail + b"cd") == [tail + b"cd"]
        assert R.split_bytes(b"ab" + head + tail + b"cd") == [b"ab", b"cd"]            # whole, inside one row: whitespace
        text, ptr = R.pack_rows([b"ab" + head, tail + b"cd"])
        wp, ids = R.text_words_ref(text, ptr, [0, 2])
        assert wp.tolist() == [0, 1, 2] and ids.tolist() == [0, 1]
    # a stray continuation byte is not whitespace
    assert R.split_bytes(b"a\x85b \xa0c") == [b"a\x85b", b"\xa0c"]
    assert R.split_bytes(b"\x85") == [b"\x85"] and R.split_bytes(b"\xa0\xa0") == [b"\xa0\xa0"]
    assert R.split_bytes(b"") == [] and R.split_bytes(b" \t\xc2\xa0") == []


def test_hand_batch_holds_what_it_says():
    rows, off = hand_batch()
    text, ptr = R.pack_rows(rows)
    wp, ids = R.text_words_ref(text, ptr, off)
    counts = np.diff(wp)
    assert (np.diff(off) == 0).any() and (counts == 0).sum() >= 4
    lens = sorted({ln for r in rows for _, ln in R.split_spans(r)})
    assert 65 in lens and 300 in lens and 365 in lens
    assert wp[-1] == len(ids) <= R.word_bound(len(rows), len(text))


# ---- ids ------------------------------------------------------------------------------------------

def str_batch(seed, B=4):
    rng = np.random.default_rng(seed)
    vocab = ["w%d" % i for i in range(12)] + ["é", "中文", "😀x", "a​b", "\ud800"]
    seps = [chr(c) for c in WS]
    docs, counts = [], []
    for _ in range(B):
        sents = []
        for _ in range(int(rng.integers(1, 7))):
            toks = [vocab[j] for j in rng.integers(0, len(vocab), int(rng.integers(0, 15)))]
            s = "".join(t + "".join(seps[j] for j in rng.integers(0, 29, int(rng.integers(1, 3)))) for t in toks)
            sents.append((" " if rng.random() < 0.3 else "") + s)
        docs.append(sents)
        counts.append(len(sents) + int(rng.integers(-1, 2)))                           # fewer, equal or more rows than sentences
    counts = [max(c, 0) for c in counts]
    return docs, counts


def ref_of_strs(docs, counts):
    rows = [R.enc(s) for sents, c in zip(docs, counts) for s in (sents[:c] + [""] * (c - len(sents[:c])))]
    text, ptr = R.pack_rows(rows)
    return R.text_words_ref(text, ptr, np.concatenate([[0], np.cumsum(counts)]))


@pytest.mark.parametrize("seed", range(6))
def test_ids_are_word_ids_partition(seed):
    from hetersumgraph_amd import evalsel
    docs, counts = str_batch(seed)
    wp, ids = ref_of_strs(docs, counts)
    pack = evalsel.pack_words([evalsel.word_ids(s, c) for s, c in zip(docs, counts)], counts, pin=False)
    hp, hi = (x.numpy() for x in pack.views())
    assert np.array_equal(wp, hp)
    o = 0
    for c in counts:                                                                   # per document: equal id <=> equal id
        a, b = ids[wp[o]:wp[o + c]], hi[wp[o]:wp[o + c]]
        assert np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])
        o += c


def test_ids_are_the_smallest_position_in_the_document():
    rows, off = hand_batch()
    text, ptr = R.pack_rows(rows)
    wp, ids = R.text_words_ref(text, ptr, off)
    words = [w for r in rows for w in R.split_bytes(r)]
    e = R.doc_rows(off, len(rows))
    doc_of = np.repeat(np.arange(len(e) - 1), np.diff(wp[e]))
    for k, w in enumerate(words):
        same = [j for j in range(len(words)) if words[j] == w and doc_of[j] == doc_of[k]]
        assert ids[k] == same[0] <= k
    # the same word in two documents: two ids
    ks = [k for k, w in enumerate(words) if w == b"abc"]
    assert len({int(doc_of[k]) for k in ks}) == 2 and len({int(ids[k]) for k in ks}) == 2


def test_doc_off_of_any_content_puts_every_row_in_one_document():
    assert R.doc_rows([0, 3, 5, 9], 9) == [0, 3, 5, 9]
    assert R.doc_rows([4, 3, 2, 7], 9) == [0, 3, 3, 9]                                 # only the inner boundaries, ascending
    assert R.doc_rows([0, -5, 100, 4, 9], 9) == [0, 0, 9, 9, 9]
    assert R.doc_rows([7, 1], 9) == [0, 9]


def test_overlapping_rows_are_capped_at_the_bound():
    text = b"a b c d e f g h"                                                          # 8 words in 15 bytes
    ptr = np.asarray([0, 15, 0, 15, -7, 99, 0], np.int32)                              # rows 0, 2, 4: the whole text; others empty
    wp, ids = R.text_words_ref(text, ptr, [0, 6])
    bound = R.word_bound(6, 15)
    assert bound == 10 and wp.tolist() == [0, 8, 8, 10, 10, 10, 10] and ids.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]


# ---- packing ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_pack_text_layout_and_bounds(seed):
    from hetersumgraph_amd import evalsel
    docs, counts = str_batch(seed)
    pack = evalsel.pack_text(docs, counts, pin=False)
    n = sum(counts)
    rows = [R.enc(s) for sents, c in zip(docs, counts) for s in (sents[:c] + [""] * (c - len(sents[:c])))]
    text, ptr = R.pack_rows(rows)
    assert (pack.n, pack.B, pack.nbytes, pack.counts) == (n, len(counts), len(text), counts)
    assert pack.buf.dtype == torch.uint8 and pack.buf.numel() == 4 * (n + 1) + len(text)
    bp, tx = pack.views()
    assert bp.dtype == torch.int32 and np.array_equal(bp.numpy(), ptr) and tx.numpy().tobytes() == text
    assert np.array_equal(pack.lens, np.diff(ptr))
    # the per-row bound covers the true count, and the table rule covers WordPack's
    true = np.asarray([len(s.split()) for s in (r.decode("utf-8", "surrogatepass") for r in rows)])
    assert (pack.word_bound() >= true).all() and int(pack.word_bound().sum()) <= R.word_bound(n, len(text))
    words = evalsel.pack_words([evalsel.word_ids(s, c) for s, c in zip(docs, counts)], counts, pin=False)
    for n_win in (1, 2, 3):
        for m in (1, 3, 5):
            assert 64 <= words.tab_cap(n_win, m) <= pack.tab_cap(n_win, m) <= 8192


def test_tab_cap_is_clamped_to_the_kernels_largest_table():
    from hetersumgraph_amd import evalsel
    pack = evalsel.pack_text([["x" * 30000, "y z"]], [2], pin=False)
    assert pack.tab_cap(3, 3) == 8192 and evalsel.TAB_CAP_MAX == 8192
    assert evalsel.words_supported(2, 3, pack.tab_cap(3, 3))


def test_pack_text_takes_any_str():
    from hetersumgraph_amd import evalsel
    pack = evalsel.pack_text([["a\ud800b \udfff", "", "é"]], [3], pin=False)
    bp, tx = pack.views()
    assert tx.numpy().tobytes() == R.enc("a\ud800b \udfff") + R.enc("é") and bp.tolist() == [0, 9, 9, 11]
    assert evalsel.pack_text([[]], [0], pin=False).buf.numel() == 4
    with pytest.raises(RuntimeError, match="different batches"):
        evalsel.pack_text([["a"]], [1, 1], pin=False)


# ---- the fixture ------------------------------------------------------------------------------------

def test_the_text_golden_needs_every_whitespace():
    """tests/golden/eval_text.json holds the generator's inputs, and its non-vacuity facts hold:
    split at 0x20 alone, at least half of the blocking walks would end elsewhere; per window
    one ends short of k and one with exactly k; every whitespace code point separates words."""
    import make_eval_text_golden as MT
    assert os.path.getsize(GOLDEN) < 100 * 1024
    with open(GOLDEN) as f:
        g = json.load(f)
    assert sorted((c["n_win"], c["m"], c["blocking"]) for c in g["cases"]) == sorted(
        (w, m, b) for w in (2, 3) for m in (0, 1, 3, 5) for b in (False, True))
    facts = MT.walk_facts(g["cases"], g["inputs"])
    for w in MT.N_WINS:
        inp = g["inputs"][str(w)]
        assert inp["texts"] == MT.make_case(w)[2]
        assert {ch for t in inp["texts"] for s in t["sents"] for ch in s if ch.isspace()} == {chr(c) for c in WS}
        assert any(not p.isascii() for t in inp["texts"] for s in t["sents"] for p in s.split())
        f = facts[w]
        assert 2 * f["differs"] >= f["n"] and f["short"] >= 1 and f["full"] >= 1, (w, f)
        o = 0
        for n in inp["counts"]:                                                        # no two scores of a document are equal
            assert len({x[1] for x in inp["logits"][o:o + n]}) == n
            o += n
