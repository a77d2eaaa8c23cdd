"""Plain-Python restatement of include/hsg_eval_text.h's contract: the yardstick for
hsg_eval_text_words.

The whitespace table is the header's, as byte strings.  A row is split by marking every byte
that a whitespace sequence lying wholly inside the row covers (no sequence starts inside
another, so the leftmost non-overlapping matches of one alternation are all of them); words are
the maximal unmarked runs.  Ids come from one dict of byte strings per document.  Nothing here
is shared with the code under test (hetersumgraph_amd/evalsel.py, csrc/hsg_eval_text.hip).
"""
import re

import numpy as np

WS_SEQS = ([bytes([b]) for b in (0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F, 0x20)]
           + [b"\xc2\x85", b"\xc2\xa0", b"\xe1\x9a\x80"]
           + [bytes([0xE2, 0x80, c]) for c in (*range(0x80, 0x8B), 0xA8, 0xA9, 0xAF)]
           + [b"\xe2\x81\x9f", b"\xe3\x80\x80"])
_WS = re.compile(b"|".join(re.escape(s) for s in WS_SEQS))


def whitespace_code_points():
    """The code points whose UTF-8 forms the table holds."""
    return {ord(s.decode("utf-8")) for s in WS_SEQS}


def enc(s):
    return s.encode("utf-8", "surrogatepass")


def split_spans(row):
    """[(first byte, length)] of the words of one row (a bytes object)."""
    covered = np.zeros(len(row) + 1, bool)
    covered[len(row)] = True
    for mt in _WS.finditer(row):
        covered[mt.start():mt.end()] = True
    spans, p = [], 0
    while p < len(row):
        if covered[p]:
            p += 1
            continue
        q = p
        while not covered[q]:
            q += 1
        spans.append((p, q - p))
        p = q
    return spans


def split_bytes(row):
    return [row[p:p + ln] for p, ln in split_spans(row)]


def word_bound(n, nbytes):
    return (nbytes + n) // 2


def doc_rows(doc_off, n):
    """e_0 .. e_B of the header: only the inner boundaries count."""
    B = len(doc_off) - 1
    e = [0]
    for d in range(1, B):
        e.append(max(e[-1], min(max(int(doc_off[d]), 0), n)))
    return e + [n]


def text_words_ref(text, byte_ptr, doc_off):
    """(word_ptr int32 [n + 1], word_ids int32 [word_ptr[n]]) of the header, for text (bytes),
    byte_ptr [n + 1] and doc_off [B + 1] of any content."""
    text = bytes(text)
    n, nbytes = len(byte_ptr) - 1, len(text)
    bound = word_bound(n, nbytes)
    rows = []
    for i in range(n):
        lo = min(max(int(byte_ptr[i]), 0), nbytes)
        hi = min(max(int(byte_ptr[i + 1]), lo), nbytes)
        rows.append(split_bytes(text[lo:hi]))
    total = np.concatenate([[0], np.cumsum([len(r) for r in rows], dtype=np.int64)])
    word_ptr = np.minimum(total, bound).astype(np.int32)
    ids = np.zeros(int(word_ptr[n]), np.int32)
    e = doc_rows(doc_off, n)
    for d in range(len(e) - 1):
        first = {}
        for i in range(e[d], e[d + 1]):
            for r, w in enumerate(rows[i][:int(word_ptr[i + 1] - word_ptr[i])]):   # words beyond the bound are dropped
                k = int(word_ptr[i]) + r
                ids[k] = first.setdefault(w, k)
    return word_ptr, ids


def pack_rows(rows):
    """(text bytes, byte_ptr int32 [n + 1]) of a list of bytes rows."""
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows], dtype=np.int64)]).astype(np.int32)
    return b"".join(rows), ptr
