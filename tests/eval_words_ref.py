"""Plain-Python restatement of include/hsg_eval_words.h's contract: the yardstick for
hsg_eval_select_words.

One document at a time over lists of word ids: the candidate order is eval_ref's, a window is
a tuple of n_win consecutive ids, the seen set a ``set`` of tuples, and the refusal rule counts
the chosen sentences' windows with repeats.  Nothing here is shared with the code under test
(hetersumgraph_amd/evalsel.py); ``split_ids`` below interns words with a dict of its own.
"""
import numpy as np

from eval_ref import candidate_order, counts_doc


def windows(words, n_win):
    """The windows of one sentence: t = 0 .. len - n_win - 1 (never the last n-gram)."""
    return [tuple(words[t:t + n_win]) for t in range(len(words) - n_win)]


def select_doc_words(p, m, sent_words=None, n_win=3, tab_cap=None):
    """Chosen local indices of one document in choice order, or None when the document is
    refused.  p float32 [N, 2]; sent_words: None (no blocking) or N lists of word ids;
    tab_cap: None (no limit) or the number of windows that may be stored."""
    N = len(p)
    if m == 0:
        return [i for i in range(N) if not np.isnan(p[i, 0]) and (np.isnan(p[i, 1]) or p[i, 1] > p[i, 0])]
    k = min(m, N)
    order = candidate_order([np.float32(v) for v in p[:, 1]])
    if sent_words is None:
        return order[:k]
    seen, chosen, stored = set(), [], 0
    for i in order:
        if len(chosen) >= k:
            break
        wins = windows(sent_words[i], n_win)
        if any(w in seen for w in wins):
            continue
        if tab_cap is not None and stored + len(wins) > tab_cap:
            return None
        stored += len(wins)
        chosen.append(i)
        seen.update(wins)
    return chosen


def row_words(word_ptr, word_ids, row):
    """The ids of one row under the header's clamping rule."""
    T = max(int(word_ptr[-1]), 0)
    lo = min(max(int(word_ptr[row]), 0), T)
    hi = min(max(int(word_ptr[row + 1]), lo), T)
    return [int(x) for x in word_ids[lo:hi]]


def select_words_ref(logits, labels, doc_off, m, n_max, sel_ld, n_win=3, word_ptr=None, word_ids=None, tab_cap=64):
    """(sel int32 [B, sel_ld], nsel int32 [B], doc_counts int32 [B, 4], totals delta int64 [4])."""
    logits = np.asarray(logits, np.float32).reshape(-1, 2)
    n, B = len(logits), len(doc_off) - 1
    sel = np.full((B, sel_ld), -1, np.int32)
    nsel = np.zeros(B, np.int32)
    counts = np.zeros((B, 4), np.int32)
    blocking = m > 0 and word_ptr is not None
    for d in range(B):
        beg = min(max(int(doc_off[d]), 0), n)
        end = min(max(int(doc_off[d + 1]), beg), n)
        N = end - beg
        chosen = None
        if N <= n_max:
            words = [row_words(word_ptr, word_ids, beg + i) for i in range(N)] if blocking else None
            chosen = select_doc_words(logits[beg:end], m, words, n_win, tab_cap)
        if chosen is None:
            nsel[d] = -1
            continue
        sel[d, :len(chosen)] = chosen
        nsel[d] = len(chosen)
        counts[d] = counts_doc(chosen, labels[beg:end])
    return sel, nsel, counts, counts.astype(np.int64).sum(0)


def split_ids(sents):
    """Word ids of a document's sentences from ``str.split`` and a dict, first appearance first."""
    table = {}
    return [[table.setdefault(p, len(table)) for p in s.split()] for s in sents]
