"""numpy restatement of the eval view of a resident batch, written from the contract in
include/hsg_resident_eval.h: per document the local (ptr, ids) pair of ``evalsel.word_ids``, the
store's three columns, the word running offsets of a pick list and the pack
[word_ptr (n_sent + 1) | word_ids (max(n_words, 1))].  Shared by the CPU tests, which pin it
against ``evalsel.pack_words``, and by the GPU tests as the expected value.

The documents are tests/resident_ref.py's "extremes" (1, 40, 3, 4, 2 and 1 sentence rows) and
one of 5 rows; the word lists are made here so that the kernel can go wrong: a document with no
word at all, rows of 0 and 1 word, a document of a single word, and 3,000 words in 5 rows (one
of them empty), more than any tile of the kernel holds."""
import numpy as np

import resident_ref as R

COLUMNS = ("wstart", "wend", "wid")
# words per row of each document; None: drawn (0 .. 12 words, a 0 and a 1 among them)
ROW_WORDS = [[0], None, [0, 1, 7], None, [1, 0], [4], [1000, 0, 1500, 499, 1]]


def eval_docs():
    from hetersumgraph_amd import synth
    rng = np.random.default_rng(23)
    small = dict(vocab_size=500, sent_max_len=8, doc_max_timesteps=5)
    return R.case_docs("extremes") + [synth.make_hsg_doc(rng, 5, 30, 4, **small)]


def word_lists(docs):
    """Per document its ``(ptr int32 [N + 1], ids int32 [W])``, in ``evalsel.word_ids``' form."""
    rng = np.random.default_rng(29)
    out = []
    for d, rows in zip(docs, ROW_WORDS):
        N = len(d.sent_nodes)
        lens = np.asarray(rows if rows is not None else rng.integers(0, 13, N), np.int64)
        if rows is None:
            lens[0], lens[-1] = 0, 1
        assert len(lens) == N
        ptr = np.zeros(N + 1, np.int32)
        np.cumsum(lens, out=ptr[1:])
        W = int(ptr[-1])
        out.append((ptr, rng.integers(0, max(W // 2, 1), W).astype(np.int32)))
    return out


def store_columns(words):
    """The store's eval-view columns for the documents' word lists."""
    wstart = np.concatenate([[0], np.cumsum([len(ids) for _, ids in words])]).astype(np.int64)
    return dict(wstart=wstart, wend=np.concatenate([p[1:] for p, _ in words]).astype(np.int32),
                wid=np.concatenate([ids for _, ids in words]).astype(np.int32))


def wordbase(words, pick):
    """int32 [B + 1]: the running word counts of the picked documents (0 for a pick outside)."""
    cnt = [len(words[s][1]) if 0 <= s < len(words) else 0 for s in pick]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)


def eval_pack(store, words, pick):
    """hsg_res_eval's output for the numpy store ``store`` (resident_ref.build_store)."""
    cols = store_columns(words)
    offs, wb = R.offsets(store, pick)[R.SENT], wordbase(words, pick)
    n_sent, n_words = int(offs[-1]), int(wb[-1])
    pack = np.zeros(n_sent + 1 + max(n_words, 1), np.int32)
    ss = store["starts"][R.SENT]
    for d, s in enumerate(pick):
        if not 0 <= s < store["n_docs"]:
            continue
        W = cols["wstart"][s + 1] - cols["wstart"][s]
        pack[1 + offs[d]:1 + offs[d + 1]] = wb[d] + np.clip(cols["wend"][ss[s]:ss[s + 1]], 0, W)
        pack[n_sent + 1 + wb[d]:n_sent + 1 + wb[d] + W] = cols["wid"][cols["wstart"][s]:cols["wstart"][s + 1]]
    return pack
