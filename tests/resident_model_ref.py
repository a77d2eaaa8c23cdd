"""numpy restatement of the model view of a resident batch, written from the contract in
include/hsg_resident_model.h: every output of hsg_res_model from the documents' ``DocArrays``
and the pick list, plus the host facts the store keeps beside them (row counts, distinct
tokens, the largest token id).  A pick outside the documents is an empty document.

Shared by the CPU tests, which pin it against today's host constructions on ``graph.batch`` of
the same members, and by the GPU tests as the expected value."""
import numpy as np

OUTPUTS = ("sent_nodes", "sent_ids", "sent_pos", "sent_len", "rowoff", "doc_off", "prev", "tfidf_index")


def doc_lengths(doc):
    """(length [N] = (words != 0).sum(1), the exclusive prefix of length + 1 inside the document)."""
    length = (np.asarray(doc.words) != 0).sum(1).astype(np.int64)
    pre = np.concatenate([[0], np.cumsum(length + 1)[:-1]]).astype(np.int64) if len(length) else np.zeros(0, np.int64)
    return length, pre


def doc_rows(doc):
    return int((doc_lengths(doc)[0] + 1).sum())


def doc_distinct(doc):
    w = np.unique(np.asarray(doc.words))
    return int((w != 0).sum())


def rowbase(docs, pick):
    """int32 [B + 1]: the CNN rows of the documents before each picked one."""
    rows = [doc_rows(docs[s]) if 0 <= s < len(docs) else 0 for s in pick]
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)


def model_view(docs, pick):
    """The eight outputs of hsg_res_model for ``pick`` (positions into ``docs``), named as the header names them."""
    picked = [docs[s] if 0 <= s < len(docs) else None for s in pick]
    L = docs[0].words.shape[1]
    n_s = sum(len(d.sent_nodes) for d in picked if d is not None)
    out = dict(sent_nodes=[], sent_ids=[], sent_pos=[], sent_len=[], rowoff=[], prev=[], tfidf_index=[])
    doc_off, base = [0], rowbase(docs, pick)
    node0 = g0 = 0
    for d, doc in enumerate(picked):
        if doc is None:
            doc_off.append(g0)
            continue
        N = len(doc.sent_nodes)
        length, pre = doc_lengths(doc)
        rank = np.full(doc.n_nodes, -1, np.int64)
        rank[doc.sent_nodes] = np.arange(N)
        nodes = np.zeros(N, np.int64)
        for i in range(doc.n_nodes):                      # the node with rank r writes row r
            if rank[i] >= 0:
                nodes[rank[i]] = node0 + i
        g = g0 + np.arange(N, dtype=np.int64)
        out["sent_nodes"].append(nodes)
        out["sent_ids"].append(np.asarray(doc.words, np.int64))
        out["sent_pos"].append(np.arange(1, N + 1, dtype=np.int64))
        out["sent_len"].append(length)
        out["rowoff"].append((base[d] + pre).astype(np.int32))
        out["prev"].append(np.stack([np.where(np.arange(N) > 0, g - 1, n_s), np.where(np.arange(N) < N - 1, g + 1, n_s)], 1))
        out["tfidf_index"].append(np.where(np.asarray(doc.edtype) == 0, np.asarray(doc.tffrac, np.int64), -1))
        node0 += doc.n_nodes
        g0 += N
        doc_off.append(g0)
    cat = lambda k, shape, dt: np.concatenate(out[k]).astype(dt) if out[k] else np.zeros(shape, dt)
    res = dict(sent_nodes=cat("sent_nodes", 0, np.int64), sent_ids=cat("sent_ids", (0, L), np.int64),
               sent_pos=cat("sent_pos", 0, np.int64), sent_len=cat("sent_len", 0, np.int64),
               prev=cat("prev", (0, 2), np.int64), tfidf_index=cat("tfidf_index", 0, np.int64),
               doc_off=np.asarray(doc_off, np.int32))
    res["rowoff"] = np.concatenate([cat("rowoff", 0, np.int32), base[-1:]]).astype(np.int32)
    return res


def host_facts(docs, pick):
    """(rows, bound, max_token, glen): the CNN row count, 1 + the sum of the documents' distinct
    non-zero tokens, the largest token id of ALL documents, the sentences per picked document."""
    picked = [docs[s] for s in pick if 0 <= s < len(docs)]
    return (int(rowbase(docs, pick)[-1]), 1 + sum(doc_distinct(d) for d in picked),
            max(int(np.asarray(d.words).max()) for d in docs), [len(d.sent_nodes) for d in picked])


def todays(G):
    """What today's code builds on the batch ``G`` (a graph on any device): the same eight
    arrays from ``node_ids``, ``G.ndata``, ``cnn._layout``'s rule stated with torch,
    ``sentence_counts`` + ``lstm.DocLayout`` and ``register_tfidf_table``'s ``torch.where``;
    plus the word node list and the row count."""
    import torch
    from hetersumgraph_amd import HiGraph, lstm
    sn = HiGraph.node_ids(G, "dtype", 1.0)
    ids = G.ndata["words"][sn]
    nz = ids != 0
    length = nz.sum(1)
    rowoff = torch.zeros(ids.shape[0] + 1, dtype=torch.int32, device=ids.device)
    torch.cumsum(length + 1, 0, out=rowoff[1:])
    glen = HiGraph.sentence_counts(G)
    lay = lstm.DocLayout(tuple(glen), G.device)
    tf = G.edata["tffrac"].long()
    out = dict(sent_nodes=sn, sent_ids=ids, sent_pos=G.ndata["position"][sn].view(-1), sent_len=length, rowoff=rowoff,
               doc_off=lay.doc_off, prev=lay.prev, tfidf_index=torch.where(G.edata["dtype"] == 0, tf, torch.full_like(tf, -1)),
               word_nodes=HiGraph.node_ids(G, "unit", 0.0))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["rows"], out["glen"] = int(rowoff[-1]), list(glen)
    return out


def view_columns(docs):
    """The store's two SENT columns (include/hsg_resident_model.h): tok_len, tok_row, int32."""
    parts = [doc_lengths(d) for d in docs]
    return (np.concatenate([p[0] for p in parts]).astype(np.int32),
            np.concatenate([p[1] for p in parts]).astype(np.int32))


# ---- documents under test --------------------------------------------------------------------
SMALL = dict(vocab_size=500, sent_max_len=12, doc_max_timesteps=8)


def with_rows(doc, rows):
    """``doc`` with token rows replaced: {sentence: number of leading tokens kept or filled}."""
    import dataclasses
    words = np.asarray(doc.words).copy()
    for i, n in rows.items():
        words[i] = 0
        words[i, :n] = 5 + np.arange(n)
    return dataclasses.replace(doc, words=words)


def model_docs(kind="hsg"):
    """Toy documents a toy model runs (positions within doc_max_timesteps = 8, L = 12): five
    HSG documents of 3, 5, 7, 1 and 5 sentences -- the second with a sentence without PAD
    (length L) and an all-PAD sentence (length 0), the fourth of one sentence -- or three HDSG
    examples with doc nodes."""
    from hetersumgraph_amd import synth
    rng = np.random.default_rng(23)
    if kind == "hdsg":
        return [synth.make_hdsg_example(rng, ds, 30, 5, 8, **SMALL) for ds in ((2, 3), (4, 1, 2), (3,))]
    docs = [synth.make_hsg_doc(rng, N, 40, 5, k_jitter=3, **SMALL) for N in (3, 5, 7, 1, 5)]
    docs[1] = with_rows(docs[1], {0: SMALL["sent_max_len"], 2: 0})
    return docs


# ---- documents that cannot carry the view (the store declines it, naming the document) ----------
def broken(doc, how):
    import dataclasses
    words = np.asarray(doc.words).copy()
    if how == "inner_pad":                        # a token behind the first PAD
        row = int(np.argmax((words != 0).sum(1) < words.shape[1] - 1))
        words[row, (words[row] != 0).sum() + 1] = 7
        return dataclasses.replace(doc, words=words)
    if how == "negative":
        words[0, 0] = -3
        return dataclasses.replace(doc, words=words)
    if how == "order":                            # the sentence nodes listed in another order
        sn = np.asarray(doc.sent_nodes).copy()
        sn[[0, 1]] = sn[[1, 0]]
        return dataclasses.replace(doc, sent_nodes=sn)
    raise KeyError(how)
