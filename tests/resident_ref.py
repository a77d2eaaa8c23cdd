"""numpy restatement of the resident store's batch assembly, written from the contract in
include/hsg_resident.h: a store of flat per-family columns with int64 starts and stored bases,
the running offsets of a pick list, and the gathers of hsg_res_graph / hsg_res_relation.

The store here is built on the host: a build chunk's relation comes from
``test_gpu_relbuild.expected`` (the numpy statement of hsg_rel_build) on the chunk's
concatenated documents.  Shared by the CPU tests, which pin it against ``graph.batch`` and the
relation of the concatenated batch, and by the GPU tests as the expected value."""
import numpy as np

NODE, EDGE, SENT, NFAM = 0, 1, 2, 9
SRC, DST, TYP = (lambda q: 3 + 3 * q), (lambda q: 4 + 3 * q), (lambda q: 5 + 3 * q)
KINDS = ("W2S", "S2W")
UNITS = {"W2S": (0.0, 1.0), "S2W": (1.0, 0.0)}
REL_ARRAYS = ("indptr", "src", "tf", "eid", "phantom", "cindptr", "cdst", "cperm", "src_nodes", "dst_nodes")
# family of each relation array's elements, and the family whose offset is added (None: none)
REL_FAMILY = dict(indptr=(DST, TYP), src=(TYP, SRC), tf=(TYP, None), eid=(TYP, lambda q: EDGE), phantom=(DST, None),
                  cindptr=(SRC, TYP), cdst=(TYP, DST), cperm=(TYP, TYP), src_nodes=(SRC, lambda q: NODE),
                  dst_nodes=(DST, lambda q: NODE))
REL_DTYPE = dict(indptr=np.int32, src=np.int32, tf=np.uint8, eid=np.int64, phantom=np.int32, cindptr=np.int32,
                 cdst=np.int32, cperm=np.int32, src_nodes=np.int64, dst_nodes=np.int64)


def concat(docs):
    """The structural columns of ``docs`` as one graph (test_gpu_relbuild.batch)."""
    from test_gpu_relbuild import batch
    if not docs:
        return {k: np.zeros(0, dt) for k, dt in (("src", np.int64), ("dst", np.int64), ("unit", np.float32),
                                                 ("tffrac", np.int64), ("edtype", np.float32))}
    return batch(docs)


def batch_relation(kind, docs):
    """Today's relation of the batch ``docs``: hsg_rel_build's arrays, restated in numpy."""
    from test_gpu_relbuild import expected
    b = concat(docs)
    return expected(kind, b["src"], b["dst"], b["unit"], b["tffrac"], b["edtype"])


def counts_of(doc):
    c = np.zeros(NFAM, np.int64)
    c[NODE], c[EDGE], c[SENT] = doc.n_nodes, len(doc.src), len(doc.sent_nodes)
    for q, kind in enumerate(KINDS):
        su, du = UNITS[kind]
        c[SRC(q)], c[DST(q)] = (doc.unit == su).sum(), (doc.unit == du).sum()
        c[TYP(q)] = ((doc.unit[doc.src] == su) & (doc.unit[doc.dst] == du)).sum() if len(doc.src) else 0
    return c


def build_store(docs, chunk):
    """The store of include/hsg_resident.h as numpy arrays (narrow types as documented)."""
    n = len(docs)
    counts = np.stack([counts_of(d) for d in docs])
    starts = np.zeros((NFAM, n + 1), np.int64)
    starts[:, 1:] = np.cumsum(counts, 0).T
    bases = np.zeros((NFAM, n), np.int64)
    cols = {k: [] for k in ("unit", "ndtype", "id", "sent_rank", "words", "label", "src", "dst", "tffrac", "edtype")}
    rel = [{k: [] for k in REL_ARRAYS} for _ in KINDS]
    for c0 in range(0, n, chunk):
        part = docs[c0:c0 + chunk]
        for i, d in enumerate(part):
            bases[:, c0 + i] = starts[:, c0 + i] - starts[:, c0]
            rank = np.full(d.n_nodes, -1, np.int32)
            rank[d.sent_nodes] = np.arange(len(d.sent_nodes))
            nb = bases[NODE, c0 + i]
            for k, v in (("unit", d.unit.astype(np.uint8)), ("ndtype", d.ndtype.astype(np.uint8)),
                         ("id", d.wid.astype(np.int32)), ("sent_rank", rank),
                         ("words", d.words.astype(np.int32).reshape(-1)), ("label", d.label.astype(np.uint8).reshape(-1)),
                         ("src", (d.src + nb).astype(np.int32)), ("dst", (d.dst + nb).astype(np.int32)),
                         ("tffrac", d.tffrac.astype(np.uint8)), ("edtype", d.edtype.astype(np.uint8))):
                cols[k].append(v)
        for q, kind in enumerate(KINDS):
            r = batch_relation(kind, part)
            for k in REL_ARRAYS:
                a = r[k][:-1] if k in ("indptr", "cindptr") else r[k]          # no closing element
                rel[q][k].append(np.asarray(a).astype(np.uint8 if k == "tf" else np.int32))
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
    return dict(n_docs=n, counts=counts, starts=starts, bases=bases,
                sent_len=docs[0].words.shape[1], label_len=docs[0].label.shape[1],
                cols={k: cat(v, np.int32) for k, v in cols.items()},
                rel=[{k: cat(v, np.int32) for k, v in r.items()} for r in rel])


def offsets(store, pick):
    """hsg_res_offsets: int64 [NFAM][B + 1]."""
    pick = np.asarray(pick, np.int64)
    ok = (pick >= 0) & (pick < store["n_docs"])
    cnt = np.where(ok[None, :], store["counts"][np.where(ok, pick, 0)].T, 0)
    offs = np.zeros((NFAM, len(pick) + 1), np.int64)
    offs[:, 1:] = np.cumsum(cnt, 1)
    return offs


def _gather(store, pick, offs, col, fam, add, dtype, total):
    out = np.zeros(total, dtype)
    st = store["starts"][fam]
    for d, s in enumerate(pick):
        if not 0 <= s < store["n_docs"]:
            continue
        v = col[st[s]:st[s + 1]].astype(np.int64)
        if add is not None:
            v = v + (offs[add, d] - store["bases"][add, s])
        out[offs[fam, d]:offs[fam, d] + len(v)] = v
    return out


def graph(store, pick):
    """hsg_res_graph's ten outputs, named as the batched graph's columns name them."""
    offs, c = offsets(store, pick), store["cols"]
    n, E = int(offs[NODE, -1]), int(offs[EDGE, -1])
    L, M = store["sent_len"], store["label_len"]
    g = lambda k, fam, add, dt, tot: _gather(store, pick, offs, c[k], fam, add, dt, tot)
    out = dict(unit=g("unit", NODE, None, np.float32, n), ndtype=g("ndtype", NODE, None, np.float32, n),
               id=g("id", NODE, None, np.int64, n), src=g("src", EDGE, NODE, np.int64, E),
               dst=g("dst", EDGE, NODE, np.int64, E), tffrac=g("tffrac", EDGE, None, np.int64, E),
               edtype=g("edtype", EDGE, None, np.float32, E))
    words, label, pos = np.zeros((n, L), np.int64), np.zeros((n, M), np.int64), np.zeros((n, 1), np.int64)
    ns, ss = store["starts"][NODE], store["starts"][SENT]
    for d, s in enumerate(pick):
        if not 0 <= s < store["n_docs"]:
            continue
        rank = c["sent_rank"][ns[s]:ns[s + 1]]
        rows = np.nonzero((rank >= 0) & (rank < ss[s + 1] - ss[s]))[0]
        at = offs[NODE, d] + rows
        r = ss[s] + rank[rows]
        words[at] = c["words"].reshape(-1, L)[r]
        label[at] = c["label"].reshape(-1, M)[r]
        pos[at, 0] = rank[rows] + 1
    out.update(words=words, label=label, position=pos)
    return out


def relation(store, q, pick):
    """hsg_res_relation's ten outputs for kind ``q``."""
    offs, out = offsets(store, pick), {}
    for k in REL_ARRAYS:
        fam, add = REL_FAMILY[k]
        closing = k in ("indptr", "cindptr")
        a = _gather(store, pick, offs, store["rel"][q][k], fam(q), None if add is None else add(q), REL_DTYPE[k],
                    int(offs[fam(q), -1]) + closing)
        if closing:
            a[-1] = offs[TYP(q), -1]
        out[k] = a
    return out


# ---- documents under test (shared by the CPU and GPU tests) ---------------------------------
def drop_sentence_links(doc, i):
    """``doc`` with the word links of its i-th sentence removed: a sentence without a typed edge."""
    import dataclasses
    s = doc.sent_nodes[i]
    keep = ~((doc.edtype == 0) & ((doc.src == s) | (doc.dst == s)))
    return dataclasses.replace(doc, src=doc.src[keep], dst=doc.dst[keep], tffrac=doc.tffrac[keep],
                               edtype=doc.edtype[keep])


def case_docs(name):
    from hetersumgraph_amd import synth
    rng = np.random.default_rng(11)
    small = dict(vocab_size=500, sent_max_len=8, doc_max_timesteps=5)
    if name == "jitter":
        return [synth.make_hsg_doc(rng, 12, 80, 9, k_jitter=8, isolated_words=5, **small) for _ in range(5)]
    if name == "extremes":
        return [synth.make_hsg_doc(rng, 1, 3, 2, **small),                      # one sentence
                synth.make_hsg_doc(rng, 40, 300, 20, **small),                  # a large neighbour
                drop_sentence_links(synth.make_hsg_doc(rng, 3, 5, 2, **small), 1),
                synth.make_hsg_doc(rng, 4, 0, 0, **small),                      # no word node
                synth.make_hsg_doc(rng, 2, 6, 0, **small),                      # no typed edge at all
                synth.make_hsg_doc(rng, 1, 3, 2, **small)]
    if name == "tiny257":
        return [synth.make_hsg_doc(rng, 1 + i % 3, 4, 2, k_jitter=2, **small) for i in range(257)]
    return synth.make_batch_docs(name, seed=5, n_docs=3)                      # cfg1 / cfg4 / cfg5


def todays_batch(docs):
    """``graph.batch`` of the ``to_graph`` members, on the host."""
    from hetersumgraph_amd import graph as hg, synth
    return hg.batch([synth.to_graph(d, hg.DGLGraph) for d in docs])


def upload(store, device):
    """The numpy store on ``device``: (ctypes hsg_res_store, the tensors that back it)."""
    import torch
    from hetersumgraph_amd import _lib
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    keep = dict(starts=t(store["starts"]), bases=t(store["bases"]), cols={k: t(v) for k, v in store["cols"].items()},
                rel=[{k: t(v) for k, v in r.items()} for r in store["rel"]])
    p = _lib.ptr
    cs = _lib.HsgResStore(store["n_docs"], p(keep["starts"]), p(keep["bases"]), store["sent_len"], store["label_len"],
                          *[p(keep["cols"][k]) for k in ("unit", "ndtype", "id", "sent_rank", "words", "label", "src",
                                                         "dst", "tffrac", "edtype")],
                          (_lib.HsgResRel * 2)(*[_lib.HsgResRel(*[p(r[k]) for k in REL_ARRAYS]) for r in keep["rel"]]))
    return cs, keep
