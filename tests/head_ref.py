"""The model glue restated with plain torch on the CPU (fp64 or fp32): the formulas of
include/hsg_model.h and their gradients written out, not differentiated, plus the seeded
cases and HDSG layouts the CPU and GPU tests share.

    x = ngram + P[pos];  F = [x Wc^T + bc | L Wl^T + bl];  S = F Wn^T
    init[row(s)] = S[s];  init[row(d)] = (inv_cnt[d] * sum_{(s, d)} S[s]) Wd^T
    logits_i = Wh[:, :Hs] state[sent_super[i]] + Wh[:, Hs:] state[doc_super[i]] + bh
"""
import numpy as np
import torch

DIMS = [(300, 128, 256, 64), (300, 128, 128, 64)]          # (E, Fn, Lw, Hs)
N_POS = 51
ROWS_PER_BLOCK = 4                                         # hsg_sentfeat_rows (asserted on the GPU)
ROW_COUNTS = [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 2 * ROWS_PER_BLOCK + 1, 70]


def cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


# ------------------------------------------------------------------ sentence features
def linear_init(out_f, in_f, gen, bias=True):
    """nn.Linear's init scale: U(-1/sqrt(in), 1/sqrt(in))."""
    b = 1.0 / np.sqrt(in_f)
    w = (torch.rand(out_f, in_f, generator=gen) * 2 - 1) * b
    return (w, (torch.rand(out_f, generator=gen) * 2 - 1) * b) if bias else w


def sent_case(n, dims, seed=0):
    """fp32 inputs of one sentence-feature case; L is a strided view (pitch Lw + 24)."""
    E, Fn, Lw, Hs = dims
    g = torch.Generator().manual_seed(1000 * seed + n + Lw)
    pos = torch.randint(0, N_POS, (n,), generator=g)
    pos[0] = 0
    pos[-1] = N_POS - 1
    if n > 2:
        pos[1] = 0
    Wc, bc = linear_init(Fn, E, g)
    Wl, bl = linear_init(Fn, Lw, g)
    Lbuf = torch.randn(n, Lw + 24, generator=g)
    return dict(ngram=torch.randn(n, E, generator=g), pos=pos, P=torch.randn(N_POS, E, generator=g),
                L=Lbuf[:, 8:8 + Lw], Wc=Wc, bc=bc, Wl=Wl, bl=bl, Wn=linear_init(Hs, 2 * Fn, g, bias=False),
                dS=torch.randn(n, Hs, generator=g))


def sent_features(c, dtype):
    """All outputs and gradients of one case in `dtype`: x, F, S, dF, dngram, dL, dWc, dbc,
    dWl, dbl, dWn."""
    c = cast(c, dtype)
    Fn = c["Wc"].shape[0]
    x = c["ngram"] + c["P"][c["pos"]]
    F = torch.cat([x @ c["Wc"].t() + c["bc"], c["L"] @ c["Wl"].t() + c["bl"]], 1)
    S = F @ c["Wn"].t()
    dF = c["dS"] @ c["Wn"]
    dFc, dFl = dF[:, :Fn], dF[:, Fn:]
    return dict(x=x, F=F, S=S, dF=dF, dngram=dFc @ c["Wc"], dL=dFl @ c["Wl"], dWc=dFc.t() @ x, dbc=dFc.sum(0),
                dWl=dFl.t() @ c["L"], dbl=dFl.sum(0), dWn=c["dS"].t() @ F)


# ------------------------------------------------------------------------ HDSG layouts
def make_layout(doc_of_sent, doc_after_sentences=False, shuffle_pairs=False):
    """A layout from each sentence's doc.  Supernode order: all sentences then all docs, or
    each doc node right after its last sentence.  Returns the host lists HeadLayout takes."""
    doc_of = np.asarray(doc_of_sent, np.int64)
    n_s, n_docs = len(doc_of), int(doc_of.max()) + 1
    ps, pd = np.arange(n_s), doc_of.copy()
    if shuffle_pairs:
        perm = np.random.RandomState(3).permutation(n_s)
        ps, pd = ps[perm], pd[perm]
    if doc_after_sentences:
        last = {int(d): int(np.nonzero(doc_of == d)[0].max()) for d in range(n_docs)}
        seq = []
        for i in range(n_s):
            seq.append(i)
            seq += [n_s + d for d in range(n_docs) if last[d] == i]
    else:
        seq = list(range(n_s + n_docs))
    pos = np.asarray(seq, np.int64)
    rank = np.empty(n_s + n_docs, np.int64)
    rank[pos] = np.arange(len(pos))
    cnt = np.bincount(pd, minlength=n_docs)
    return dict(pair_s=ps, pair_d=pd, n_s=n_s, n_docs=n_docs, super_pos=pos, sent_super=rank[:n_s],
                doc_super=rank[n_s + doc_of], inv_cnt=(1.0 / cnt).astype(np.float32))


LAYOUTS = {
    "one_doc_one_sentence": make_layout([0]),
    "docs_1_2_7": make_layout([0] + [1] * 2 + [2] * 7),
    "doc_130": make_layout([0] * 130),
    "interleaved": make_layout([0, 1, 0, 1, 1, 0, 1], shuffle_pairs=True),
    "doc_after_sentences": make_layout([0] + [1] * 2 + [2] * 7, doc_after_sentences=True),
    "interleaved_doc_after": make_layout([0, 1, 0, 1, 1, 0, 1], doc_after_sentences=True),
}


def doc_case(lay, Hs=64, seed=0):
    g = torch.Generator().manual_seed(77 + seed + lay["n_s"])
    n_super = len(lay["super_pos"])
    Wh, bh = linear_init(2, 2 * Hs, g)
    return dict(S=torch.randn(lay["n_s"], Hs, generator=g), Wd=linear_init(Hs, Hs, g, bias=False),
                dInit=torch.randn(n_super, Hs, generator=g), state=torch.randn(n_super, Hs, generator=g), Wh=Wh, bh=bh,
                dlogits=torch.randn(lay["n_s"], 2, generator=g))


def hsg_case(n, Hs=64, seed=0):
    g = torch.Generator().manual_seed(99 + seed + n)
    Wh, bh = linear_init(2, Hs, g)
    return dict(state=torch.randn(n, Hs, generator=g), Wh=Wh, bh=bh, dlogits=torch.randn(n, 2, generator=g))


def doc_init(c, lay, dtype):
    """mean, init, dS, dWd of one case in `dtype` (sums in pair-list / doc order)."""
    c = cast(c, dtype)
    n_s, n_docs = lay["n_s"], lay["n_docs"]
    S, Wd, dInit = c["S"], c["Wd"], c["dInit"]
    inv = torch.from_numpy(lay["inv_cnt"]).to(dtype)
    order = np.argsort(lay["pair_d"], kind="stable")
    acc = torch.zeros(n_docs, S.shape[1], dtype=dtype)
    for e in order:
        acc[lay["pair_d"][e]] += S[lay["pair_s"][e]]
    mean = acc * inv[:, None]
    init = torch.cat([S, mean @ Wd.t()], 0)[torch.from_numpy(lay["super_pos"])]
    row = np.empty(n_s + n_docs, np.int64)
    row[lay["super_pos"]] = np.arange(len(lay["super_pos"]))
    dDoc = dInit[torch.from_numpy(row[n_s:])]
    back = dDoc @ Wd                                      # d mean-before-scale, per doc
    dS = dInit[torch.from_numpy(row[:n_s])].clone()
    for e in np.argsort(lay["pair_s"], kind="stable"):
        d = lay["pair_d"][e]
        dS[lay["pair_s"][e]] += inv[d] * back[d]
    return dict(mean=mean, init=init, dS=dS, dWd=dDoc.t() @ mean)


# ------------------------------------------------------------------------------ logits
def logits(c, lay, dtype):
    """logits, dstate and dWh | dbh (one vector: the kernels sum them together) in `dtype`.
    lay None: HSG (state rows are the sentences, Wh is [2, Hs])."""
    c = cast(c, dtype)
    state, dl = c["state"], c["dlogits"]
    Hs = state.shape[1]
    if lay is None:
        Wh = c["Wh"]
        out = state @ Wh.t() + c["bh"]
        return dict(logits=out, dstate=dl @ Wh, dWhb=torch.cat([(dl.t() @ state).reshape(-1), dl.sum(0)]))
    a, b = torch.from_numpy(lay["sent_super"]), torch.from_numpy(lay["doc_super"])
    Wh = c["Wh"]
    out = state[a] @ Wh[:, :Hs].t() + state[b] @ Wh[:, Hs:].t() + c["bh"]
    dstate = torch.zeros_like(state)
    dstate[a] = dl @ Wh[:, :Hs]
    contrib = dl @ Wh[:, Hs:]
    for i in range(len(b)):
        dstate[b[i]] += contrib[i]
    dWh = torch.cat([dl.t() @ state[a], dl.t() @ state[b]], 1)
    return dict(logits=out, dstate=dstate, dWhb=torch.cat([dWh.reshape(-1), dl.sum(0)]))


SENT_KEYS = ("x", "F", "S", "dF", "dngram", "dL", "dWc", "dbc", "dWl", "dbl", "dWn")
DOC_KEYS = ("init", "dS", "dWd")                 # mean is an exact copy for a one-sentence doc: no yardstick
LOGIT_KEYS = ("logits", "dstate", "dWhb")
FACTOR = 4                                       # tests/test_gpu_lstm.py's factor over the fp32-CPU error


def yard(c32, c64):
    """max |fp32-CPU - fp64| per output: the parity yardstick."""
    return {k: float((c32[k].double() - c64[k]).abs().max()) for k in c64}
