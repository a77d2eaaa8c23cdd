"""The restatement of the model glue (tests/head_ref.py) against the modules composed as
HiGraph.py composes them today, on the CPU in fp64 (<= 1e-12 relative), for the HSG and
the HDSG layouts; and the parity yardstick of tests/test_gpu_head.py -- max |fp32-CPU -
fp64| -- is nonzero for every case used there, so the GPU bound of 4 x yard is never
vacuous.  fp32 chains over 32 consecutive k summed in ascending order (the kernels' order,
without the fused multiply-add) stay inside the same bound: the reference alone does not
exhaust it."""
import numpy as np
import pytest
import torch

import head_ref as R

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _modules(c, lay):
    """nn modules carrying a case's weights, in fp64."""
    nn = torch.nn
    Fn, E = c["Wc"].shape
    Lw, Hs = c["Wl"].shape[1], c["Wn"].shape[0]
    m = dict(pe=nn.Embedding.from_pretrained(c["P"].double(), freeze=True), cnn=nn.Linear(E, Fn), lstm=nn.Linear(Lw, Fn),
             nf=nn.Linear(2 * Fn, Hs, bias=False), dn=nn.Linear(Hs, Hs, bias=False), wh=nn.Linear(Hs if lay is None else 2 * Hs, 2))
    for k, mod in m.items():
        mod.double()
    with torch.no_grad():
        m["cnn"].weight.copy_(c["Wc"]); m["cnn"].bias.copy_(c["bc"])
        m["lstm"].weight.copy_(c["Wl"]); m["lstm"].bias.copy_(c["bl"])
        m["nf"].weight.copy_(c["Wn"]); m["wh"].weight.copy_(c["Wh"]); m["wh"].bias.copy_(c["bh"])
        if "Wd" in c:
            m["dn"].weight.copy_(c["Wd"])
    return m


@pytest.mark.parametrize("layout", [None] + list(R.LAYOUTS))
@pytest.mark.parametrize("dims", R.DIMS, ids=lambda d: f"Lw{d[2]}")
def test_restatement_equals_the_composed_modules(layout, dims):
    lay = R.LAYOUTS[layout] if layout else None
    n = lay["n_s"] if lay else 9
    c = R.sent_case(n, dims)
    c.update(R.doc_case(lay) if lay else R.hsg_case(n))
    m = _modules(c, lay)
    ngram = c["ngram"].double().requires_grad_()
    L = c["L"].double().requires_grad_()
    # HiGraph.py's lines (hetersumgraph_amd/HiGraph.py: _sent_cnn_feature, set_snfeature, forward)
    cnn = m["cnn"](ngram + m["pe"](c["pos"]))
    S = m["nf"](torch.cat([cnn, m["lstm"](L)], dim=1))
    if lay is None:
        state = S
        logits = m["wh"](state)
    else:
        pd, ps = torch.from_numpy(lay["pair_d"]), torch.from_numpy(lay["pair_s"])
        acc = S.new_zeros(lay["n_docs"], S.shape[1]).index_add(0, pd, S[ps])
        doc = m["dn"](acc * torch.from_numpy(lay["inv_cnt"]).double().unsqueeze(1))
        state = torch.cat([S, doc], 0)[torch.from_numpy(lay["super_pos"])]
        logits = m["wh"](torch.cat([state[torch.from_numpy(lay["sent_super"])],
                                    state[torch.from_numpy(lay["doc_super"])]], dim=-1))
    state.retain_grad(); S.retain_grad()
    (logits * c["dlogits"].double()).sum().backward()

    # the restatement, chained the same way
    sf = R.sent_features(c, F64)
    assert _rel(sf["S"], S.detach()) <= 1e-12
    cl = dict(c, state=state.detach())
    lg = R.logits(cl, lay, F64)
    assert _rel(lg["logits"], logits.detach()) <= 1e-12
    assert _rel(lg["dstate"], state.grad) <= 1e-12
    dWhb = torch.cat([m["wh"].weight.grad.reshape(-1), m["wh"].bias.grad])
    assert _rel(lg["dWhb"], dWhb) <= 1e-12
    dS = lg["dstate"]
    if lay is not None:
        di = R.doc_init(dict(c, S=sf["S"], dInit=lg["dstate"]), lay, F64)
        assert _rel(di["init"], state.detach()) <= 1e-12
        assert _rel(di["dWd"], m["dn"].weight.grad) <= 1e-12
        dS = di["dS"]
    assert _rel(dS, S.grad) <= 1e-12
    sb = R.sent_features(dict(c, dS=dS), F64)
    for key, got in (("dngram", ngram.grad), ("dL", L.grad), ("dWc", m["cnn"].weight.grad), ("dbc", m["cnn"].bias.grad),
                     ("dWl", m["lstm"].weight.grad), ("dbl", m["lstm"].bias.grad), ("dWn", m["nf"].weight.grad)):
        assert _rel(sb[key], got) <= 1e-12, key


def _assert_nonzero(y, keys, what):
    for k in keys:
        assert y[k] > 0.0, (what, k)


@pytest.mark.parametrize("dims", R.DIMS, ids=lambda d: f"Lw{d[2]}")
@pytest.mark.parametrize("n", R.ROW_COUNTS)
def test_yardstick_nonzero_sentence_features(n, dims):
    c = R.sent_case(n, dims)
    r32, r64 = R.sent_features(c, torch.float32), R.sent_features(c, F64)
    y = R.yard(r32, r64)
    _assert_nonzero(y, R.SENT_KEYS, (n, dims))
    # the kernels' summation order: fp32 chains over 32 consecutive k, their sums added ascending
    x, Wc, Wl, Wn = (t.numpy() for t in (r32["x"], c["Wc"], c["Wl"], c["Wn"]))
    Lm = c["L"].contiguous().numpy()

    def chain(A, B):                                   # A [n, K] @ B [m, K]^T: 32-wide chains, summed ascending
        acc = np.zeros((A.shape[0], B.shape[0]), np.float32)
        loc = np.zeros_like(acc)
        for k in range(A.shape[1]):
            loc += A[:, k:k + 1] * B[None, :, k]
            if (k + 1) % 32 == 0 or k + 1 == A.shape[1]:
                acc, loc = acc + loc, np.zeros_like(acc)
        return acc
    F = np.concatenate([chain(x, Wc) + c["bc"].numpy(), chain(Lm, Wl) + c["bl"].numpy()], 1)
    S = chain(F, Wn)
    dF = chain(c["dS"].numpy(), np.ascontiguousarray(Wn.T))
    dng = chain(dF[:, :128], np.ascontiguousarray(Wc.T))
    for k, got in (("F", F), ("S", S), ("dF", dF), ("dngram", dng)):
        err = float(np.abs(got.astype(np.float64) - r64[k].numpy()).max())
        assert err <= R.FACTOR * y[k], (k, err, y[k])


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
def test_yardstick_nonzero_hdsg(layout):
    lay = R.LAYOUTS[layout]
    c = R.doc_case(lay)
    _assert_nonzero(R.yard(R.doc_init(c, lay, torch.float32), R.doc_init(c, lay, F64)), R.DOC_KEYS, layout)
    _assert_nonzero(R.yard(R.logits(c, lay, torch.float32), R.logits(c, lay, F64)), R.LOGIT_KEYS, layout)


@pytest.mark.parametrize("n", R.ROW_COUNTS)
def test_yardstick_nonzero_hsg_logits(n):
    c = R.hsg_case(n)
    _assert_nonzero(R.yard(R.logits(c, None, torch.float32), R.logits(c, None, F64)), R.LOGIT_KEYS, n)


def test_layouts_cover_the_issue_list():
    sizes = {k: np.bincount(v["pair_d"]).tolist() for k, v in R.LAYOUTS.items()}
    assert sizes["one_doc_one_sentence"] == [1] and sizes["docs_1_2_7"] == [1, 2, 7] and sizes["doc_130"] == [130]
    il = R.LAYOUTS["interleaved"]
    d_of = il["pair_d"][np.argsort(il["pair_s"])]
    assert (np.diff(d_of) != 0).sum() > 2                          # a doc's sentences are not contiguous
    da = R.LAYOUTS["doc_after_sentences"]
    assert (da["doc_super"] > da["sent_super"]).all() and da["super_pos"][-1] >= da["n_s"] and da["super_pos"][1] >= da["n_s"]
