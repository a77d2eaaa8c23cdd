"""``g.edata['e']`` after a forward, as the reference leaves it (VERDICT r5 boundary
divergence #1; /root/reference/module/GATLayer.py:89-93, 112, 148).

Every reference head writes its attention logits on its typed edges and the column
stays on the graph, so after a forward each typed edge holds the last head's logit of
the last application over its relation. The HIP path never forms per-edge logits.
`graph.EdgeScoreColumn` keeps the last application's projected features and head
parameters per relation, and forms the rows when the column is read. Checked against
oracle/dgl_udf.py, which keeps the column as the reference's `apply_edges` writes it
(UdfGraph.e): the per-layer module path (W2S then S2W) and the fused n_iter = 2 stack,
both in eval mode.

The column is the forward's whatever happens to the parameters afterwards: read after a
backward and an optimizer step (torch's Adam, the native one) it still equals the oracle's
column at the parameters snapshotted before the step, and after a second forward it is
the second forward's -- the fused stack, the per-layer path with the T table and with a
dense foreign ``tfidfembed`` column, and S2S (the cases at the end of this file).
"""
import numpy as np
import pytest
import torch

from helpers import build_graph, gat_inputs, seeded_gat_params, synth_fixture

pytestmark = pytest.mark.gpu


def _setup(n_docs, seed):
    from hetersumgraph_amd import synth
    from hetersumgraph_amd.HiGraph import register_tfidf_table
    from oracle import dgl_udf, fused
    z = synth_fixture(synth.make_batch_docs("cfg2", seed=0)[:n_docs])
    dev = torch.device("cuda")
    G = build_graph(z).to(dev)
    Xw, Xs, T = gat_inputs(seed, int(z["n_w"]), int(z["n_s"]))
    Td = T.to(dev)
    register_tfidf_table(G, Td)
    w2s, s2w = seeded_gat_params(seed * 100 + 1, seed * 100 + 2)
    ug = dgl_udf.UdfGraph(z["g_src"], z["g_dst"], z["g_unit"], z["g_tffrac"], z["g_edtype"])
    p1 = fused.as_params(w2s, dtype=torch.float32)
    p2 = fused.as_params(s2w, dtype=torch.float32)
    return G, ug, (Xw, Xs, T, Td), w2s.to(dev), s2w.to(dev), p1, p2


def test_edge_scores_per_layer_path():
    from oracle import dgl_udf
    G, ug, (Xw, Xs, T, _), w2s, s2w, p1, p2 = _setup(4, 7)
    dev = torch.device("cuda")
    with torch.no_grad():
        s = w2s(G, Xw.to(dev), Xs.to(dev))
        w = s2w(G, Xw.to(dev), s)
    te = dgl_udf.tfidf_embed(ug, T)
    so = dgl_udf.wswgat(ug, "W2S", Xw, Xs, p1, te)
    dgl_udf.wswgat(ug, "S2W", Xw, so, p2, te)
    e = G.edata["e"].cpu()
    assert e.shape == ug.e.shape
    assert ug.e.abs().max() > 0
    assert (e - ug.e).abs().max().item() <= 1e-4, (e - ug.e).abs().max().item()
    assert torch.isfinite(w).all()


def test_edge_scores_fused_stack():
    from hetersumgraph_amd.stack import fused_stack_ok, gat_stack
    from oracle import dgl_udf
    G, ug, (Xw, Xs, T, Td), w2s, s2w, p1, p2 = _setup(6, 8)
    dev = torch.device("cuda")
    Xwd, Xsd = Xw.to(dev), Xs.to(dev).requires_grad_()
    assert fused_stack_ok(G, w2s, s2w, Td, Xwd, Xsd)
    s = gat_stack(G, w2s, s2w, Td, Xwd, Xsd, 2)
    s.sum().backward()                                   # the column outlives the backward
    dgl_udf.stack_step(ug, Xw, Xs, p1, p2, T, n_iter=2)
    e = G.edata["e"].cpu()
    err = (e - ug.e).abs().max().item()
    print(f"fused stack edata['e'] max|diff| {err:.3e}")
    assert ug.e.abs().max() > 0 and err <= 1e-4
    # the typed rows only; every other edge keeps the zero initializer
    typed = np.zeros(len(e), bool)
    for kind in ("W2S", "S2W"):
        typed[G.relation(kind).dev["eid"].cpu().numpy()] = True
    assert not e[torch.from_numpy(~typed)].any()


# --- the column after an optimizer step -------------------------------------------------
# The reference's column is a tensor written during the forward: an optimizer.step()
# between the forward and the read does not touch it.  The HIP path forms the rows on
# read, so whatever it keeps for that must not follow the parameters (updated in place;
# by the native optimizer through raw pointers).  Each case: forward, backward, one Adam
# step (lr 1e-2, so every entry moves by 1e-2), read the column -- it is the forward's,
# i.e. the oracle's at the parameters snapshotted BEFORE the step, within this file's
# 1e-4 -- then a second forward, after which it is the second forward's.  The oracle's
# own columns at the two snapshots differ by more than 1000 x 1e-4 (asserted), so a
# column formed from new weights and old features is far outside.

STEP_LR = 1e-2


def _optimizer(kind, params):
    if kind == "torch":
        return torch.optim.Adam(params, lr=STEP_LR)
    from hetersumgraph_amd import optim
    return optim.Adam(params, lr=STEP_LR)


def _dense_tfidf(G, T):
    """A foreign caller's dense per-edge tfidfembed column (HiGraph.py:146-151 gathered)."""
    idx = torch.where(G.edata["dtype"] == 0, G.edata["tffrac"], torch.full_like(G.edata["tffrac"], -1))
    return torch.where((idx >= 0).unsqueeze(1), T[idx.clamp_min(0)], torch.zeros((), device=T.device))


def _forward(path, G, w2s, s2w, T, Xw, Xs, n_iter):
    from hetersumgraph_amd.HiGraph import register_tfidf_table
    from hetersumgraph_amd.stack import fused_stack_ok, gat_stack
    if path == "layers_dense":
        G.edata["tfidfembed"] = _dense_tfidf(G, T)
    else:
        register_tfidf_table(G, T)
    if path == "fused":
        assert fused_stack_ok(G, w2s, s2w, T, Xw, Xs)
        s = gat_stack(G, w2s, s2w, T, Xw, Xs, n_iter)
        assert not torch.is_grad_enabled() or type(s.grad_fn).__name__.startswith("_GatStack")
        return s
    w, s = Xw, w2s(G, Xw, Xs)
    for _ in range(n_iter):
        w = s2w(G, w, s)
        s = w2s(G, w, s)
    return s


@pytest.mark.parametrize("opt_kind", ["torch", "native"])
@pytest.mark.parametrize("path,n_iter", [("fused", 2), ("layers_table", 1), ("layers_dense", 1)])
def test_edge_scores_after_optimizer_step(path, n_iter, opt_kind):
    import step_ref
    seed = step_ref.SEEDS["cfg2"]
    z, _, _ = step_ref.workload("cfg2")
    dev = torch.device("cuda")
    G = build_graph(z).to(dev)
    Xw, Xs, T = gat_inputs(seed, int(z["n_w"]), int(z["n_s"]))
    Xw, Xs = Xw.to(dev), Xs.to(dev).requires_grad_()
    T = T.to(dev).requires_grad_()
    w2s, s2w = seeded_gat_params(seed * 100 + 1, seed * 100 + 2)
    w2s, s2w = w2s.to(dev), s2w.to(dev)
    params = list(w2s.parameters()) + list(s2w.parameters()) + [T]
    opt = _optimizer(opt_kind, params)
    R = step_ref.upstream(seed, 0, int(z["n_s"])).to(dev, torch.float32)

    snap0 = step_ref.snapshot(w2s, s2w, T)
    col0 = step_ref.edge_column_at(z, snap0, Xw, Xs, n_iter)
    s = _forward(path, G, w2s, s2w, T, Xw, Xs, n_iter)
    s.backward(R)
    opt.step()
    torch.cuda.synchronize()
    snap1 = step_ref.snapshot(w2s, s2w, T)
    col1 = step_ref.edge_column_at(z, snap1, Xw, Xs, n_iter)
    moved = (col1 - col0).abs().max().item()
    e = G.edata["e"].cpu()
    err = (e - col0).abs().max().item()
    print(f"{path} {opt_kind}: column after the step vs the forward's {err:.3e} (vs the moved parameters' "
          f"{(e - col1).abs().max().item():.3e}; the oracle's two columns differ by {moved:.3f})")
    assert moved >= 1000 * 1e-4
    assert e.shape == col0.shape and col0.abs().max() > 0
    assert err <= 1e-4
    # a second forward: the column is now the second forward's
    opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        _forward(path, G, w2s, s2w, T, Xw, Xs, n_iter)
    err = (G.edata["e"].cpu() - col1).abs().max().item()
    print(f"{path} {opt_kind}: column after the second forward {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("opt_kind", ["torch", "native"])
def test_s2s_edge_scores_after_optimizer_step(opt_kind):
    """The same for S2S (module.GATLayer.SGATScores): the last head's attn_fc row."""
    import step_ref
    import weights
    from helpers import concat_arrays
    from hetersumgraph_amd.module.GAT import WSWGAT
    from oracle import dgl_udf, fused
    z, _, _ = step_ref.workload("cfg2")
    dev = torch.device("cuda")
    G = build_graph(z).to(dev)
    m = weights.seed_module(WSWGAT(64, 64, 8, 0.1, 512, 0.1, 50, "S2S"), 4003).eval().to(dev)
    Xs = torch.from_numpy(weights.feature(40, "Xs", (int(z["n_s"]), 64), 1.0))
    Xd = Xs.to(dev).requires_grad_()
    opt = _optimizer(opt_kind, list(m.parameters()))
    a = concat_arrays(z)

    def column():
        ug = dgl_udf.UdfGraph(a["src"], a["dst"], a["unit"], a["tffrac"], a["edtype"])
        p = fused.as_params(m, dtype=torch.float64, requires_grad=False)
        dgl_udf.wswgat(ug, "S2S", Xs.double(), Xs.double(), p, None)
        return ug.e

    col0 = column()
    out = m(G, Xd, Xd)
    out.backward(step_ref.upstream(40, 0, int(z["n_s"])).to(dev, torch.float32))
    opt.step()
    torch.cuda.synchronize()
    col1 = column()
    moved = (col1 - col0).abs().max().item()
    e = G.edata["e"].cpu()
    err = (e - col0).abs().max().item()
    print(f"S2S {opt_kind}: column after the step vs the forward's {err:.3e} (the oracle's two columns differ "
          f"by {moved:.3f})")
    assert moved >= 1000 * 1e-4
    assert col0.abs().max() > 0 and err <= 1e-4
    with torch.no_grad():
        m(G, Xd, Xd)
    assert (G.edata["e"].cpu() - col1).abs().max().item() <= 1e-4
