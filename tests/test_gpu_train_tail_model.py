"""The two training-step tails on identical inputs: one forward and backward of HSumGraph
on the four cfg1-shaped documents of tests/test_gpu_model.py, then -- from clones of the
same logits, gradients and parameters -- train.py:115-135's tail as torch runs it (cross
entropy + sum_nodes + mean, clip_grad_norm_, torch.optim.Adam) and the native one
(loss.sentence_loss, optim.Adam(max_grad_norm=1.0)).  Loss, dlogits and the parameters
after one step agree within the tolerances of test_gpu_doc_ce.py / test_gpu_optim.py (2x
the torch fp32 tail's error against the CPU fp64 oracle, floored at 4 ulp).  Comparing the
tails alone keeps the chaotic drift between two whole trainings out of the check."""
import pytest
import torch
import torch.nn.functional as F

import train_ref
from helpers import build_graph, load_fixture

pytestmark = pytest.mark.gpu

LR, MAX_NORM = 5e-4, 1.0


def test_native_tail_matches_torch_tail():
    from hetersumgraph_amd import HiGraph, loss, optim
    from hetersumgraph_amd import graph as hg
    from test_gpu_model import build_model
    z = load_fixture("model_hsg_cfg1")
    G = build_graph(z, z["sent_words"], z["sent_label"])
    G.to(torch.device("cuda"))
    model = build_model("HSumGraph", 6, z.get("vocab_size", 500), z.get("n_iter", 2), z.get("doc_max_timesteps", 50))
    model.lstm.train()
    model.lstm.dropout = 0.0
    logits = model(G)
    snode = G.filter_nodes(lambda n: n.data["dtype"] == 1)
    label = G.ndata["label"][snode].sum(-1)
    lens = HiGraph.sentence_counts(G)
    assert len(lens) == 4 and sum(lens) == logits.shape[0]

    # --- the torch tail's loss (train.py:115-119), and the backward both tails share
    zt = logits.detach().clone().requires_grad_()
    G.nodes[snode].data["loss"] = F.cross_entropy(zt, label, reduction="none").unsqueeze(-1)
    loss_t = hg.sum_nodes(G, "loss").mean()
    (dz_t,) = torch.autograd.grad(loss_t, zt)
    G.ndata.pop("loss")
    logits.backward(dz_t)
    named = [(k, p) for k, p in model.named_parameters() if p.grad is not None]
    assert len(named) >= 40
    p0 = [p.detach().clone() for _, p in named]
    g0 = [p.grad.detach().clone() for _, p in named]

    # --- the native loss
    zn = logits.detach().clone().requires_grad_()
    loss_n = loss.sentence_loss(G, zn)
    (dz_n,) = torch.autograd.grad(loss_n, zn)
    assert "loss" not in G.ndata
    r64 = train_ref.doc_ce(logits, label, lens, torch.float64)
    train_ref.assert_within(loss_n, r64[2], loss_t, "loss")
    train_ref.assert_within(dz_n, r64[3], dz_t, "dlogits")
    kept = loss.sentence_loss(G, zn, keep_node_loss=True)
    assert torch.equal(kept, loss_n)
    train_ref.assert_within(G.ndata["loss"][snode].squeeze(-1), r64[0], F.cross_entropy(zt, label, reduction="none"),
                            "node loss column")
    G.ndata.pop("loss")

    # --- clip + Adam: torch on the device, native, and the fp64 oracle on the CPU
    def copies():
        ps = [torch.nn.Parameter(p.clone()) for p in p0]
        for p, g in zip(ps, g0):
            p.grad = g.clone()
        return ps
    pt = copies()
    norm_t = torch.nn.utils.clip_grad_norm_(pt, MAX_NORM)
    torch.optim.Adam(pt, lr=LR).step()
    pn = copies()
    opt = optim.Adam(pn, lr=LR, max_grad_norm=MAX_NORM)
    opt.step()
    flat = lambda ts: [t.reshape(-1) for t in ts]
    p64, _, _, n64, _ = train_ref.adam_run(flat(p0), [flat(g0)], torch.float64, max_norm=MAX_NORM, lr=LR)
    print(f"grad norm: native {float(opt.last_grad_norm):.9g}, torch {float(norm_t):.9g}, fp64 {float(n64[0]):.12g}")
    assert abs(float(opt.last_grad_norm) - float(n64[0])) <= 1e-6 * float(n64[0])
    worst = 0.0
    for (k, _), a, b, c in zip(named, pn, p64, pt):
        e, y, w = train_ref.excess(a.detach().reshape(-1), b, c.detach().reshape(-1))
        worst = max(worst, w)
        assert w <= 1.0, f"{k}: error {e:.3e}, torch fp32 {y:.3e}, error / allowed {w:.3f}"
    print(f"parameters after one step: worst error / allowed {worst:.3f} over {len(named)} tensors")
    for a, g in zip(pn, g0):
        assert torch.equal(a.grad, g)                    # the fold-in leaves .grad unscaled

    # --- a second native step in the same process
    opt.step()
    assert opt.step_count() == 2
    assert all(bool(torch.isfinite(a).all()) for a in pn)
