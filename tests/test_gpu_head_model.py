"""HSumGraph / HSumDocGraph on the native model glue (path_options(HSG_MODEL_GLUE="1")):
the golden contract of tests/test_gpu_model.py with its rules unchanged, the same set of
parameter gradients and state_dict keys as the default path, no stale derived weight at
the second step, bitwise-reproducible HDSG logits, and a default path that does not touch
the new code."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_ref as R
from helpers import build_graph, load_fixture, projections
from test_gpu_model import build_model

pytestmark = pytest.mark.gpu

CASES = [("model_hsg", "HSumGraph", 4), ("model_hdsg", "HSumDocGraph", 5), ("model_hsg_cfg1", "HSumGraph", 6)]


def _setup(name, cls, seed):
    z = load_fixture(name)
    G = build_graph(z, z["sent_words"], z["sent_label"])
    G.to(torch.device("cuda"))
    model = build_model(cls, seed, z.get("vocab_size", 500), z.get("n_iter", 2), z.get("doc_max_timesteps", 50))
    # MIOpen has no RNN backward in eval mode (tests/test_gpu_model.py): train-mode LSTM, dropout 0
    model.lstm.train()
    model.lstm.dropout = 0.0
    return z, G, model


def _loss(G, logits):
    from hetersumgraph_amd import graph as hg
    snode = G.filter_nodes(lambda n: n.data["dtype"] == 1)
    label = G.ndata["label"][snode].sum(-1)
    G.nodes[snode].data["loss"] = F.cross_entropy(logits, label, reduction="none").unsqueeze(-1)
    loss = hg.sum_nodes(G, "loss").mean()
    G.ndata.pop("loss")
    return loss


class Spy:
    """Counts (and records the tensors of) the calls of the three head functions."""

    def __init__(self, monkeypatch):
        from hetersumgraph_amd import head
        self.calls = {"sent_features": [], "doc_init": [], "sent_logits": []}
        for k in self.calls:
            monkeypatch.setattr(head, k, self._wrap(k, getattr(head, k)))

    def _wrap(self, k, fn):
        def f(*a):
            out = fn(*a)
            self.calls[k].append((a, out))
            return out
        return f


@pytest.mark.parametrize("sent_lstm", ["0", "1"])
@pytest.mark.parametrize("name,cls,seed", CASES)
def test_goldens_on_the_native_glue(monkeypatch, name, cls, seed, sent_lstm):
    from hetersumgraph_amd._lib import path_options
    from hetersumgraph_amd.module.GATStackLayer import reference_named_grads
    z, G, model = _setup(name, cls, seed)
    spy = Spy(monkeypatch)
    with path_options(HSG_MODEL_GLUE="1", HSG_SENT_LSTM=sent_lstm):
        logits = model(G)
        assert len(spy.calls["sent_features"]) == 1 and len(spy.calls["sent_logits"]) == 1
        assert len(spy.calls["doc_init"]) == (1 if cls == "HSumDocGraph" else 0)
        # tests/test_gpu_model.py:54-94, unchanged
        err = np.abs(logits.detach().cpu().double().numpy() - z["logits"]).max()
        print(f"{name}: logit max |diff| vs reference fp32 = {err:.3e}")
        assert err <= 1e-4, f"logit max |diff| {err:.3e}"
        err64 = np.abs(logits.detach().cpu().double().numpy() - z["logits64"]).max()
        assert err64 <= 1e-4
        loss = _loss(G, logits)
        assert abs(loss.item() - float(z["loss64"])) <= 1e-4
        loss.backward()
    n = 0
    for k, grad in reference_named_grads(model):
        key = f"grad.{k}"
        if grad is None:
            continue
        if key in z:
            ref = z[key].astype(np.float64)
            got = grad.detach().cpu().double().numpy()
            assert np.abs(got - ref).max() <= 2e-3 * max(np.abs(ref).max(), 1e-3), k
            n += 1
        elif "proj." + key in z:
            got = projections(grad, seed, key)
            ref = z["proj." + key]
            assert np.abs(got - ref).max() <= 2e-3 * np.abs(ref).max() + 1e-5, k
            n += 1
    assert n >= 90


@pytest.mark.parametrize("name,cls,seed", CASES[:2])
def test_same_gradient_set_and_state_dict_keys(name, cls, seed):
    from hetersumgraph_amd._lib import path_options
    have = {}
    for glue in ("0", "1"):
        z, G, model = _setup(name, cls, seed)
        with path_options(HSG_MODEL_GLUE=glue):
            _loss(G, model(G)).backward()
        have[glue] = ({k for k, p in model.named_parameters() if p.grad is not None}, list(model.state_dict()))
    assert have["0"][0] == have["1"][0] and len(have["1"][0]) > 50
    assert have["0"][1] == have["1"][1]
    assert "sent_pos_embed.weight" not in have["1"][0]


@pytest.mark.parametrize("name,cls,seed", CASES[:2])
def test_second_forward_uses_the_updated_weights(monkeypatch, name, cls, seed):
    """forward, backward, optimizer.step(), forward: the second forward's sentence features
    and logits match tests/head_ref.py evaluated with the UPDATED weights (4 x yard), and
    are far from the same formulas with the first step's weights."""
    from hetersumgraph_amd._lib import path_options
    z, G, model = _setup(name, cls, seed)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
    glue = ("cnn_proj", "lstm_proj", "n_feature_proj", "wh")

    def weights():
        w = {k: getattr(model, k).weight.detach().cpu().clone() for k in glue}
        w.update({k + ".b": getattr(model, k).bias.detach().cpu().clone() for k in glue if getattr(model, k).bias is not None})
        return w
    old = weights()
    with path_options(HSG_MODEL_GLUE="1"):
        _loss(G, model(G)).backward()
        opt.step()
        spy = Spy(monkeypatch)
        with torch.no_grad():
            model(G)
    new = weights()
    (ngram, pos, P, L, *_), S = spy.calls["sent_features"][0]
    (state, lay, _), logits = spy.calls["sent_logits"][0]

    def ref_S(w, dtype):
        c = dict(ngram=ngram.cpu(), pos=pos.cpu(), P=P.detach().cpu(), L=L.cpu(), Wc=w["cnn_proj"], bc=w["cnn_proj.b"],
                 Wl=w["lstm_proj"], bl=w["lstm_proj.b"], Wn=w["n_feature_proj"], dS=torch.zeros(len(pos), 64))
        return R.sent_features(c, dtype)["S"]

    def ref_logits(w, dtype):
        c = R.cast(dict(state=state.cpu(), Wh=w["wh"], bh=w["wh.b"]), dtype)
        if lay is None:
            return c["state"] @ c["Wh"].t() + c["bh"]
        a, b = lay.sent_super.cpu().long(), lay.doc_super.cpu().long()
        return c["state"][a] @ c["Wh"][:, :64].t() + c["state"][b] @ c["Wh"][:, 64:].t() + c["bh"]

    for what, got, ref in (("S", S, ref_S), ("logits", logits, ref_logits)):
        r64 = ref(new, torch.float64)
        yard = float((ref(new, torch.float32).double() - r64).abs().max())
        err = float((got.double().cpu() - r64).abs().max())
        stale = float((ref(old, torch.float64) - r64).abs().max())
        print(f"{name} {what}: err {err:.3e} yard {yard:.3e} stale-weight distance {stale:.3e}")
        assert yard > 0 and err <= R.FACTOR * yard, (what, err, yard)
        assert stale > 100 * R.FACTOR * yard, (what, stale, yard)


def test_hdsg_logits_are_bitwise_reproducible():
    from hetersumgraph_amd._lib import path_options
    z, G, model = _setup("model_hdsg", "HSumDocGraph", 5)
    model.eval()
    outs = []
    with path_options(HSG_MODEL_GLUE="1", HSG_SENT_LSTM="1"), torch.no_grad():
        for _ in range(2):
            outs.append(model(G).clone())
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("name,cls,seed", CASES[:2])
def test_default_path_does_not_touch_the_new_code(monkeypatch, name, cls, seed):
    from hetersumgraph_amd import head
    z, G, model = _setup(name, cls, seed)

    def boom(*a, **k):
        raise AssertionError("the default path called the native glue")
    for k in ("sent_features", "doc_init", "sent_logits"):
        monkeypatch.setattr(head, k, boom)
    logits = model(G)
    assert np.abs(logits.detach().cpu().double().numpy() - z["logits"]).max() <= 1e-4
