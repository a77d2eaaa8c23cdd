"""HSumGraph with the sentence CNN on its token paths (path_options(HSG_SENT_CNN="dw" |
"tokens")) against the switch off, on the 4 config-1-shaped documents of
tests/test_gpu_model.py with the word embedding frozen (the reference's default): logits and
loss within the model goldens' 1e-4, every parameter gradient within 2e-3 of its largest entry,
in eval and in train mode (same seeds: the dropout draws of the other layers are unchanged), on
their own and with HSG_SENT_LSTM, HSG_MODEL_GLUE and HSG_WORD_EMBED all on -- where the frozen
table's word nodes go through the plain embedding lookup and the encoder reads the ids itself."""
import numpy as np
import pytest
import torch

from helpers import build_graph, load_fixture
from test_gpu_head_model import _loss
from test_gpu_model import build_model

pytestmark = pytest.mark.gpu

OTHERS = dict(HSG_SENT_LSTM="1", HSG_MODEL_GLUE="1", HSG_WORD_EMBED="1")


@pytest.fixture(scope="module")
def setup():
    z = load_fixture("model_hsg_cfg1")
    G = build_graph(z, z["sent_words"], z["sent_label"])
    G.to(torch.device("cuda"))
    model = build_model("HSumGraph", 6, z.get("vocab_size", 500), z.get("n_iter", 2), z.get("doc_max_timesteps", 50))
    model._embed.weight.requires_grad_(False)
    return z, G, model


def _step(model, G, train, **options):
    from hetersumgraph_amd import rng
    from hetersumgraph_amd._lib import path_options
    model.train(train)
    if not train:                       # MIOpen has no RNN backward in eval mode (tests/test_gpu_model.py)
        model.lstm.train()
        model.lstm.dropout = 0.0
    torch.manual_seed(1234)
    torch.cuda.manual_seed_all(1234)
    rng.manual_seed(1234)
    model.zero_grad(set_to_none=True)
    with path_options(**options):
        logits = model(G)
        loss = _loss(G, logits)
        loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return logits.detach().clone(), loss.item(), grads


@pytest.mark.parametrize("others", [False, True], ids=["alone", "all_switches"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_model_with_each_switch_value(monkeypatch, setup, train, others):
    from hetersumgraph_amd import HiGraph, cnn
    z, G, model = setup
    calls = dict(tokens=[], embed_batch=0)
    real, real_eb = cnn.sent_cnn_tokens, HiGraph.embed_batch

    def spy(*a, mode="tokens", **kw):
        calls["tokens"].append(mode)
        return real(*a, mode=mode, **kw)

    def spy_eb(*a, **kw):
        calls["embed_batch"] += 1
        return real_eb(*a, **kw)
    monkeypatch.setattr(cnn, "sent_cnn_tokens", spy)
    monkeypatch.setattr(HiGraph, "embed_batch", spy_eb)
    base = OTHERS if others else {}
    logits0, loss0, g0 = _step(model, G, train, HSG_SENT_CNN="0", **base)
    assert calls["tokens"] == [] and calls["embed_batch"] == (1 if others else 0)
    assert "_embed.weight" not in g0 and len(g0) > 50
    if not train:
        assert np.abs(logits0.cpu().double().numpy() - z["logits"]).max() <= 1e-4
    for mode in ("dw", "tokens"):
        calls["tokens"].clear()
        calls["embed_batch"] = 0
        logits, loss, g = _step(model, G, train, HSG_SENT_CNN=mode, **base)
        assert calls["tokens"] == [mode] and calls["embed_batch"] == 0
        err = (logits - logits0).abs().max().item()
        print(f"{mode} train={train} others={others}: logits {err:.3e}, loss {abs(loss - loss0):.3e}")
        assert bool(torch.isfinite(logits).all()) and logits.shape == logits0.shape
        assert err <= 1e-4 and abs(loss - loss0) <= 1e-4
        if not train:
            assert np.abs(logits.cpu().double().numpy() - z["logits"]).max() <= 1e-4
            assert abs(loss - float(z["loss64"])) <= 1e-4
        assert set(g) == set(g0)
        for k in g:
            bound = 2e-3 * max(g0[k].abs().max().item(), 1e-3)
            assert (g[k] - g0[k]).abs().max().item() <= bound, k
