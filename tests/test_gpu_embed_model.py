"""HSumGraph / HSumDocGraph with a TRAINABLE word embedding on the native path
(path_options(HSG_WORD_EMBED="1")): bitwise the logits of the torch path, an embedding
gradient inside the derived bound of the fp64 sum of the same row gradients, exactly zero
padding and absent rows, bitwise reproducible; every other parameter's gradient bitwise
what the torch path gives; no stale plan at the second step; and all three opt-in switches
together in train mode.

The batches are the tiny HSG / HDSG fixtures of tests/test_gpu_head_model.py with their
token ids folded into a 200-word vocabulary and one sentence cut to a single token:
V = 200, D = 300, padding_idx = 0, requires_grad = True."""
import numpy as np
import pytest
import torch

import embed_ref as R
from helpers import build_graph, load_fixture
from test_gpu_head_model import _loss
from test_gpu_model import build_model

pytestmark = pytest.mark.gpu

V = 200
CASES = [("model_hsg", "HSumGraph", 4), ("model_hdsg", "HSumDocGraph", 5)]


def _setup(name, cls, seed):
    z = load_fixture(name)
    fold = lambda a: np.where(a > 0, (a - 1) % (V - 1) + 1, a)          # [1, 499] -> [1, 199], PAD stays 0
    z["g_wid"] = fold(z["g_wid"])
    words = fold(z["sent_words"])
    words[1, 1:] = 0                                                     # one sentence of a single token
    lens = (words != 0).sum(1)
    assert lens[1] == 1 and len(set(lens.tolist())) > 2 and len(z["g_n_nodes"]) >= 2
    G = build_graph(z, words, z["sent_label"])
    G.to(torch.device("cuda"))
    model = build_model(cls, seed, V, z.get("n_iter", 2), z.get("doc_max_timesteps", 50))
    # MIOpen has no RNN backward in eval mode (tests/test_gpu_model.py): train-mode LSTM, dropout 0
    model.lstm.train()
    model.lstm.dropout = 0.0
    assert model._embed.weight.requires_grad and model._embed.padding_idx == 0
    assert tuple(model._embed.weight.shape) == (V, 300)
    return z, G, model, words


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _step(model, G, **options):
    from hetersumgraph_amd._lib import path_options
    model.zero_grad(set_to_none=True)
    with path_options(**options):
        logits = model(G)
        _loss(G, logits).backward()
    return logits.detach().clone(), _grads(model)


@pytest.mark.parametrize("name,cls,seed", CASES)
def test_logits_bitwise_equal_to_the_torch_path(name, cls, seed):
    from hetersumgraph_amd._lib import path_options
    z, G, model, _ = _setup(name, cls, seed)
    out = {}
    for sw in ("0", "1"):
        with path_options(HSG_WORD_EMBED=sw), torch.no_grad():
            out[sw] = model(G).clone()
    assert bool(torch.isfinite(out["1"]).all())
    assert torch.equal(_bits(out["0"]), _bits(out["1"]))


@pytest.mark.parametrize("name,cls,seed", CASES)
def test_embedding_gradient_and_the_other_gradients(monkeypatch, name, cls, seed):
    from hetersumgraph_amd import HiGraph, _lib
    z, G, model, words = _setup(name, cls, seed)
    seen = {}
    real = HiGraph.embed_batch

    def spy(weight, wid, ids, pos_w, padding_idx):
        w_embed, X, layout = real(weight, wid, ids, pos_w, padding_idx)
        seen.update(wid=wid.detach().cpu().numpy(), ids=ids.detach().cpu().numpy(), calls=seen.get("calls", 0) + 1)
        w_embed.register_hook(lambda g: seen.__setitem__("dW", g.detach().cpu().numpy()))
        X.register_hook(lambda g: seen.__setitem__("dX", g.detach().cpu().numpy()))
        return w_embed, X, layout
    monkeypatch.setattr(HiGraph, "embed_batch", spy)

    _, off = _step(model, G, HSG_WORD_EMBED="0")
    assert "calls" not in seen                                           # the switch is off: today's code
    _, on = _step(model, G, HSG_WORD_EMBED="1")
    assert seen["calls"] == 1                                            # ONE node over both uses
    _, on2 = _step(model, G, HSG_WORD_EMBED="1")
    key = "_embed.weight"
    assert set(on) == set(off) and key in on

    # every other parameter: the same launches on the same inputs
    for k in on:
        if k != key:
            assert torch.equal(_bits(on[k]), _bits(off[k])), k

    # the embedding gradient against the fp64 index_add_ of the same dW and dX
    tok = np.concatenate([seen["wid"], R.cnn_tokens(seen["ids"])])
    rows = np.concatenate([seen["dW"], seen["dX"]])
    assert np.array_equal(seen["ids"], words) and rows.shape == (len(tok), 300)
    kept = torch.from_numpy(tok != 0)
    ref = torch.zeros(V, 300, dtype=torch.float64).index_add_(0, torch.from_numpy(tok)[kept],
                                                              torch.from_numpy(rows).double()[kept]).numpy()
    ref64, bound = R.reduce_f64(tok, rows, V, 0)
    assert np.abs(ref - ref64).max() <= 1e-12
    g_on, g_off = on[key].cpu().numpy(), off[key].cpu().numpy()
    err_on, err_off = np.abs(g_on - ref), np.abs(g_off - ref)
    print(f"{name}: max err on {err_on.max():.3e} off {err_off.max():.3e} max bound {bound.max():.3e}")
    assert (err_on <= bound).all() and (err_off <= bound).all()
    assert (np.abs(g_on.astype(np.float64) - g_off) <= 2 * bound).all()
    # and bit for bit the contract's order
    P = _lib.load().hsg_embed_piece_rows()
    assert np.array_equal(g_on.view(np.int32), R.reduce_f32(tok, rows, V, P, 0).view(np.int32))

    assert (g_on[0].view(np.int32) == 0).all()                           # row 0: exactly +0.0
    absent = np.setdiff1d(np.arange(V), tok)
    assert absent.size > 20 and (g_on[absent].view(np.int32) == 0).all() # tokens the batch does not hold
    assert g_on.any()
    assert torch.equal(_bits(on[key]), _bits(on2[key]))                  # two runs, bitwise


@pytest.mark.parametrize("name,cls,seed", CASES)
def test_second_forward_uses_the_updated_embedding(name, cls, seed):
    """forward, backward, Adam step with the embedding in the parameter list, forward: the
    second forward equals, bitwise, a freshly built model loaded with the updated state
    dict -- nothing cached by the first forward is read again."""
    from hetersumgraph_amd import optim
    from hetersumgraph_amd._lib import path_options
    z, G, model, _ = _setup(name, cls, seed)
    params = [p for p in model.parameters() if p.requires_grad]
    assert any(p is model._embed.weight for p in params)
    opt = optim.Adam(params, lr=1e-2)
    before = model._embed.weight.detach().clone()
    with path_options(HSG_WORD_EMBED="1"):
        first = model(G)
        _loss(G, first).backward()
        opt.step()
        with torch.no_grad():
            second = model(G).clone()
    assert not torch.equal(before, model._embed.weight.detach())
    assert not torch.equal(first.detach(), second)
    _, G2, fresh, _ = _setup(name, cls, seed + 100)
    fresh.load_state_dict(model.state_dict())
    with path_options(HSG_WORD_EMBED="1"), torch.no_grad():
        again = fresh(G2)
    assert torch.equal(_bits(second), _bits(again))
    with torch.no_grad():                                                # and the torch path agrees
        assert torch.equal(_bits(fresh(G2)), _bits(second))


@pytest.mark.parametrize("name,cls,seed", CASES)
def test_all_switches_on_in_train_mode(name, cls, seed):
    from hetersumgraph_amd import rng
    z, G, model, _ = _setup(name, cls, seed)
    model.train()
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        torch.cuda.manual_seed_all(1234)
        rng.manual_seed(1234)
        logits, grads = _step(model, G, HSG_SENT_LSTM="1", HSG_MODEL_GLUE="1", HSG_WORD_EMBED="1")
        assert bool(torch.isfinite(logits).all())
        for k, g in grads.items():
            assert bool(torch.isfinite(g).all()), k
        runs.append(grads["_embed.weight"])
    assert bool(runs[0].any())
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
