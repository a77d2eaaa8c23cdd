"""HSumGraph with path_options(HSG_SENT_LSTM="2") -- the sentence LSTM with packed weights
and one weight-gradient kernel per layer -- against HSG_SENT_LSTM="1", in train mode over
three optimizer steps from the same weights and the same dropout seed (the smallest golden
graph of tests/test_gpu_model.py, the small _HPS of tests/test_gpu_lstm.py).

Step 1 starts from equal weights, and the forward of "2" is bitwise that of "1", so its
logits are bitwise equal.  The LSTM's weight gradients then differ by rounding (another
summation order), so from step 2 on the weights do: the loss at steps 2 and 3 agrees within
the project's 1e-4 contract.  A shape the kernels do not cover (lstm_hidden_state=64) falls
back to the vendor nn.LSTM exactly as "0" does.
"""
import pytest
import torch

import model_ref as M
import test_gpu_lstm as T
import weights
from helpers import build_graph, load_fixture
from test_gpu_head_model import _loss

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
SEED = M.SEEDS["model_hsg"]


def _model_and_graph(**kw):
    from hetersumgraph_amd import HiGraph
    z = load_fixture("model_hsg")
    G = build_graph(z, z["sent_words"], z["sent_label"])
    G.to(torch.device("cuda"))
    hps = T._HPS(vocab_size=int(z.get("vocab_size", 500)), doc_max_timesteps=int(z.get("doc_max_timesteps", 50)), **kw)
    torch.manual_seed(4)
    model = HiGraph.HSumGraph(hps, torch.nn.Embedding(hps.vocab_size, 300, padding_idx=0))
    weights.seed_module(model, 4)
    return model.cuda(), G


def trajectory(mode, steps=3):
    from hetersumgraph_amd import lstm as hl, rng
    from hetersumgraph_amd._lib import path_options
    model, G = _model_and_graph()
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=M.LR)
    rng.manual_seed(SEED)
    node = hl._SentLSTMFused if mode == "2" else hl._SentLSTM
    calls, real = [], node.apply
    out = []
    with pytest.MonkeyPatch.context() as mp, path_options(HSG_SENT_LSTM=mode):
        mp.setattr(node, "apply", lambda *a: (calls.append(1), real(*a))[1])
        for _ in range(steps):
            rng.advance_all()
            logits = model(G)
            loss = _loss(G, logits)
            loss.backward()
            out.append((logits.detach().clone(), loss.detach().clone(),
                        {n: p.grad.clone() for n, p in model.lstm.named_parameters()}))
            opt.step()
            opt.zero_grad(set_to_none=True)
    assert len(calls) == steps, f"HSG_SENT_LSTM={mode} did not reach its autograd node"
    return out


def test_three_train_steps_against_mode_1():
    one, two = trajectory("1"), trajectory("2")
    assert torch.equal(two[0][0], one[0][0])              # step 1: bitwise
    assert torch.equal(two[0][1], one[0][1])
    for k in (1, 2):
        d = abs(two[k][1].item() - one[k][1].item())
        print(f"step {k + 1}: loss {two[k][1].item():.6f} vs {one[k][1].item():.6f}, |diff| {d:.3e}")
        assert d <= LOSS_TOL
        assert (two[k][0] - one[k][0]).abs().max().item() <= 1e-4
    # the new weight-gradient kernel ran: the same gradients up to rounding, not the same bits
    g1, g2 = one[0][2], two[0][2]
    assert any(not torch.equal(g1[n], g2[n]) for n in g1)
    for n in g1:
        scale = max(g1[n].abs().max().item(), 1e-3)
        assert (g1[n] - g2[n]).abs().max().item() <= 2e-3 * scale, n
        if n.startswith("bias_ih"):
            assert torch.equal(g2[n], g2[n.replace("bias_ih", "bias_hh")]), n


def test_uncovered_shape_falls_back_as_mode_0():
    from hetersumgraph_amd import _lib, lstm as hl
    model, _ = _model_and_graph(lstm_hidden_state=64)
    model.eval()
    lens = [5, 3, 1]                                      # today's path packs with enforce_sorted
    x = T.make_rows(31, lens, 1)[0].cuda()
    assert not hl.native_lstm_ok(x, model.lstm) and not hl.fused_lstm_ok(x, model.lstm)
    with torch.no_grad():
        off = model._sent_lstm_rows(x, lens)
        with _lib.path_options(HSG_SENT_LSTM="2"):
            on = model._sent_lstm_rows(x, lens)
    assert torch.equal(on, off)
