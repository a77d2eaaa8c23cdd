"""HSumGraph with the native sentence LSTM switched on (path_options(HSG_SENT_LSTM="1"))
against the reference's own modules (the smallest golden of tests/test_gpu_model.py) and
against the switch-off path: eval-mode logits within the 1e-4 contract of both, and the
same state_dict keys either way."""
import numpy as np
import pytest
import torch

import weights
from helpers import build_graph, load_fixture

pytestmark = pytest.mark.gpu


class _HPS:
    def __init__(self, **kw):
        d = dict(n_iter=2, word_emb_dim=300, feat_embed_size=50, n_feature_size=128, hidden_size=64, n_head=8,
                 atten_dropout_prob=0.1, ffn_inner_hidden_size=512, ffn_dropout_prob=0.1, doc_max_timesteps=50,
                 lstm_hidden_state=128, lstm_layers=2, bidirectional=True, sent_max_len=100, cuda=True,
                 vocab_size=500)
        d.update(kw)
        self.__dict__.update(d)


def test_model_logits_with_native_lstm():
    from hetersumgraph_amd import HiGraph, _lib, lstm as hl
    z = load_fixture("model_hsg")
    G = build_graph(z, z["sent_words"], z["sent_label"])
    G.to(torch.device("cuda"))
    hps = _HPS(vocab_size=int(z.get("vocab_size", 500)), n_iter=int(z.get("n_iter", 2)),
               doc_max_timesteps=int(z.get("doc_max_timesteps", 50)))
    torch.manual_seed(4)
    model = HiGraph.HSumGraph(hps, torch.nn.Embedding(hps.vocab_size, 300, padding_idx=0))
    weights.seed_module(model, 4)
    model = model.eval().cuda()
    calls = []
    real = hl._SentLSTM.apply
    with torch.no_grad():
        keys_off = list(model.state_dict().keys())
        logits_off = model(G)
        with _lib.path_options(HSG_SENT_LSTM="1"):
            hl._SentLSTM.apply = lambda *a: (calls.append(1), real(*a))[1]
            try:
                logits_on = model(G)
            finally:
                hl._SentLSTM.apply = real
            keys_on = list(model.state_dict().keys())
    assert calls, "the switch did not reach the native LSTM"
    on = logits_on.cpu().double().numpy()
    err = np.abs(on - z["logits"]).max()
    err_off = np.abs(on - logits_off.cpu().double().numpy()).max()
    print(f"native-LSTM logits: max|diff| vs golden {err:.3e}, vs switch-off {err_off:.3e}")
    assert err <= 1e-4 and err_off <= 1e-4
    assert keys_on == keys_off
