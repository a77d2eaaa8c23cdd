"""The HSG_SENT_LSTM switch without a GPU: on CPU tensors native_lstm_ok is false, so
HSumGraph._sent_lstm_rows runs today's nn.LSTM path bit for bit and nothing raises; and
the row-offset cache of hetersumgraph_amd.lstm is keyed by the glen tuple."""
import torch
import torch.nn as nn

from hetersumgraph_amd import lstm as hl


class _HPS:
    def __init__(self, **kw):
        d = dict(n_iter=1, word_emb_dim=300, feat_embed_size=50, n_feature_size=128, hidden_size=64, n_head=8,
                 atten_dropout_prob=0.1, ffn_inner_hidden_size=512, ffn_dropout_prob=0.1, doc_max_timesteps=50,
                 lstm_hidden_state=128, lstm_layers=2, bidirectional=True, sent_max_len=100, cuda=False,
                 vocab_size=50)
        d.update(kw)
        self.__dict__.update(d)


def test_switch_on_cpu_is_todays_path():
    from hetersumgraph_amd import HiGraph, _lib
    torch.manual_seed(0)
    hps = _HPS()
    model = HiGraph.HSumGraph(hps, nn.Embedding(hps.vocab_size, 300, padding_idx=0)).eval()
    glen = [6, 3, 2, 1]                                   # today's path packs with enforce_sorted
    x = torch.randn(sum(glen), 300)
    assert not hl.native_lstm_ok(x, model.lstm)
    with torch.no_grad():
        off = model._sent_lstm_rows(x, glen)
        with _lib.path_options(HSG_SENT_LSTM="1"):
            on = model._sent_lstm_rows(x, glen)
            on_list = model._sent_lstm_feature(list(torch.split(x, glen)), glen)
    assert off.shape == (sum(glen), hps.n_feature_size)
    assert torch.equal(on, off) and torch.equal(on_list, off)
    try:
        hl.sent_lstm(x, glen, model.lstm)
    except RuntimeError as e:                             # the native entry itself has no CPU fallback
        assert "no fallback" in str(e)
    else:
        raise AssertionError("sent_lstm ran on CPU tensors")


def test_doc_offset_cache_is_keyed_by_glen():
    a = hl.doc_offsets([3, 0, 2], "cpu")
    assert a.dtype == torch.int32 and a.tolist() == [0, 3, 3, 5]
    assert hl.doc_offsets((3, 0, 2), "cpu") is a          # same glen: the cached tensor
    b = hl.doc_offsets([3, 2], "cpu")
    assert b is not a and b.tolist() == [0, 3, 5]
    assert hl.doc_offsets([3, 0, 2], "cpu") is a          # and a second key does not evict the first
    lay = hl.doc_layout([3, 0, 2], "cpu")
    # h_{t-1} rows: direction 0 looks one row back, direction 1 one row ahead; 5 = the zero row
    assert lay.prev.tolist() == [[5, 1], [0, 2], [1, 5], [5, 4], [3, 5]]
    assert hl.doc_layout([], "cpu").doc_off.tolist() == [0]
