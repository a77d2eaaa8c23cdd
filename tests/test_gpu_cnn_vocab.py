"""The sentence CNN's vocabulary path on the GPU (path_options(HSG_SENT_CNN_VOCAB="1"),
hetersumgraph_amd.cnn.VocabTable / sent_cnn_vocab -> include/hsg_cnn_vocab.h).

Bitwise: TW is the two GEMMs made directly; feat / arg are the pool's value contract on the
device's own TW (tests/cnn_tokens_ref.py with U = V and the identity slot map) and what
hsg_cnn_tok_pool gives with the identity map on the same TW, at both row pitches; two runs are
equal.  An id outside [0, V) is read as PAD: the restatement gets a slot map of V + 1 entries whose
last one is 0, which both -1 and V index.

Parity of the encoder, at exactly the bounds tests/test_gpu_encoder.py holds today's path to:
feat within 5e-5 of the reference's golden (feat64 and feat32) and of the fp64 oracle.  The path
is taken only where no gradient is recorded; a warm forward is graph-capturable; a changed conv
weight -- by an in-place op or by optim.Adam.step -- is seen by the next forward.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import cnn_tokens_ref as R
from helpers import load_fixture
from oracle import cnn as ocnn
from test_encoder_oracle import encoder_params
from test_gpu_encoder import cnndm_ids

pytestmark = pytest.mark.gpu

ON = dict(HSG_SENT_CNN_VOCAB="1")


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({4: np.int32, 8: np.int64}[a.itemsize])


# ---------------------------------------------------------------------------- the kernel, bitwise
def device_pool(ids, TW, cb, V, entry):
    """feat, arg of one entry point on the device tensor TW [V + Pn, pitch]."""
    from hetersumgraph_amd._lib import check, load, ptr, stream_of
    lib = load()
    n, L = ids.shape
    ids_d = torch.from_numpy(ids).cuda()
    rowoff = torch.zeros(n + 1, dtype=torch.int32)
    rowoff[1:] = torch.cumsum(torch.from_numpy(R.lengths(ids) + 1), 0)
    rowoff = rowoff.cuda()
    bias = [torch.from_numpy(b).cuda() for b in cb]
    bptr = (ctypes.c_void_p * 6)(*[b.data_ptr() for b in bias])
    feat = torch.full((n, R.NF), float("nan"), device="cuda")
    arg = torch.full((n, R.NF), -7, dtype=torch.int32, device="cuda")
    st = stream_of(TW)
    if entry == "vocab":
        check(lib.hsg_cnn_vocab_pool(n, L, V, ptr(ids_d), ptr(rowoff), ptr(TW), TW.stride(0), bptr, ptr(feat), ptr(arg),
                                     st), "hsg_cnn_vocab_pool")
    else:
        slot = torch.arange(V, dtype=torch.int32, device="cuda")
        check(lib.hsg_cnn_tok_pool(n, L, V, V, ptr(ids_d), ptr(rowoff), ptr(slot), ptr(TW), TW.stride(0), bptr,
                                   ptr(feat), ptr(arg), st), "hsg_cnn_tok_pool")
    torch.cuda.synchronize()
    return feat.cpu().numpy(), arg.cpu().numpy()


@pytest.mark.parametrize("n,L,V,D", [(130, 100, 200, 300), (3, 7, 200, 300), (5, 400, 37, 4)])
def test_kernel_bitwise(n, L, V, D):
    from hetersumgraph_amd.cnn import LDY, NY, VocabTable, stack_taps
    from hetersumgraph_amd.dense import gemm
    ids = cnndm_ids(n, L, V, 3).numpy() if n > 100 else R.small_ids(n, L, V, 3)
    lens = R.lengths(ids)
    if n > 100:
        ids[4, :lens[4]] = 7                                    # one token repeated
        assert lens[10] > 3 and lens[11] > 3
        ids[10, 2], ids[11, 0], ids[12, lens[12] - 1] = -1, V, V    # outside [0, V): read as PAD, still a position
        assert set(lens[:4]) == {0, 1, 6, L} and ids.max() == V and ids.min() == -1
    elif n == 5:
        assert list(lens[:4]) == [0, 1, 6, L] and (ids[4, :lens[4]] == 7).all() and lens[4] > 1
    E, Pm, cw, cb = [[np.float32(x) for x in a] if isinstance(a, list) else np.float32(a) for a in R.params(V, D, L, 4)]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    E_d, P_d, cw_d = d(E), d(Pm), [d(w) for w in cw]

    # the table is the two GEMMs made directly
    table = VocabTable().get(E_d, P_d, cw_d)
    assert table.V == V and tuple(table.TW.shape) == (V + L + 1, LDY) == (V + L + 1, 1352) and table.builds == 1
    assert table.nbytes() == (V + L + 1) * 1352 * 4
    wall = stack_taps(cw_d)
    assert np.array_equal(bits(wall), bits(R.stack_taps(cw)))
    direct = torch.empty(V + L + 1, LDY, device="cuda")
    gemm(E_d, wall, b_t=True, out=direct[:V, :NY])
    gemm(P_d, wall, b_t=True, out=direct[V:, :NY])
    torch.cuda.synchronize()
    TW = table.TW[:, :NY].cpu().numpy()
    assert np.array_equal(bits(TW), bits(direct[:, :NY]))
    assert table.get(E_d, P_d, cw_d) is table and table.builds == 1            # current: not rebuilt

    # the value contract on the device's own TW
    slot = np.concatenate([np.arange(V), [0]]).astype(np.int32)                # slot[V] = slot[-1] = PAD
    want_f, want_a = R.pool(ids, slot, V, TW, cb)
    got_f, got_a = device_pool(ids, table.TW, cb, V, "vocab")
    assert np.array_equal(bits(got_f), bits(want_f)) and np.array_equal(got_a, want_a)
    assert (got_f > 0).mean() > 0.2 and not np.isnan(got_f).any()
    # ... which is hsg_cnn_tok_pool's with the identity map
    tok_f, tok_a = device_pool(ids, table.TW, cb, V, "tok")
    assert np.array_equal(bits(got_f), bits(tok_f)) and np.array_equal(got_a, tok_a)
    # a wider pitch, poison in the pad columns
    wide = torch.full((V + L + 1, 1360), float("nan"), device="cuda")
    wide[:, :NY] = table.TW[:, :NY]
    f2, a2 = device_pool(ids, wide, cb, V, "vocab")
    assert np.array_equal(bits(got_f), bits(f2)) and np.array_equal(got_a, a2)
    f3, a3 = device_pool(ids, wide, cb, V, "tok")
    assert np.array_equal(bits(f3), bits(f2)) and np.array_equal(a3, a2)
    # two runs
    f4, a4 = device_pool(ids, table.TW, cb, V, "vocab")
    assert np.array_equal(bits(got_f), bits(f4)) and np.array_equal(got_a, a4)


# ---------------------------------------------------------------------------- the encoder
def make_encoder(cw=None, cb=None):
    """sentEncoder with the golden script's seeded parameters (V = 64, D = 300, L = 20)."""
    from hetersumgraph_amd.module.Encoder import sentEncoder
    emb, pos, cw0, cb0 = encoder_params(torch.float32)
    enc = sentEncoder(types.SimpleNamespace(sent_max_len=pos.shape[0] - 1, word_emb_dim=emb.shape[1]),
                      torch.nn.Embedding(emb.shape[0], emb.shape[1], padding_idx=0))
    with torch.no_grad():
        enc.embed.weight.copy_(emb)
        assert torch.equal(enc.position_embedding.weight, pos)
        for conv, w, b in zip(enc.convs, cw or cw0, cb or cb0):
            conv.weight.copy_(w)
            conv.bias.copy_(b)
    return enc.cuda()


@pytest.fixture
def spy(monkeypatch):
    from hetersumgraph_amd import cnn
    calls, real = [], cnn.sent_cnn_vocab

    def wrapped(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(cnn, "sent_cnn_vocab", wrapped)
    return calls


def test_encoder_matches_reference_golden_and_oracle(spy):
    from hetersumgraph_amd._lib import path_options
    z = load_fixture("encoder")
    ids = torch.from_numpy(z["ids"])
    enc = make_encoder().eval()
    with path_options(**ON), torch.no_grad():
        assert enc.takes_token_path(ids.cuda())
        feat = enc(ids.cuda())
        again = enc(ids.cuda())
    torch.cuda.synchronize()
    assert spy == [1, 1] and enc._vocab_table.builds == 1 and not feat.requires_grad
    assert feat.shape == (ids.shape[0], 300) and np.array_equal(bits(feat), bits(again))
    emb, pos, cw, cb = encoder_params()
    ref = ocnn.sent_encoder(ids, emb, pos, cw, cb)
    got = feat.cpu().double()
    e64 = (got - torch.from_numpy(z["feat64"]).double()).abs().max().item()
    e32 = (got - torch.from_numpy(z["feat32"]).double()).abs().max().item()
    eo = (got - ref).abs().max().item()
    print(f"vocab: feat vs feat64 {e64:.3g}, vs feat32 {e32:.3g}, vs the fp64 oracle {eo:.3g}")
    assert e64 < 5e-5 and e32 < 5e-5 and eo < 5e-5
    # no sentences; ids outside the vocabulary are refused where the layout is built
    with path_options(**ON), torch.no_grad():
        assert enc(torch.zeros(0, 20, dtype=torch.long, device="cuda")).shape == (0, 300)
        for bad in (64, -1):
            x = torch.ones(3, 20, dtype=torch.long, device="cuda")
            x[1, 4] = bad
            with pytest.raises(ValueError, match="outside the vocabulary"):
                enc(x)
        with pytest.raises(ValueError, match="trailing"):
            enc(torch.tensor([[1, 0, 2] + [0] * 17], device="cuda"))
    # the switch off, or train mode: today's path
    n = len(spy)
    with torch.no_grad():
        off = enc(ids.cuda())
    with path_options(**ON), torch.no_grad():
        enc.train()
        assert not enc.takes_token_path(ids.cuda())
        tr = enc(ids.cuda())
    assert len(spy) == n and np.array_equal(bits(off), bits(tr))
    assert (off - feat).abs().max().item() < 1e-4          # both are within 5e-5 of the golden


def test_not_taken_where_a_gradient_is_recorded(spy):
    from hetersumgraph_amd._lib import path_options
    ids = torch.from_numpy(load_fixture("encoder")["ids"]).cuda()
    enc = make_encoder().eval()
    assert all(c.weight.requires_grad for c in enc.convs)
    with path_options(**ON):
        assert not enc.takes_token_path(ids)
        on = enc(ids)
        (on.sum()).backward()
        g_on = [c.weight.grad.clone() for c in enc.convs]
    enc.zero_grad(set_to_none=True)
    off = enc(ids)
    off.sum().backward()
    assert spy == [] and on.requires_grad and enc._vocab_table.TW is None
    assert np.array_equal(bits(on), bits(off))
    assert all(np.array_equal(bits(a), bits(c.weight.grad)) for a, c in zip(g_on, enc.convs))


def test_warm_forward_is_graph_capturable(spy):
    from hetersumgraph_amd._lib import path_options
    from hetersumgraph_amd.cnn import BatchLayout, _layout
    ids = torch.from_numpy(load_fixture("encoder")["ids"]).cuda()
    enc = make_encoder().eval()
    layout = BatchLayout(*_layout(ids), max_token=int(ids.max()))
    with path_options(**ON), torch.no_grad():
        warm = enc(ids, layout=layout)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = enc(ids, layout=layout)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        first = out.clone()
        graph.replay()
        torch.cuda.synchronize()
    assert spy == [1, 1] and enc._vocab_table.builds == 1
    assert np.array_equal(bits(first), bits(warm)) and np.array_equal(bits(out), bits(warm))


def test_a_changed_conv_weight_is_seen(spy):
    from hetersumgraph_amd._lib import path_options
    ids = torch.from_numpy(load_fixture("encoder")["ids"]).cuda()
    enc = make_encoder().eval()
    with path_options(**ON), torch.no_grad():
        before = enc(ids)
        enc.convs[3].weight.add_(0.01 * torch.randn_like(enc.convs[3].weight))
        after = enc(ids)
        fresh = make_encoder([c.weight.detach().cpu() for c in enc.convs], [c.bias.detach().cpu() for c in enc.convs])
        want = fresh.eval()(ids)
    assert spy == [1, 1, 1] and enc._vocab_table.builds == 2 and fresh._vocab_table.builds == 1
    assert not np.array_equal(bits(before), bits(after))
    assert np.array_equal(bits(after), bits(want))


def test_an_adam_step_between_two_eval_spans_is_seen(spy):
    from hetersumgraph_amd import optim
    from hetersumgraph_amd._lib import path_options
    from hetersumgraph_amd.cnn import VocabTable
    ids = torch.from_numpy(load_fixture("encoder")["ids"]).cuda()
    enc = make_encoder()
    enc.embed.weight.requires_grad_(False)
    adam = optim.Adam([p for p in enc.parameters() if p.requires_grad], lr=1e-2)
    with path_options(**ON):
        enc.eval()
        with torch.no_grad():
            before = enc(ids)
        enc.train()
        enc(ids).square().sum().backward()
        key = VocabTable.key_of(*enc._vocab_args()[:3])
        adam.step()
        assert VocabTable.key_of(*enc._vocab_args()[:3]) != key          # the step moved the version counters
        assert all(a[:1] + a[2:] == b[:1] + b[2:] for a, b in zip(VocabTable.key_of(*enc._vocab_args()[:3])[:-1], key))
        enc.eval()
        with torch.no_grad():
            after = enc(ids)
            fresh = make_encoder([c.weight.detach().cpu() for c in enc.convs],
                                 [c.bias.detach().cpu() for c in enc.convs])
            want = fresh.eval()(ids)
    assert spy == [1, 1, 1]
    assert not np.array_equal(bits(before), bits(after))
    assert np.array_equal(bits(after), bits(want))
