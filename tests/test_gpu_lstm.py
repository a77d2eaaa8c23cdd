"""The native sentence LSTM (hetersumgraph_amd.lstm: hsg_lstm_fwd / hsg_lstm_bwd plus the
fp32 GEMMs around them) against torch's own CPU nn.LSTM in fp64 on the same seeded
weights, run on pack_padded_sequence(..., enforce_sorted=False).

Tolerance, per compared tensor: the max-abs error of torch's fp32 CPU nn.LSTM against
the fp64 oracle on the same inputs is the yardstick; the native result may err at most
4x that (its summation order differs: a register dot over 128 plus three-limb GEMMs),
and forward outputs never more than the project's 1e-4 contract.  Train-mode cases
restate the oracle as single-layer LSTMs with the CPU-built keep-mask
(oracle.masks.ffn_keep) applied between them.  The per-step cell states of the oracle
are the final cell states of every prefix (reverse direction: suffix) of a document.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.utils.rnn as rnn

from hetersumgraph_amd import lstm as hl
from model_ref import run_packed as _run_packed, single_layers as _single_layers
from oracle import masks

pytestmark = pytest.mark.gpu

LENS = [1, 2, 7, 50, 3, 0, 80]      # single step, unsorted ragged, empty, > doc_max_timesteps
DEV = "cuda"
P = 0.1


def make_lstm(seed, layers=2, bidir=True, hid=128, inp=300):
    torch.manual_seed(seed)
    return nn.LSTM(inp, hid, num_layers=layers, dropout=P if layers > 1 else 0.0, batch_first=True,
                   bidirectional=bidir)


def make_rows(seed, lens, width):
    g = torch.Generator().manual_seed(seed)
    n = sum(lens)
    return torch.randn(n, 300, generator=g), torch.randn(n, width, generator=g)


def _cell_states(mod, x, lens):
    """c_t of every row: the final cell state of the prefix ending (direction 0) / the
    suffix starting (direction 1) at that row."""
    ndir = 2 if mod.bidirectional else 1
    seqs_f, seqs_b, off = [], [], 0
    for g in lens:
        for t in range(g):
            seqs_f.append(x[off:off + t + 1])
            seqs_b.append(x[off + t:off + g])
        off += g
    cs = []
    for d, seqs in enumerate((seqs_f, seqs_b)[:ndir]):
        ln = [len(s) for s in seqs]
        pad = rnn.pad_sequence(seqs, batch_first=True)
        _, (_, cn) = mod(rnn.pack_padded_sequence(pad, ln, batch_first=True, enforce_sorted=False))
        cs.append(cn[d])
    return torch.cat(cs, 1)


def cpu_reference(lstm, x, R, lens, dtype, keep=None, want_c=False):
    """out, c per layer (eval only), grad of sum(out * R) wrt x and the parameters in
    hl.lstm_params order -- torch CPU in ``dtype``.  keep: per layer None or a bool mask
    [n, ndir*hid] applied (scaled) to that layer's output (the train-mode restatement)."""
    x = x.detach().clone().to(dtype).requires_grad_()     # a leaf of its own: the shared rows stay as they are
    res = {}
    if keep is None:
        mod = copy.deepcopy(lstm).to(dtype).eval()
        out = _run_packed(mod, x, lens)
        params = hl.lstm_params(mod)
        if want_c:
            with torch.no_grad():
                cs, xi = [], x.detach()
                for m in _single_layers(lstm, dtype):
                    cs.append(_cell_states(m, xi, lens))
                    xi = _run_packed(m, xi, lens)
                res["c"] = cs
    else:
        mods = _single_layers(lstm, dtype)
        out = x
        for layer, m in enumerate(mods):
            out = _run_packed(m, out, lens)
            if keep[layer] is not None:
                out = out * (torch.from_numpy(keep[layer]).to(dtype) * masks.ffn_scale(P))
        ndir = 2 if lstm.bidirectional else 1
        params = [getattr(m, nm.replace(f"_l{layer}", "_l0")) for layer, m in enumerate(mods)
                  for names in hl._names(layer, ndir) for nm in names]
    (out * R.to(dtype)).sum().backward()
    res["out"] = out.detach()
    res["grads"] = [x.grad] + [q.grad for q in params]
    return res


def references(lstm, x, R, lens, keep=None, want_c=False):
    return (cpu_reference(lstm, x, R, lens, torch.float64, keep, want_c),
            cpu_reference(lstm, x, R, lens, torch.float32, keep, want_c))


def native(lstm_d, x, R, lens, between=None):
    """(out, grads) of sent_lstm on the GPU; ``between`` runs after the forward."""
    xd = x.to(DEV).requires_grad_()
    params = hl.lstm_params(lstm_d)
    out = hl.sent_lstm(xd, lens, lstm_d)
    if between is not None:
        between()
    grads = torch.autograd.grad((out * R.to(DEV)).sum(), [xd] + params)
    torch.cuda.synchronize()
    return out.detach(), list(grads)


def check(name, got, ref64, ref32, forward=False):
    got = got.detach().cpu().double()
    yard = (ref32.double() - ref64).abs().max().item()
    err = (got - ref64).abs().max().item()
    print(f"{name}: native max|err| {err:.3e}  fp32 CPU nn.LSTM max|err| {yard:.3e}  (bound {4 * yard:.3e})")
    assert got.shape == ref64.shape, name
    assert err <= 4 * yard, f"{name}: {err:.3e} > 4 x {yard:.3e}"
    if forward:
        assert err <= 1e-4, f"{name}: {err:.3e} > 1e-4"


def grad_names(lstm):
    ndir = 2 if lstm.bidirectional else 1
    return ["rows"] + [nm for layer in range(lstm.num_layers) for names in hl._names(layer, ndir) for nm in names]


def check_grads(lstm, got, r64, r32):
    names = grad_names(lstm)
    assert len(got) == len(names) == len(r64["grads"])
    for nm, g, a, b in zip(names, got, r64["grads"], r32["grads"]):
        check("grad " + nm, g, a, b)
    for i, nm in enumerate(names):
        if nm.startswith("bias_ih"):
            assert names[i + 1] == nm.replace("bias_ih", "bias_hh")
            assert torch.equal(got[i], got[i + 1]), nm


@pytest.fixture(scope="module")
def case():
    lstm = make_lstm(11).eval()
    x, R = make_rows(12, LENS, 256)
    r64, r32 = references(lstm, x, R, LENS, want_c=True)
    return dict(lstm=lstm, lstm_d=copy.deepcopy(lstm).to(DEV).eval(), x=x, R=R, r64=r64, r32=r32)


@pytest.fixture(scope="module")
def train_case(case):
    """Train mode after rng.manual_seed(SEED): the one inter-layer mask of the call is
    (SEED, offset 1); its CPU restatement feeds the oracle."""
    n = sum(LENS)
    keep = [masks.ffn_keep(TRAIN_SEED, 1, n, 256, P), None]
    r64, r32 = references(case["lstm"], case["x"], case["R"], LENS, keep=keep)
    return dict(r64=r64, r32=r32, lstm_d=copy.deepcopy(case["lstm"]).to(DEV).train())


TRAIN_SEED = 4242


def test_forward_eval(case):
    assert hl.native_lstm_ok(case["x"].to(DEV), case["lstm_d"])
    states = hl.sent_lstm_states(case["x"].to(DEV), LENS, case["lstm_d"])
    out = hl.sent_lstm(case["x"].to(DEV), LENS, case["lstm_d"])
    assert torch.equal(out, states[-1][0])
    check("out", out, case["r64"]["out"], case["r32"]["out"], forward=True)
    for layer, st in enumerate(states):
        check(f"c layer {layer}", st[1], case["r64"]["c"][layer], case["r32"]["c"][layer], forward=True)


def test_backward_eval(case):
    _, grads = native(case["lstm_d"], case["x"], case["R"], LENS)
    check_grads(case["lstm"], grads, case["r64"], case["r32"])


@pytest.mark.parametrize("advance", [False, True])
def test_train_mode_masks(case, train_case, advance):
    from hetersumgraph_amd import rng
    rng.manual_seed(TRAIN_SEED, torch.device(DEV, torch.cuda.current_device()))
    r = rng.get(DEV)
    # advancing the stream between forward and backward must not change the backward's
    # mask (the seed-snapshot rule of rng.py)
    out, grads = native(train_case["lstm_d"], case["x"], case["R"], LENS, between=r.advance if advance else None)
    assert r.offset == 1                                  # one draw: the output of layer 0
    check("train out", out, train_case["r64"]["out"], train_case["r32"]["out"], forward=True)
    check_grads(case["lstm"], grads, train_case["r64"], train_case["r32"])


_g = torch.Generator().manual_seed(5)
VARIANTS = {"one_layer_unidirectional": (dict(layers=1, bidir=False), [5, 0, 3]),
            "one_doc_one_step": (dict(), [1]),
            "more_blocks_than_cus": (dict(), [int(v) for v in torch.randint(1, 4, (300,), generator=_g)])}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_small_variants(name):
    kw, lens = VARIANTS[name]
    lstm = make_lstm(21, **kw).eval()
    width = lstm.hidden_size * (2 if lstm.bidirectional else 1)
    x, R = make_rows(22, lens, width)
    r64, r32 = references(lstm, x, R, lens)
    out, grads = native(copy.deepcopy(lstm).to(DEV).eval(), x, R, lens)
    check(name + " out", out, r64["out"], r32["out"], forward=True)
    check_grads(lstm, grads, r64, r32)


def test_deterministic(case):
    runs = []
    for _ in range(2):
        st = hl.sent_lstm_states(case["x"].to(DEV), LENS, case["lstm_d"])
        out, grads = native(case["lstm_d"], case["x"], case["R"], LENS)
        runs.append([out] + grads + [s[1] for s in st])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


class _HPS:
    def __init__(self, **kw):
        d = dict(n_iter=1, word_emb_dim=300, feat_embed_size=50, n_feature_size=128, hidden_size=64, n_head=8,
                 atten_dropout_prob=0.1, ffn_inner_hidden_size=512, ffn_dropout_prob=0.1, doc_max_timesteps=50,
                 lstm_hidden_state=128, lstm_layers=2, bidirectional=True, sent_max_len=100, cuda=True, vocab_size=50)
        d.update(kw)
        self.__dict__.update(d)


def test_fallback_for_uncovered_shape():
    from hetersumgraph_amd import HiGraph, _lib
    assert _lib.load().hsg_lstm_supported(64, 2) == 0
    assert _lib.load().hsg_lstm_supported(128, 1) and _lib.load().hsg_lstm_supported(128, 2)
    torch.manual_seed(3)
    hps = _HPS(lstm_hidden_state=64)
    model = HiGraph.HSumGraph(hps, nn.Embedding(hps.vocab_size, 300, padding_idx=0)).eval().to(DEV)
    lens = [5, 3, 1]                                      # today's path packs with enforce_sorted
    x = make_rows(31, lens, 1)[0].to(DEV)
    assert not hl.native_lstm_ok(x, model.lstm)
    with torch.no_grad():
        off = model._sent_lstm_rows(x, lens)
        with _lib.path_options(HSG_SENT_LSTM="1"):
            on = model._sent_lstm_rows(x, lens)
    assert torch.equal(on, off)


def test_graph_capture(case):
    lstm_d, R = case["lstm_d"], case["R"].to(DEV)
    params = hl.lstm_params(lstm_d)
    xs = case["x"].to(DEV).clone().requires_grad_()

    def step(x):
        out = hl.sent_lstm(x, LENS, lstm_d)
        return [out] + list(torch.autograd.grad((out * R).sum(), [x] + params))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # single stream: no parallel branches
        static = step(xs)
    for seed in (41, 42):
        new = make_rows(seed, LENS, 256)[0].to(DEV)
        with torch.no_grad():
            xs.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(new.clone().requires_grad_())
        for a, b in zip(static, eager):
            assert torch.equal(a, b)
