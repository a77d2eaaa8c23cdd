"""The sentence LSTM's training path (include/hsg_lstm_train.h, lstm.sent_lstm(...,
fused=True)): hsg_lstm_pack and hsg_lstm_dw called directly, then the whole autograd node.

hsg_lstm_dw against its fp64 restatement (tests/lstm_train_ref.py, pinned against torch
autograd in tests/test_lstm_train_cpu.py).  Yardstick and factor are
tests/test_gpu_lstm.py's: the max-abs error of torch's fp32 CPU result against fp64 on the
same inputs is the yardstick -- here the same three products by torch's fp32 CPU matmul on
the same float32 operands -- and the kernel may err at most 4 x that.  The cases
(lstm_train_ref.CASES) cover single-row and empty documents, in = 300 (no tile multiple),
row counts that are no chunk multiple, one direction, more documents than compute units and
32 x 35 rows, where several chunks and every tile of the cfg2 shape are live.

Through sent_lstm(..., fused=True): the output and the row gradient are torch.equal to
fused=False (same operands, same pitches, same GEMMs); the parameter gradients hold the
bound of tests/test_gpu_lstm.py against torch's CPU nn.LSTM in fp64 (eval and train mode, the
CPU-built keep mask between the layers); bias_ih and bias_hh gradients are equal; a captured
forward + backward on a single stream replays equal to eager.
"""
import copy

import numpy as np
import pytest
import torch

import lstm_train_ref as R
import test_gpu_lstm as T
from hetersumgraph_amd import lstm as hl
from hetersumgraph_amd._lib import check, load, ptr, stream_of
from oracle import masks

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENS = T.LENS


def run_dw(name, dg, x, h, ld_x=None, ld_h=None):
    """hsg_lstm_dw on device copies of the operands -> (dW_ih, dW_hh, db) CPU tensors."""
    lens, inp, ndir = R.CASES[name]
    lib, n, M = load(), sum(lens), ndir * R.G
    off = torch.from_numpy(R.doc_offsets(lens).astype(np.int32)).to(DEV)

    def pitched(a, ld):
        buf = torch.full((a.shape[0], ld or a.shape[1]), float("nan"), device=DEV)
        buf[:, :a.shape[1]] = torch.from_numpy(a)
        return buf[:, :a.shape[1]]
    dgd, xd, hd = torch.from_numpy(dg).to(DEV), pitched(x, ld_x), pitched(h, ld_h)
    nws = lib.hsg_lstm_dw_ws_floats(n, ndir, inp)
    ws = torch.full((nws,), float("nan"), device=DEV)
    dwih, dwhh, db = (torch.full(s, float("nan"), device=DEV) for s in ((M, inp), (ndir, R.G, R.HID), (M,)))
    check(lib.hsg_lstm_dw(len(lens), n, R.HID, ndir, inp, ptr(off), ptr(dgd), ptr(xd), xd.stride(0), ptr(hd),
                          hd.stride(0), ptr(ws), ptr(dwih), ptr(dwhh), ptr(db), stream_of(dgd)), "hsg_lstm_dw")
    torch.cuda.synchronize()
    return dwih.cpu(), dwhh.cpu(), db.cpu()


@pytest.mark.parametrize("name", list(R.CASES))
def test_dw_against_fp64(name):
    lens, inp, ndir = R.CASES[name]
    dg, x, h = R.random_operands(name)
    got = run_dw(name, dg, x, h)
    r64, r32 = R.dw_ref(dg, x, h, lens, ndir), R.dw_f32(dg, x, h, lens, ndir)
    for i, nm in enumerate(("dW_ih", "dW_hh", "db")):
        R.within_yardstick(f"{name} {nm}", got[i].numpy(), r64[i], r32[i])
    # a second run, with other pitches and in other buffers, is bitwise the first
    again = run_dw(name, dg, x, h, ld_x=inp + 12, ld_h=ndir * R.HID + 4)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_dw_of_nothing_is_zero():
    lib = load()
    outs = [torch.full(s, float("nan"), device=DEV) for s in ((1024, 300), (2, 512, 128), (1024,))]
    off = torch.zeros(3, dtype=torch.int32, device=DEV)
    for n_docs, n_rows in ((2, 0), (0, 0)):
        for o in outs:
            o.fill_(float("nan"))
        check(lib.hsg_lstm_dw(n_docs, n_rows, 128, 2, 300, ptr(off), None, None, 300, None, 256, None,
                              *[ptr(o) for o in outs], stream_of(off)), "hsg_lstm_dw")
        for o in outs:
            assert not o.any() and not torch.signbit(o).any()


@pytest.mark.parametrize("layers,bidir,inp", [(2, True, 300), (1, False, 256), (4, True, 4)])
def test_pack_is_bitwise_stacked(layers, bidir, inp):
    lstm = T.make_lstm(31, layers=layers, bidir=bidir, inp=inp).to(DEV)
    ndir = 2 if bidir else 1
    params = [q.detach() for q in hl.lstm_params(lstm)]
    packed = hl._packed(params, (layers, ndir, 128, 0.0), inp)
    assert packed[0][0].data_ptr() % 16 == 0
    for layer in range(layers):
        for got, want in zip(packed[layer], hl._stacked(params, layer, ndir)):
            assert got.shape == want.shape and got.is_contiguous()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    flat = R.pack_ref([q.cpu().numpy() for q in params], layers, ndir, inp)
    o, M = R.pack_offsets(layers, ndir, inp), ndir * R.G
    assert packed[-1][2].data_ptr() + 4 * M - packed[0][0].data_ptr() == 4 * o[-1] == 4 * flat.shape[0]


# ---- through sent_lstm(..., fused=True) ---------------------------------------------------------

def native(lstm_d, x, R_, lens, fused):
    xd = x.to(DEV).requires_grad_()
    params = hl.lstm_params(lstm_d)
    out = hl.sent_lstm(xd, lens, lstm_d, fused=fused)
    grads = torch.autograd.grad((out * R_.to(DEV)).sum(), [xd] + params)
    torch.cuda.synchronize()
    return out.detach(), list(grads)


@pytest.fixture(scope="module")
def case():
    lstm = T.make_lstm(11).eval()
    x, R_ = T.make_rows(12, LENS, 256)
    r64, r32 = T.references(lstm, x, R_, LENS)
    return dict(lstm=lstm, lstm_d=copy.deepcopy(lstm).to(DEV).eval(), x=x, R=R_, r64=r64, r32=r32)


def check_fused(lstm, lstm_d, x, R_, lens, r64, r32, seed=None):
    from hetersumgraph_amd import rng
    runs = []
    for fused in (False, True):
        if seed is not None:
            rng.manual_seed(seed, torch.device(DEV, torch.cuda.current_device()))
        runs.append(native(lstm_d, x, R_, lens, fused))
    (out0, g0), (out1, g1) = runs
    assert hl.fused_lstm_ok(x.to(DEV), lstm_d)
    assert torch.equal(out1, out0)                        # the forward is bitwise fused=False's
    assert torch.equal(g1[0], g0[0])                      # ... and so is the row gradient
    T.check("out", out1, r64["out"], r32["out"], forward=True)
    T.check_grads(lstm, g1, r64, r32)                     # every gradient in bound; bias_ih == bias_hh
    assert any(not torch.equal(a, b) for a, b in zip(g1[1:], g0[1:])) or sum(lens) <= 1   # another order ran


def test_fused_eval(case):
    check_fused(case["lstm"], case["lstm_d"], case["x"], case["R"], LENS, case["r64"], case["r32"])
    st0 = hl.sent_lstm_states(case["x"].to(DEV), LENS, case["lstm_d"])
    st1 = hl.sent_lstm_states(case["x"].to(DEV), LENS, case["lstm_d"], fused=True)
    for a, b in zip(st0, st1):
        assert all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))


def test_fused_train_mode(case):
    n = sum(LENS)
    keep = [masks.ffn_keep(T.TRAIN_SEED, 1, n, 256, T.P), None]
    r64, r32 = T.references(case["lstm"], case["x"], case["R"], LENS, keep=keep)
    lstm_d = copy.deepcopy(case["lstm"]).to(DEV).train()
    check_fused(case["lstm"], lstm_d, case["x"], case["R"], LENS, r64, r32, seed=T.TRAIN_SEED)


@pytest.mark.parametrize("name", list(T.VARIANTS))
def test_fused_small_variants(name):
    kw, lens = T.VARIANTS[name]
    lstm = T.make_lstm(21, **kw).eval()
    width = lstm.hidden_size * (2 if lstm.bidirectional else 1)
    x, R_ = T.make_rows(22, lens, width)
    r64, r32 = T.references(lstm, x, R_, lens)
    check_fused(lstm, copy.deepcopy(lstm).to(DEV).eval(), x, R_, lens, r64, r32)


def test_fused_is_deterministic_and_refuses_uncovered_shapes(case):
    a = native(case["lstm_d"], case["x"], case["R"], LENS, True)
    b = native(case["lstm_d"], case["x"], case["R"], LENS, True)
    for u, v in zip([a[0]] + a[1], [b[0]] + b[1]):
        assert torch.equal(u, v)
    deep = T.make_lstm(5, layers=5).to(DEV).eval()
    x = case["x"].to(DEV)
    assert hl.native_lstm_ok(x, deep) and not hl.fused_lstm_ok(x, deep)
    with pytest.raises(RuntimeError):
        hl.sent_lstm(x, LENS, deep, fused=True)


def test_fused_graph_capture(case):
    lstm_d, R_ = case["lstm_d"], case["R"].to(DEV)
    params = hl.lstm_params(lstm_d)
    xs = case["x"].to(DEV).clone().requires_grad_()

    def step(x):
        out = hl.sent_lstm(x, LENS, lstm_d, fused=True)
        return [out] + list(torch.autograd.grad((out * R_).sum(), [x] + params))

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
        new = T.make_rows(seed, LENS, 256)[0].to(DEV)
        with torch.no_grad():
            xs.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(new.clone().requires_grad_())
        for a, b in zip(static, eager):
            assert torch.equal(a, b)
