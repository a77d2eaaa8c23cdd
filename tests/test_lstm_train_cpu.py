"""The fp64 restatements of include/hsg_lstm_train.h (tests/lstm_train_ref.py) against torch
autograd on the CPU, before any GPU is involved: per case a one-layer nn.LSTM in fp64 on
pack_padded_sequence gives the gradients of weight_ih, weight_hh and both biases; the
step-by-step restatement of the same layer gives h and dgates; and dw_ref on those must
reproduce nn.LSTM's gradients.  This fixes the h_prev rule at document edges -- the row
above for direction 0, the row below for direction 1, zero at a document's first / last
row, empty and single-row documents included.  The pack layout is pinned against
lstm._stacked.  fp64 throughout: the bound is a few thousand roundings of 2^-53 on sums of
at most 1120 terms of magnitude <= ~1, far below 1e-10.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import lstm_train_ref as R
from hetersumgraph_amd import lstm as hl
from model_ref import run_packed

TOL = 1e-10


@pytest.mark.parametrize("name", list(R.CASES))
def test_dw_restatement_equals_autograd(name):
    lens, inp, ndir = R.CASES[name]
    torch.manual_seed(3)
    mod = nn.LSTM(inp, R.HID, num_layers=1, batch_first=True, bidirectional=ndir == 2).double()
    g = torch.Generator().manual_seed(4)
    n = sum(lens)
    x = torch.randn(n, inp, generator=g, dtype=torch.float64)
    up = torch.randn(n, ndir * R.HID, generator=g, dtype=torch.float64)

    out = run_packed(mod, x, lens)
    want = torch.autograd.grad((out * up).sum(), hl.lstm_params(mod))

    h, pre = R.unrolled_layer(mod, x, lens)
    assert (h - out).abs().max().item() <= TOL
    (h * up).sum().backward()
    dwih, dwhh, db = R.dw_ref(pre.grad.numpy(), x.numpy(), h.detach().numpy(), lens, ndir)
    for d in range(ndir):
        w_ih, w_hh, b_ih, b_hh = (t.numpy() for t in want[4 * d:4 * d + 4])
        assert np.abs(dwih[d * R.G:(d + 1) * R.G] - w_ih).max() <= TOL
        assert np.abs(dwhh[d] - w_hh).max() <= TOL
        assert np.abs(db[d * R.G:(d + 1) * R.G] - b_ih).max() <= TOL
        assert np.abs(db[d * R.G:(d + 1) * R.G] - b_hh).max() <= TOL
    if n > 1:
        assert np.abs(dwhh).max() > 0 or max(lens) == 1      # the recurrent term is live


def test_h_prev_at_document_edges():
    lens = [1, 3, 0, 2]
    h = np.arange(6 * 2 * R.HID, dtype=np.float64).reshape(6, 2 * R.HID) + 1
    hp = R.h_prev(h, lens, 2)
    zero = np.zeros(R.HID)
    for r, (up, down) in enumerate([(None, None), (None, 2), (1, 3), (2, None), (None, 5), (4, None)]):
        assert np.array_equal(hp[0, r], zero if up is None else h[up, :R.HID]), r
        assert np.array_equal(hp[1, r], zero if down is None else h[down, R.HID:]), r


@pytest.mark.parametrize("layers,bidir,inp", [(2, True, 300), (1, False, 256), (3, True, 4)])
def test_pack_restatement_equals_stacked(layers, bidir, inp):
    torch.manual_seed(5)
    mod = nn.LSTM(inp, R.HID, num_layers=layers, batch_first=True, bidirectional=bidir)
    ndir = 2 if bidir else 1
    params = [p.detach() for p in hl.lstm_params(mod)]
    buf = R.pack_ref([p.numpy() for p in params], layers, ndir, inp)
    off = R.pack_offsets(layers, ndir, inp)
    assert all(o % 4 == 0 for o in off)
    for layer in range(layers):
        wih, whh, bias = hl._stacked(params, layer, ndir)
        want = np.concatenate([wih.numpy().reshape(-1), whh.numpy().reshape(-1), bias.numpy()])
        got = buf[off[layer]:off[layer + 1]]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_workspace_formula():
    assert R.ws_floats(0, 2, 300) == 0
    assert R.ws_floats(1, 1, 4) == 512 * (4 + 128 + 1)
    assert R.ws_floats(192, 2, 300) == 1024 * 429 and R.ws_floats(193, 2, 300) == 2 * 1024 * 429
