"""fp64 restatements of include/hsg_lstm_train.h for the tests (numpy, no GPU): the pack
layout of hsg_lstm_pack and the three weight gradients of hsg_lstm_dw, plus the cases both
the CPU and the GPU tests run and a torch restatement of one LSTM layer whose gate
pre-activations are a tensor of their own (so autograd hands out dgates, which nn.LSTM
keeps to itself).  tests/test_lstm_train_cpu.py pins all of it against torch's nn.LSTM.
"""
import numpy as np
import torch

HID = 128
G = 4 * HID
CHUNK = 192                                  # HSG_LSTM_DW_CHUNK

_g = torch.Generator().manual_seed(5)
# name -> (lens, in, ndir): single-row and empty documents, a width that is no tile multiple,
# row counts that are no chunk multiple; one document of one row; one direction; more
# documents than compute units; 1120 rows = 5.8 chunks with every tile of the cfg2 shape live
CASES = {
    "ragged_in300": ([1, 2, 7, 50, 3, 0, 80], 300, 2),
    "ragged_in256": ([1, 2, 7, 50, 3, 0, 80], 256, 2),
    "one_doc_one_step": ([1], 300, 2),
    "unidirectional": ([5, 0, 3], 300, 1),
    "many_short_docs": ([int(v) for v in torch.randint(1, 4, (300,), generator=_g)], 256, 2),
    "docs_32x35": ([35] * 32, 300, 2),
}


def doc_offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(lens, np.int64))
    return off


def h_prev(h, lens, ndir):
    """[ndir][n_rows][HID] fp64: direction 0 reads the row above, direction 1 the row below,
    zero at a document's first / last row."""
    h = np.asarray(h, np.float64)
    n = h.shape[0]
    off = doc_offsets(lens)
    out = np.zeros((ndir, n, HID))
    for a, b in zip(off[:-1], off[1:]):
        if b - a > 1:
            out[0, a + 1:b] = h[a:b - 1, :HID]
            if ndir > 1:
                out[1, a:b - 1] = h[a + 1:b, HID:2 * HID]
    return out


def dw_ref(dg, x, h, lens, ndir):
    """(dW_ih [M, in], dW_hh [ndir, G, HID], db [M]) of hsg_lstm_dw in fp64."""
    dg, x = np.asarray(dg, np.float64), np.asarray(x, np.float64)
    hp = h_prev(h, lens, ndir)
    dwih = dg.T @ x
    dwhh = np.stack([dg[:, d * G:(d + 1) * G].T @ hp[d] for d in range(ndir)])
    return dwih, dwhh, dg.sum(0)


def dw_f32(dg, x, h, lens, ndir):
    """The same three products by torch's fp32 CPU matmul / sum on the same float32 inputs:
    the yardstick of the GPU tests (its error against :func:`dw_ref`)."""
    dg, x = torch.from_numpy(np.asarray(dg, np.float32)), torch.from_numpy(np.asarray(x, np.float32))
    hp = torch.from_numpy(h_prev(h, lens, ndir).astype(np.float32))      # exact: copies and zeros
    dwhh = [dg[:, d * G:(d + 1) * G].T @ hp[d] for d in range(ndir)]
    return (dg.T @ x).numpy(), torch.stack(dwhh).numpy(), dg.sum(0).numpy()


def within_yardstick(name, got, ref64, ref32, factor=4):
    """tests/test_gpu_lstm.py's rule: ``got`` may err against fp64 at most ``factor`` x what
    torch's fp32 CPU result errs on the same inputs.  Returns (err, yardstick)."""
    got = np.asarray(got, np.float64).reshape(ref64.shape)
    yard = np.abs(np.asarray(ref32, np.float64) - ref64).max() if ref64.size else 0.0
    err = np.abs(got - ref64).max() if ref64.size else 0.0
    print(f"{name}: max|err| {err:.3e}  fp32 CPU max|err| {yard:.3e}  ratio {err / yard if yard else 0.0:.2f}"
          f"  (bound {factor * yard:.3e})")
    assert np.isfinite(got).all(), name
    assert err <= factor * yard, f"{name}: {err:.3e} > {factor} x {yard:.3e}"
    return err, yard


def ws_floats(n_rows, ndir, inp):
    return -(-n_rows // CHUNK) * ndir * G * (inp + HID + 1) if n_rows > 0 else 0


def pack_offsets(n_layers, ndir, inp):
    """Float offset of every layer in hsg_lstm_pack's buffer, and its length last."""
    off = [0]
    for layer in range(n_layers):
        off.append(off[-1] + ndir * G * ((inp if layer == 0 else ndir * HID) + HID + 1))
    return off


def pack_ref(params, n_layers, ndir, inp):
    """hsg_lstm_pack's buffer (float32) from the parameters in lstm_params order (float32
    arrays): per layer W_ih rows stacked by direction, W_hh by direction, b_ih + b_hh."""
    out = []
    for layer in range(n_layers):
        q = [params[(layer * ndir + d) * 4:(layer * ndir + d) * 4 + 4] for d in range(ndir)]
        out += [p[0].reshape(-1) for p in q] + [p[1].reshape(-1) for p in q] + [p[2] + p[3] for p in q]
    out = np.concatenate([np.asarray(a, np.float32) for a in out])
    assert out.shape[0] == pack_offsets(n_layers, ndir, inp)[-1]
    return out


def unrolled_layer(mod, x, lens):
    """One nn.LSTM layer (``mod``: num_layers == 1) written out step by step on the rows laid
    end to end: (h [n, ndir * HID], pre [n, ndir * G]) with ``pre`` = x W_ih^T + b_ih + b_hh a
    tensor that keeps its gradient, so after a backward ``pre.grad`` is dgates."""
    ndir = 2 if mod.bidirectional else 1
    sfx = ["", "_reverse"]
    wih = torch.cat([getattr(mod, "weight_ih_l0" + sfx[d]) for d in range(ndir)], 0)
    bias = torch.cat([getattr(mod, "bias_ih_l0" + sfx[d]) + getattr(mod, "bias_hh_l0" + sfx[d]) for d in range(ndir)])
    pre = x @ wih.T + bias
    pre.retain_grad()
    off = doc_offsets(lens)
    rows = [[None] * ndir for _ in range(x.shape[0])]
    for d in range(ndir):
        whh = getattr(mod, "weight_hh_l0" + sfx[d])
        for a, b in zip(off[:-1], off[1:]):
            hcur = x.new_zeros(HID)
            c = x.new_zeros(HID)
            for r in (range(a, b) if d == 0 else range(b - 1, a - 1, -1)):
                gi, gf, gg, go = (pre[r, d * G:(d + 1) * G] + whh @ hcur).view(4, HID)
                c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
                hcur = torch.sigmoid(go) * torch.tanh(c)
                rows[r][d] = hcur
    if not rows:
        return x.new_zeros(0, ndir * HID), pre
    return torch.stack([torch.cat(r) for r in rows]), pre


def random_operands(name, seed=7):
    """(dgates [n, M], x [n, in], h [n, ndir * HID]) float32 for a case: what hsg_lstm_dw
    reads, at the magnitudes of a training step (gate gradients are small, h lies in (-1, 1))."""
    lens, inp, ndir = CASES[name]
    n = sum(lens)
    rng = np.random.default_rng(seed)
    f = np.float32
    return (f(0.05 * rng.standard_normal((n, ndir * G))), f(rng.standard_normal((n, inp))),
            f(np.tanh(rng.standard_normal((n, ndir * HID)))))
