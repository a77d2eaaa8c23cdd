"""Kernel parity of the model glue (hetersumgraph_amd.head) against tests/head_ref.py.

Bound: every output and every gradient may err against the fp64 restatement by at most
4 x yard, yard = max |fp32-CPU - fp64| of the same quantity measured in the same test (the
factor is tests/test_gpu_lstm.py's; tests/test_head_cpu.py shows that yard is never zero
and that the kernels' summation order on the CPU stays inside the bound).

Shapes: row counts 1, one below / at / one above the 4 rows of a block, one above twice
that, and 70; both LSTM widths; L a strided view; positions 0 and n_pos - 1; the HDSG
layouts of head_ref.LAYOUTS (docs of 1, 2, 7 and 130 sentences, interleaved docs, doc
nodes after their sentences).
"""
import functools

import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


def _linear(W, b=None, grad=True):
    m = torch.nn.Linear(W.shape[1], W.shape[0], bias=b is not None)
    with torch.no_grad():
        m.weight.copy_(W)
        if b is not None:
            m.bias.copy_(b)
    m = m.to(DEV)
    for p in m.parameters():
        p.requires_grad_(grad)
    return m


def _layout(name):
    from hetersumgraph_amd.head import HeadLayout
    lay = R.LAYOUTS[name]
    h = HeadLayout(lay["pair_s"], lay["pair_d"], lay["n_s"], lay["n_docs"], lay["super_pos"], lay["sent_super"],
                   lay["doc_super"], lay["inv_cnt"], DEV)
    assert h.ok
    return h


def _check(got, r32, r64, keys, what):
    y = R.yard(r32, r64)
    for k in keys:
        err = float((got[k].detach().double().cpu() - r64[k]).abs().max())
        print(f"{what} {k}: err {err:.3e} yard {y[k]:.3e} ratio {err / y[k]:.2f}")
    for k in keys:
        err = float((got[k].detach().double().cpu() - r64[k]).abs().max())
        assert y[k] > 0 and err <= R.FACTOR * y[k], (what, k, err, y[k])


def _bitwise(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _sent_refs(n, dims):
    c = R.sent_case(n, dims)
    return c, R.sent_features(c, torch.float32), R.sent_features(c, F64)


def _run_sent(c, grads=(True,) * 7, pos=None):
    """One forward + backward of head.sent_features; grads: (ngram, L, Wc, bc, Wl, bl, Wn)."""
    from hetersumgraph_amd import head
    Lw = c["L"].shape[1]
    ngram = c["ngram"].to(DEV).requires_grad_(grads[0])
    Lbuf = torch.randn(c["L"].shape[0], Lw + 24, device=DEV)
    with torch.no_grad():
        Lbuf[:, 8:8 + Lw] = c["L"].to(DEV)
    Lbuf.requires_grad_(grads[1])
    cnn, lstm, nf = _linear(c["Wc"], c["bc"]), _linear(c["Wl"], c["bl"]), _linear(c["Wn"])
    for p, g in zip((cnn.weight, cnn.bias, lstm.weight, lstm.bias, nf.weight), grads[2:]):
        p.requires_grad_(g)
    L = Lbuf[:, 8:8 + Lw]
    assert not L.is_contiguous() or L.shape[0] == 1
    S = head.sent_features(ngram, (c["pos"] if pos is None else pos).to(DEV), c["P"].to(DEV), L, cnn, lstm, nf)
    if S.requires_grad:
        S.backward(c["dS"].to(DEV))
    return dict(S=S.detach(), dngram=ngram.grad, dL=None if Lbuf.grad is None else Lbuf.grad[:, 8:8 + Lw],
                dWc=cnn.weight.grad, dbc=cnn.bias.grad, dWl=lstm.weight.grad, dbl=lstm.bias.grad, dWn=nf.weight.grad)


SENT_OUT = ("S", "dngram", "dL", "dWc", "dbc", "dWl", "dbl", "dWn")


@pytest.mark.parametrize("dims", R.DIMS, ids=lambda d: f"Lw{d[2]}")
@pytest.mark.parametrize("n", R.ROW_COUNTS)
def test_sent_features_parity_and_determinism(n, dims):
    from hetersumgraph_amd import head
    assert head.rows_per_block() == R.ROWS_PER_BLOCK
    c, r32, r64 = _sent_refs(n, dims)
    assert int(c["pos"].max()) == R.N_POS - 1 and (n == 1 or int(c["pos"].min()) == 0)      # one row holds one index
    got = _run_sent(c)
    _check(got, r32, r64, SENT_OUT, f"sent n={n} Lw={dims[2]}")
    again = _run_sent(c)
    assert _bitwise([got[k] for k in SENT_OUT], [again[k] for k in SENT_OUT])


def test_out_of_range_position_gives_a_nan_row_only():
    c, _, _ = _sent_refs(9, R.DIMS[0])
    clean = _run_sent(c, grads=(False,) * 7)["S"]
    for bad in (R.N_POS, -1, 2 ** 40):
        pos = c["pos"].clone()
        pos[5] = bad
        S = _run_sent(c, grads=(False,) * 7, pos=pos)["S"]
        assert bool(torch.isnan(S[5]).all())
        keep = [i for i in range(9) if i != 5]
        assert torch.equal(S[keep].view(torch.int32), clean[keep].view(torch.int32))


@pytest.mark.parametrize("grads", [(False, True, True, True, True, True, True), (True, False, False, False, True, True, True),
                                   (True, True, True, False, False, True, False), (False, False, False, False, False, False, True)])
def test_sent_features_needs_input_grad(grads):
    c, _, _ = _sent_refs(5, R.DIMS[1])
    full, got = _run_sent(c), _run_sent(c, grads=grads)
    for k, g in zip(SENT_OUT[1:], grads):
        if g:
            assert torch.equal(got[k].view(torch.int32), full[k].view(torch.int32)), k
        else:
            assert got[k] is None, k


def _run_doc(name, c, grads=(True, True)):
    from hetersumgraph_amd import head
    h = _layout(name)
    S = c["S"].to(DEV).requires_grad_(grads[0])
    dn = _linear(c["Wd"], grad=grads[1])
    init = head.doc_init(S, h, dn)
    if init.requires_grad:
        init.backward(c["dInit"].to(DEV))
    return dict(init=init.detach(), dS=S.grad, dWd=dn.weight.grad)


def _run_logits(name, c, grads=(True, True, True)):
    from hetersumgraph_amd import head
    h = _layout(name) if name else None
    state = c["state"].to(DEV).requires_grad_(grads[0])
    wh = _linear(c["Wh"], c["bh"])
    wh.weight.requires_grad_(grads[1])
    wh.bias.requires_grad_(grads[2])
    out = head.sent_logits(state, h, wh)
    if out.requires_grad:
        out.backward(c["dlogits"].to(DEV))
    both = wh.weight.grad is not None and wh.bias.grad is not None
    return dict(logits=out.detach(), dstate=state.grad, dWh=wh.weight.grad, dbh=wh.bias.grad,
                dWhb=torch.cat([wh.weight.grad.reshape(-1), wh.bias.grad]) if both else None)


@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_hdsg_parity_and_determinism(name):
    lay = R.LAYOUTS[name]
    c = R.doc_case(lay)
    got = _run_doc(name, c)
    _check(got, R.doc_init(c, lay, torch.float32), R.doc_init(c, lay, F64), R.DOC_KEYS, f"doc_init {name}")
    again = _run_doc(name, c)
    assert _bitwise([got[k] for k in R.DOC_KEYS], [again[k] for k in R.DOC_KEYS])
    got = _run_logits(name, c)
    _check(got, R.logits(c, lay, torch.float32), R.logits(c, lay, F64), R.LOGIT_KEYS, f"logits {name}")
    again = _run_logits(name, c)
    assert _bitwise([got[k] for k in R.LOGIT_KEYS], [again[k] for k in R.LOGIT_KEYS])


@pytest.mark.parametrize("n", R.ROW_COUNTS)
def test_hsg_logits_parity_and_determinism(n):
    c = R.hsg_case(n)
    got = _run_logits(None, c)
    _check(got, R.logits(c, None, torch.float32), R.logits(c, None, F64), R.LOGIT_KEYS, f"logits hsg n={n}")
    again = _run_logits(None, c)
    assert _bitwise([got[k] for k in R.LOGIT_KEYS], [again[k] for k in R.LOGIT_KEYS])


def test_hdsg_needs_input_grad():
    name = "docs_1_2_7"
    c = R.doc_case(R.LAYOUTS[name])
    full = _run_doc(name, c)
    a, b = _run_doc(name, c, (False, True)), _run_doc(name, c, (True, False))
    assert a["dS"] is None and torch.equal(a["dWd"], full["dWd"])
    assert b["dWd"] is None and torch.equal(b["dS"], full["dS"])
    full = _run_logits(name, c)
    a, b, d = (_run_logits(name, c, g) for g in ((False, True, True), (True, False, False), (True, True, False)))
    assert a["dstate"] is None and torch.equal(a["dWh"], full["dWh"]) and torch.equal(a["dbh"], full["dbh"])
    assert b["dWh"] is None and b["dbh"] is None and torch.equal(b["dstate"], full["dstate"])
    assert d["dbh"] is None and torch.equal(d["dWh"], full["dWh"])


def test_three_functions_capture_into_one_graph():
    """Forward and backward of the three functions, chained, in one torch.cuda.graph on one
    stream; two replays over refilled static inputs equal the eager results bitwise."""
    from hetersumgraph_amd import head
    name, dims = "docs_1_2_7", R.DIMS[0]
    lay = R.LAYOUTS[name]
    h = _layout(name)
    n, Lw = lay["n_s"], dims[2]
    cases = [dict(R.sent_case(n, dims, seed=s), **R.doc_case(lay, seed=s)) for s in (1, 2, 3)]
    c0 = cases[0]
    cnn, lstm, nf = _linear(c0["Wc"], c0["bc"]), _linear(c0["Wl"], c0["bl"]), _linear(c0["Wn"])
    dn, wh = _linear(c0["Wd"]), _linear(c0["Wh"], c0["bh"])
    params = [p for m in (cnn, lstm, nf, dn, wh) for p in m.parameters()]
    ngram = c0["ngram"].to(DEV).requires_grad_()
    Lbuf = torch.zeros(n, Lw + 24, device=DEV).requires_grad_()
    pos, Ptab, dl = c0["pos"].to(DEV), c0["P"].to(DEV), c0["dlogits"].to(DEV)

    def fill(c):
        with torch.no_grad():
            ngram.copy_(c["ngram"])
            Lbuf[:, 8:8 + Lw] = c["L"].to(DEV)
            pos.copy_(c["pos"])
            dl.copy_(c["dlogits"])

    def step():
        S = head.sent_features(ngram, pos, Ptab, Lbuf[:, 8:8 + Lw], cnn, lstm, nf)
        logits = head.sent_logits(head.doc_init(S, h, dn), h, wh)
        return (logits,) + torch.autograd.grad(logits, [ngram, Lbuf] + params, dl)

    fill(c0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    for c in cases[1:]:
        fill(c)
        g.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        eager = step()
        torch.cuda.synchronize()
        assert _bitwise(replayed, eager)
        assert all(bool(torch.isfinite(o).all()) for o in replayed)
