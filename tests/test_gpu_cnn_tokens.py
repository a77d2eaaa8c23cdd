"""The sentence CNN's token paths on the GPU (path_options(HSG_SENT_CNN="dw" | "tokens"),
hetersumgraph_amd.cnn.sent_cnn_tokens -> include/hsg_cnn_tokens.h).

Bitwise: Tb is a bit copy, feat / arg are the pool's value contract on the device's own TW,
dWall / dbias are the order contract (tests/cnn_tokens_ref.py), two runs are equal.

Parity, at exactly the bounds tests/test_gpu_encoder.py holds today's path to: feat within 5e-5
of the reference's golden (feat64 and feat32) and of the fp64 oracle, conv weight and bias
gradients within 1e-4 relative to the largest entry.  A max-pool gradient is discontinuous
where two windows tie within rounding, and the "tokens" forward rounds differently from the
reference (the golden's closest top-two windows are 1e-5 apart: one token repeated, height 2),
so both parity tests multiply the upstream gradient by ``test_gpu_encoder.unambiguous(...,
tol=1e-4)`` and assert that the mask keeps >= 0.99 of the pairs.  The golden's gradients were
recorded for the unmasked upstream gradient; the gradient is linear in it, so the golden minus
the fp64 oracle's gradient for the few masked-out pairs is the reference for the masked run.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cnn_tokens_ref as R
import weights
from helpers import load_fixture
from oracle import cnn as ocnn
from test_encoder_oracle import SEED, encoder_params
from test_gpu_encoder import cnndm_ids, rel_err, unambiguous

pytestmark = pytest.mark.gpu

MODES = ("dw", "tokens")


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({4: np.int32, 8: np.int64}[a.itemsize])


def run(mode, ids, emb, pos, cw, cb, Rm, train_embed=False):
    """(feat, conv weight grads, conv bias grads) of the switched encoder on the GPU."""
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.cnn import sent_cnn_switched
    e = emb.float().cuda().requires_grad_(train_embed)
    w = [t.float().cuda().requires_grad_() for t in cw]
    b = [t.float().cuda().requires_grad_() for t in cb]
    with _lib.path_options(HSG_SENT_CNN=mode):
        feat = sent_cnn_switched(ids.cuda(), e, pos.float().cuda(), w, b, padding_idx=0)
        (feat * Rm.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    return feat.detach(), [t.grad for t in w], [t.grad for t in b], e.grad


def oracle(ids, emb, pos, cw, cb, Rm):
    leaves = [t.double().clone().requires_grad_() for t in list(cw) + list(cb)]
    ref = ocnn.sent_encoder(ids, emb.double(), pos.double(), leaves[:6], leaves[6:])
    (ref * Rm.double()).sum().backward()
    return ref.detach(), [t.grad for t in leaves[:6]], [t.grad for t in leaves[6:]]


# ---------------------------------------------------------------------------- kernels, bitwise
def device_steps(ids, E, Pm, wall, cb):
    """The entry points one by one, as sent_cnn_tokens calls them."""
    from hetersumgraph_amd._lib import check, load, ptr, stream_of
    from hetersumgraph_amd.cnn import LDY, NY
    from hetersumgraph_amd.dense import gemm
    lib = load()
    n, L = ids.shape
    V, D = E.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ids_d, E_d, P_d = d(ids), d(E), d(Pm)
    st = stream_of(E_d)
    present = torch.zeros(V + 1, dtype=torch.int32, device="cuda")
    check(lib.hsg_cnn_tok_mark(n, L, V, ptr(ids_d), ptr(present), ptr(present[V:]), st), "mark")
    slot = torch.cumsum(present[:V], 0, dtype=torch.int32) - 1
    U = int(slot[-1]) + 1
    Tb = torch.empty(U + L + 1, D, device="cuda")
    check(lib.hsg_cnn_tok_table(V, D, U, L, ptr(present), ptr(slot), ptr(E_d), ptr(P_d), ptr(Tb), D, st), "table")
    TW = torch.empty(U + L + 1, LDY, device="cuda")
    gemm(Tb, d(wall), b_t=True, out=TW[:, :NY])
    rowoff = torch.zeros(n + 1, dtype=torch.int32)
    rowoff[1:] = torch.cumsum(torch.from_numpy(R.lengths(ids) + 1), 0)
    rowoff = rowoff.cuda()
    bias = [d(b) for b in cb]
    bptr = (ctypes.c_void_p * 6)(*[b.data_ptr() for b in bias])
    feat = torch.empty(n, R.NF, device="cuda")
    arg = torch.empty(n, R.NF, dtype=torch.int32, device="cuda")
    check(lib.hsg_cnn_tok_pool(n, L, V, U, ptr(ids_d), ptr(rowoff), ptr(slot), ptr(TW), LDY, bptr, ptr(feat), ptr(arg),
                               st), "pool")

    def dw(dfeat):
        ws = torch.empty(lib.hsg_cnn_tok_dw_ws_floats(n, D), device="cuda")
        dwall = torch.empty(R.NY, D, device="cuda")
        db = torch.empty(R.NF, device="cuda")
        check(lib.hsg_cnn_tok_dw(n, L, V, D, ptr(ids_d), ptr(rowoff), ptr(E_d), ptr(P_d), ptr(feat), ptr(arg),
                                 ptr(d(dfeat)), ptr(ws), ptr(dwall), D, ptr(db), st), "dw")
        torch.cuda.synchronize()
        return dwall.cpu().numpy(), db.cpu().numpy()
    torch.cuda.synchronize()
    return dict(present=present[:V].cpu().numpy(), bad=int(present[V]), slot=slot.cpu().numpy(), U=U,
                Tb=Tb.cpu().numpy(), TW=TW[:, :NY].cpu().numpy(), feat=feat.cpu().numpy(), arg=arg.cpu().numpy(), dw=dw)


@pytest.mark.parametrize("n,L,V,D", [(130, 100, 200, 300), (3, 7, 200, 300)])
def test_kernels_bitwise(n, L, V, D):
    from hetersumgraph_amd._lib import load
    C = load().hsg_cnn_tok_chunk()
    ids = cnndm_ids(n, L, V, 3).numpy() if n > 4 else R.small_ids(n, L, V, 3)
    E, Pm, cw, cb = [[np.float32(x) for x in a] if isinstance(a, list) else np.float32(a) for a in R.params(V, D, L, 4)]
    wall = R.stack_taps(cw)
    out = device_steps(ids, E, Pm, wall, cb)
    present, slot, U = R.slot_map(ids, V)
    if n == 130:
        assert -(-n // C) == 3 and n % C == 2                 # three chunks: 64 + 64 + 2 sentences
        assert U == V and set(R.lengths(ids)[:4]) == {0, 1, 6, L}
    assert out["bad"] == 0 and out["U"] == U
    assert np.array_equal(out["present"], present) and np.array_equal(out["slot"], slot)
    want_tb, _ = R.table(ids, V, E, Pm)
    assert np.array_equal(bits(out["Tb"]), bits(want_tb))                      # a bit copy
    feat, arg = R.pool(ids, slot, U, out["TW"], cb)                            # on the device's own TW
    assert np.array_equal(bits(out["feat"]), bits(feat)) and np.array_equal(out["arg"], arg)
    assert (out["feat"] > 0).mean() > 0.2
    dfeat = np.random.default_rng(5).standard_normal(feat.shape).astype(np.float32)
    dwall, db = out["dw"](dfeat)
    ww, wb = R.dw(ids, E, Pm, out["feat"], out["arg"], dfeat, C)
    assert np.array_equal(bits(dwall), bits(ww)) and np.array_equal(bits(db), bits(wb))
    dwall2, db2 = out["dw"](dfeat)                                             # two runs
    assert np.array_equal(bits(dwall), bits(dwall2)) and np.array_equal(bits(db), bits(db2))
    w64, b64 = R.dw(ids, E, Pm, out["feat"], out["arg"], dfeat, C, np.float64)
    assert np.abs(dwall - w64).max() <= 1e-4 * np.abs(w64).max()


# ---------------------------------------------------------------------------- parity
@functools.lru_cache(None)
def golden_case():
    z = load_fixture("encoder")
    ids = torch.from_numpy(z["ids"])
    emb, pos, cw, cb = encoder_params()
    mask = unambiguous(ids, emb, pos, cw, cb, tol=1e-4)
    Rfull = torch.from_numpy(weights.feature(SEED, "dfeat", (ids.shape[0], 300))).double()
    _, dropped_w, dropped_b = oracle(ids, emb, pos, cw, cb, Rfull * (~mask))
    ref_w = [torch.from_numpy(z[f"conv{i}_wgrad64"]).double() - dropped_w[i] for i in range(6)]
    ref_b = [torch.from_numpy(z[f"conv{i}_bgrad64"]).double() - dropped_b[i] for i in range(6)]
    return z, ids, (emb, pos, cw, cb), mask, Rfull * mask, ref_w, ref_b


@pytest.mark.parametrize("mode", MODES)
def test_matches_reference_golden(mode):
    z, ids, prm, mask, Rm, ref_w, ref_b = golden_case()
    keep = mask.double().mean().item()
    print(f"golden: mask keeps {keep:.5f} of the pairs")
    assert keep >= 0.99
    feat, gw, gb, ge = run(mode, ids, *prm, Rm)
    e64 = (feat.cpu().double() - torch.from_numpy(z["feat64"]).double()).abs().max().item()
    e32 = (feat.cpu().double() - torch.from_numpy(z["feat32"]).double()).abs().max().item()
    errs = [(rel_err(gw[i], ref_w[i]), rel_err(gb[i], ref_b[i])) for i in range(6)]
    print(f"{mode}: feat vs feat64 {e64:.3g}, vs feat32 {e32:.3g}; grad rel errs {errs}")
    assert feat.shape == (ids.shape[0], 300) and ge is None
    assert e64 < 5e-5 and e32 < 5e-5
    for i in range(6):
        assert errs[i][0] < 1e-4 and errs[i][1] < 1e-4, i


@functools.lru_cache(None)
def oracle_case():
    n, L, V, D = 130, 100, 200, 300
    torch.manual_seed(3)
    ids = cnndm_ids(n, L, V, 3)
    emb = 0.5 * torch.randn(V, D, dtype=torch.float64)
    from hetersumgraph_amd.module.PositionEmbedding import get_sinusoid_encoding_table
    pos = get_sinusoid_encoding_table(L + 1, D, padding_idx=0).double()
    cw = [torch.randn(50, 1, h, D, dtype=torch.float64) / np.sqrt(h * D) for h in range(2, 8)]
    cb = [0.1 * torch.randn(50, dtype=torch.float64) for _ in range(6)]
    mask = unambiguous(ids, emb, pos, cw, cb, tol=1e-4)
    Rm = torch.randn(n, 300, dtype=torch.float64) * mask
    return ids, (emb, pos, cw, cb), mask, Rm, oracle(ids, emb, pos, cw, cb, Rm)


@pytest.mark.parametrize("mode", MODES)
def test_cnndm_shape_vs_oracle(mode):
    ids, prm, mask, Rm, (ref, ref_w, ref_b) = oracle_case()
    keep = mask.double().mean().item()
    print(f"130 sentences: mask keeps {keep:.5f} of the pairs")
    assert keep >= 0.99
    feat, gw, gb, _ = run(mode, ids, *prm, Rm)
    err = (feat.cpu().double() - ref).abs().max().item()
    errs = [(rel_err(gw[i], ref_w[i]), rel_err(gb[i], ref_b[i])) for i in range(6)]
    print(f"{mode}: feat vs oracle {err:.3g}; grad rel errs {errs}")
    assert err < 5e-5
    for i in range(6):
        assert errs[i][0] < 1e-4 and errs[i][1] < 1e-4, i


def test_dw_against_todays_path():
    """ "dw" keeps today's forward, so feat is bitwise today's; its gradients are today's sums in
    another order."""
    ids, prm, mask, Rm, _ = oracle_case()
    feat0, gw0, gb0, _ = run("0", ids, *prm, Rm)
    feat1, gw1, gb1, _ = run("dw", ids, *prm, Rm)
    assert np.array_equal(bits(feat0), bits(feat1))
    for i in range(6):
        assert rel_err(gw1[i], gw0[i].cpu()) < 1e-4 and rel_err(gb1[i], gb0[i].cpu()) < 1e-4, i
    feat2, gw2, gb2, _ = run("dw", ids, *prm, Rm)                              # deterministic
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(gw1 + gb1, gw2 + gb2))


# ---------------------------------------------------------------------------- edge cases
def small_params():
    emb, pos, cw, cb = encoder_params(torch.float32)              # V = 64, D = 300, L = 20
    return emb, pos, cw, cb


@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(monkeypatch, mode):
    from hetersumgraph_amd import _lib, cnn
    from hetersumgraph_amd.cnn import sent_cnn_switched, token_path_ok
    emb, pos, cw, cb = small_params()
    V, L = emb.shape[0], 20
    one = torch.ones(1, 300, dtype=torch.float64)

    def both(ids):
        Rm = one.expand(ids.shape[0], 300)
        feat, gw, gb, _ = run(mode, ids, emb, pos, cw, cb, Rm)
        ref, rw, rb = oracle(ids, emb, pos, cw, cb, Rm)
        assert (feat.cpu().double() - ref).abs().max() < 5e-5
        return gw, gb, rw, rb

    with _lib.path_options(HSG_SENT_CNN=mode):
        e, p = emb.cuda(), pos.cuda()
        w, b = [t.cuda() for t in cw], [t.cuda() for t in cb]
        assert token_path_ok(torch.zeros(2, L, dtype=torch.long, device="cuda"), e, p)
        # no sentences
        out = sent_cnn_switched(torch.zeros(0, L, dtype=torch.long, device="cuda"), e, p, w, b)
        assert out.shape == (0, 300)
        # an id >= V and a negative id: refused before any table row is read
        for bad in (V, -1):
            ids = torch.ones(3, L, dtype=torch.long, device="cuda")
            ids[1, 4] = bad
            with pytest.raises(ValueError, match="outside the vocabulary"):
                sent_cnn_switched(ids, e, p, w, b)
        with pytest.raises(ValueError, match="trailing"):
            sent_cnn_switched(torch.tensor([[1, 0, 2] + [0] * 17], device="cuda"), e, p, w, b)
        # outside token_path_ok: exactly today's path and today's errors
        with pytest.raises(ValueError, match="widest kernel"):
            sent_cnn_switched(torch.ones(2, 6, dtype=torch.long, device="cuda"), e, p, w, b)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sent_cnn_switched(torch.zeros(3, L, dtype=torch.long), emb, pos, cw, cb)
        assert not token_path_ok(torch.zeros(3, L, dtype=torch.long), emb, pos)
    # an all-padding batch: U = 1, every window is the pad window; the gradient lands on the pad row
    gw, gb, rw, rb = both(torch.zeros(3, L, dtype=torch.long))
    for i in range(6):
        assert rel_err(gw[i], rw[i]) < 1e-4 and rel_err(gb[i], rb[i]) < 1e-4
    # every sentence of length L (no pad window), token V - 1 among them
    ids = torch.from_numpy(np.random.default_rng(6).integers(1, V, (5, L)))
    ids[2, L - 1] = V - 1
    both(ids)
    # a trainable embedding stays on today's path: the same launches (its embedding gradient is an
    # index_add_, whose order is not fixed, so that one is compared in value)
    ids = torch.from_numpy(R.small_ids(9, L, V, 7))
    Rm = torch.from_numpy(np.random.default_rng(8).standard_normal((9, 300)))
    taken = []
    monkeypatch.setattr(cnn, "sent_cnn_tokens", lambda *a, **kw: taken.append(1))
    got = run(mode, ids, emb, pos, cw, cb, Rm, train_embed=True)
    want = run("0", ids, emb, pos, cw, cb, Rm, train_embed=True)
    assert not taken and got[3] is not None and rel_err(got[3], want[3].cpu()) < 1e-5
    assert np.array_equal(bits(got[0]), bits(want[0]))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[1] + got[2], want[1] + want[2]))
