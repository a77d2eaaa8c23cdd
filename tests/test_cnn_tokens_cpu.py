"""The algebra and the order contract of the sentence CNN's token paths
(include/hsg_cnn_tokens.h, tests/cnn_tokens_ref.py), without a GPU: EW[token] + PW[position] is
the reference's convolution, the direct sparse weight gradient is dY^T X, the chunked order is
a pure function of the inputs, the slot map is ascending and dense and holds PAD, and the
switch refuses values it does not know."""
import numpy as np
import pytest
import torch

import cnn_tokens_ref as R
from oracle import cnn as ocnn

small_ids, params = R.small_ids, R.params


def test_tokens_forward_is_the_reference_convolution():
    n, L, V, D = 9, 11, 23, 8
    ids = small_ids(n, L, V, 0)
    E, P, cw, cb = params(V, D, L, 1)
    feat, arg = R.conv_tokens64(ids, V, E, P, cw, cb)
    t = torch.from_numpy
    ref = ocnn.sent_encoder(t(ids), t(E), t(P), [t(w) for w in cw], [t(b) for b in cb])
    assert np.abs(feat - ref.numpy()).max() < 1e-12
    assert (arg >= 0).all() and (arg <= R.lengths(ids)[:, None]).all()


def test_sparse_dw_is_the_dense_weight_gradient():
    n, L, V, D = 9, 11, 23, 8
    ids = small_ids(n, L, V, 2)
    E, P, cw, cb = params(V, D, L, 3)
    feat, arg = R.conv_tokens64(ids, V, E, P, cw, cb)
    dfeat = np.random.default_rng(4).standard_normal(feat.shape)
    dense_w, dense_b = R.dw_dense64(ids, E, P, feat, arg, dfeat)
    for chunk in (4, 64):
        w, b = R.dw(ids, E, P, feat, arg, dfeat, chunk, np.float64)
        assert np.abs(w - dense_w).max() < 1e-12 and np.abs(b - dense_b).max() < 1e-12
    # ... and autograd's gradient of the reference's own formulation, through stack_taps' layout
    t = torch.from_numpy
    leaves = [t(w).clone().requires_grad_() for w in cw] + [t(b).clone().requires_grad_() for b in cb]
    ref = ocnn.sent_encoder(t(ids), t(E), t(P), leaves[:6], leaves[6:])
    (ref * t(dfeat)).sum().backward()
    for got, leaf in zip(R.unstack_taps(dense_w), leaves[:6]):
        assert np.abs(got - leaf.grad.numpy()).max() < 1e-12
    assert np.abs(dense_b - np.concatenate([l.grad.numpy() for l in leaves[6:]])).max() < 1e-12


def _dw_scalar(ids, E, P, feat, arg, dfeat, chunk):
    """The order contract once more, one float32 operation at a time."""
    f = np.float32
    n, D = ids.shape[0], E.shape[1]
    parts_w, parts_b = [], []
    for s0 in range(0, n, chunk):
        pw, pb = np.zeros((R.NY, D), f), np.zeros(R.NF, f)
        for s in range(s0, min(s0 + chunk, n)):
            for gi, h in enumerate(R.HEIGHTS):
                for c in range(R.CH):
                    j = gi * R.CH + c
                    if not feat[s, j] > 0 or dfeat[s, j] == 0:
                        continue
                    g = f(dfeat[s, j])
                    pb[j] = f(pb[j] + g)
                    for i in range(h):
                        tok, pos = R.token_pos(ids, s, int(arg[s, j]) + i)
                        q = R.tap(h, i) * R.CH + c
                        for d in range(D):
                            x = f(f(E[tok, d]) + f(P[pos, d]))
                            pw[q, d] = f(pw[q, d] + f(g * x))
        parts_w.append(pw), parts_b.append(pb)
    w, b = parts_w[0], parts_b[0]
    for pw, pb in zip(parts_w[1:], parts_b[1:]):
        w, b = (w + pw).astype(f), (b + pb).astype(f)
    return w, b


@pytest.mark.parametrize("n", [3, 4, 5, 9])
def test_chunked_order_reproduces_itself(n):
    """n below, at and above a chunk boundary (chunk = 4), and three chunks: the vectorised
    restatement equals the scalar one bit for bit, and a chunk boundary is where the order
    changes (n <= chunk is the plain ascending sum)."""
    chunk, L, V, D = 4, 9, 17, 4
    ids = small_ids(n, L, V, 5)
    E, P, cw, cb = [np.float32(a) if not isinstance(a, list) else [np.float32(x) for x in a] for a in params(V, D, L, 6)]
    feat, arg = R.conv_tokens64(ids, V, E, P, cw, cb)
    feat = feat.astype(np.float32)
    dfeat = np.random.default_rng(7).standard_normal(feat.shape).astype(np.float32)
    w, b = R.dw(ids, E, P, feat, arg, dfeat, chunk)
    ws, bs = _dw_scalar(ids, E, P, feat, arg, dfeat, chunk)
    assert w.dtype == np.float32 and np.array_equal(w.view(np.int32), ws.view(np.int32))
    assert np.array_equal(b.view(np.int32), bs.view(np.int32))
    w2, b2 = R.dw(ids, E, P, feat, arg, dfeat, chunk)
    assert np.array_equal(w.view(np.int32), w2.view(np.int32)) and np.array_equal(b.view(np.int32), b2.view(np.int32))
    one_w, one_b = R.dw(ids, E, P, feat, arg, dfeat, 1 << 20)
    if n <= chunk:
        assert np.array_equal(w.view(np.int32), one_w.view(np.int32))
    w64, b64 = R.dw(ids, E, P, feat, arg, dfeat, chunk, np.float64)
    assert np.abs(w - w64).max() < 1e-5 and np.abs(one_w - w64).max() < 1e-5 and np.abs(b - b64).max() < 1e-5


def test_slot_map_is_ascending_dense_and_holds_pad():
    V = 40
    ids = small_ids(12, 9, V, 8)
    ids[ids == 5] = 6                                     # a token that is absent
    present, slot, U = R.slot_map(ids, V)
    tokens = np.unique(np.concatenate([[0], ids.reshape(-1)]))
    assert present[0] == 1 and slot[0] == 0 and present[5] == 0
    assert U == len(tokens) == present.sum()
    assert np.array_equal(slot[tokens], np.arange(U))     # ascending with the id, dense
    assert (np.diff(slot) >= 0).all() and slot.dtype == np.int32
    full = np.full((2, 9), 3, np.int64)                   # no PAD in the batch: PAD is a row all the same
    present, slot, U = R.slot_map(full, V)
    assert U == 2 and slot[0] == 0 and slot[3] == 1
    present, slot, U = R.slot_map(np.zeros((3, 9), np.int64), V)
    assert U == 1 and present.sum() == 1
    Tb, U = R.table(ids, V, np.arange(V * 4.).reshape(V, 4), -np.arange(10 * 4.).reshape(10, 4))
    assert Tb.shape == (U + 10, 4) and np.array_equal(Tb[:U, 0], tokens * 4.) and np.array_equal(Tb[U:, 0], -np.arange(10) * 4.)


def test_unknown_switch_value_raises():
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.cnn import MODES, sent_cnn_mode, sent_cnn_switched
    assert MODES == ("0", "dw", "tokens")
    for ok in MODES:
        with _lib.path_options(HSG_SENT_CNN=ok):
            assert sent_cnn_mode() == ok
    for bad in ("1", "token", "", "DW"):
        with _lib.path_options(HSG_SENT_CNN=bad):
            with pytest.raises(ValueError, match="HSG_SENT_CNN"):
                sent_cnn_mode()
            with pytest.raises(ValueError, match="HSG_SENT_CNN"):
                sent_cnn_switched(torch.zeros(2, 9, dtype=torch.long), torch.zeros(4, 8), torch.zeros(10, 8), [], [])
