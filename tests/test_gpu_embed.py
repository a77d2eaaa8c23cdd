"""The word-embedding kernels (hsg_embed.hip) and ``wordembed.embed_batch``.

``hsg_embed_grad`` against the numpy restatement of its order contract (tests/embed_ref.py)
BITWISE, and against the fp64 sum within the derived bound n_v * 2^-24 * sum|terms|.
V = 37, D in {4, 300} (300 is no multiple of the 256 columns of a wave: the lane tail).
The "mixed" case holds runs of length 0, 1, P-1, P, P+1 and 3P+1, a run that starts and
one that ends exactly on a chunk boundary, a run over two whole chunks, the last run of the
list, tokens only among the word rows / only among the CNN rows / in both, and token V-1;
each with padding_idx 0 (token-0 occurrences present) and None.  Then the degenerate
shapes, the heavy-hitter merge chain (about 5,000 occurrences of one token), pitch
independence and reproducibility; and the autograd node's two outputs and gradients.
"""
import numpy as np
import pytest
import torch

import embed_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
V = R.V_CASE


def _lib():
    from hetersumgraph_amd import _lib
    return _lib.load()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _pitched(a, pitch):
    buf = torch.full((a.shape[0], pitch), float("nan"), device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return buf[:, :a.shape[1]]


def run_grad(c, D, padding_idx, pitch_w=None, pitch_x=None, poison=True):
    """hsg_embed_grad through the binding on a grad_case -> dE as numpy."""
    from hetersumgraph_amd._lib import check, ptr
    lib = _lib()
    keys = torch.from_numpy(R.keys_of(np.concatenate([c["tok_w"], c["tok_c"]]), padding_idx)).to(DEV)
    n_w, rows, n_occ = len(c["tok_w"]), len(c["tok_c"]), keys.shape[0]
    dW = _pitched(c["dW"], pitch_w or D) if n_w else None
    dX = _pitched(c["dX"], pitch_x or D) if rows else None
    dE = torch.full((V, D), float("nan"), device=DEV) if poison else torch.empty(V, D, device=DEV)
    n_ws = lib.hsg_embed_ws_floats(n_occ, D)
    ws = torch.full((n_ws,), float("nan"), device=DEV) if n_ws else None
    check(lib.hsg_embed_grad(V, D, n_occ, ptr(keys) if n_occ else None, n_w, ptr(dW), dW.stride(0) if n_w else 0, rows,
                             ptr(dX), dX.stride(0) if rows else 0, ptr(dE), ptr(ws),
                             torch.cuda.current_stream().cuda_stream), "hsg_embed_grad")
    return dE.cpu().numpy()


def _assert_case(c, D, padding_idx, **kw):
    P = _lib().hsg_embed_piece_rows()
    got = run_grad(c, D, padding_idx, **kw)
    want, ref, bound = R.case_reference(c, P, padding_idx)
    diff = np.argwhere(_bits(got) != _bits(want))
    assert diff.size == 0, f"{len(diff)} elements differ from the contract's order, first (token, column) {diff[0]}"
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    return got


def test_mixed_case_holds_what_it_claims():
    """The shared case really contains the runs and boundary positions the tests rely on."""
    P = _lib().hsg_embed_piece_rows()
    for pad in (0, None):
        c = R.grad_case(P, "mixed", 4, pad)
        tok = np.concatenate([c["tok_w"], c["tok_c"]])
        ts, ss = R.sorted_occurrences(tok, pad)
        runs = {v: (a, b) for v, a, b in R.runs(ts)}
        assert {b - a for a, b in runs.values()} >= {1, P - 1, P, P + 1, 3 * P + 1} and 1 not in runs
        a, b = runs[R.ALIGNED]
        assert a % P == 0 and b % P == 0 and b - a == 2 * P               # starts / ends on a boundary, two whole chunks
        assert any(a % P and b % P == 0 for a, b in runs.values()) and any(a % P == 0 and b % P for a, b in runs.values())
        assert runs[V - 1][1] == len(ts)                                  # the last run of the list
        n_w = len(c["tok_w"])
        side = {v: {bool(s < n_w) for s in ss[a:b]} for v, (a, b) in runs.items()}
        assert side[R.ONLY_W] == {True} and side[R.ONLY_C] == {False} and side[6] == {True, False}
        assert (0 in runs) == (pad is None) and (tok == 0).sum() == 3


@pytest.mark.parametrize("padding_idx", [0, None])
@pytest.mark.parametrize("D", [4, 300])
def test_grad_bitwise_against_the_order_contract(D, padding_idx):
    P = _lib().hsg_embed_piece_rows()
    c = R.grad_case(P, "mixed", D, padding_idx)
    got = _assert_case(c, D, padding_idx)
    absent = np.setdiff1d(np.arange(V), np.concatenate([c["tok_w"], c["tok_c"]]))
    assert absent.size and (_bits(got[absent]) == 0).all()               # exactly +0.0
    if padding_idx == 0:
        assert (_bits(got[0]) == 0).all()
    else:
        assert got[0].any()


@pytest.mark.parametrize("kind", ["no_words", "no_rows", "empty"])
@pytest.mark.parametrize("padding_idx", [0, None])
def test_degenerate_shapes(kind, padding_idx):
    P = _lib().hsg_embed_piece_rows()
    c = R.grad_case(P, kind, 4, padding_idx)
    assert (len(c["tok_w"]) == 0) == (kind != "no_rows") and (len(c["tok_c"]) == 0) == (kind != "no_words")
    got = _assert_case(c, 4, padding_idx)
    if kind == "empty":
        assert (_bits(got) == 0).all()                                    # cleared to +0.0 from the NaN poison


@pytest.mark.parametrize("D", [4, 300])
def test_heavy_hitter_merge_chain(D):
    P = _lib().hsg_embed_piece_rows()
    c = R.grad_case(P, "heavy", D, 0)
    assert (np.concatenate([c["tok_w"], c["tok_c"]]) == R.HEAVY).sum() > 64 * P     # more than one ballot of chunks
    _assert_case(c, D, 0)


def test_reproducible_and_pitch_independent():
    P = _lib().hsg_embed_piece_rows()
    D = 300
    for kind in ("mixed", "heavy"):
        c = R.grad_case(P, kind, D, 0)
        a = run_grad(c, D, 0)
        b = run_grad(c, D, 0, poison=False)
        w = run_grad(c, D, 0, pitch_w=D + 4, pitch_x=D + 24)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(w))


# ---- embed_batch: the autograd node ---------------------------------------------------------
L = 9


def _batch(D, seed=0):
    g = torch.Generator().manual_seed(seed)
    E = torch.randn(V, D, generator=g)
    pos = torch.randn(L + 1, D, generator=g)
    ids = torch.tensor([[5, 6, 7, 8, 0, 0, 0, 0, 0], [9, 0, 0, 0, 0, 0, 0, 0, 0], [3, 3, 4, 5, 6, 7, 8, 36, 2],
                        [6, 6, 6, 6, 6, 6, 0, 0, 0]], dtype=torch.int64)
    wid = torch.tensor([2, 3, 4, 5, 6, 7, 8, 9, 36, 11, 6], dtype=torch.int64)
    return E.to(DEV), pos.to(DEV), ids.to(DEV), wid.to(DEV)


def _direct_gather(E, pos, ids):
    from hetersumgraph_amd._lib import check, ptr
    from hetersumgraph_amd.cnn import _layout
    length, rowoff, rows = _layout(ids)
    X = torch.empty(rows, E.shape[1], device=DEV)
    check(_lib().hsg_cnn_gather(ids.shape[0], ids.shape[1], E.shape[1], ptr(ids), ptr(E), ptr(pos), ptr(rowoff), rows,
                                ptr(X), torch.cuda.current_stream().cuda_stream), "hsg_cnn_gather")
    return X, rowoff, rows


@pytest.mark.parametrize("D", [4, 300])
def test_embed_batch_outputs_bitwise(D):
    from hetersumgraph_amd.wordembed import embed_batch
    E, pos, ids, wid = _batch(D)
    E.requires_grad_(True)
    w_embed, X, (length, rowoff, rows) = embed_batch(E, wid, ids, pos, 0)
    assert torch.equal(w_embed.view(torch.int32), torch.nn.functional.embedding(wid, E.detach()).view(torch.int32))
    Xd, rowoff_d, rows_d = _direct_gather(E.detach(), pos, ids)
    assert rows == rows_d == int((ids != 0).sum()) + ids.shape[0] and torch.equal(rowoff, rowoff_d)
    assert torch.equal(X.view(torch.int32), Xd.view(torch.int32))
    assert length.tolist() == [4, 1, 9, 6]


def _want_grad(wid, ids, gW, gX, padding_idx, D):
    P = _lib().hsg_embed_piece_rows()
    tok = np.concatenate([wid.cpu().numpy() if gW is not None else np.zeros(0, np.int64),
                          R.cnn_tokens(ids.cpu().numpy()) if gX is not None else np.zeros(0, np.int64)])
    rows = np.concatenate([g.cpu().numpy() for g in (gW, gX) if g is not None])
    ref, bound = R.reduce_f64(tok, rows, V, padding_idx)
    return R.reduce_f32(tok, rows, V, P, padding_idx), ref, bound


@pytest.mark.parametrize("use", ["both", "words", "rows"])
@pytest.mark.parametrize("padding_idx", [0, None])
def test_embed_batch_gradient(use, padding_idx):
    from hetersumgraph_amd.wordembed import embed_batch
    D = 300
    E, pos, ids, wid = _batch(D)
    E.requires_grad_(True)
    w_embed, X, _ = embed_batch(E, wid, ids, pos, padding_idx)
    g = torch.Generator().manual_seed(9)
    gW = torch.randn(w_embed.shape, generator=g).to(DEV) if use != "rows" else None
    gX = torch.randn(X.shape, generator=g).to(DEV) if use != "words" else None
    loss = sum((o * gg).sum() for o, gg in ((w_embed, gW), (X, gX)) if gg is not None)
    loss.backward()
    want, ref, bound = _want_grad(wid, ids, gW, gX, padding_idx, D)
    got = E.grad.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    if padding_idx == 0:
        assert (_bits(got[0]) == 0).all()
    elif use != "words":
        assert got[0].any()                                               # the pad rows count for token 0


def test_frozen_weight_launches_no_reduce(monkeypatch):
    from hetersumgraph_amd import cnn
    from hetersumgraph_amd.wordembed import embed_batch
    lib = _lib()
    calls = []
    real = lib.hsg_embed_grad
    monkeypatch.setattr(lib, "hsg_embed_grad", lambda *a: calls.append(a) or real(*a), raising=False)
    D = 300
    E, pos, ids, wid = _batch(D)
    convs = [torch.randn(50, 1, h, D, device=DEV, requires_grad=True) for h in cnn.HEIGHTS]
    biases = [torch.zeros(50, device=DEV, requires_grad=True) for _ in cnn.HEIGHTS]

    def step(weight):
        w_embed, X, layout = embed_batch(weight, wid, ids, pos, 0)
        feat = cnn.sent_cnn_rows(X, layout, tuple(ids.shape), convs, biases)
        (feat.sum() + w_embed.sum()).backward()
    step(E)                                                               # frozen: no plan, no reduce
    assert not calls and E.grad is None and convs[0].grad is not None
    Et = E.clone().requires_grad_(True)
    step(Et)
    assert len(calls) == 1 and Et.grad is not None
