"""Sentence CNN encoder on the MFMA GEMM + HIP gather / max-pool kernels (C ABI ops).

Reference: module/Encoder.py:56-76 -- x = embed(ids) + pos_embed(pos) over the padded
sentence ([n, L, D]), six Conv2d(1, 50, (h, D)) for h = 2..7, ReLU, max-pool over time,
concat -> [n, 300].

Here (hsg_cnn.hip, include/hsg.h "sentence CNN encoder"):
  X    = gathered rows: the len_s real rows of each sentence plus ONE pad row
         (embed[0] + pos[0]: every padded position has that value)   hsg_cnn_gather
  Y    = X Wall^T, Wall = the 27 conv taps x 50 channels stacked     hsg_gemm_f32
  feat = relu(max_t (b_h + sum_i Y[t+i, tap(h,i)]))  + first argmax   hsg_cnn_pool
Backward: dY = scatter of the ReLU-masked dfeat into each max window (hsg_cnn_pool_bwd),
dWall = dY^T X (split-K GEMM), db_h = column sums of the masked dfeat, and -- only when
the word embedding trains (train.py:342 ``--embed_train``) -- dX = dY Wall scattered
into the embedding rows.

The GEMM covers sum_s (len_s + 1) rows instead of the reference's n * L padded rows,
and computes each (row, tap) product once instead of once per window.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check, load, ptr, stream_of
from .dense import gemm, splits_for

HEIGHTS = tuple(range(2, 8))     # Encoder.py:37-38 min/max kernel size
CHANNELS = 50                    # Encoder.py:36
TAPS = sum(HEIGHTS)              # 27
NY = TAPS * CHANNELS             # 1350 columns of Y
LDY = (NY + 3) // 4 * 4          # hsg_gemm_f32 wants 16-byte row pitch


def stack_taps(weights):
    """Conv2d weights [50, 1, h, D] (h = 2..7) -> Wall [27*50, D], row (tap(h,i))*50 + c."""
    rows = []
    for h, w in zip(HEIGHTS, weights):
        rows.append(w.reshape(CHANNELS, h, w.shape[-1]).transpose(0, 1).reshape(h * CHANNELS, w.shape[-1]))
    return torch.cat(rows, 0).contiguous()


class BatchLayout(tuple):
    """A prebuilt ``(length, rowoff, rows)`` of :func:`_layout` (the resident store's model view
    assembles it on the device), checked where it was built: padding is trailing and no id is
    negative.  ``max_token``: the largest id any batch can hold, for the range check on the host.
    With one, :func:`sent_cnn` and the "dw" path read nothing back; "tokens" reads back the number
    of distinct tokens only."""

    def __new__(cls, length, rowoff, rows, max_token):
        self = super().__new__(cls, (length, rowoff, int(rows)))
        self.max_token = int(max_token)
        return self

    def check(self, ids, V=None):
        n = ids.shape[0]
        if tuple(self[0].shape) != (n,) or tuple(self[1].shape) != (n + 1,) or self[1].dtype != torch.int32:
            raise ValueError("sentEncoder: the layout given is not that of these token rows")
        if V is not None and self.max_token >= V:
            raise ValueError(f"sentEncoder: token ids outside the vocabulary [0, {V})")
        return self


def _layout(ids):
    """Per-sentence lengths (Encoder.py:57 ``(input != 0).sum``), rowoff [n+1] int32 and
    the total row count (one host sync).  Padding must be trailing: the reference gives
    every position t >= len_s position 0, which equals the shared pad row only if the
    token there is PAD too (the dataloader always pads at the end, dataloader.py:97-109)."""
    n, L = ids.shape
    nz = ids != 0
    length = nz.sum(1)
    ar = torch.arange(L, device=ids.device)
    bad = (nz & (ar.unsqueeze(0) >= length.unsqueeze(1))).any()
    rowoff = torch.zeros(n + 1, dtype=torch.int32, device=ids.device)
    torch.cumsum(length + 1, 0, out=rowoff[1:])
    rows, bad = torch.stack([rowoff[-1].long(), bad.long()]).tolist()
    if bad:
        raise ValueError("sentEncoder: token ids after the first PAD (0) -- padding must be trailing")
    return length, rowoff, rows


def _conv_pool(X, n, L, rowoff, wall, bias):
    """Y = X Wall^T, then the shifted sum / ReLU / max-pool with argmax -> (feat, arg)."""
    rows = X.shape[0]
    Y = X.new_empty(rows, LDY)
    gemm(X, wall, b_t=True, out=Y[:, :NY])
    feat = X.new_empty(n, len(HEIGHTS) * CHANNELS)
    arg = torch.empty(n, len(HEIGHTS) * CHANNELS, dtype=torch.int32, device=X.device)
    bptr = (ctypes.c_void_p * len(bias))(*[b.data_ptr() for b in bias])
    check(load().hsg_cnn_pool(n, L, ptr(rowoff), ptr(Y), LDY, bptr, ptr(feat), ptr(arg), stream_of(X)), "hsg_cnn_pool")
    return feat, arg


def _pool_bwd(X, n, rowoff, feat, arg, dfeat):
    """dY [rows, LDY]: the ReLU-masked dfeat routed to the rows of each max window."""
    dY = X.new_zeros(X.shape[0], LDY)
    check(load().hsg_cnn_pool_bwd(n, ptr(rowoff), ptr(feat), ptr(arg), ptr(dfeat), ptr(dY), LDY, stream_of(X)),
          "hsg_cnn_pool_bwd")
    return dY


def _dbias(dfeat, feat, needed):
    masked = (dfeat * (feat > 0)).view(feat.shape[0], len(HEIGHTS), CHANNELS)
    return [masked[:, g].sum(0) if needed[g] else None for g in range(len(HEIGHTS))]


class _SentCNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, embed_w, pos_w, wall, padding_idx, layout, *bias):
        lib = load()
        n, L = ids.shape
        D = embed_w.shape[1]
        st = stream_of(embed_w)
        length, rowoff, rows = _layout(ids) if layout is None else layout.check(ids)
        X = embed_w.new_empty(rows, D)
        check(lib.hsg_cnn_gather(n, L, D, ptr(ids), ptr(embed_w), ptr(pos_w), ptr(rowoff), rows, ptr(X), st),
              "hsg_cnn_gather")
        feat, arg = _conv_pool(X, n, L, rowoff, wall, bias)
        ctx.save_for_backward(ids, X, wall, rowoff, length, feat, arg)
        ctx.n_embed, ctx.padding_idx = embed_w.shape[0], padding_idx
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        ids, X, wall, rowoff, length, feat, arg = ctx.saved_tensors
        n, L = ids.shape
        rows, D = X.shape
        dfeat = dfeat.contiguous()
        dY = _pool_bwd(X, n, rowoff, feat, arg, dfeat)
        d_embed = dwall = None
        if ctx.needs_input_grad[3]:
            dwall = gemm(dY[:, :NY], X, a_t=True, splits=splits_for(NY, D, rows))
        if ctx.needs_input_grad[1]:
            dX = gemm(dY[:, :NY], wall)                                      # [rows, D]
            sent = torch.repeat_interleave(torch.arange(n, device=X.device), length + 1)
            t = torch.arange(rows, device=X.device) - rowoff[:-1].long()[sent]
            tok = torch.where(t < length[sent], ids[sent, t.clamp(max=L - 1)], torch.zeros_like(t))
            d_embed = X.new_zeros(ctx.n_embed, D).index_add_(0, tok, dX)
            if ctx.padding_idx is not None:
                d_embed[ctx.padding_idx] = 0                  # nn.Embedding(padding_idx=...) semantics
        dbias = _dbias(dfeat, feat, ctx.needs_input_grad[6:])
        return (None, d_embed, None, dwall, None, None, *dbias)


def sent_cnn(ids, embed_weight, pos_weight, conv_weights, conv_biases, padding_idx=None, layout=None):
    """Encoder.py:56-76 forward on the HIP path: ids [n, L] int64 (PAD = 0, trailing),
    embed_weight [V, D] (``padding_idx``: the embedding row that gets no gradient, as
    nn.Embedding), pos_weight [sent_max_len+1, D] (row 0 = padding position),
    conv_weights / conv_biases of the six Conv2d(1, 50, (h, D)).  Returns [n, 300].
    ``layout``: a :class:`BatchLayout` of ``ids`` in place of the one computed (and read back)
    here."""
    if not ids.is_cuda or embed_weight.dtype != torch.float32:
        raise RuntimeError("hetersumgraph_amd sentence CNN runs only on a ROCm device in fp32 (no CPU fallback)")
    n, L = ids.shape
    D = embed_weight.shape[1]
    if L < max(HEIGHTS):
        raise ValueError(f"sentEncoder: sentence length {L} < the widest kernel {max(HEIGHTS)}")
    if L > pos_weight.shape[0] - 1:
        raise ValueError(f"sentEncoder: {L} tokens but only {pos_weight.shape[0] - 1} positions")
    if D % 4:
        raise ValueError("sentEncoder: word_emb_dim must be a multiple of 4 (GEMM row pitch)")
    if n == 0:
        return embed_weight.new_zeros(0, len(HEIGHTS) * CHANNELS)
    wall = stack_taps([w.float() for w in conv_weights])
    return _SentCNN.apply(ids.long().contiguous(), embed_weight.contiguous(), pos_weight.contiguous(), wall,
                          padding_idx, layout, *[b.contiguous() for b in conv_biases])


# ---------------------------------------------------------------------------------------------
# Opt-in (``path_options(HSG_SENT_CNN="dw" | "tokens")``, include/hsg_cnn_tokens.h), for a frozen
# embedding and position table:
#   "dw"      today's forward; the weight gradient summed directly from the max windows
#             (hsg_cnn_tok_dw: no dY, no saved X, no GEMM)
#   "tokens"  also the forward on the batch's DISTINCT tokens: Y[row] = (E Wall^T)[token] +
#             (P Wall^T)[position], so the GEMM covers U + L + 1 rows instead of sum_s (len_s + 1)
MODES = ("0", "dw", "tokens")


def sent_cnn_mode():
    """The value of the ``HSG_SENT_CNN`` switch ("0", "dw" or "tokens"); anything else raises."""
    mode = _lib.path_option("HSG_SENT_CNN", "0")
    if mode not in MODES:
        raise ValueError(f"HSG_SENT_CNN={mode!r}: one of {', '.join(MODES)}")
    return mode


def token_path_ok(ids, embed_weight, pos_weight) -> bool:
    """The token paths cover this call: a ROCm device, fp32, contiguous tables, a width and a
    sentence length the kernels take (D % 4 == 0, 7 <= L <= 400), the word embedding and the
    position table both frozen, and HSG_CHECK_NAN off (its assertions live on today's path)."""
    from .module.GATLayer import CHECK_NAN
    if CHECK_NAN or not (ids.is_cuda and embed_weight.is_cuda and pos_weight.is_cuda) or ids.dim() != 2:
        return False
    if embed_weight.dtype != torch.float32 or pos_weight.dtype != torch.float32:
        return False
    if embed_weight.requires_grad or pos_weight.requires_grad:
        return False
    if embed_weight.dim() != 2 or not embed_weight.is_contiguous() or not pos_weight.is_contiguous():
        return False
    L, D = ids.shape[1], embed_weight.shape[1]
    return L <= pos_weight.shape[0] - 1 and bool(load().hsg_cnn_tok_supported(L, D))


def _layout_tokens(ids, V, slots):
    """:func:`_layout` plus the range check of the ids and -- ``slots`` -- the slot map of the
    batch's distinct tokens (PAD included), all behind the same single read-back.  Returns
    (length, rowoff, rows, present int32 [V] | None, slot int32 [V] | None, U)."""
    n, L = ids.shape
    nz = ids != 0
    length = nz.sum(1)
    ar = torch.arange(L, device=ids.device)
    inner = (nz & (ar.unsqueeze(0) >= length.unsqueeze(1))).any()
    rowoff = torch.zeros(n + 1, dtype=torch.int32, device=ids.device)
    torch.cumsum(length + 1, 0, out=rowoff[1:])
    present = slot = None
    if slots:
        present = torch.zeros(V + 1, dtype=torch.int32, device=ids.device)      # [V] flags, then *bad
        check(load().hsg_cnn_tok_mark(n, L, V, ptr(ids), ptr(present), ptr(present[V:]), stream_of(ids)),
              "hsg_cnn_tok_mark")
        slot = torch.cumsum(present[:V], 0, dtype=torch.int32) - 1
        oob, U = present[V].long(), slot[V - 1].long() + 1
    else:
        oob, U = ((ids < 0) | (ids >= V)).any().long(), inner.new_zeros((), dtype=torch.long)
    rows, inner, oob, U = torch.stack([rowoff[-1].long(), inner.long(), oob, U]).tolist()
    if oob:
        raise ValueError(f"sentEncoder: token ids outside the vocabulary [0, {V})")
    if inner:
        raise ValueError("sentEncoder: token ids after the first PAD (0) -- padding must be trailing")
    return length, rowoff, rows, present, slot, U


class _SentCNNTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, embed_w, pos_w, wall, mode, layout, *bias):
        lib = load()
        n, L = ids.shape
        V, D = embed_w.shape
        st = stream_of(embed_w)
        if layout is None:
            _, rowoff, rows, present, slot, U = _layout_tokens(ids, V, mode == "tokens")
            Tb = embed_w.new_empty(U + L + 1, D) if mode == "tokens" else None
        else:
            # the range check is the host's.  U, which sizes the token table, stays a read-back:
            # sizing it by an upper bound kept with the store measured slower
            _, rowoff, rows = layout.check(ids, V)
            if mode == "tokens":
                present = torch.zeros(V + 1, dtype=torch.int32, device=ids.device)
                check(lib.hsg_cnn_tok_mark(n, L, V, ptr(ids), ptr(present), ptr(present[V:]), st), "hsg_cnn_tok_mark")
                slot = torch.cumsum(present[:V], 0, dtype=torch.int32) - 1
                U = int(slot[V - 1]) + 1
                Tb = embed_w.new_empty(U + L + 1, D)
        if mode == "tokens":
            check(lib.hsg_cnn_tok_table(V, D, U, L, ptr(present), ptr(slot), ptr(embed_w), ptr(pos_w), ptr(Tb), D,
                                        st), "hsg_cnn_tok_table")
            TW = embed_w.new_empty(U + L + 1, LDY)
            gemm(Tb, wall, b_t=True, out=TW[:, :NY])
            feat = embed_w.new_empty(n, len(HEIGHTS) * CHANNELS)
            arg = torch.empty(n, len(HEIGHTS) * CHANNELS, dtype=torch.int32, device=ids.device)
            bptr = (ctypes.c_void_p * len(bias))(*[b.data_ptr() for b in bias])
            check(lib.hsg_cnn_tok_pool(n, L, V, U, ptr(ids), ptr(rowoff), ptr(slot), ptr(TW), LDY, bptr, ptr(feat),
                                       ptr(arg), st), "hsg_cnn_tok_pool")
        else:
            X = embed_w.new_empty(rows, D)
            check(lib.hsg_cnn_gather(n, L, D, ptr(ids), ptr(embed_w), ptr(pos_w), ptr(rowoff), rows, ptr(X), st),
                  "hsg_cnn_gather")
            feat, arg = _conv_pool(X, n, L, rowoff, wall, bias)
        ctx.save_for_backward(ids, embed_w, pos_w, rowoff, feat, arg)     # X, Y / Tb, TW end with the forward
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        ids, embed_w, pos_w, rowoff, feat, arg = ctx.saved_tensors
        lib = load()
        n, L = ids.shape
        V, D = embed_w.shape
        dfeat = dfeat.contiguous()
        nws = lib.hsg_cnn_tok_dw_ws_floats(n, D)
        ws = embed_w.new_empty(nws)
        dwall = embed_w.new_empty(NY, D)
        db = embed_w.new_empty(len(HEIGHTS) * CHANNELS)
        check(lib.hsg_cnn_tok_dw(n, L, V, D, ptr(ids), ptr(rowoff), ptr(embed_w), ptr(pos_w), ptr(feat), ptr(arg),
                                 ptr(dfeat), ptr(ws), ptr(dwall), D, ptr(db), stream_of(embed_w)), "hsg_cnn_tok_dw")
        db = db.view(len(HEIGHTS), CHANNELS)
        dbias = [db[g] if need else None for g, need in enumerate(ctx.needs_input_grad[6:])]
        return (None, None, None, dwall if ctx.needs_input_grad[3] else None, None, None, *dbias)


def sent_cnn_tokens(ids, embed_weight, pos_weight, conv_weights, conv_biases, mode="tokens", layout=None):
    """:func:`sent_cnn` for a frozen embedding on the token paths (``mode``: "dw" or "tokens",
    see above).  The caller has asked :func:`token_path_ok`; the arguments and the result are
    :func:`sent_cnn`'s.  An id outside the vocabulary raises ``ValueError`` before any table row
    is read."""
    if mode not in MODES[1:]:
        raise ValueError(f"sent_cnn_tokens: mode {mode!r} is not one of {', '.join(MODES[1:])}")
    if not token_path_ok(ids, embed_weight, pos_weight):
        raise RuntimeError("sent_cnn_tokens: the call is outside token_path_ok (frozen fp32 tables on a ROCm device)")
    n, L = ids.shape
    if n == 0:
        return embed_weight.new_zeros(0, len(HEIGHTS) * CHANNELS)
    wall = stack_taps([w.float() for w in conv_weights])
    return _SentCNNTokens.apply(ids.long().contiguous(), embed_weight, pos_weight, wall, mode, layout,
                                *[b.contiguous() for b in conv_biases])


def sent_cnn_switched(ids, embed_weight, pos_weight, conv_weights, conv_biases, padding_idx=None, layout=None):
    """:func:`sent_cnn` behind the ``HSG_SENT_CNN`` switch: a token path where it is selected and
    :func:`token_path_ok` holds, today's path (and its errors) for every other call."""
    mode = sent_cnn_mode()
    if mode != "0" and token_path_ok(ids, embed_weight, pos_weight):
        return sent_cnn_tokens(ids, embed_weight, pos_weight, conv_weights, conv_biases, mode=mode, layout=layout)
    return sent_cnn(ids, embed_weight, pos_weight, conv_weights, conv_biases, padding_idx=padding_idx, layout=layout)


# ---------------------------------------------------------------------------------------------
# Opt-in (``path_options(HSG_SENT_CNN_VOCAB="1")``, include/hsg_cnn_vocab.h), for a forward that
# records no gradient (model.eval() under torch.no_grad()): the identity of the "tokens" path with
# the products taken over the WHOLE vocabulary, once per evaluation pass.  TW = [E ; P] Wall^T is
# a constant while no parameter changes, so a batch's forward is one launch that gathers TW rows
# by token id: no mark, scan, table copy, GEMM or read-back per batch.
VOCAB_SWITCH = "HSG_SENT_CNN_VOCAB"
VOCAB_BUDGET = "HSG_SENT_CNN_VOCAB_MB"        # the largest table built, MiB; 1024 covers vocab_size = 50000


def sent_cnn_vocab_on():
    """The value of the ``HSG_SENT_CNN_VOCAB`` switch as a bool ("0" or "1"); anything else raises."""
    v = _lib.path_option(VOCAB_SWITCH, "0")
    if v not in ("0", "1"):
        raise ValueError(f"{VOCAB_SWITCH}={v!r}: one of 0, 1")
    return v == "1"


def vocab_table_bytes(V, Pn):
    return (V + Pn) * LDY * 4


def vocab_path_ok(ids, embed_weight, pos_weight, conv_weights, conv_biases) -> bool:
    """The vocabulary path covers this call: :func:`token_path_ok`'s conditions on device, dtype,
    contiguity, shape and HSG_CHECK_NAN, without the frozen-table one; no gradient will be recorded
    (grad mode off, or no parameter of the encoder requires grad); and the table over the whole
    vocabulary fits ``HSG_SENT_CNN_VOCAB_MB`` (a path option, default 1024)."""
    from .module.GATLayer import CHECK_NAN
    conv_weights, conv_biases = list(conv_weights), list(conv_biases)
    floats = [embed_weight, pos_weight] + conv_weights + conv_biases
    if CHECK_NAN or len(conv_weights) != len(HEIGHTS) or len(conv_biases) != len(HEIGHTS):
        return False
    if not ids.is_cuda or ids.dim() != 2 or any(not t.is_cuda or t.dtype != torch.float32 for t in floats):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in floats):
        return False
    if embed_weight.dim() != 2 or pos_weight.dim() != 2 or not embed_weight.is_contiguous() \
            or not pos_weight.is_contiguous():
        return False
    L, (V, D) = ids.shape[1], embed_weight.shape
    if pos_weight.shape[1] != D or D % 4 or D < 4 or V < 1 or L > pos_weight.shape[0] - 1:
        return False
    for h, w, b in zip(HEIGHTS, conv_weights, conv_biases):
        if tuple(w.shape) != (CHANNELS, 1, h, D) or tuple(b.shape) != (CHANNELS,):
            return False
    budget = float(_lib.path_option(VOCAB_BUDGET, "1024")) * (1 << 20)
    if vocab_table_bytes(V, pos_weight.shape[0]) > budget:
        return False
    return bool(load().hsg_cnn_vocab_supported(L))


class VocabTable:
    """``TW [V + Pn, LDY]``: rows 0..V-1 = E Wall^T, rows V + p = P[p] Wall^T (two GEMMs), built on
    first use and rebuilt when its key changes.  The key holds numbers only -- ``data_ptr()``,
    ``_version``, shape and device of the embedding, the position table and the six conv weights,
    and the GEMM mode -- so the table keeps no parameter alive.  A write that moves no version
    counter (``.data``, a foreign kernel) is not seen: :meth:`drop` (``sentEncoder.train()`` /
    ``.eval()`` call it)."""

    def __init__(self):
        self.drop()

    def drop(self):
        self.key = self.TW = None
        self.V = 0
        self.builds = getattr(self, "builds", 0)

    @staticmethod
    def key_of(embed_weight, pos_weight, conv_weights):
        from .dense import get_gemm_dtype
        return tuple((t.data_ptr(), t._version, tuple(t.shape), str(t.device))
                     for t in [embed_weight, pos_weight] + list(conv_weights)) + (get_gemm_dtype(),)

    def nbytes(self):
        return 0 if self.TW is None else self.TW.numel() * 4

    def get(self, embed_weight, pos_weight, conv_weights):
        """This table, current for these parameters."""
        key = self.key_of(embed_weight, pos_weight, conv_weights)
        if key != self.key:
            self.drop()                               # the old table is freed before the new one is made
            with torch.no_grad():
                V, Pn = embed_weight.shape[0], pos_weight.shape[0]
                wall = stack_taps([w.detach().float() for w in conv_weights])
                TW = embed_weight.new_empty(V + Pn, LDY)
                gemm(embed_weight.detach(), wall, b_t=True, out=TW[:V, :NY])
                gemm(pos_weight.detach(), wall, b_t=True, out=TW[V:, :NY])
            self.key, self.TW, self.V = key, TW, V
            self.builds += 1
        return self


def sent_cnn_vocab(ids, table, conv_biases, layout=None):
    """:func:`sent_cnn`'s forward on a current :class:`VocabTable` (the caller has asked
    :func:`vocab_path_ok`): one ``hsg_cnn_vocab_pool`` launch -> [n, 300], no autograd node.  The
    row layout is path "0"'s: computed from ``ids`` (one read-back, with the range check of the
    ids), or the resident ``layout`` with its host-side range check."""
    if table.TW is None:
        raise RuntimeError("sent_cnn_vocab: the table is not built (VocabTable.get)")
    n, L = ids.shape
    TW, V = table.TW, table.V
    if n == 0:
        return TW.new_zeros(0, len(HEIGHTS) * CHANNELS)
    ids = ids.long().contiguous()
    if layout is None:
        _, rowoff, _, _, _, _ = _layout_tokens(ids, V, False)
    else:
        _, rowoff, _ = layout.check(ids, V)
    feat = TW.new_empty(n, len(HEIGHTS) * CHANNELS)
    arg = torch.empty(n, len(HEIGHTS) * CHANNELS, dtype=torch.int32, device=TW.device)
    bias = [b.detach().contiguous() for b in conv_biases]
    bptr = (ctypes.c_void_p * len(bias))(*[b.data_ptr() for b in bias])
    check(load().hsg_cnn_vocab_pool(n, L, V, ptr(ids), ptr(rowoff), ptr(TW), TW.stride(0), bptr, ptr(feat), ptr(arg),
                                    stream_of(TW)), "hsg_cnn_vocab_pool")
    return feat


class _SentCNNRows(torch.autograd.Function):
    """:class:`_SentCNN` behind its gather: the row matrix X is a differentiable input."""

    @staticmethod
    def forward(ctx, X, rowoff, n, L, wall, *bias):
        feat, arg = _conv_pool(X, n, L, rowoff, wall, bias)
        ctx.save_for_backward(X, wall, rowoff, feat, arg)
        ctx.n = n
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        X, wall, rowoff, feat, arg = ctx.saved_tensors
        n, D = ctx.n, X.shape[1]
        dfeat = dfeat.contiguous()
        dY = _pool_bwd(X, n, rowoff, feat, arg, dfeat)
        dX = dwall = None
        if ctx.needs_input_grad[4]:
            dwall = gemm(dY[:, :NY], X, a_t=True, splits=splits_for(NY, D, X.shape[0]))
        if ctx.needs_input_grad[0]:
            dX = gemm(dY[:, :NY], wall)                                      # [rows, D]
        return (dX, None, None, None, dwall, *_dbias(dfeat, feat, ctx.needs_input_grad[5:]))


def sent_cnn_rows(X, layout, shape, conv_weights, conv_biases):
    """:func:`sent_cnn` from the gathered rows on: ``X [rows, D]`` and ``layout`` as
    :func:`hetersumgraph_amd.wordembed.embed_batch` returns them for ``ids`` of
    ``shape = (n, L)``.  X is a differentiable input (its gradient is ``dY Wall``, computed
    only when X requires it); the embedding gradient belongs to the node that made X."""
    n, L = shape
    _, rowoff, rows = layout
    if L < max(HEIGHTS):
        raise ValueError(f"sentEncoder: sentence length {L} < the widest kernel {max(HEIGHTS)}")
    if X.shape[0] != rows or X.shape[1] % 4 or not X.is_contiguous():
        raise ValueError("sentEncoder: X must be the contiguous [rows, D] row matrix of the layout, D a multiple of 4")
    if n == 0:
        return X.new_zeros(0, len(HEIGHTS) * CHANNELS)
    wall = stack_taps([w.float() for w in conv_weights])
    return _SentCNNRows.apply(X, rowoff, n, L, wall, *[b.contiguous() for b in conv_biases])
