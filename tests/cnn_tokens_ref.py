"""Numpy restatements of include/hsg_cnn_tokens.h, written from the header: the slot map of a
batch's distinct tokens, the pool's value contract given a TW, and the order contract of the
sparse weight gradient (float32, multiply and add rounded separately, so every line below is
bit for bit what the kernels must give), plus the fp64 algebra the two paths rest on.  No GPU,
no import of the package."""
import numpy as np

HEIGHTS = tuple(range(2, 8))
CH = 50
NY = sum(HEIGHTS) * CH          # 1350
NF = len(HEIGHTS) * CH          # 300


def tap(h, i):
    return (h - 2) * (h + 1) // 2 + i


def lengths(ids):
    return (np.asarray(ids) != 0).sum(1)


def slot_map(ids, V):
    """(present int32 [V], slot int32 [V], U): PAD always present, slots ascending with the id."""
    present = np.zeros(V, np.int32)
    present[0] = 1
    present[np.asarray(ids).reshape(-1)] = 1
    slot = (np.cumsum(present, dtype=np.int64) - 1).astype(np.int32)
    return present, slot, int(slot[-1]) + 1


def token_pos(ids, s, r):
    """(token, position) of row r of sentence s: the r < len_s rule of the header."""
    ln = int((ids[s] != 0).sum())
    return (int(ids[s, r]), r + 1) if 0 <= r < ln else (0, 0)


def stack_taps(conv_w):
    """Conv2d weights [50, 1, h, D] -> Wall [1350, D], row tap(h, i) * 50 + c."""
    return np.concatenate([np.asarray(w)[:, 0].transpose(1, 0, 2).reshape(h * CH, -1)
                           for h, w in zip(HEIGHTS, conv_w)], 0)


def unstack_taps(wall):
    """The inverse of stack_taps: six [50, 1, h, D]."""
    out, base = [], 0
    for h in HEIGHTS:
        out.append(wall[base * CH:(base + h) * CH].reshape(h, CH, -1).transpose(1, 0, 2)[:, None])
        base += h
    return out


def table(ids, V, E, P):
    """Tb [U + L + 1, D]: the present embedding rows in slot order, then the position rows."""
    present, _, U = slot_map(ids, V)
    L = ids.shape[1]
    return np.concatenate([E[present != 0], P[:L + 1]], 0), U


def pool(ids, slot, U, TW, biases, dtype=np.float32):
    """feat [n, 300], arg int32 [n, 300] from TW by the header's value contract:
    v = b; v = v + (TW[slot row][q] + TW[U + pos][q]) for i ascending; first maximum by strict >
    over t = 0 .. min(len, T) - 1, then the pad window at t = len when len < T."""
    ids = np.asarray(ids)
    n, L = ids.shape
    TW = np.asarray(TW, dtype)
    feat = np.zeros((n, NF), dtype)
    arg = np.zeros((n, NF), np.int32)
    ln = lengths(ids)
    for s in range(n):
        m = int(ln[s])
        rw = np.concatenate([slot[ids[s, :m]], np.full(L + 8 - m, slot[0])]).astype(np.int64)
        ps = np.concatenate([U + 1 + np.arange(m), np.full(L + 8 - m, U)]).astype(np.int64)
        for g, h in enumerate(HEIGHTS):
            T = L - h + 1
            nt = min(m, T) + (1 if m < T else 0)          # scanned windows; the last is t = len when len < T
            v = np.broadcast_to(np.asarray(biases[g], dtype), (nt, CH)).copy()
            for i in range(h):
                c0 = tap(h, i) * CH
                v = v + (TW[rw[i:i + nt], c0:c0 + CH] + TW[ps[i:i + nt], c0:c0 + CH])
            bt = np.argmax(v, 0)                          # the first maximum
            best = v[bt, np.arange(CH)]
            feat[s, g * CH:(g + 1) * CH] = np.maximum(best, dtype(0))
            arg[s, g * CH:(g + 1) * CH] = bt
    return feat, arg


def x_rows(ids, s, E, P, dtype=np.float32):
    """x(s, r) for r = 0 .. len_s (row len_s = the pad row), one add per element."""
    m = int((ids[s] != 0).sum())
    tok = np.concatenate([ids[s, :m], [0]])
    pos = np.concatenate([1 + np.arange(m), [0]])
    return np.asarray(E, dtype)[tok] + np.asarray(P, dtype)[pos]


def dw(ids, E, P, feat, arg, dfeat, chunk, dtype=np.float32):
    """(dWall [1350, D], dbias [300]) in the header's order: aligned chunks of `chunk` sentences,
    each partial from +0.0 adding acc = acc + g * x in ascending sentence order, partials added in
    ascending chunk order.  (g == 0 pairs add exact zeros here; the kernels skip them.)"""
    ids = np.asarray(ids)
    n = ids.shape[0]
    D = E.shape[1]
    g = np.where(np.asarray(feat) > 0, np.asarray(dfeat, dtype), dtype(0)).astype(dtype)
    total_w, total_b = np.zeros((NY, D), dtype), np.zeros(NF, dtype)
    for k, s0 in enumerate(range(0, n, chunk)):
        pw, pb = np.zeros((NY, D), dtype), np.zeros(NF, dtype)
        for s in range(s0, min(s0 + chunk, n)):
            x = x_rows(ids, s, E, P, dtype)
            m = x.shape[0] - 1
            pb = pb + g[s]
            for gi, h in enumerate(HEIGHTS):
                gs = g[s, gi * CH:(gi + 1) * CH]
                for i in range(h):
                    r = arg[s, gi * CH:(gi + 1) * CH].astype(np.int64) + i
                    r = np.where((r >= 0) & (r < m), r, m)
                    q0 = tap(h, i) * CH
                    pw[q0:q0 + CH] = pw[q0:q0 + CH] + gs[:, None] * x[r]
        total_w, total_b = (pw, pb) if k == 0 else (total_w + pw, total_b + pb)
    return total_w, total_b


# ---- inputs of the tests ---------------------------------------------------------------------
def small_ids(n, L, V, seed):
    """Trailing padding; lengths 0, 1, 6, L first, then U(2, L); a repeated token."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, L + 1, n)
    lens[:4] = [0, 1, 6, L][:min(n, 4)]
    ids = np.zeros((n, L), np.int64)
    for i, m in enumerate(lens):
        ids[i, :m] = rng.integers(1, V, m)
    if n > 4:
        ids[4, :lens[4]] = 7
    return ids


def params(V, D, L, seed):
    rng = np.random.default_rng(seed)
    E = 0.5 * rng.standard_normal((V, D))
    P = rng.standard_normal((L + 1, D))
    cw = [rng.standard_normal((50, 1, h, D)) / np.sqrt(h * D) for h in HEIGHTS]
    cb = [0.1 * rng.standard_normal(50) for _ in HEIGHTS]
    return E, P, cw, cb


# ---- the fp64 algebra ------------------------------------------------------------------------
def conv_tokens64(ids, V, E, P, conv_w, conv_b):
    """The encoder as the "tokens" path computes it, in fp64: TW = Tb Wall^T, then the pool."""
    E, P = np.asarray(E, np.float64), np.asarray(P, np.float64)
    Tb, U = table(ids, V, E, P)
    _, slot, _ = slot_map(ids, V)
    TW = Tb @ stack_taps([np.asarray(w, np.float64) for w in conv_w]).T
    return pool(ids, slot, U, TW, [np.asarray(b, np.float64) for b in conv_b], np.float64)


def dw_dense64(ids, E, P, feat, arg, dfeat):
    """dWall = dY^T X of the dense formulation (today's backward), fp64: dY holds the masked dfeat
    in the rows of each max window, X the sentences' rows plus one pad row each."""
    ids = np.asarray(ids)
    n = ids.shape[0]
    g = np.where(feat > 0, np.asarray(dfeat, np.float64), 0.0)
    X = [x_rows(ids, s, E, P, np.float64) for s in range(n)]
    dY = [np.zeros((x.shape[0], NY)) for x in X]
    for s in range(n):
        m = X[s].shape[0] - 1
        for gi, h in enumerate(HEIGHTS):
            for c in range(CH):
                for i in range(h):
                    r = int(arg[s, gi * CH + c]) + i
                    dY[s][r if r < m else m, tap(h, i) * CH + c] += g[s, gi * CH + c]
    return np.concatenate(dY, 0).T @ np.concatenate(X, 0), g.sum(0)
