"""The order contract of include/hsg_embed.h restated in numpy, for the embedding tests.

An occurrence is (token v, source row s): the word rows are sources [0, n_w), CNN row r is
source n_w + r.  The kept occurrences, sorted by (v, s), form the list; P = the library's
``hsg_embed_piece_rows()`` cuts it into aligned chunks [kP, (k+1)P); the pieces of a token
are the intersections of its run with the chunks; a piece is summed in ascending position
starting from its first element, the piece sums are added in ascending order.  All in fp32.

Also the fp64 sum of the same occurrences and the derived bound: a sequential fp32 sum of
n terms differs from the exact sum by at most n * 2^-24 * sum|terms| (each of the n - 1
additions rounds a partial sum no larger than sum|terms| by at most 2^-24 relative), and
any bracketing of the same terms -- pieces first, then the piece sums -- obeys the same
bound.  So no measured tolerance is needed.
"""
import numpy as np

U = 2.0 ** -24


def cnn_tokens(ids):
    """Token of every row of hsg_cnn_gather's layout for ids [n, L] (PAD = 0, trailing):
    each sentence's real tokens, then 0 for its pad row."""
    out = []
    for row in np.asarray(ids):
        ln = int((row != 0).sum())
        out.extend(int(t) for t in row[:ln])
        out.append(0)
    return np.asarray(out, np.int64)


def sorted_occurrences(tok, padding_idx):
    """tok [n_src]: the token of every source.  -> (token, source) of the kept occurrences,
    sorted by (token, source)."""
    tok = np.asarray(tok, np.int64)
    src = np.arange(len(tok), dtype=np.int64)
    if padding_idx is not None:
        keep = tok != padding_idx
        tok, src = tok[keep], src[keep]
    order = np.lexsort((src, tok))
    return tok[order], src[order]


def keys_unsorted(tok, padding_idx):
    """The int64 key of every source, in source order: v << 32 | s, INT64_MAX for a dropped one."""
    tok = np.asarray(tok, np.int64)
    key = (tok << 32) | np.arange(len(tok), dtype=np.int64)
    if padding_idx is not None:
        key = np.where(tok == padding_idx, np.iinfo(np.int64).max, key)
    return key


def keys_of(tok, padding_idx):
    """The keys the reduce takes: keys_unsorted, sorted."""
    return np.sort(keys_unsorted(tok, padding_idx))


def runs(tok_sorted):
    """[(v, a, b)]: token v occupies list positions [a, b)."""
    out, a = [], 0
    n = len(tok_sorted)
    while a < n:
        b = a
        while b < n and tok_sorted[b] == tok_sorted[a]:
            b += 1
        out.append((int(tok_sorted[a]), a, b))
        a = b
    return out


def pieces(a, b, P):
    """The intersections of the run [a, b) with the aligned chunks [kP, (k+1)P)."""
    out = []
    while a < b:
        e = min(b, (a // P + 1) * P)
        out.append((a, e))
        a = e
    return out


def reduce_f32(tok, rows, V, P, padding_idx):
    """dE [V, D] fp32 in the contract's order.  rows [n_src, D] fp32: all sources stacked."""
    rows = np.asarray(rows, np.float32)
    dE = np.zeros((V, rows.shape[1]), np.float32)
    ts, ss = sorted_occurrences(tok, padding_idx)
    for v, a, b in runs(ts):
        total = None
        for lo, hi in pieces(a, b, P):
            acc = rows[ss[lo]].copy()
            for i in range(lo + 1, hi):
                acc = (acc + rows[ss[i]]).astype(np.float32)
            total = acc if total is None else (total + acc).astype(np.float32)
        dE[v] = total
    return dE


def reduce_f64(tok, rows, V, padding_idx):
    """(fp64 sum [V, D], derived bound [V, D]) of the same occurrences."""
    rows = np.asarray(rows, np.float64)
    ts, ss = sorted_occurrences(tok, padding_idx)
    ref = np.zeros((V, rows.shape[1]))
    mag = np.zeros((V, rows.shape[1]))
    np.add.at(ref, ts, rows[ss])
    np.add.at(mag, ts, np.abs(rows[ss]))
    n_v = np.bincount(ts, minlength=V).astype(np.float64)
    return ref, n_v[:, None] * U * mag


def run_lengths_case(P, V, lengths, n_w_share=0.5, seed=0):
    """Tokens of the sources (word rows first, then CNN rows) such that token v has
    lengths[v] occurrences (v < len(lengths) <= V): about n_w_share of a token's occurrences
    are word rows.  Returns (tok_w, tok_c)."""
    rng = np.random.default_rng(seed)
    tw, tc = [], []
    for v, n in enumerate(lengths):
        k = int(round(n * n_w_share))
        tw += [v] * k
        tc += [v] * (n - k)
    tw, tc = np.asarray(tw, np.int64), np.asarray(tc, np.int64)
    return rng.permutation(tw), rng.permutation(tc)


# ---- the shared kernel cases (tests/test_gpu_embed.py, tests/test_gpu_embed_guard.py) ------
V_CASE = 37
ONLY_W, ONLY_C, ALIGNED, HEAVY = 9, 10, 8, 7


def grad_case(P, kind, D, padding_idx=0, seed=0):
    """dict(tok_w, tok_c, dW, dX): the tokens of the word rows and of the CNN rows, and the
    two source matrices.  Kinds:

    "mixed": runs of length 0, 1, P-1, P, P+1, 3P+1; token ALIGNED covers exactly two whole
      chunks of the kept list (it starts and ends on a chunk boundary, for the given
      padding_idx); ONLY_W occurs among the word rows only, ONLY_C among the CNN rows only,
      the others in both; V-1 is the last run; token 0 occurs 3 times.
    "heavy": about 5,000 occurrences of token HEAVY beside two short runs.
    "no_words" / "no_rows": "mixed" with every source on one side; "empty": no source."""
    V = V_CASE
    rng = np.random.default_rng(seed)
    if kind == "heavy":
        lengths = {3: 2, HEAVY: 5003, 20: 5}
    elif kind == "empty":
        lengths = {}
    else:
        lengths = {0: 3, 2: 1, 3: P - 1, 4: P, 5: P + 1, 6: 3 * P + 1}
        pos = sum(n for v, n in lengths.items() if v != padding_idx)
        lengths[7] = (-pos) % P or P                     # filler up to the next chunk boundary
        lengths.update({ALIGNED: 2 * P, ONLY_W: 3, ONLY_C: 3, V - 1: P + 2})
    tw, tc = [], []
    for v, n in lengths.items():
        if kind in ("no_rows", "no_words"):
            k = n if kind == "no_rows" else 0
        else:
            k = n if v == ONLY_W else 0 if v == ONLY_C else (n + 1) // 2
        tw += [v] * k
        tc += [v] * (n - k)
    tok_w = rng.permutation(np.asarray(tw, np.int64))
    tok_c = rng.permutation(np.asarray(tc, np.int64))
    return dict(tok_w=tok_w, tok_c=tok_c, dW=rng.standard_normal((len(tok_w), D)).astype(np.float32),
                dX=rng.standard_normal((len(tok_c), D)).astype(np.float32))


def case_reference(c, P, padding_idx):
    """(fp32 in the contract's order, fp64 sum, derived bound) of a grad_case."""
    tok = np.concatenate([c["tok_w"], c["tok_c"]])
    rows = np.concatenate([c["dW"], c["dX"]])
    ref, bound = reduce_f64(tok, rows, V_CASE, padding_idx)
    return reduce_f32(tok, rows, V_CASE, P, padding_idx), ref, bound
