"""The numpy restatement of the embedding gradient's order contract (tests/embed_ref.py)
against torch.index_add_ in fp64, and the contract's structural properties.  No GPU."""
import numpy as np
import pytest
import torch

import embed_ref as R

V, D = 37, 8


def _case(P, padding_idx_tokens=True, seed=3):
    lengths = [5 if padding_idx_tokens else 0, 0, 1, P - 1, P, P + 1, 3 * P + 1, 2, 0, 7]
    tw, tc = R.run_lengths_case(P, V, lengths, seed=seed)
    tok = np.concatenate([tw, tc, [V - 1, V - 1]])
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((len(tok), D)).astype(np.float32)
    return tok, rows


@pytest.mark.parametrize("P", [2, 5, 32])
@pytest.mark.parametrize("padding_idx", [0, None])
def test_restatement_against_index_add_fp64(P, padding_idx):
    tok, rows = _case(P)
    got = R.reduce_f32(tok, rows, V, P, padding_idx)
    ts, ss = R.sorted_occurrences(tok, padding_idx)
    want = torch.zeros(V, D, dtype=torch.float64).index_add_(0, torch.from_numpy(ts),
                                                             torch.from_numpy(rows.astype(np.float64))[ss])
    ref, bound = R.reduce_f64(tok, rows, V, padding_idx)
    assert np.array_equal(ref, want.numpy()) or np.allclose(ref, want.numpy(), rtol=0, atol=1e-13)
    err = np.abs(got.astype(np.float64) - want.numpy())
    assert (err <= bound).all(), float((err - bound).max())
    absent = np.setdiff1d(np.arange(V), ts)
    assert absent.size and not got[absent].any() and not np.signbit(got[absent]).any()


def test_dropping_padding_occurrences_equals_zeroing_the_row():
    P = 4
    tok, rows = _case(P)
    dropped = R.reduce_f32(tok, rows, V, P, 0)
    # the other tokens' list positions shift by the dropped count, so compare at the level the
    # contract promises: the row is +0.0 and every other row is the sum of the same terms
    kept = R.reduce_f32(tok, rows, V, P, None)
    assert kept[0].any()
    assert not dropped[0].any() and not np.signbit(dropped[0]).any()
    ref, bound = R.reduce_f64(tok, rows, V, None)
    ref[0], bound[0] = 0, 0
    assert (np.abs(dropped.astype(np.float64) - ref) <= bound).all()
    # and exactly: dropping equals reducing the list from which those sources were removed
    keep = tok != 0
    again = R.reduce_f32(tok[keep], rows[keep], V, P, None)
    assert np.array_equal(dropped.view(np.int32), again.view(np.int32))
    # with a multiple of P dropped in front, every other run keeps its place inside its chunks:
    # then dropping IS zeroing the row afterwards, bit for bit
    tok8 = np.concatenate([[0] * 3, tok])
    rows8 = np.concatenate([rows[:3], rows])
    assert (tok8 == 0).sum() == 2 * P
    zeroed = R.reduce_f32(tok8, rows8, V, P, None)
    zeroed[0] = 0
    assert np.array_equal(R.reduce_f32(tok8, rows8, V, P, 0).view(np.int32), zeroed.view(np.int32))


def test_pad_rows_land_on_row_zero_without_a_padding_index():
    ids = np.array([[5, 6, 7, 0, 0, 0, 0], [9, 0, 0, 0, 0, 0, 0], [3, 3, 4, 5, 6, 7, 8]])
    tok_c = R.cnn_tokens(ids)
    assert tok_c.tolist() == [5, 6, 7, 0, 9, 0, 3, 3, 4, 5, 6, 7, 8, 0]
    rows = np.random.default_rng(0).standard_normal((len(tok_c), D)).astype(np.float32)
    got = R.reduce_f32(tok_c, rows, V, 4, None)
    want = ((rows[3] + rows[5]).astype(np.float32) + rows[13]).astype(np.float32)
    assert np.array_equal(got[0], want)
    assert not R.reduce_f32(tok_c, rows, V, 4, 0)[0].any()


def test_pieces_depend_only_on_list_position():
    P = 4
    assert R.pieces(0, 0, P) == []
    assert R.pieces(3, 4, P) == [(3, 4)]
    assert R.pieces(4, 8, P) == [(4, 8)]                       # starts and ends on a boundary
    assert R.pieces(2, 13, P) == [(2, 4), (4, 8), (8, 12), (12, 13)]
    assert R.pieces(4, 12, P) == [(4, 8), (8, 12)]             # two whole chunks
    # the same run of the same rows at the same positions gives the same bits whatever
    # tokens surround it ...
    rng = np.random.default_rng(1)
    run = rng.standard_normal((9, D)).astype(np.float32)
    before = rng.standard_normal((6, D)).astype(np.float32)
    a = R.reduce_f32(np.array([1] * 6 + [5] * 9 + [8] * 3), np.concatenate([before, run, run[:3]]), V, P, None)
    b = R.reduce_f32(np.array([1, 2, 2, 3, 3, 4] + [5] * 9), np.concatenate([before, run]), V, P, None)
    assert np.array_equal(a[5].view(np.int32), b[5].view(np.int32))
    # ... while one position further right the same nine rows group differently
    assert R.pieces(5, 14, P) == [(5, 8), (8, 12), (12, 14)] and R.pieces(6, 15, P) == [(6, 8), (8, 12), (12, 15)]


def test_keys_sort_as_the_occurrence_list():
    tok, _ = _case(5)
    for pad in (0, None):
        ts, ss = R.sorted_occurrences(tok, pad)
        keys = R.keys_of(tok, pad)
        kept = keys[keys != np.iinfo(np.int64).max]
        assert np.array_equal(kept >> 32, ts) and np.array_equal(kept & 0xFFFFFFFF, ss)
        assert (keys[len(kept):] == np.iinfo(np.int64).max).all()
