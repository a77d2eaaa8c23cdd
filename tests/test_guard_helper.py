"""tests/guard.py on CPU tensors: every assertion passes on an untouched (or properly
written) buffer and fails after one element is written where it must not be -- or, for
assert_fully_written, after one element is left unwritten."""
import pytest
import torch

from guard import GUARD_BYTES, guard_elems, guarded, poisoned_input

DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.uint8, torch.int64]


def _one(dtype):
    return torch.ones((), dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout(dtype):
    view, h = guarded(5, 13, dtype, pitch=16)
    g = guard_elems(dtype)
    assert g % 64 == 0 and g * view.element_size() >= GUARD_BYTES
    assert (g * view.element_size()) % 256 == 0           # the payload keeps the allocation's alignment
    assert view.shape == (5, 13) and view.stride() == (16, 1)
    assert view.data_ptr() == h.flat.data_ptr() + g * view.element_size()
    assert h.flat.numel() == 2 * g + 5 * 16
    if dtype.is_floating_point:
        assert bool(torch.isnan(h.flat.float()).all())    # payload, pad and guards alike


@pytest.mark.parametrize("dtype", DTYPES)
def test_untouched_buffer_passes_guards_and_pad(dtype):
    _, h = guarded(5, 13, dtype, pitch=16)
    h.assert_guards_intact()
    h.assert_pad("untouched")
    with pytest.raises(AssertionError):
        h.assert_pad("zero")
    with pytest.raises(AssertionError):
        h.assert_fully_written()                            # nothing was written yet


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["front_last", "front_first", "back_first", "back_last"])
def test_one_guard_element_fails(dtype, where):
    view, h = guarded(3, 8, dtype, pitch=8)
    view.fill_(1)
    h.assert_guards_intact()
    g = h.g
    idx = {"front_last": g - 1, "front_first": 0, "back_first": g + 3 * 8, "back_last": h.flat.numel() - 1}[where]
    h.flat[idx] = _one(dtype)
    with pytest.raises(AssertionError, match="guard overwritten"):
        h.assert_guards_intact()
    h.assert_pad("untouched")                               # no pad columns: vacuous
    h.assert_fully_written()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_pad_element_fails(dtype):
    view, h = guarded(4, 13, dtype, pitch=16)
    view.fill_(1)
    h.assert_pad("untouched")
    h.full[2, 14] = _one(dtype)
    with pytest.raises(AssertionError, match="pad columns"):
        h.assert_pad("untouched")
    h.assert_guards_intact()
    # the zero promise: all pad zero passes, one element off fails
    h.full[:, 13:] = 0
    h.assert_pad("zero")
    h.full[3, 15] = _one(dtype)
    with pytest.raises(AssertionError, match="pad columns"):
        h.assert_pad("zero")
    _, h2 = guarded(4, 13, dtype, pitch=16)
    h2.full[:, 13:] = 0
    h2.full[0, 13] = h2.flat[0]                             # one pad element left at the pattern
    with pytest.raises(AssertionError):
        h2.assert_pad("zero")


def test_pad_zero_up_to_a_column():
    """zero_cols: the first pad columns promised zero, the rest untouched (bf16 rows whose
    header zeroes columns d .. ceil8(d) - 1 of a wider pitch)."""
    view, h = guarded(3, 12, torch.bfloat16, pitch=24)
    view.fill_(1)
    h.full[:, 12:16] = 0
    h.assert_pad("zero", zero_cols=4)
    with pytest.raises(AssertionError):
        h.assert_pad("zero")                                # columns 16 .. 23 are not zero
    h.full[1, 16] = 0                                       # one element written past the promised zeros
    with pytest.raises(AssertionError, match="pad columns"):
        h.assert_pad("zero", zero_cols=4)
    h.full[1, 16] = h.flat[0]
    h.full[2, 15] = 1                                       # one promised zero missing
    with pytest.raises(AssertionError, match="pad columns"):
        h.assert_pad("zero", zero_cols=4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_unwritten_payload_element_fails(dtype):
    view, h = guarded(4, 13, dtype, pitch=16)
    keep = h.flat[0].clone()
    view.fill_(1)
    h.assert_fully_written()
    h.full[1, 12] = keep                                    # one element still the pattern
    with pytest.raises(AssertionError, match="never written"):
        h.assert_fully_written()
    mask = torch.ones(4, 13, dtype=torch.bool)
    mask[1, 12] = False                                     # ... unless the header says it is conditional
    h.assert_fully_written(mask)
    mask[1, 12] = True
    with pytest.raises(AssertionError):
        h.assert_fully_written(mask)


def test_finite_check():
    view, h = guarded(2, 5, torch.float32, pitch=8)
    view.fill_(2.0)
    h.assert_finite()
    view[1, 3] = float("inf")
    with pytest.raises(AssertionError, match="NaN / Inf"):
        h.assert_finite()
    view[1, 3] = 0.0
    h.assert_finite()
    view[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        h.assert_finite()


def test_written_nan_is_not_the_pattern():
    """The canonical NaN arithmetic produces is a written value, not the pattern."""
    view, h = guarded(1, 4, torch.float32)
    view.copy_(torch.tensor([[0.0, 1.0, 2.0, 3.0]]) * float("nan"))
    h.assert_fully_written()
    view16, h16 = guarded(1, 4, torch.bfloat16)
    view16.copy_((torch.zeros(1, 4) * float("nan")).bfloat16())
    h16.assert_fully_written()


def test_empty_extents():
    for rows, cols in ((0, 7), (3, 0)):
        view, h = guarded(rows, cols, torch.float32, pitch=8)
        assert view.numel() == 0
        h.assert_guards_intact()
        h.assert_fully_written()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_poisoned_input(dtype):
    t = torch.arange(15, dtype=torch.float32).view(3, 5).to(dtype)
    v = poisoned_input(t, 3, 5, 8)
    assert v.shape == (3, 5) and v.stride() == (8, 1) and torch.equal(v, t)
    base = v.as_strided((3, 8), (8, 1))
    assert bool(torch.isnan(base[:, 5:].float()).all())
    g = guard_elems(dtype)
    before = v.as_strided((g,), (1,), v.storage_offset() - g)
    after = v.as_strided((g,), (1,), v.storage_offset() + 3 * 8)
    assert bool(torch.isnan(before.float()).all()) and bool(torch.isnan(after.float()).all())
    # the poison differs from the output pattern: a leaked operand NaN is not "unwritten"
    _, h = guarded(1, 1, dtype)
    assert int(before.view(h._front().dtype)[0]) != h.pattern
    # the bf16-A contract: zero pad up to ceil8, poison after it
    z = poisoned_input(t, 3, 5, 16, zero_cols=3).as_strided((3, 16), (16, 1))
    assert not z[:, 5:8].float().any() and bool(torch.isnan(z[:, 8:].float()).all())
