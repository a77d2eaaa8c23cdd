"""Guarded buffers for the C ABI tests (tests/test_gpu_guard_bands.py).

``guarded`` allocates one flat tensor

    [front guard | rows x pitch | back guard]

filled -- guards, payload and the ``pitch - cols`` pad columns alike -- with a bit
pattern arithmetic cannot produce: a NaN with a non-canonical payload for the floating
types (the hardware's own NaN is the canonical 0x7FC00000 / 0x7FC0), a fixed odd word
for the integer types.  After the call under test the handle tells, bit for bit through
an integer view, whether anything outside the documented extent was written, whether the
pad columns are untouched (or zero where the header promises zero), and whether every
documented element was written at all.

``poisoned_input`` builds an input operand the same way with a second NaN pattern, so a
NaN that leaked from an operand's slack can be told from an element that was never
written.

Each guard is a multiple of 64 elements and at least 4096 bytes, so the payload base
keeps the 256-byte alignment of the allocation.  Works on CPU tensors too
(tests/test_guard_helper.py).
"""
import torch

GUARD_BYTES = 4096

# dtype -> (integer view dtype, output pattern, input-poison pattern)
_PATTERNS = {
    torch.float32: (torch.int32, 0x7FC5A5A5, 0x7FD3C3C3),
    torch.bfloat16: (torch.int16, 0x7FC5, 0x7FD3),
    torch.int32: (torch.int32, 0x5A5A5A5B, None),
    torch.uint8: (torch.uint8, 0xA5, None),
    torch.int64: (torch.int64, 0x5A5A5A5B5A5A5A5B, None),
}
if hasattr(torch, "uint32"):
    _PATTERNS[torch.uint32] = (torch.int32, 0x5A5A5A5B, None)


def guard_elems(dtype):
    item = torch.empty(0, dtype=dtype).element_size()
    return (GUARD_BYTES // item + 63) // 64 * 64


def _bits(t):
    return t.view(_PATTERNS[t.dtype][0])


def _filled(n, dtype, device, pattern):
    idt = _PATTERNS[dtype][0]
    return torch.full((n,), pattern, dtype=idt, device=device).view(dtype)


class Guarded:
    def __init__(self, rows, cols, dtype, pitch, device):
        self.rows, self.cols, self.pitch, self.dtype = rows, cols, pitch, dtype
        self.pattern = _PATTERNS[dtype][1]
        self.g = guard_elems(dtype)
        self.n = rows * pitch
        self.flat = _filled(self.g + self.n + self.g, dtype, device, self.pattern)
        self.full = self.flat[self.g:self.g + self.n].view(rows, pitch)
        self.view = self.full[:, :cols]

    # --- integer views ---------------------------------------------------------
    def _front(self):
        return _bits(self.flat[:self.g])

    def _back(self):
        return _bits(self.flat[self.g + self.n:])

    def _pad(self):
        return _bits(self.full)[:, self.cols:]

    def _payload(self):
        return _bits(self.full)[:, :self.cols]

    # --- assertions ------------------------------------------------------------
    def assert_guards_intact(self, what=""):
        for name, gd in (("front", self._front()), ("back", self._back())):
            bad = (gd != self.pattern).nonzero()
            assert bad.numel() == 0, (f"{what}: {name} guard overwritten at {bad.numel()} elements, first at "
                                      f"offset {int(bad[0])} of {self.g}")

    def assert_pad(self, want="untouched", what="", zero_cols=None):
        """Pad columns still the pattern, or all exactly zero; zero_cols = k with "zero":
        only the first k pad columns are promised zero, the rest must be untouched."""
        assert want in ("untouched", "zero"), want
        pad = self._pad()
        expect = torch.full_like(pad, self.pattern if want == "untouched" else 0)
        if want == "zero" and zero_cols is not None:
            expect[:, zero_cols:] = self.pattern
        bad = (pad != expect).nonzero()
        assert bad.numel() == 0, (f"{what}: pad columns {self.cols}..{self.pitch - 1} not {want} at {bad.shape[0]} "
                                  f"elements, first (row, pad column) {bad[0].tolist()}")

    def assert_fully_written(self, mask=None, what=""):
        """No payload element still holds the pattern; mask (bool [rows, cols]) selects
        the elements the header says are written."""
        left = self._payload() == self.pattern
        if mask is not None:
            left = left & mask.to(left.device).view(self.rows, self.cols)
        bad = left.nonzero()
        assert bad.numel() == 0, (f"{what}: {bad.shape[0]} of {self.rows * self.cols} documented elements never "
                                  f"written, first (row, column) {bad[0].tolist()}")

    def assert_finite(self, mask=None, what=""):
        if not self.dtype.is_floating_point:
            return
        bad = ~torch.isfinite(self.view.float())
        if mask is not None:
            bad = bad & mask.to(bad.device).view(self.rows, self.cols)
        bad = bad.nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} NaN / Inf elements, first (row, column) {bad[0].tolist()}"

    def payload(self):
        return self.view.clone().contiguous()


def guarded(rows, cols, dtype=torch.float32, pitch=None, device="cpu"):
    """(payload view [rows, cols] of pitch `pitch`, handle)."""
    pitch = cols if pitch is None else pitch
    assert pitch >= cols >= 0 and rows >= 0
    h = Guarded(rows, cols, dtype, pitch, device)
    return h.view, h


def poisoned_input(t, rows=None, cols=None, pitch=None, zero_cols=0):
    """t's values in [:rows, :cols] of a [rows, pitch] operand whose pad columns, and
    guards before and after, hold the input NaN pattern (the first `zero_cols` pad
    columns zero instead: the bf16-A contract).  Returns the [rows, cols] view."""
    t2 = t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(1, -1)
    rows = t2.shape[0] if rows is None else rows
    cols = t2.shape[1] if cols is None else cols
    pitch = cols if pitch is None else pitch
    assert t.dtype.is_floating_point and pitch >= cols + zero_cols and (rows, cols) == tuple(t2.shape)
    g = guard_elems(t.dtype)
    flat = _filled(g + rows * pitch + g, t.dtype, t.device, _PATTERNS[t.dtype][2])
    full = flat[g:g + rows * pitch].view(rows, pitch)
    full[:, :cols] = t2
    full[:, cols:cols + zero_cols] = 0
    return full[:, :cols]
