"""hsg_doc_ce through hetersumgraph_amd.loss: the per-document cross entropy of
train.py:115-119 against the fp64 oracle (tests/train_ref.py).

Tolerance: forward values and dlogits within 2x the fp32 CPU run's own error against
fp64 (its maximum over the tensor), floored at 4 fp32 ulp of the value.  Measured on an
MI355X over all cases below, native (fp32 torch) maximum error -- N(0, 1) logits: row
loss 2.3e-7 (2.8e-7), document sums 7.9e-6 (1.2e-4: index_add sums a 257-row document
serially, the kernel through a tree), mean 1.8e-6 (3.7e-5), dlogits 7.3e-8 (8.0e-8);
logits of +-100, where a 257-row document sums to ~25,000: document sums 7.8e-4 (2.0e-2),
mean 3.5e-4 (1.7e-2), row loss and dlogits 1.9e-9 / 9.9e-9 (the same); exact ties: row
loss 1.9e-9 (the same), mean 4.6e-6 (2.8e-4).  Worst error / allowed over all: 0.66.
"""
import functools

import pytest
import torch

import train_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAYOUTS = {
    "b1": [35], "b1_long": [257],
    "b3_a": [0, 257, 1], "b3_b": [1, 2, 0], "b3_c": [257, 0, 2], "b3_d": [2, 35, 257], "b3_e": [35, 1, 35],
    "b32": ([0, 1, 2, 35, 257] * 7)[:31] + [0],
}
KINDS = ("normal", "pm100", "ties")
UP = 0.37                                    # a non-unit grad_output


@functools.lru_cache(maxsize=None)
def inputs(layout, kind):
    lens = LAYOUTS[layout]
    n = sum(lens)
    g = torch.Generator().manual_seed(sorted(LAYOUTS).index(layout) * 10 + KINDS.index(kind))
    if kind == "normal":
        z = torch.randn(n, 2, generator=g)
    elif kind == "pm100":
        z = (torch.randint(0, 2, (n, 2), generator=g) * 2 - 1) * 100.0
    else:
        z = torch.randn(n, 1, generator=g).expand(n, 2).contiguous()
    lab = torch.randint(0, 2, (n,), generator=g)
    refs = {dt: (train_ref.doc_ce(z, lab, lens, dt), train_ref.doc_ce(z, lab, lens, dt, UP)[3])
            for dt in (torch.float64, torch.float32)}
    return lens, z, lab, refs


def label_operands(lab, form):
    """(labels, rows) on the device in the direct or the (label matrix, node ids) form."""
    if form == "direct":
        return lab.to(DEV), None
    n, L = lab.numel(), 6
    rows = torch.arange(n) * 3 + 2                     # sentence nodes among other nodes, ascending
    mat = torch.zeros(3 * n + 5, L, dtype=torch.int64)
    mat[rows, torch.arange(n) % L] = lab
    return mat.to(DEV), rows.to(DEV)


def run(z, lab, lens, form, upstream=None):
    from hetersumgraph_amd import loss
    labels, rows = label_operands(lab, form)
    zd = z.to(DEV).requires_grad_()
    mean, doc, row = loss.doc_cross_entropy(zd, labels, train_ref.offsets(lens).to(DEV), rows)
    assert not doc.requires_grad and not row.requires_grad
    (g,) = torch.autograd.grad(mean, zd, None if upstream is None else torch.tensor(upstream, device=DEV))
    return row, doc, mean, g


@pytest.mark.parametrize("form", ["direct", "rows"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_parity_with_fp64(layout, kind, form):
    lens, z, lab, refs = inputs(layout, kind)
    (r64, d64, m64, g64), gu64 = refs[torch.float64]
    (r32, d32, m32, g32), gu32 = refs[torch.float32]
    row, doc, mean, g = run(z, lab, lens, form)
    what = f"{layout}-{kind}-{form}"
    train_ref.assert_within(row, r64, r32, what + " row_loss")
    train_ref.assert_within(doc, d64, d32, what + " doc_loss")
    train_ref.assert_within(mean, m64, m32, what + " mean")
    train_ref.assert_within(g, g64, g32, what + " dlogits")
    assert bool(torch.isfinite(row).all()) and bool(torch.isfinite(g).all())
    for i, L in enumerate(lens):
        if L == 0:
            assert float(doc[i]) == 0.0                # an empty document contributes exactly 0
    # backward through autograd with a non-unit grad_output
    gu = run(z, lab, lens, form, UP)[3]
    train_ref.assert_within(gu, gu64, gu32, what + f" dlogits x {UP}")
    assert torch.equal(gu, g * UP)


@pytest.mark.parametrize("layout,kind", [("b32", "normal"), ("b3_a", "pm100"), ("b1", "ties")])
def test_two_runs_are_bitwise_equal(layout, kind):
    lens, z, lab, _ = inputs(layout, kind)
    a, b = run(z, lab, lens, "rows"), run(z, lab, lens, "rows")
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for x, y in zip(a, run(z, lab, lens, "direct")):   # both label forms, the same numbers
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("bad", ["label2", "label-1", "row_high", "row_negative"])
def test_out_of_range_label(bad):
    """NaN loss for that row, its document and the mean; a finite, zero gradient row; every
    other row, document and gradient row bitwise what the clean run gives."""
    lens = [2, 35, 1]
    _, z, lab, _ = inputs("b3_d", "normal")
    n = sum(lens)
    z, lab = z[:n].contiguous(), lab[:n].clone()
    clean = run(z, lab, lens, "rows" if bad.startswith("row") else "direct")
    r = 2 + 17                                         # a row of document 1
    from hetersumgraph_amd import loss
    zd = z.to(DEV).requires_grad_()
    off = train_ref.offsets(lens).to(DEV)
    if bad.startswith("label"):
        lab2 = lab.clone()
        lab2[r] = 2 if bad == "label2" else -1
        mean, doc, row = loss.doc_cross_entropy(zd, lab2.to(DEV), off)
    else:
        labels, rows = label_operands(lab, "rows")
        rows = rows.clone()
        rows[r] = labels.shape[0] if bad == "row_high" else -1
        mean, doc, row = loss.doc_cross_entropy(zd, labels, off, rows)
    (g,) = torch.autograd.grad(mean, zd)
    torch.cuda.synchronize()
    assert torch.isnan(mean) and torch.isnan(doc[1]) and torch.isnan(row[r])
    keep = torch.arange(n, device=DEV) != r
    assert torch.equal(row[keep], clean[0][keep]) and torch.equal(doc[[0, 2]], clean[1][[0, 2]])
    assert torch.equal(g[r], torch.zeros(2, device=DEV))
    assert torch.equal(g[keep], clean[3][keep]) and bool(torch.isfinite(g).all())


def test_refusals():
    from hetersumgraph_amd import loss
    off = train_ref.offsets([2]).to(DEV)
    lab = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        loss.doc_mean_cross_entropy(torch.zeros(2, 3, device=DEV), lab, off)          # C != 2
    with pytest.raises(RuntimeError):
        loss.doc_mean_cross_entropy(torch.zeros(2, 2, device=DEV).double(), lab, off)
    with pytest.raises(RuntimeError):
        loss.doc_mean_cross_entropy(torch.zeros(2, 2), lab.cpu(), off.cpu())          # no CPU fallback
