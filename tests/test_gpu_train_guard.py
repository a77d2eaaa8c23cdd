"""Guard bands and poison around every buffer the training-tail entry points write
(include/hsg_train.h), with the machinery of tests/test_gpu_guard_bands.py: each case runs
once on ``guard.guarded`` outputs of EXACTLY the documented size with
``guard.poisoned_input`` inputs, once on plain tensors, and the shared body asserts the
bands intact, the inputs bitwise unchanged, every documented element written, no poison
consumed (nothing NaN that should not be), the two runs bitwise equal and the values
against the fp64 oracle (tests/train_ref.py).  The buffers a call updates in place --
hyper, and p, m and v of the Adam mode -- start from their initial values, not from the
guard pattern, so for them "written" is shown by the value check alone, not by the
pattern check.

CASES is this header's table (tests/test_train_abi.py checks that every writing entry
point has a case); the shapes are the smallest at which the kernels can go wrong: 1-, 3-
and chunk+1-element tensors (the scalar tail, and a second block that owns one element),
documents of 0, 1, 2 and 3 rows, an empty document first and last.
"""
import pytest
import torch

import train_ref
from test_gpu_guard_bands import P, call, run_case      # run_case builds each case's allocator `mk`
from train_ref import CHUNK

pytestmark = pytest.mark.gpu

CASES = {}                                   # entry point -> [(case id, fn, kwargs)]


def case(entry, *variants):
    def deco(fn):
        for kw in (variants or ({},)):
            cid = entry + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "")
            CASES.setdefault(entry, []).append((cid, fn, kw))
        return fn
    return deco


TOL = (1e-6, 1e-5)                           # atol, rtol: a value check; the parity tests hold the tight bound
LENS = [0, 1, 3, 0, 2, 0]


@case("hsg_doc_ce", dict(form="direct"), dict(form="rows"))
def c_doc_ce(lib, mk, form):
    n, B = sum(LENS), len(LENS)
    logits = torch.randn(n, 2)
    lab = torch.randint(0, 2, (n,))
    if form == "rows":
        N, L = 2 * n + 3, 5
        rows = torch.arange(n) * 2 + 1
        mat = torch.zeros(N, L, dtype=torch.int64)
        mat[rows, torch.randint(0, L, (n,))] = lab
        labels, rows_d = mk.ints(mat), mk.ints(rows)
    else:
        N, L, labels, rows_d = n, 1, mk.ints(lab), None
    row_loss, doc_loss = mk.out("row_loss", 1, n), mk.out("doc_loss", 1, B)
    mean, dlogits = mk.out("mean", 1, 1), mk.out("dlogits", 1, 2 * n)
    call(lib, "hsg_doc_ce", n, 2, B, P(mk.inp(logits.view(1, -1))), P(labels), L, N, P(rows_d),
         P(mk.ints(train_ref.offsets(LENS))), P(row_loss), P(doc_loss), P(mean), P(dlogits))
    r, d, m, g = train_ref.doc_ce(logits, lab, LENS, torch.float64)
    return {"row_loss": (r, *TOL), "doc_loss": (d, *TOL), "mean": (m.view(1, 1), *TOL), "dlogits": (g.view(1, -1), *TOL)}


MT_SIZES = [1, 3, CHUNK + 1]


def _table(entries):
    from hetersumgraph_amd._lib import HsgMtTensor
    return (HsgMtTensor * len(entries))(*[HsgMtTensor(*e) for e in entries])


def _hyper(mk, name, vals):
    """hyper: double [8], guarded through its int64 view (tests/guard.py has no fp64 pattern)."""
    init = torch.tensor([vals], dtype=torch.float64).view(torch.int64)
    return mk.out(name, 1, 8, torch.int64, init=init)


@case("hsg_mt_sqnorm")
def c_mt_sqnorm(lib, mk):
    gs = [torch.randn(n) for n in MT_SIZES]
    tab = _table([(None, P(mk.inp(g)), None, None, g.numel()) for g in gs])
    nb = lib.hsg_mt_blocks(tab, len(gs))
    assert nb == sum(-(-n // CHUNK) for n in MT_SIZES) == 4
    partials = mk.out("partials", 1, nb)
    vals = [1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 41.0, 0.0]
    hyper = _hyper(mk, "hyper", vals)
    call(lib, "hsg_mt_sqnorm", tab, len(gs), P(partials), P(hyper))
    ref = torch.cat([torch.stack([c.double().pow(2).sum() for c in g.split(CHUNK)]) for g in gs]).view(1, -1)

    def check_hyper(got):
        want = list(vals)
        want[6] = 42.0                                   # the step counter advanced by exactly one
        assert got.view(torch.float64).view(-1).tolist() == want
    return {"partials": (ref, 0.0, 1e-5), "hyper": (check_hyper, 0, 0)}


@case("hsg_mt_adam", dict(mode="adam"), dict(mode="scale"))
def c_mt_adam(lib, mk, mode):
    ps = [torch.randn(n) for n in MT_SIZES]
    gs = [torch.randn(n) for n in MT_SIZES]
    hp = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.01)
    max_norm = 1.0
    # state after one oracle step on other gradients, so m and v are not zero
    _, m0, v0, _, _ = train_ref.adam_run(ps, [[torch.randn(n) for n in MT_SIZES]], torch.float32, **hp)
    partials = torch.cat([torch.stack([c.pow(2).sum() for c in g.split(CHUNK)]) for g in gs])
    hyper = torch.tensor([hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], max_norm, 2.0, 0.0], dtype=torch.float64)
    norm = mk.out("norm", 1, 1)
    entries, outs = [], {}
    for i, n in enumerate(MT_SIZES):
        g = mk.inp(gs[i])
        if mode == "scale":
            outs[f"p{i}"] = mk.out(f"p{i}", 1, n)
            entries.append((P(outs[f"p{i}"]), P(g), None, None, n))
        else:
            for k, init in (("p", ps[i]), ("m", m0[i]), ("v", v0[i])):
                outs[f"{k}{i}"] = mk.out(f"{k}{i}", 1, n, init=init.detach().view(1, -1))
            entries.append((P(outs[f"p{i}"]), P(g), P(outs[f"m{i}"]), P(outs[f"v{i}"]), n))
    call(lib, "hsg_mt_adam", _table(entries), len(entries), P(mk.inp(partials)), P(mk.ints(hyper)),
         1 if mode == "scale" else 0, P(norm))
    total = torch.cat(gs).double().norm()
    assert float(total) > max_norm
    refs = {"norm": (total.view(1, 1), 0.0, 1e-6)}
    if mode == "scale":
        coef = max_norm / (total + 1e-6)
        for i in range(len(MT_SIZES)):
            refs[f"p{i}"] = ((gs[i].double() * coef).view(1, -1), 1e-7, 1e-5)
        return refs
    # the second step of the oracle: start from (ps, m0, v0, step 1) in fp64
    sd = train_ref.adam_run(ps, [[torch.zeros(n) for n in MT_SIZES]], torch.float64, **hp)[4].state_dict()
    for i in range(len(MT_SIZES)):
        sd["state"][i]["exp_avg"], sd["state"][i]["exp_avg_sq"] = m0[i].double(), v0[i].double()
    p1, m1, v1, _, _ = train_ref.adam_run(ps, [gs], torch.float64, max_norm=max_norm, state=sd, **hp)
    for i in range(len(MT_SIZES)):
        for k, r in (("p", p1), ("m", m1), ("v", v1)):
            refs[f"{k}{i}"] = (r[i].view(1, -1), 1e-7, 1e-5)
    return refs


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=cid) for cs in CASES.values() for cid, fn, kw in cs])
def test_train_guard_bands(fn, kw):
    run_case(fn, kw)
