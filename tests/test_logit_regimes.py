"""The oracle at any logit magnitude (no GPU needed).

tests/test_gpu_logit_range.py measures the edge kernels against the fp64 restatement with
the same restatement in fp32 as the yardstick, under five logit regimes (tests/edge_ref.py).
This is the evidence that the references handle those inputs on their own: the op-level
oracle (oracle.fused.gat_aggregate_ref, with autograd) and the formula-level restatement
(edge_ref.restate) are finite in fp32 and in fp64 in every regime, agree with each other, the
fp32 runs agree with the fp64 ones, and regime 'ties' equals its closed form.

Bound of fp32 against fp64: an attention weight alpha = exp(s - m) / l takes the rounding of
the logit, of s - m and of exp -- each at most 2^-24 max(1, |s|) relative -- in numerator and
normaliser (6 such terms); the backward multiplies alpha by the difference G.Z - rho, whose
two sides carry the same error again (12).  16 x 2^-24 x max(1, |s|_max) x max(1, |ref|_max)
leaves a third for the fp32 accumulation of the sums.
"""
import pytest
import torch

import edge_ref as er

SHAPES = [(8, 8), (6, 50)]
CASES = [(k, o, r) for k in ("short", "long") for r in er.REGIMES for o in (None,)] + [
    ("long", o, "spread") for o in ("asc", "desc")]


def _inputs(kind, order, H, D, regime):
    arrays = er.relation_host(kind, order)[1:]
    torch.manual_seed(er.SEED)
    return arrays, er.draw(H, D, regime, dout=True)


def _oracle(arrays, v, H, D, dtype):
    from oracle.fused import gat_aggregate_ref
    e_src, e_dst, tf, phantom = arrays
    Z, a1, tau, org = (v[k].to(dtype).clone().requires_grad_() for k in ("Z", "a1", "tau", "origin"))
    out = gat_aggregate_ref(e_src, e_dst, tf, phantom, er.N_DST, Z, a1, tau, org)
    (out * v["dout"].to(dtype)).sum().backward()
    return dict(out=out.detach(), dZ=Z.grad, da1=a1.grad, dtau=tau.grad, dorigin=org.grad)


def _tol(smax, ref):
    return 16 * 2.0 ** -24 * max(1.0, smax) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("kind,order,regime", CASES)
def test_oracle_finite_and_fp32_agrees_with_fp64(kind, order, regime, H, D):
    arrays, v = _inputs(kind, order, H, D, regime)
    o64, o32 = _oracle(arrays, v, H, D, torch.float64), _oracle(arrays, v, H, D, torch.float32)
    r64, _ = er.restate(arrays, v, H, D, torch.float64)
    r32, _ = er.restate(arrays, v, H, D, torch.float32)
    es, tfl = torch.as_tensor(arrays[0]).long(), torch.as_tensor(arrays[2]).long()
    pre = r64["sigma"][es] + v["tau"].double()[tfl]
    smax = torch.where(pre > 0, pre, 0.01 * pre).abs().max().item()
    for tag, a64, a32 in (("oracle", o64, o32), ("restate", r64, r32)):
        for name in a64:
            assert torch.isfinite(a64[name]).all(), (tag, name, "fp64")
            assert torch.isfinite(a32[name]).all(), (tag, name, "fp32")
            err = (a32[name].double() - a64[name]).abs().max().item()
            print(f"{tag}.{name} {kind} {order} {H}x{D} {regime}: fp32 - fp64 {err:.3g}, bound {_tol(smax, a64[name]):.3g}")
            assert err <= _tol(smax, a64[name]), (tag, name, err, _tol(smax, a64[name]))
    # the restatement is the oracle's operation (it rounds sigma to fp32 as the kernels' input is)
    for a, b in (("x", "out"), ("dZ", "dZ"), ("da1", "da1"), ("dtau", "dtau")):
        err = (r64[a].reshape(-1) - o64[b].reshape(-1)).abs().max().item()
        assert err <= _tol(smax, o64[b]) / 4, (a, err)
    if regime == "ties":
        want = er.ties_closed_form(arrays, v["Z"], H, D)
        assert (r64["h"] - want).abs().max().item() <= 1e-12
        assert (o64["out"] - (torch.nn.functional.elu(want) + v["origin"].double())).abs().max().item() <= 1e-12
        assert (r32["h"].double() - want).abs().max().item() <= _tol(1.0, want)


def test_oracle_nan_free_where_the_unfixed_denominator_was_not():
    """The case that made this necessary: phantom-free destinations whose logits are all
    below -88.7 (regime 'offset-').  phantom * exp(-max) is 0 * inf there."""
    arrays, v = _inputs("short", None, 6, 50, "offset-")
    r32, _ = er.restate(arrays, v, 6, 50, torch.float32)
    ph = torch.as_tensor(arrays[3]).float().unsqueeze(1)
    assert torch.isnan(ph * torch.exp(-r32["m"])).any()          # what the denominator used to add
    assert all(torch.isfinite(t).all() for t in r32.values())


def test_ordered_relations_put_the_maximum_last_and_first():
    for order, pos in (("asc", -1), ("desc", 0)):
        _, e_src, e_dst, tf, _ = er.relation_host("long", order)
        _, e_src0, e_dst0, tf0, _ = er.relation_host("long")
        seg = e_dst == er.LONG_DST
        assert seg.sum() == 200 and tf[seg][pos] == tf[seg].max() == 10
        assert (e_src == e_src0).all() and (tf[~seg] == tf0[~seg]).all()
        assert sorted(tf[seg]) == sorted(tf0[seg])
