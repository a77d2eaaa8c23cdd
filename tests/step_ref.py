"""The fp64 oracle of the fused WSWGAT stack at a module's CURRENT parameters.

``oracle_stack`` / ``gpu_stack`` of test_gpu_stack_parity.py build their parameters
from seeds, so they can only check the first step after initialisation.  A training
step leaves state behind (parameters updated in place, ``.grad`` views of one flat
buffer, work-list arrival counters, dropout seed and offset, the optimizer's pointer
table, the lazily formed ``g.edata['e']``, a captured graph).  The helpers here take
the parameters from the modules as they are now, so a test can follow a trajectory:
snapshot, run the GPU step, run the oracle at the snapshot, compare, update, repeat
(test_gpu_second_step.py, test_gpu_edge_scores.py; pinned on the CPU by
test_step_ref.py).  No GPU code of its own: ``gpu_step`` imports the product lazily.
"""
import copy

import numpy as np
import torch

from helpers import concat_arrays

# the small workloads of the multi-step tests: (synth config, documents).  cfg2[:4] has
# 19,880 graph edges and no long node; cfg4[:2] has doc supernodes, i.e. pieced
# destinations (W2S) and sources (S2W) -- relations with work lists
WORKLOADS = {"cfg2": 4, "cfg4": 2}
# the seeds test_gpu_stack_parity.py's eval cases use for these configs; the GPU tests
# use them too, so the condition test_step_ref.py asserts is the one they rely on.  How
# far the edge logits move depends on the seed (0.2 - 0.7 over eight seeds tried per
# config, one other seed 0.098 at step 2): a changed seed has to pass those assertions
SEEDS = {"cfg2": 31, "cfg4": 32}
LR, MAX_NORM = 5e-4, 1.0                 # train.py's tail: clip 1.0, Adam lr 5e-4


def workload(config):
    """(fixture-like arrays, n_docs, n_edges) of a multi-step workload."""
    from helpers import synth_fixture
    from hetersumgraph_amd import synth
    docs = synth.make_batch_docs(config, seed=0)[:WORKLOADS[config]]
    z = synth_fixture(docs)
    return z, len(docs), int(z["g_n_edges"].sum())


def upstream(seed, k, n_s):
    """R_k, the upstream gradient of step k: fp64 [n_s, 64] from default_rng(seed + k)."""
    return torch.from_numpy(np.random.default_rng(seed + k).standard_normal((n_s, 64)))


def snapshot(w2s, s2w, T, dtype=torch.float64):
    """(p1, p2, T) -- the two modules' current state dicts (reference key names) and
    the tf-idf table as fresh CPU leaves of ``dtype``: nothing shares storage with the
    modules, so a later in-place update cannot reach the snapshot."""
    from oracle import fused
    T64 = T.detach().cpu().to(dtype).clone().requires_grad_()
    return fused.as_params(w2s, dtype=dtype), fused.as_params(s2w, dtype=dtype), T64


def recast(snap, dtype):
    """A snapshot's values as fresh leaves of another dtype (the fp32 restatement)."""
    p1, p2, T = snap
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    return {k: leaf(v) for k, v in p1.items()}, {k: leaf(v) for k, v in p2.items()}, leaf(T)


def leaves(snap):
    p1, p2, T = snap
    return list(p1.values()) + list(p2.values()) + [T]


def _cpu(t, dtype):
    return torch.as_tensor(np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)).to(dtype)


def oracle_at(z, snap, Xw, Xs, R, n_iter, masks=None, gates=None, want_gates=False):
    """``oracle_stack``'s body with the parameters (``snap``), the inputs and the
    upstream gradient passed in: s1 = W2S(w0, s0), then n_iter x (w = S2W(w, s);
    s = W2S(w, s)), backward of sum(s * R), in the snapshot's dtype.  Same dict layout
    (s, Xw, Xs, T, p1, p2, R), so test_gpu_stack_parity.compare takes it unchanged.
    ``masks`` / ``gates`` as there.  ``want_gates``: also return the ReLU gates this run
    took per application ({"W2S": [...], "S2W": [...]}, the layout ``gates`` takes)."""
    from oracle import fused
    p1, p2, T = snap
    dt = T.dtype
    for t in leaves(snap):
        t.grad = None
    a = concat_arrays(z)
    rws = fused.typed_relation("W2S", a["src"], a["dst"], a["unit"], a["tffrac"], a["edtype"])
    rsw = fused.typed_relation("S2W", a["src"], a["dst"], a["unit"], a["tffrac"], a["edtype"])
    Xw, Xs = (_cpu(t, dt).clone().requires_grad_() for t in (Xw, Xs))
    m = iter(masks) if masks is not None else None
    nxt = (lambda: next(m)) if m is not None else (lambda: None)
    gw = iter(gates["W2S"]) if gates is not None else None
    gs = iter(gates["S2W"]) if gates is not None else None
    gate = (lambda it: next(it) if it is not None else None)
    taken = {"W2S": [], "S2W": []}
    plain_ffn = fused.ffn

    def recording_ffn(x, params, prefix="", **kw):
        w1 = params[f"{prefix}ffn.w_1.weight"].squeeze(-1)
        with torch.no_grad():
            taken["W2S" if x.shape[1] == 64 else "S2W"].append((x @ w1.t() + params[f"{prefix}ffn.w_1.bias"]) > 0)
        return plain_ffn(x, params, prefix, **kw)

    if want_gates:
        fused.ffn = recording_ffn
    try:
        w, s = Xw, fused.wswgat_layer("W2S", rws, Xw, Xs, p1, T, masks=nxt(), gate=gate(gw))
        for _ in range(n_iter):
            w = fused.wswgat_layer("S2W", rsw, w, s, p2, T, masks=nxt(), gate=gate(gs))
            s = fused.wswgat_layer("W2S", rws, w, s, p1, T, masks=nxt(), gate=gate(gw))
    finally:
        fused.ffn = plain_ffn
    R = _cpu(R, dt)
    (s * R).sum().backward()
    out = dict(s=s.detach(), Xw=Xw.grad, Xs=Xs.grad, T=T.grad, p1=p1, p2=p2, R=R)
    if want_gates:
        out["gates"] = taken
    return out


def edge_column_at(z, snap, Xw, Xs, n_iter):
    """``g.edata['e']`` as the reference's heads leave it after the stack's forward at
    the snapshot's parameters: oracle/dgl_udf.stack_step on a UdfGraph, its ``e``."""
    from oracle import dgl_udf
    p1, p2, T = snap
    ug = dgl_udf.UdfGraph(z["g_src"], z["g_dst"], z["g_unit"], z["g_tffrac"], z["g_edtype"])
    with torch.no_grad():
        dgl_udf.stack_step(ug, _cpu(Xw, T.dtype), _cpu(Xs, T.dtype), p1, p2, T.detach(), n_iter=n_iter)
    return ug.e


class ParamGrads:
    """An oracle run's name -> leaf dict in the shape ``compare`` reads a module's
    gradients in (GATStackLayer.reference_named_grads: named_modules, then
    named_parameters with ``.grad``) -- for comparing one oracle run with another."""

    def __init__(self, params):
        self.params = params

    def named_modules(self):
        return iter(())

    def named_parameters(self):
        return iter(self.params.items())


def as_run(o):
    """An ``oracle_at`` result in the layout of a GPU run (``compare``'s first operand)."""
    return dict(s=o["s"], Xw=o["Xw"], Xs=o["Xs"], T=o["T"], w2s=ParamGrads(o["p1"]), s2w=ParamGrads(o["p2"]))


def read_gates(ctx):
    """The FFN ReLU gates each application of a fused-stack forward took (the per-layer
    hidden buffers of its autograd node, before the backward frees them)."""
    return {kind: [(h > 0).cpu() for h in ctx.bufs[id(lay)][1]]
            for kind, lay in (("W2S", ctx.cfg[1]), ("S2W", ctx.cfg[2]))}


def read_draws(ctx):
    """(seed, [FFN dropout offset per application]) of a train-mode forward, from what
    its applications saved (the head projection's draw is one offset earlier), or None
    in eval mode."""
    fs = [saved[3] for _, saved, *_ in ctx.apps if saved[3][8] > 0]
    if not fs:
        return None
    seeds = {int(f[9].item()) for f in fs}
    assert len(seeds) == 1, seeds                                  # one seed snapshot per step
    return seeds.pop(), [int(f[10]) for f in fs]


def collect(s, Xw, Xs, T, w2s, s2w, gates=None):
    """Clones of a step's results in ``compare``'s layout: the output, the state
    gradients, and copies of both modules carrying clones of every parameter and its
    ``.grad`` -- a captured step rewrites all of these in place at the next replay and
    an optimizer moves the parameters."""
    g = lambda t: None if t.grad is None else t.grad.detach().clone()
    r = dict(s=s.detach().clone(), Xw=g(Xw), Xs=g(Xs), T=g(T), w2s=copy.deepcopy(w2s), s2w=copy.deepcopy(s2w),
             gates=gates)
    for tag, mod in (("w2s", w2s), ("s2w", s2w)):                  # deepcopy leaves .grad behind
        for p, q in zip(mod.parameters(), r[tag].parameters()):
            q.grad = g(p)
    r["pgrads"] = {f"{tag}.{n}": p.grad for tag in ("w2s", "s2w") for n, p in r[tag].named_parameters()}
    return r


def gpu_step(G, w2s, s2w, T, Xw, Xs, R, n_iter):
    """One forward and backward of the fused stack at the modules' current parameters
    (no zero_grad: gradients accumulate as autograd has them).  Returns ``collect``'s
    clones plus the forward's ReLU gates and, in train mode, its dropout draws."""
    from hetersumgraph_amd.stack import fused_stack_ok, gat_stack
    assert fused_stack_ok(G, w2s, s2w, T, Xw, Xs)
    s = gat_stack(G, w2s, s2w, T, Xw, Xs, n_iter)
    assert type(s.grad_fn).__name__.startswith("_GatStack")        # the timed node, not the layer path
    gates, draws = read_gates(s.grad_fn), read_draws(s.grad_fn)
    s.backward(torch.as_tensor(R).to(s.device, torch.float32))
    torch.cuda.synchronize()
    return dict(collect(s, Xw, Xs, T, w2s, s2w, gates), draws=draws)
