"""Parity of the fused WSWGAT stack at the SECOND and THIRD training step.

Every other comparison with the fp64 oracle runs on freshly seeded parameters and ends
after one forward and backward.  A step leaves state behind: parameters updated in
place (by the native optimizer through raw pointers, so no autograd version counter
moves), ``.grad`` tensors that are views of one flat buffer, the work lists' arrival
counters inside the cached relation, the dropout seed and offset, the optimizer's
cached pointer table, a captured graph that is replayed.  Here each step k of a short
trajectory is compared on its own: snapshot the modules' parameters (tests/step_ref.py),
run the GPU step with the upstream gradient R_k, run the oracle at the snapshot (with
the GPU's ReLU gates inside the fp32 band, and in train mode the step's keep-masks
restated on the host), and put both through test_gpu_stack_parity.compare -- the
project's existing fp32 bounds, nothing new.  Then update the parameters and go on.

tests/test_step_ref.py shows on the CPU that between two steps of this trajectory every
output row moves by more than 1000 x the output bound, so a step computed from anything
stale is far outside, and that a plain fp32 restatement of the oracle stays inside the
same bounds at the moved parameters.

Workloads: cfg2[:4] (19,880 edges, no long node) and cfg4[:2] (doc supernodes: pieced
W2S destinations and S2W sources, i.e. relations with work lists and arrival counters).
n_iter = 2, train.py's tail (clip 1.0, Adam lr 5e-4).  Where two runs must agree
exactly (accumulation, interleaved forwards, the optimizer's shadow) the check is
bitwise.
"""
import copy

import pytest
import torch

import step_ref
import weights
from helpers import build_graph, gat_inputs, seeded_gat_params
from test_gpu_stack_parity import _f64, compare, grad_stats, train_masks
from test_gpu_worklist import check_counters

pytestmark = pytest.mark.gpu

N_ITER = 2
DEV = "cuda"


class Case:
    """Graph, modules (from seeded_gat_params), the leaf T the optimizer also updates
    and the fixed inputs Xw, Xs (requires_grad) of one workload, on the GPU."""

    def __init__(self, config, train=False):
        from hetersumgraph_amd.HiGraph import register_tfidf_table
        self.config, self.seed = config, step_ref.SEEDS[config]
        self.z, self.n_docs, self.n_edges = step_ref.workload(config)
        self.n_w, self.n_s = int(self.z["n_w"]), int(self.z["n_s"])
        self.G = build_graph(self.z).to(torch.device(DEV))
        Xw, Xs, T = gat_inputs(self.seed, self.n_w, self.n_s)
        self.Xw, self.Xs, self.T = (t.to(DEV).requires_grad_() for t in (Xw, Xs, T))
        register_tfidf_table(self.G, self.T)
        w2s, s2w = seeded_gat_params(self.seed * 100 + 1, self.seed * 100 + 2)
        self.w2s, self.s2w = w2s.to(DEV), s2w.to(DEV)
        if train:
            self.w2s.train()
            self.s2w.train()
        self.params = list(self.w2s.parameters()) + list(self.s2w.parameters()) + [self.T]

    def R(self, k):
        return step_ref.upstream(self.seed, k, self.n_s)

    def snapshot(self):
        return step_ref.snapshot(self.w2s, self.s2w, self.T)

    def step(self, R):
        return step_ref.gpu_step(self.G, self.w2s, self.s2w, self.T, self.Xw, self.Xs, R, N_ITER)

    def oracle(self, snap, R, **kw):
        return step_ref.oracle_at(self.z, snap, self.Xw, self.Xs, R, N_ITER, **kw)

    def zero(self):
        for p in self.params + [self.Xw, self.Xs]:
            p.grad = None

    def compare(self, tag, r, o):
        report(f"{self.config} {tag}", r, o)
        compare(f"{self.config} {tag}", "f32", r, o, self.n_docs, self.n_edges)


def report(tag, r, o):
    """Print the worst error over its allowed value among everything ``compare`` checks
    (its fp32 bounds restated; this asserts nothing, ``compare`` does) -- the figures of
    DESIGN.md section 4's table."""
    from hetersumgraph_amd.module.GATStackLayer import reference_named_grads
    worst = {"out": (_f64(r["s"]) - o["s"]).abs().max().item() / 2e-5}
    for k, rk in (("Xs", "Xs"), ("Xw", "Xw"), ("_TFembed", "T")):
        s = grad_stats(r[rk], o[rk])
        worst[k] = max(s["fro"] / 2e-4, s["worst"] / 1e-2, s["bad_rows"] / max(2, int(0.005 * s["rows"])))
    ratio = 0.0
    for mod, pd in ((r["w2s"], o["p1"]), (r["s2w"], o["p2"])):
        for k, g in reference_named_grads(mod):
            sref = pd[k[:-4] + "weight"].grad if k.endswith("feat_fc.bias") else None
            s = grad_stats(g, pd[k].grad, scale_ref=sref)
            ratio = max(ratio, s["fro"] / 5e-4, s["worst"] / 5e-3)
    worst["params"] = ratio
    print(f"RATIO {tag}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          f" | worst {max(worst.values()):.3f}")


def changed(a, b):
    """Every tensor of snapshot ``b`` differs from snapshot ``a``'s: the update reached it."""
    return all(not torch.equal(x, y) for x, y in zip(step_ref.leaves(a), step_ref.leaves(b)))


class Shadow:
    """The native optimizer's update restated on tensors of its own: copies of the
    parameters, a second optimizer, and every step the real step's gradients assigned as
    fresh tensors.  The native kernels are layout independent bit for bit
    (test_gpu_optim.py), so the real parameters -- whose gradients are views of the
    stack's flat buffer at whatever address this step's backward got, behind the
    optimizer's cached pointer table -- must equal the shadow's exactly."""

    def __init__(self, params):
        from hetersumgraph_amd import optim
        self.params = [p.detach().clone().requires_grad_() for p in params]
        self.opt = optim.Adam(self.params, lr=step_ref.LR, max_grad_norm=step_ref.MAX_NORM)

    def step(self, grads):
        for q, g in zip(self.params, grads):
            q.grad = None if g is None else g.detach().clone()
        self.opt.step()

    def check(self, params):
        torch.cuda.synchronize()
        for i, (p, q) in enumerate(zip(params, self.params)):
            assert torch.equal(p.detach(), q.detach()), f"parameter {i} differs from the shadow optimizer's"


def updater(kind, c):
    """(update, zero): train.py's tail on ``c.params`` -- torch's clip_grad_norm_ + Adam,
    or the native optimizer with the clip folded in (which leaves .grad unscaled)."""
    if kind == "torch":
        opt = torch.optim.Adam(c.params, lr=step_ref.LR)

        def update():
            torch.nn.utils.clip_grad_norm_(c.params, step_ref.MAX_NORM)
            opt.step()
    else:
        from hetersumgraph_amd import optim
        opt = optim.Adam(c.params, lr=step_ref.LR, max_grad_norm=step_ref.MAX_NORM)
        update = opt.step

    def zero():
        opt.zero_grad(set_to_none=True)
        c.Xw.grad = c.Xs.grad = None
    return update, zero


def test_cfg4_small_batch_has_work_lists():
    c = Case("cfg4")
    assert "dwork" in c.G.relation("W2S").dev and "swork" in c.G.relation("S2W").dev


@pytest.mark.parametrize("kind", ["torch", "native"])
@pytest.mark.parametrize("config", list(step_ref.WORKLOADS))
def test_trajectory_eval(config, kind):
    """3a: three steps in eval mode; gradients compared before the update."""
    c = Case(config)
    update, zero = updater(kind, c)
    shadow = Shadow(c.params) if kind == "native" else None
    prev = None
    for k in range(3):
        snap = c.snapshot()
        assert prev is None or changed(prev, snap)
        r = c.step(c.R(k))
        o = c.oracle(snap, c.R(k), gates=r["gates"])
        c.compare(f"eval {kind} step {k}", r, o)
        grads = [p.grad for p in c.params]
        update()
        if shadow is not None:
            shadow.step(grads)
            shadow.check(c.params)
        zero()
        prev = snap
    if config == "cfg4":
        # nine W2S forwards and six S2W backwards later: the arrival counters of the
        # in-kernel piece merge are still whole multiples of the piece counts
        check_counters(c.G.relation("W2S").dev["dwork"])
        check_counters(c.G.relation("S2W").dev["swork"], inline=False)


def test_trajectory_train():
    """3b: train mode (dropout 0.1 on head inputs and FFN outputs), native updater.  One
    rng.manual_seed, one rng.advance_all() per step as bench.py does; the step's seed and
    offsets are read from the forward's saved state and the oracle gets the keep-masks
    restated on the host.  As test_gpu_replay_masks.py documents: one seed snapshot per
    step, the seed one higher every step, and per application the head projection's draw
    one offset before the FFN's -- the host-side offset runs on across steps."""
    from hetersumgraph_amd import rng
    c = Case("cfg2", train=True)
    update, zero = updater("native", c)
    shadow = Shadow(c.params)
    seed0 = 7070
    rng.manual_seed(seed0)
    prev = None
    for k in range(3):
        snap = c.snapshot()
        assert prev is None or changed(prev, snap)
        rng.advance_all()
        r = c.step(c.R(k))
        seed, offs = r["draws"]
        assert seed == seed0 + 1 + k
        n_app = 2 * N_ITER + 1
        assert offs == [2 * n_app * k + 2 * (i + 1) for i in range(n_app)]
        assert rng.get(DEV).offset == 2 * n_app * (k + 1)
        ms = train_masks(seed, offs[0] - 2, c.n_w, c.n_s, n_iter=N_ITER)
        o = c.oracle(snap, c.R(k), masks=ms, gates=r["gates"])
        c.compare(f"train native step {k}", r, o)
        grads = [p.grad for p in c.params]
        update()
        shadow.step(grads)
        shadow.check(c.params)
        zero()
        prev = snap


@pytest.mark.parametrize("captured_opt", [False, True], ids=["opt_eager", "opt_captured"])
def test_captured_step(captured_opt):
    """3c: bench.py's step() -- grads set to None, the fused stack, backward with a
    static R buffer -- captured once and replayed three times, the native optimizer
    stepped eagerly between replays or captured in the same graph.  Each replay's cloned
    outputs and gradients against the oracle at the parameters just before it."""
    from hetersumgraph_amd import optim
    from hetersumgraph_amd.stack import gat_stack
    c = Case("cfg2")
    opt = optim.Adam(c.params, lr=step_ref.LR, max_grad_norm=step_ref.MAX_NORM)
    Rbuf = torch.zeros(c.n_s, 64, device=DEV)
    hold = {}

    def step():
        c.zero()
        s = gat_stack(c.G, c.w2s, c.s2w, c.T, c.Xw, c.Xs, N_ITER)
        ctx = s.grad_fn
        # the hidden-activation buffers (the ReLU gates), kept past the backward
        hold["H"] = {kind: ctx.bufs[id(lay)][1] for kind, lay in (("W2S", ctx.cfg[1]), ("S2W", ctx.cfg[2]))}
        s.backward(Rbuf)
        hold["s"] = s
        if captured_opt:
            opt.step()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()                      # with the optimizer: allocates its state and workspace
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    prev = None
    for k in range(3):
        torch.cuda.synchronize()
        snap = c.snapshot()
        assert prev is None or changed(prev, snap)
        Rbuf.copy_(c.R(k))
        g.replay()
        torch.cuda.synchronize()
        gates = {kind: [(h > 0).cpu() for h in H] for kind, H in hold["H"].items()}
        r = step_ref.collect(hold["s"], c.Xw, c.Xs, c.T, c.w2s, c.s2w, gates)
        if captured_opt:
            # the replay has already moved the parameters; what it computed belongs to
            # the snapshot taken before it
            assert changed(snap, c.snapshot())
        else:
            opt.step()
        o = c.oracle(snap, c.R(k), gates=gates)
        c.compare(f"captured {'opt captured' if captured_opt else 'opt eager'} replay {k}", r, o)
        prev = snap


def test_accumulation_without_zero_grad():
    """3d: two steps at the same parameters with R_1, R_2 and no zero_grad in between:
    every .grad is bitwise g(R_1) + g(R_2) of two isolated runs (summed in torch fp32),
    and a native optimizer step on the accumulated gradients is bitwise the step from
    freshly assigned summed gradients."""
    c = Case("cfg2")
    alone = []
    for k in (1, 2):
        c.zero()
        alone.append(c.step(c.R(k)))
    c.zero()
    c.step(c.R(1))
    acc = c.step(c.R(2))
    a, b = alone
    for key in ("Xw", "Xs", "T"):
        assert torch.equal(acc[key], a[key] + b[key]), key
    assert acc["pgrads"].keys() == a["pgrads"].keys()
    for n in acc["pgrads"]:
        assert torch.equal(acc["pgrads"][n], a["pgrads"][n] + b["pgrads"][n]), n
    assert not torch.equal(a["Xs"], b["Xs"])                   # two different steps
    assert torch.equal(acc["s"], b["s"])
    # the optimizer on the accumulated .grad tensors vs on fresh sums
    shadow = Shadow(c.params)
    real = [p.grad for p in c.params]
    summed = [x.grad + y.grad for x, y in zip(_params(a), _params(b))] + [a["T"] + b["T"]]
    assert all(torch.equal(x, y) for x, y in zip(real, summed))
    update, _ = updater("native", c)
    update()
    shadow.step(summed)
    shadow.check(c.params)


def _params(r):
    return list(r["w2s"].parameters()) + list(r["s2w"].parameters())


@pytest.mark.parametrize("config", list(step_ref.WORKLOADS))
def test_two_forwards_in_flight(config):
    """3e: forward A, forward B (same graph and modules, another Xs), then B's backward,
    then A's, all on one stream: outputs and every gradient bitwise equal to each run
    done alone (the second forward must not disturb what the first saved, nor the work
    lists' counters the first left)."""
    from hetersumgraph_amd.stack import gat_stack
    c = Case(config)
    XsB = torch.from_numpy(weights.feature(c.seed + 1, "Xs", (c.n_s, 64), 1.0)).to(DEV).requires_grad_()
    assert not torch.equal(XsB, c.Xs)
    Ra, Rb = c.R(1).to(DEV, torch.float32), c.R(2).to(DEV, torch.float32)
    fwd = lambda Xs: gat_stack(c.G, c.w2s, c.s2w, c.T, c.Xw, Xs, N_ITER)
    bwd = lambda s, Xs, R: torch.autograd.grad(s, [c.Xw, Xs] + c.params, grad_outputs=R)
    alone = []
    for Xs, R in ((c.Xs, Ra), (XsB, Rb)):
        s = fwd(Xs)
        alone.append([s.detach().clone()] + [t.clone() for t in bwd(s, Xs, R)])
    sA = fwd(c.Xs)
    sB = fwd(XsB)
    outB = [sB.detach().clone()] + [t.clone() for t in bwd(sB, XsB, Rb)]
    outA = [sA.detach().clone()] + [t.clone() for t in bwd(sA, c.Xs, Ra)]
    torch.cuda.synchronize()
    for name, got, ref in (("A", outA, alone[0]), ("B", outB, alone[1])):
        assert len(got) == len(ref) == 2 + 1 + len(c.params)
        for i, (x, y) in enumerate(zip(got, ref)):
            assert torch.equal(x, y), (name, i)
    assert not torch.equal(outA[0], outB[0])


def _move_in_place(params, seed):
    """One in-place optimizer step (SGD, lr 1) that moves every entry by 1e-2 .. 2e-2."""
    g = torch.Generator().manual_seed(seed)
    for p in params:
        sign = torch.where(torch.rand(p.shape, generator=g) < 0.5, -1.0, 1.0)
        p.grad = (sign * (1e-2 + 1e-2 * torch.rand(p.shape, generator=g))).to(p.device)
    before = [p.detach().clone() for p in params]
    torch.optim.SGD(params, lr=1.0).step()
    for p, q in zip(params, before):
        assert (p.detach() - q).abs().min().item() >= 0.99e-2       # fp32 rounding of p + 1e-2
        p.grad = None


def test_sent_lstm_after_in_place_update():
    """3f: the native sentence LSTM called once, its nn.LSTM parameters then moved by an
    in-place optimizer step, called again: against torch's CPU nn.LSTM at the moved
    parameters, test_gpu_lstm.py's yardstick and its smallest variant."""
    import test_gpu_lstm as tl
    kw, lens = tl.VARIANTS["one_doc_one_step"]
    assert sum(lens) == min(sum(v[1]) for v in tl.VARIANTS.values())
    lstm = tl.make_lstm(21, **kw).eval()
    width = lstm.hidden_size * (2 if lstm.bidirectional else 1)
    x, R = tl.make_rows(22, lens, width)
    lstm_d = copy.deepcopy(lstm).to(DEV).eval()
    tl.native(lstm_d, x, R, lens)                               # whatever a first call leaves behind
    before64, _ = tl.references(lstm, x, R, lens)
    _move_in_place(list(lstm_d.parameters()), 5)
    lstm.load_state_dict({k: v.cpu() for k, v in lstm_d.state_dict().items()})
    r64, r32 = tl.references(lstm, x, R, lens)
    out, grads = tl.native(lstm_d, x, R, lens)
    bound = min(4 * (r32["out"].double() - r64["out"]).abs().max().item(), 1e-4)
    assert (r64["out"] - before64["out"]).abs().max().item() >= 1000 * bound
    tl.check("moved out", out, r64["out"], r32["out"], forward=True)
    tl.check_grads(lstm, grads, r64, r32)


def test_sent_cnn_after_in_place_update():
    """3f: the sentence CNN on the encoder golden's ids, called once, parameters moved in
    place, called again: against oracle.cnn.sent_encoder at the moved parameters, at
    test_gpu_encoder.py's bounds (outputs 5e-5; gradients 1e-4 of the largest entry, the
    upstream gradient zeroed where the max-pool winner is ambiguous, as that file does)."""
    import test_gpu_encoder as te
    from helpers import load_fixture
    from hetersumgraph_amd.cnn import sent_cnn
    from oracle import cnn as ocnn
    ids = torch.from_numpy(load_fixture("encoder")["ids"])
    emb, pos, cw, cb = te.gpu_params()
    leaves = [emb] + cw + cb
    f64 = lambda: [t.detach().cpu().double() for t in leaves]
    first = sent_cnn(ids.cuda(), emb, pos, cw, cb, padding_idx=0)
    p0 = f64()
    before = ocnn.sent_encoder(ids, p0[0], pos.cpu().double(), p0[1:7], p0[7:])
    assert (first.detach().cpu().double() - before).abs().max().item() < 5e-5
    _move_in_place(leaves, 6)
    p1 = [t.requires_grad_() for t in f64()]
    ref = ocnn.sent_encoder(ids, p1[0], pos.cpu().double(), p1[1:7], p1[7:])
    assert (ref.detach() - before).abs().max().item() >= 1000 * 5e-5
    mask = te.unambiguous(ids, p1[0].detach(), pos.cpu().double(), [t.detach() for t in p1[1:7]],
                          [t.detach() for t in p1[7:]])
    assert mask.float().mean() > 0.95
    R = torch.from_numpy(weights.feature(te.SEED, "dfeat", tuple(ref.shape))).double() * mask
    (ref * R).sum().backward()
    feat = sent_cnn(ids.cuda(), emb, pos, cw, cb, padding_idx=0)
    (feat * R.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert (feat.detach().cpu().double() - ref.detach()).abs().max().item() < 5e-5
    for i, (a, b) in enumerate(zip(leaves, p1)):
        assert te.rel_err(a.grad, b.grad) < 1e-4, i
