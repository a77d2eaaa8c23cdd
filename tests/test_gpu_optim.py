"""hetersumgraph_amd.optim: the multi-tensor clip + Adam (hsg_mt_sqnorm / hsg_mt_adam)
against torch on the CPU in fp64 (tests/train_ref.py), over tensors of 1, 2, 3, 5, 63, 64,
65, chunk - 1, chunk, chunk + 1 and 153,600 elements (the chunk is the 4,096 elements one
block owns), as separate tensors and as views at odd element offsets of one flat buffer.

Tolerance: p, exp_avg and exp_avg_sq within 2x the error of fp32 torch.optim.Adam on the
same inputs (its maximum over the tensor), floored at 4 fp32 ulp of the value.  Measured
on an MI355X over three steps, both hyper-parameter sets and both layouts, native (fp32
torch) maximum error: p 3.2e-7 (3.2e-7), exp_avg 1.3e-7 (1.3e-7), exp_avg_sq 1.5e-7
(1.3e-7); worst error / allowed 0.77.  The gradient norm is asserted within 1e-6 relative
of fp64.  Worst case: a partial is one square, 16 serial adds and 8 tree levels per
element path, <= 25 fp32 roundings, so the sum of squares is within 25 * 2^-24 = 1.5e-6 and
its root within 7.5e-7; the double sum of the partials (49 here, 464 for the model's
1,762,166 parameters in 55 tensors) adds ~1e-13 and the fp32 scalar that holds the norm
6e-8.  Measured: 1.4e-8.
"""
import pytest
import torch

import train_ref
from train_ref import CHUNK, SIZES

pytestmark = pytest.mark.gpu

DEV = "cuda"
HYPERS = {"default": {}, "custom": dict(betas=(0.8, 0.95), eps=1e-6, weight_decay=0.01)}
SENTINEL = 0x7FC5A5A5                        # a NaN no arithmetic produces (tests/guard.py)


def host_data(sizes, steps, seed=0, gscale=1.0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g) for n in sizes]
    gs = [[torch.randn(n, generator=g) * gscale for n in sizes] for _ in range(steps)]
    return ps, gs


class Layout:
    """The parameters and their gradient tensors on the device: separate tensors, or views
    at odd element offsets (4-byte aligned only) of one flat buffer each for p and g, the
    gaps between the views holding a sentinel."""

    def __init__(self, ps, layout):
        self.sizes = [p.numel() for p in ps]
        self.flat = layout == "flat"
        if self.flat:
            offs, cur = [], 1
            for n in self.sizes:
                offs.append(cur)
                cur = (cur + n + 2) | 1                # at least two sentinel elements, then odd again
            self.offs, total = offs, cur + 8
            assert all(o % 2 == 1 for o in offs)
            mk = lambda: torch.full((total,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            self.pflat, self.gflat = mk(), mk()
            self.params = [torch.nn.Parameter(self.pflat[o:o + n]) for o, n in zip(offs, self.sizes)]
            self.gviews = [self.gflat[o:o + n] for o, n in zip(offs, self.sizes)]
            assert all(p.data_ptr() % 16 != 0 for p in self.params)
        else:
            self.params = [torch.nn.Parameter(torch.empty(n, device=DEV)) for n in self.sizes]
            self.gviews = [torch.empty(n, device=DEV) for n in self.sizes]
        with torch.no_grad():
            for p, v in zip(self.params, ps):
                p.copy_(v)
        for p, g in zip(self.params, self.gviews):
            p.grad = g

    def set_grads(self, gs):
        for v, g in zip(self.gviews, gs):
            v.copy_(g)

    def assert_gaps_untouched(self):
        if not self.flat:
            return
        for flat in (self.pflat, self.gflat):
            keep = torch.ones(flat.numel(), dtype=torch.bool, device=DEV)
            for o, n in zip(self.offs, self.sizes):
                keep[o:o + n] = False
            assert bool((flat.view(torch.int32)[keep] == SENTINEL).all()), "an element between two views was written"


def native_run(ps, gs, layout, max_norm=None, **hyper):
    from hetersumgraph_amd import optim
    lay = Layout(ps, layout)
    opt = optim.Adam(lay.params, max_grad_norm=max_norm, **hyper)
    norms = []
    for step in gs:
        lay.set_grads(step)
        opt.step()
        norms.append(opt.last_grad_norm.clone())
    lay.assert_gaps_untouched()
    p = [q.detach().clone() for q in lay.params]
    m = [opt.state[q]["exp_avg"].clone() for q in lay.params]
    v = [opt.state[q]["exp_avg_sq"].clone() for q in lay.params]
    return p, m, v, norms, opt, lay


def assert_parity(got, ref64, ref32, what):
    worst = {}
    for name, g, r, y in zip("pmv", got, ref64, ref32):
        for i, (a, b, c) in enumerate(zip(g, r, y)):
            e, ye = train_ref.assert_within(a, b, c, f"{what} {name}[{i}] n={a.numel()}")
            worst[name] = max(worst.get(name, (0, 0)), (e, ye))
    print(what, "maxima (ours, fp32 torch):", worst)


def bitwise(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_constants():
    from hetersumgraph_amd import _lib
    assert _lib.load().hsg_mt_chunk() == CHUNK
    assert {CHUNK - 1, CHUNK, CHUNK + 1} <= set(SIZES)


@pytest.mark.parametrize("layout", ["separate", "flat"])
@pytest.mark.parametrize("hyper", sorted(HYPERS))
def test_parity_three_steps(hyper, layout):
    ps, gs = host_data(SIZES, 3)
    hp = HYPERS[hyper]
    p64, m64, v64, _, _ = train_ref.adam_run(ps, gs, torch.float64, **hp)
    p32, m32, v32, _, _ = train_ref.adam_run(ps, gs, torch.float32, **hp)
    p, m, v, _, opt, _ = native_run(ps, gs, layout, **hp)
    assert_parity((p, m, v), (p64, m64, v64), (p32, m32, v32), f"{hyper}-{layout}")
    assert opt.step_count() == 3


@pytest.mark.parametrize("max_norm", [None, 1.0])
@pytest.mark.parametrize("hyper", sorted(HYPERS))
def test_layout_independence_is_bitwise(hyper, max_norm):
    """The update is elementwise, and a thread owns the same elements whether its block
    uses 16-byte or 4-byte accesses: separate tensors and odd-offset views agree bit for bit."""
    ps, gs = host_data(SIZES, 3, seed=1)
    a = native_run(ps, gs, "separate", max_norm, **HYPERS[hyper])
    b = native_run(ps, gs, "flat", max_norm, **HYPERS[hyper])
    for k in range(3):
        assert bitwise(a[k], b[k]), "pmv"[k]
    assert bitwise(a[3], b[3])


@pytest.mark.parametrize("layout", ["separate", "flat"])
def test_clipping_above_max_norm(layout):
    ps, gs = host_data(SIZES, 3, seed=2)
    p64, m64, v64, n64, _ = train_ref.adam_run(ps, gs, torch.float64, max_norm=1.0)
    p32, m32, v32, _, _ = train_ref.adam_run(ps, gs, torch.float32, max_norm=1.0)
    p, m, v, norms, _, lay = native_run(ps, gs, layout, 1.0)
    for got, want in zip(norms, n64):
        assert float(want) > 1.0
        rel = abs(float(got) - float(want)) / float(want)
        print(f"grad norm {float(got):.9g} vs fp64 {float(want):.12g}: rel {rel:.2e}")
        # the fp32 scalar it is stored in rounds at 6e-8; the sum itself is far inside 1e-6
        assert rel <= 1e-6
    assert_parity((p, m, v), (p64, m64, v64), (p32, m32, v32), f"clip-{layout}")
    # the fold-in never rewrites .grad
    assert bitwise([q.grad for q in lay.params], [g.to(DEV) for g in gs[-1]])


def test_clipping_below_max_norm_is_the_unclipped_run():
    ps, gs = host_data(SIZES, 2, seed=3, gscale=1e-4)
    a = native_run(ps, gs, "separate", 1.0)
    b = native_run(ps, gs, "separate", None)
    assert all(0.0 < float(n) < 1.0 for n in a[3])
    for k in range(3):
        assert bitwise(a[k], b[k]), "pmv"[k]
    assert bitwise(a[3], b[3])                       # the norm is reported either way


@pytest.mark.parametrize("layout", ["separate", "flat"])
def test_standalone_clip_grad_norm(layout):
    from hetersumgraph_amd import optim
    ps, gs = host_data(SIZES, 1, seed=4)
    lay = Layout(ps, layout)
    lay.set_grads(gs[0])
    norm = optim.clip_grad_norm_(lay.params, 1.0)
    lay.assert_gaps_untouched()
    ref = {}
    for dt in (torch.float64, torch.float32):
        qs = [torch.nn.Parameter(p.to(dt)) for p in ps]
        for q, g in zip(qs, gs[0]):
            q.grad = g.to(dt).clone()
        ref[dt] = (torch.nn.utils.clip_grad_norm_(qs, 1.0, foreach=False), [q.grad for q in qs])
    assert norm.is_cuda and norm.dim() == 0
    assert abs(float(norm) - float(ref[torch.float64][0])) <= 1e-6 * float(ref[torch.float64][0])
    for i, q in enumerate(lay.params):
        train_ref.assert_within(q.grad, ref[torch.float64][1][i], ref[torch.float32][1][i], f"clipped grad[{i}]")
    # the same norm as the fold-in reports for these gradients
    folded = native_run(ps, gs, layout, 1.0)[3][0]
    assert torch.equal(norm, folded)
    # below max_norm the gradients are multiplied by exactly 1
    lay.set_grads([g * 1e-4 for g in gs[0]])
    before = [q.grad.clone() for q in lay.params]
    small = optim.clip_grad_norm_(lay.params, 1.0)
    assert 0.0 < float(small) < 1.0 and bitwise([q.grad for q in lay.params], before)


def test_more_tensors_than_one_launch_holds():
    from hetersumgraph_amd import _lib
    K = _lib.load().hsg_mt_tensors_per_launch()
    sizes = [1 + i % 5 for i in range(K + 3)]
    ps, gs = host_data(sizes, 1, seed=5)
    p64, m64, v64, n64, _ = train_ref.adam_run(ps, gs, torch.float64, max_norm=1.0)
    p32, m32, v32, _, _ = train_ref.adam_run(ps, gs, torch.float32, max_norm=1.0)
    p, m, v, norms, opt, _ = native_run(ps, gs, "separate", 1.0)
    assert opt.step_count() == 1                     # one step, however many launches
    assert abs(float(norms[0]) - float(n64[0])) <= 1e-6 * float(n64[0])
    assert_parity((p, m, v), (p64, m64, v64), (p32, m32, v32), "two-launches")


def test_parameter_without_gradient_is_skipped():
    from hetersumgraph_amd import optim
    ps, gs = host_data([5, 65, 3], 2, seed=6)
    lay = Layout(ps, "separate")
    lay.params[1].grad = None
    opt = optim.Adam(lay.params)
    for step in gs:
        lay.set_grads(step)
        opt.step()
    assert lay.params[1] not in opt.state or not opt.state[lay.params[1]]
    assert torch.equal(lay.params[1].detach().cpu(), ps[1])
    grads = [[g[0], None, g[2]] for g in gs]
    p64 = train_ref.adam_run(ps, grads, torch.float64)[0]
    p32 = train_ref.adam_run(ps, grads, torch.float32)[0]
    for i in (0, 2):
        train_ref.assert_within(lay.params[i], p64[i], p32[i], f"p[{i}]")
    assert len(opt.state_dict()["state"]) == 2


def test_non_finite_gradient_is_a_value_not_a_fault():
    """One inf element with clipping on: the norm is inf, the coefficient 0, inf * 0 = NaN
    at that element and 0 elsewhere -- p, m and v as torch computes them, NaN positions
    included."""
    ps, gs = host_data([5, CHUNK + 1, 65], 2, seed=7)
    gs[1][1][CHUNK] = float("inf")
    p64, m64, v64, _, _ = train_ref.adam_run(ps, gs, torch.float64, max_norm=1.0)
    p32, m32, v32, _, _ = train_ref.adam_run(ps, gs, torch.float32, max_norm=1.0)
    assert int(torch.isnan(p64[1]).sum()) == 1 and bool(torch.isnan(p64[1][CHUNK]))
    p, m, v, norms, _, _ = native_run(ps, gs, "separate", 1.0)
    assert torch.isinf(norms[1])
    assert_parity((p, m, v), (p64, m64, v64), (p32, m32, v32), "inf-gradient")


def _third_step_refs(ps2, sd, g3, hp):
    out = {}
    for dt in (torch.float64, torch.float32):
        out[dt] = train_ref.adam_run(ps2, [g3], dt, state=sd, **hp)[:3]
    return out


def test_state_dict_from_torch():
    from hetersumgraph_amd import optim
    hp = HYPERS["custom"]
    ps, gs = host_data([5, 65, CHUNK + 1], 3, seed=8)
    p2, _, _, _, topt = train_ref.adam_run(ps, gs[:2], torch.float32, **hp)
    sd = topt.state_dict()
    lay = Layout(p2, "separate")
    opt = optim.Adam(lay.params, **hp)
    opt.load_state_dict(sd)
    assert opt.step_count() == 2
    lay.set_grads(gs[2])
    opt.step()
    refs = _third_step_refs(p2, sd, gs[2], hp)
    got = ([q.detach() for q in lay.params], [opt.state[q]["exp_avg"] for q in lay.params],
           [opt.state[q]["exp_avg_sq"] for q in lay.params])
    assert_parity(got, refs[torch.float64], refs[torch.float32], "torch -> native")


def test_state_dict_to_torch():
    hp = HYPERS["custom"]
    ps, gs = host_data([5, 65, CHUNK + 1], 3, seed=9)
    p, m, v, _, opt, lay = native_run(ps, gs[:2], "separate", **hp)
    sd = opt.state_dict()
    assert all(float(st["step"]) == 2.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    p2 = [q.cpu() for q in p]
    refs = _third_step_refs(p2, sd, gs[2], hp)       # torch.optim.Adam loads the native state dict
    lay.set_grads(gs[2])
    opt.step()
    got = ([q.detach() for q in lay.params], [opt.state[q]["exp_avg"] for q in lay.params],
           [opt.state[q]["exp_avg_sq"] for q in lay.params])
    assert_parity(got, refs[torch.float64], refs[torch.float32], "native -> torch")
    assert "step" not in opt.state[lay.params[0]]


def test_third_step_references_start_from_the_same_step():
    """The oracle and the yardstick of the state-dict tests both take step 3: running one
    must not advance the state dict the other starts from."""
    ps, gs = host_data([5, 3], 3, seed=12)
    sd = train_ref.adam_run(ps, gs[:2], torch.float32)[4].state_dict()
    sd = {"state": {k: dict(v, step=v["step"].clone()) for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]}
    refs = _third_step_refs(ps, sd, gs[2], {})
    assert all(float(st["step"]) == 2.0 for st in sd["state"].values())
    for dt in refs:
        opt = train_ref.adam_run(ps, [gs[2]], dt, state=sd)[4]
        assert all(float(st["step"]) == 3.0 for st in opt.state.values())
    # fp32 and fp64 third steps differ by rounding, not by a bias correction
    for a, b in zip(refs[torch.float64][0], refs[torch.float32][0]):
        assert float((a - b.double()).abs().max()) <= 1e-6


def test_replaced_state_tensor_is_followed():
    """The cached table is keyed on the state tensors' pointers too: after exp_avg is
    replaced by hand, the next step reads and writes the new tensor."""
    ps, gs = host_data([5, CHUNK + 1], 2, seed=13)
    p, m, v, _, opt, lay = native_run(ps, gs[:1], "separate")
    q = lay.params[1]
    old = opt.state[q]["exp_avg"]
    opt.state[q]["exp_avg"] = old.clone()
    kept = old.clone()
    lay.set_grads(gs[1])
    opt.step()
    assert torch.equal(old, kept)
    p64, m64, _, _, _ = train_ref.adam_run(ps, gs, torch.float64)
    p32, m32, _, _, _ = train_ref.adam_run(ps, gs, torch.float32)
    train_ref.assert_within(opt.state[q]["exp_avg"], m64[1], m32[1], "replaced exp_avg")
    train_ref.assert_within(q, p64[1], p32[1], "p after the replacement")


def test_clip_grad_norm_without_gradients():
    from hetersumgraph_amd import optim
    a = torch.nn.Parameter(torch.zeros(4, device=DEV))
    norm = optim.clip_grad_norm_([a], 1.0)
    assert norm.is_cuda and norm.dim() == 0 and float(norm) == 0.0


def test_unequal_steps_are_refused():
    from hetersumgraph_amd import optim
    ps, gs = host_data([5, 3], 1, seed=10)
    topt = train_ref.adam_run(ps, gs, torch.float32)[4]
    sd = topt.state_dict()
    sd["state"][1]["step"] = sd["state"][1]["step"] + 1
    opt = optim.Adam(Layout(ps, "separate").params)
    with pytest.raises(ValueError, match="one step count"):
        opt.load_state_dict(sd)


def test_graph_capture_and_refresh():
    """One step() captured on a single stream (a linear graph) and replayed over static
    gradient tensors is bitwise the eager steps; the step count advances on the device;
    refresh() carries a new learning rate into the replays."""
    from hetersumgraph_amd import optim
    sizes = [1, 5, 65, CHUNK + 1]
    ps, gs = host_data(sizes, 6, seed=11)
    eager, graphed = Layout(ps, "separate"), Layout(ps, "flat")
    oe = optim.Adam(eager.params, lr=1e-2, max_grad_norm=1.0)
    og = optim.Adam(graphed.params, lr=1e-2, max_grad_norm=1.0)
    stale = Layout(ps, "separate")
    os_ = optim.Adam(stale.params, lr=1e-2, max_grad_norm=1.0)

    def eager_step(i):
        eager.set_grads(gs[i])
        oe.step()

    eager_step(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.set_grads(gs[0])
        og.step()                                     # allocates the state and the workspace
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        og.step()
    for i in (1, 2, 3):
        graphed.set_grads(gs[i])
        g.replay()
        eager_step(i)
    assert bitwise([q.detach() for q in graphed.params], [q.detach() for q in eager.params])
    assert og.step_count() == oe.step_count() == 4
    for o in (oe, og):
        o.param_groups[0]["lr"] = 1e-3
    og.refresh()
    graphed.set_grads(gs[4])
    g.replay()
    eager_step(4)                                     # an eager step pushes the change itself
    assert bitwise([q.detach() for q in graphed.params], [q.detach() for q in eager.params])
    assert bitwise([og.state[a]["exp_avg_sq"] for a in graphed.params], [oe.state[a]["exp_avg_sq"] for a in eager.params])
    # ... and the change took effect: the old rate gives other parameters
    for i in range(5):
        stale.set_grads(gs[i])
        os_.step()
    assert not bitwise([q.detach() for q in graphed.params], [q.detach() for q in stale.params])
    assert og.step_count() == 5
    graphed.assert_gaps_untouched()


def test_constructor_refusals():
    from hetersumgraph_amd import optim
    a, b = (torch.nn.Parameter(torch.zeros(4, device=DEV)) for _ in range(2))
    with pytest.raises(ValueError):
        optim.Adam([{"params": [a]}, {"params": [b]}])
    with pytest.raises(ValueError):
        optim.Adam([a], amsgrad=True)
    with pytest.raises(ValueError):
        optim.Adam([a], maximize=True)
    with pytest.raises(RuntimeError):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.bfloat16))])
    with pytest.raises(RuntimeError):
        optim.Adam([torch.nn.Parameter(torch.zeros(4))])                     # not on the device
    with pytest.raises(RuntimeError):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, 4, device=DEV).t())])  # not contiguous
    c = torch.nn.Parameter(torch.zeros(4, 4, device=DEV))
    opt = optim.Adam([c])
    c.grad = torch.zeros(4, 4, device=DEV).t()                               # gradients: at the first step
    with pytest.raises(RuntimeError):
        opt.step()
