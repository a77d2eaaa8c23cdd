"""Oracle and yardstick of the training-step tail's tests (test_gpu_doc_ce.py,
test_gpu_optim.py, test_gpu_train_guard.py, test_gpu_train_tail_model.py).

The oracle is torch on the CPU in fp64 -- ``F.cross_entropy`` + ``index_add`` + ``mean``,
``clip_grad_norm_``, ``torch.optim.Adam(foreach=False)`` -- and the yardstick the same
code in fp32.  The native result must lie within TWICE the yardstick's own error against
the oracle (its maximum over the tensor), floored at 4 fp32 ulp of the oracle's value:
the kernels' sum order and exp / log forms differ from ATen's by rounding only.
"""
import copy

import torch
import torch.nn.functional as F

CHUNK = 4096          # elements per block of the multi-tensor kernels (asserted against hsg_mt_chunk())
SIZES = [1, 2, 3, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 153600]


def ulp32(x):
    """fp32 spacing at |x| (x: fp64 tensor), the subnormal spacing 2^-149 at the least."""
    a = x.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23).clamp_min(2.0 ** -149)


def excess(got, ref64, yard32):
    """(max error of got, max error of the yardstick, worst got-error / allowed) against
    the fp64 oracle.  NaN / Inf positions must coincide and are excluded from the errors."""
    got, ref64, yard = got.detach().cpu().double(), ref64.detach().cpu().double(), yard32.detach().cpu().double()
    assert got.shape == ref64.shape == yard.shape, (got.shape, ref64.shape, yard.shape)
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), "NaN positions differ from the oracle's"
    assert torch.equal(got[~fin & ~torch.isnan(ref64)], ref64[~fin & ~torch.isnan(ref64)]), "Inf positions differ"
    if not bool(fin.any()):
        return 0.0, 0.0, 0.0
    e_got = (got - ref64)[fin].abs()
    e_yard = (yard - ref64)[fin & torch.isfinite(yard)].abs()
    yard_max = float(e_yard.max()) if e_yard.numel() else 0.0
    allowed = torch.maximum(torch.full_like(e_got, 2.0 * yard_max), 4.0 * ulp32(ref64[fin]))
    return float(e_got.max()), yard_max, float((e_got / allowed).max())


def assert_within(got, ref64, yard32, what):
    e, y, worst = excess(got, ref64, yard32)
    print(f"{what}: max err {e:.3e}, fp32 torch max err {y:.3e}, worst err / allowed {worst:.3f}")
    assert worst <= 1.0, f"{what}: error {e:.3e} exceeds max(2 x {y:.3e}, 4 ulp) by a factor {worst:.3f}"
    return e, y


# ---- loss ---------------------------------------------------------------------------
def doc_ce(logits, labels, lens, dtype, upstream=1.0):
    """train.py:117-119 on the CPU in `dtype`: (row_loss [n], doc_loss [B], mean, dlogits)
    with dlogits the gradient of upstream * mean."""
    z = logits.detach().cpu().to(dtype).requires_grad_()
    row = F.cross_entropy(z, labels.cpu(), reduction="none")
    gid = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens, dtype=torch.int64))
    doc = torch.zeros(len(lens), dtype=dtype).index_add(0, gid, row)
    mean = doc.mean()
    (mean * upstream).backward()
    return row.detach(), doc.detach(), mean.detach(), z.grad


def offsets(lens):
    off = torch.zeros(len(lens) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0)
    return off


# ---- clip + Adam ----------------------------------------------------------------------
def adam_run(params, grads_per_step, dtype, max_norm=None, state=None, **hyper):
    """Steps of clip_grad_norm_ (when max_norm is given) + torch.optim.Adam(foreach=False)
    on the CPU in `dtype`.  params: list of tensors; grads_per_step: list (steps) of lists
    of tensors (None: that parameter has no gradient).  state: a torch state_dict to start
    from (left unchanged).  Returns (p, m, v lists -- m / v None for a parameter without
    state --, norms, the optimizer)."""
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
    opt = torch.optim.Adam(ps, foreach=False, **hyper)
    if state is not None:
        # load_state_dict keeps the caller's `step` tensors, which step() then advances in place
        opt.load_state_dict(copy.deepcopy(state))
    norms = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.detach().cpu().to(dtype).clone()
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False).detach().clone())
        opt.step()
    m = [opt.state[p]["exp_avg"] if p in opt.state and len(opt.state[p]) else None for p in ps]
    v = [opt.state[p]["exp_avg_sq"] if p in opt.state and len(opt.state[p]) else None for p in ps]
    return [p.detach() for p in ps], m, v, norms, opt
