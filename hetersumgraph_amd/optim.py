"""Gradient clipping and Adam of train.py:132-135 on the native multi-tensor kernels
(C ABI: hsg_mt_sqnorm / hsg_mt_adam, include/hsg_train.h, csrc/hsg_train.hip).

Reference: ``torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)`` followed
by ``torch.optim.Adam.step()``.  :class:`Adam` does both in two kinds of launch over all
parameters at once: a squared-norm pass that leaves one partial per 4,096-element chunk,
and an update pass in which every block sums those partials in the same fixed order,
forms the clip coefficient and applies torch's Adam arithmetic to ``coef * grad``.  The
table of tensors travels in the kernel arguments, the hyper-parameters and the step count
live in a small device buffer, and nothing synchronises or allocates after the first
step -- so a step can be captured in a HIP graph and replayed (the step count advances on
the device; :meth:`Adam.refresh` pushes a changed learning rate between replays).

One divergence from the reference sequence: with ``max_grad_norm`` folded into the
optimizer, ``.grad`` is left UNSCALED (the kernel reads it as const).  The stand-alone
:func:`clip_grad_norm_` has torch's in-place semantics.

There is no fallback: parameters or gradients that are not contiguous fp32 on a ROCm
device raise.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import HsgMtTensor, check, load, stream_of

_NO_BLOCKS = ctypes.c_size_t(-1).value


def _table(entries):
    """ctypes array of hsg_mt_tensor from (p, g, m, v, n) data pointers."""
    arr = (HsgMtTensor * max(len(entries), 1))()
    for d, (p, g, m, v, n) in zip(arr, entries):
        d.p, d.g, d.m, d.v, d.n = p, g, m, v, n
    return arr


def _check_tensor(t, what, device=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.is_sparse):
        raise RuntimeError(f"{what} must be a contiguous fp32 tensor on a ROCm device (no fallback)")
    if device is not None and t.device != device:
        raise RuntimeError(f"{what} is on {t.device}, the other parameters on {device}")


def _blocks(arr, T):
    nb = load().hsg_mt_blocks(arr, T)
    if nb == _NO_BLOCKS:
        raise RuntimeError("hsg_mt_blocks: invalid tensor table")
    return int(nb)


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (one param group, no amsgrad / maximize) with the gradient
    clip of train.py:132-133 folded in: ``max_grad_norm=None`` is plain Adam.

    ``last_grad_norm`` is a device scalar holding the last step's total gradient norm
    (before clipping).  ``state_dict`` / ``load_state_dict`` use ``torch.optim.Adam``'s
    layout, so checkpoints move between the two in both directions; the step count is one
    per optimizer here, so a dict whose per-parameter steps differ is refused."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None,
                 amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise ValueError("hetersumgraph_amd.optim.Adam: amsgrad and maximize are not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError(f"Invalid max_grad_norm value: {max_grad_norm}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                        amsgrad=False, maximize=False)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("hetersumgraph_amd.optim.Adam: one param group only")
        ps = self.param_groups[0]["params"]
        if not ps:
            raise ValueError("hetersumgraph_amd.optim.Adam: no parameters")
        for p in ps:
            _check_tensor(p.data, "every parameter", ps[0].device)
        self._device = ps[0].device
        self._hyper = torch.zeros(8, dtype=torch.float64, device=self._device)
        self._stage = torch.zeros(6, dtype=torch.float64).pin_memory()
        self._staged = torch.cuda.Event()
        self._pushed = None
        self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=self._device)
        self._key = self._arr = self._partials = None
        self._updated = []
        self._T = 0
        self.refresh()

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("hetersumgraph_amd.optim.Adam: one param group only")
        super().add_param_group(param_group)

    # --- hyper-parameters ----------------------------------------------------------
    def _host_hyper(self):
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("hetersumgraph_amd.optim.Adam: amsgrad and maximize are not supported")
        mgn = g.get("max_grad_norm")
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                float(g["weight_decay"]), -1.0 if mgn is None else float(mgn))

    def refresh(self):
        """Push ``param_groups[0]``'s hyper-parameters to the device buffer the kernels
        read (a stream-ordered copy from pinned memory; the host waits only for its own
        previous push to have left that buffer, never for the device's work).  Eager steps
        do this themselves when something changed; between replays of a captured step the
        caller does."""
        h = self._host_hyper()
        self._staged.synchronize()               # the previous push has left the pinned buffer
        self._stage.copy_(torch.tensor(h, dtype=torch.float64))
        self._hyper[:6].copy_(self._stage, non_blocking=True)
        self._staged.record(torch.cuda.current_stream(self._device))
        self._pushed = h

    # --- the tensor table ----------------------------------------------------------
    def _table_key(self, ps):
        """The pointers the cached table holds: parameter, gradient, exp_avg, exp_avg_sq
        (0 where the state does not exist yet)."""
        key = []
        for p in ps:
            st = self.state.get(p) or {}
            m, v = st.get("exp_avg"), st.get("exp_avg_sq")
            key.append((p.data_ptr(), p.grad.data_ptr(), 0 if m is None else m.data_ptr(),
                        0 if v is None else v.data_ptr()))
        return tuple(key)

    def _prepare(self):
        """Rebuild the descriptor table when any pointer in it changed: a new ``.grad``
        tensor (``zero_grad(set_to_none=True)`` where the allocator hands out another
        block), a reassigned parameter, or a state tensor replaced by any route."""
        ps = [p for p in self.param_groups[0]["params"] if p.grad is not None]
        if self._table_key(ps) == self._key:
            return
        entries = []
        for p in ps:
            _check_tensor(p.data, "every parameter", self._device)
            _check_tensor(p.grad, "every gradient", self._device)
            if p.grad.shape != p.shape:
                raise RuntimeError("a gradient's shape differs from its parameter's")
            st = self.state[p]
            if "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            for k in ("exp_avg", "exp_avg_sq"):
                _check_tensor(st[k], k, self._device)
                if st[k].numel() != p.numel():
                    raise RuntimeError(f"{k} has {st[k].numel()} elements, its parameter {p.numel()}")
            entries.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                            p.numel()))
        arr = _table(entries)
        nb = _blocks(arr, len(entries))
        if self._partials is None or self._partials.numel() < nb:
            self._partials = torch.empty(max(nb, 1), dtype=torch.float32, device=self._device)
        self._arr, self._T, self._key = arr, len(entries), self._table_key(ps)
        self._updated = ps

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._host_hyper() != self._pushed:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("hyper-parameters changed: call refresh() before capturing a step")
            self.refresh()
        self._prepare()
        if self._T == 0:
            return loss
        lib, st = load(), stream_of(self._hyper)
        check(lib.hsg_mt_sqnorm(self._arr, self._T, self._partials.data_ptr(), self._hyper.data_ptr(), st),
              "hsg_mt_sqnorm")
        check(lib.hsg_mt_adam(self._arr, self._T, self._partials.data_ptr(), self._hyper.data_ptr(), 0,
                              self.last_grad_norm.data_ptr(), st), "hsg_mt_adam")
        # the kernels write through raw pointers: move the version counters as an in-place op would
        # (host-only), so that anything keyed on them (cnn.VocabTable) sees the step
        torch.autograd.graph.increment_version(self._updated)
        return loss

    # --- checkpoints in torch.optim.Adam's layout -------------------------------------
    def step_count(self) -> int:
        """The number of steps taken (read back from the device: synchronises)."""
        return int(self._hyper[6].item())

    def state_dict(self):
        sd = super().state_dict()
        step = float(self.step_count())
        sd["state"] = {k: dict(st, step=torch.tensor(step, dtype=torch.float32)) for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        steps = {float(st["step"]) for st in state_dict["state"].values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"hetersumgraph_amd.optim.Adam keeps one step count; the state dict has {sorted(steps)}")
        for g in state_dict["param_groups"]:
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("hetersumgraph_amd.optim.Adam: amsgrad and maximize are not supported")
        mgn = self.param_groups[0].get("max_grad_norm")
        super().load_state_dict(state_dict)
        self.param_groups[0].setdefault("max_grad_norm", mgn)
        for st in self.state.values():
            st.pop("step", None)
        self._hyper[6] = steps.pop() if steps else 0.0
        self._key = None
        self.refresh()


def clip_grad_norm_(parameters, max_norm):
    """``torch.nn.utils.clip_grad_norm_`` (2-norm) on the native kernels: scales every
    ``.grad`` in place by ``min(1, max_norm / (total_norm + 1e-6))`` and returns the total
    norm as a scalar on the parameters' device (zero when no parameter has a gradient).
    Two kinds of launch, no synchronisation; each call allocates its small workspace
    (partials, an 8-double hyper buffer, the norm) from torch's caching allocator."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros((), dtype=torch.float32, device=parameters[0].device if parameters else None)
    dev = grads[0].device
    for g in grads:
        _check_tensor(g, "every gradient", dev)
    arr = _table([(g.data_ptr(), g.data_ptr(), None, None, g.numel()) for g in grads])
    nb = _blocks(arr, len(grads))
    partials = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
    hyper = torch.zeros(8, dtype=torch.float64, device=dev)
    hyper[5] = float(max_norm)
    norm = torch.zeros((), dtype=torch.float32, device=dev)
    lib, st = load(), stream_of(hyper)
    check(lib.hsg_mt_sqnorm(arr, len(grads), partials.data_ptr(), None, st), "hsg_mt_sqnorm")
    check(lib.hsg_mt_adam(arr, len(grads), partials.data_ptr(), hyper.data_ptr(), 1, norm.data_ptr(), st),
          "hsg_mt_adam")
    return norm
