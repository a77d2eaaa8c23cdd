"""tests/step_ref.py on the CPU: the oracle at a module's current parameters, and the
oracle-only trajectory the multi-step GPU tests (test_gpu_second_step.py) rely on.

* At the seeded parameters ``oracle_at(snapshot(...))`` is ``oracle_stack`` bit for bit.
* Three steps of train.py's tail in fp64 (clip_grad_norm_ 1.0, Adam lr 5e-4, R_k from
  default_rng(seed + k)) on cfg2[:4] and cfg4[:2]:
  - discrimination: from one step to the next every row of the stack's output moves by
    at least 1000 x 2e-5 and the edge logits by at least 1000 x 1e-4 (max over edges),
    so a GPU step that computed from ANY stale piece of the previous step's state is a
    thousand times outside the bounds the GPU tests apply;
  - attainability: the same oracle in fp32 (fp32 parameters and inputs) goes through
    test_gpu_stack_parity.compare against the fp64 run at every step -- the existing
    fp32 bounds and allowance hold at moved parameters for a plain fp32 restatement,
    established without consulting the code under test.
"""
import pytest
import torch

import step_ref
from helpers import gat_inputs, seeded_gat_params
from test_gpu_stack_parity import compare, oracle_stack

N_ITER = 2


def test_oracle_at_seeded_parameters_is_oracle_stack():
    seed = 31
    z, _, _ = step_ref.workload("cfg2")
    o = oracle_stack(z, seed, n_iter=N_ITER)
    w2s, s2w = seeded_gat_params(seed * 100 + 1, seed * 100 + 2)
    Xw, Xs, T = gat_inputs(seed, int(z["n_w"]), int(z["n_s"]))
    snap = step_ref.snapshot(w2s, s2w, T)
    a = step_ref.oracle_at(z, snap, Xw, Xs, o["R"], N_ITER)
    for k in ("s", "Xw", "Xs", "T"):
        assert torch.equal(a[k], o[k]), k
    for tag in ("p1", "p2"):
        assert a[tag].keys() == o[tag].keys()
        for k in o[tag]:
            assert torch.equal(a[tag][k], o[tag][k]) and torch.equal(a[tag][k].grad, o[tag][k].grad), (tag, k)
    # the snapshot owns its values: moving the module in place does not reach it
    before = {k: v.detach().clone() for k, v in snap[0].items()}
    with torch.no_grad():
        for p in w2s.parameters():
            p.add_(1.0)
    assert all(torch.equal(before[k], snap[0][k]) for k in before)
    # ... and a second run on the same snapshot does not accumulate into the first's gradients
    b = step_ref.oracle_at(z, snap, Xw, Xs, o["R"], N_ITER)
    assert all(torch.equal(b["p1"][k].grad, o["p1"][k].grad) for k in o["p1"])


@pytest.mark.parametrize("config", list(step_ref.WORKLOADS))
def test_oracle_trajectory_discriminates_and_fp32_bounds_attainable(config):
    seed = step_ref.SEEDS[config]
    z, n_docs, n_edges = step_ref.workload(config)
    n_w, n_s = int(z["n_w"]), int(z["n_s"])
    w2s, s2w = seeded_gat_params(seed * 100 + 1, seed * 100 + 2)
    Xw, Xs, T = gat_inputs(seed, n_w, n_s)
    snap = step_ref.snapshot(w2s, s2w, T)             # the fp64 leaves the trajectory moves
    opt = torch.optim.Adam(step_ref.leaves(snap), lr=step_ref.LR)
    outs, cols = [], []
    for k in range(3):
        R = step_ref.upstream(seed, k, n_s)
        # the fp32 restatement first: the fp64 run follows its ReLU gates inside the fp32
        # band around zero, exactly as it follows the GPU's in the GPU tests
        o32 = step_ref.oracle_at(z, step_ref.recast(snap, torch.float32), Xw, Xs, R, N_ITER, want_gates=True)
        o64 = step_ref.oracle_at(z, snap, Xw, Xs, R, N_ITER, gates=o32["gates"])
        assert o32["s"].dtype == torch.float32 and o64["s"].dtype == torch.float64
        compare(f"{config} step {k} (fp32 oracle)", "f32", step_ref.as_run(o32), o64, n_docs, n_edges)
        outs.append(o64["s"])
        cols.append(step_ref.edge_column_at(z, snap, Xw, Xs, N_ITER).double())
        assert all(t.grad is not None for t in step_ref.leaves(snap))
        torch.nn.utils.clip_grad_norm_(step_ref.leaves(snap), step_ref.MAX_NORM)
        opt.step()
    for k in (1, 2):
        rows = (outs[k] - outs[k - 1]).abs().max(1).values
        col = (cols[k] - cols[k - 1]).abs().max().item()
        print(f"{config} step {k}: output rows move by >= {rows.min().item():.3f} (max {rows.max().item():.3f}), "
              f"edge logits by {col:.3f}")
        assert rows.min().item() >= 1000 * 2e-5
        assert col >= 1000 * 1e-4
