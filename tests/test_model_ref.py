"""tests/model_ref.py on the CPU: the whole-model oracle is pinned before it judges the GPU
step (test_gpu_model_train.py).

* Eval mode against the reference's own run (the goldens model_hsg / model_hdsg): logits,
  loss, every stored gradient and every stored gradient projection.
* The three-step train trajectory of test_gpu_model_train.py run entirely here -- fp64
  gradients into torch's clip_grad_norm_ 1.0 + Adam 5e-4, every mask restated from
  (S + k + 1, offset) -- with, at every step,
  - attainability: a plain fp32 restatement of the oracle stays within ONE TENTH of the
    bounds the GPU test applies (logits 1e-4, gradients 2e-3 of the largest entry);
  - sensitivity: a draw taken at a wrong offset, two consumers sharing a draw, eval in place
    of train, or the previous step's parameters move the logits and some gradient by more
    than 100 x those bounds, so a GPU step that composes the pieces wrongly is far outside.
"""
import numpy as np
import pytest
import torch

import model_ref as M
from helpers import load_fixture, projections

LOGIT_TOL, GRAD_TOL = 1e-4, 2e-3         # the GPU test's bounds (test_gpu_model.py's contract)


@pytest.mark.parametrize("name,cls,seed", M.CASES)
def test_eval_mode_matches_the_goldens(name, cls, seed):
    z = load_fixture(name)
    snap = M.snapshot(M.make_model(cls, seed, z))
    o = M.oracle_at(z, z["sent_words"], snap, cls)
    err = np.abs(o["logits"].numpy() - z["logits64"]).max()
    print(f"{name}: logits {err:.3e} loss {abs(o['loss'].item() - float(z['loss64'])):.3e}")
    assert err <= 1e-6                                     # the golden stores logits64 as float32
    assert abs(o["loss"].item() - float(z["loss64"])) <= 1e-9
    n, worst = 0, 0.0
    for k, g in o["grads"].items():
        key = f"grad.{k}"
        if key in z:
            got, ref = g.numpy(), z[key].astype(np.float64)
        else:
            got, ref = projections(g, seed, key), z["proj." + key]
        # of its largest entry, with test_gpu_model.py's floor: HSG's S2W feat_fc.bias gradient is
        # zero in exact arithmetic (a word has no phantom in-edge, so its softmax terms cancel) and
        # the golden holds 1e-19 there
        e = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-3)
        assert e <= 1e-6, (k, e)
        worst, n = max(worst, e), n + 1
    print(f"{name}: {n} gradients, worst {worst:.3e} of the largest entry")
    assert n >= 90
    assert n == sum(k.startswith(("grad.", "proj.grad.")) for k in z)       # every stored one


def test_snapshot_owns_its_values_and_reruns_do_not_accumulate():
    name, cls, seed = M.CASES[0]
    z = load_fixture(name)
    model = M.make_model(cls, seed, z)
    snap = M.snapshot(model)
    assert snap["ngram_enc.embed.weight"] is snap["_embed.weight"]
    assert set(M.trainable(snap)) == {k for k in snap if k not in M.FROZEN and k not in M.SHARED}
    a = M.oracle_at(z, z["sent_words"], snap, cls)
    before = {k: v.detach().clone() for k, v in snap.items()}
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    assert all(torch.equal(before[k], snap[k]) for k in before)
    b = M.oracle_at(z, z["sent_words"], snap, cls)
    assert a["grads"].keys() == b["grads"].keys() == M.trainable(snap).keys()
    assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])


def _moves(o, base):
    """(max |logit difference|, worst gradient difference over its largest entry)."""
    return ((o["logits"] - base["logits"]).abs().max().item(), M.worst_grad_error(o["grads"], base["grads"], 1.0))


@pytest.fixture(scope="module", params=M.CASES, ids=[c[0] for c in M.CASES])
def trajectory(request):
    """Three train-mode steps of one case in fp64, leg B's draws (LSTM dropout on).  Per
    step: the fp32 restatement's errors and what each wrong composition moves."""
    name, cls, seed = request.param
    z = load_fixture(name)
    words = M.short_sentence(z)
    snap = M.snapshot(M.make_model(cls, seed, z))
    leaves = M.trainable(snap)
    opt = torch.optim.Adam(list(leaves.values()), lr=M.LR)
    n_iter = int(z.get("n_iter", 2))
    steps, prev = [], None
    for k in range(3):
        draws = (M.SEEDS[name] + k + 1, k * M.n_draws(n_iter, 1), M.P_STACK, M.P_LSTM)
        run = lambda s=snap, **kw: M.oracle_at(z, words, s, cls, **kw)
        o64 = run(draws=draws)
        o32 = run(M.recast(snap, torch.float32), draws=draws)
        assert o64["logits"].dtype == torch.float64 and o32["logits"].dtype == torch.float32
        rec = dict(k=k, logits=(o32["logits"].double() - o64["logits"]).abs().max().item(),
                   grads=M.worst_grad_error(o32["grads"], o64["grads"], 1.0), wrong={})
        right = M.step_masks(z, draws)
        rec["wrong"]["LSTM mask one offset late"] = _moves(run(masks=M.step_masks(z, draws, lstm_shift=1)), o64)
        # the first application's two masks one offset late, the other applications' as they are
        late = M.step_masks(z, draws, stack_shift=1)[1]
        rec["wrong"]["first stack masks one offset late"] = _moves(run(masks=(right[0], late[:1] + right[1][1:])), o64)
        # the stack's first draw handed the offset the LSTM already took
        rec["wrong"]["LSTM and first head mask share an offset"] = _moves(
            run(masks=(right[0], M.step_masks(z, draws, stack_shift=-1)[1])), o64)
        rec["wrong"]["eval in place of train"] = _moves(run(), o64)
        if prev is not None:
            rec["wrong"]["previous step's parameters"] = _moves(run(prev, draws=draws), o64)
        steps.append(rec)
        prev = M.recast(snap, torch.float64)
        o64 = run(draws=draws)                              # the runs above cleared the leaves' gradients
        assert o64["grads"].keys() == leaves.keys()
        for key, leaf in leaves.items():
            leaf.grad = o64["grads"][key].clone()
        torch.nn.utils.clip_grad_norm_(list(leaves.values()), M.MAX_NORM)
        opt.step()
        assert all(not torch.equal(prev[key], leaf) for key, leaf in leaves.items()
                   if leaf.grad.abs().max().item() > 1e-6)
    return name, steps


def test_fp32_restatement_stays_within_a_tenth_of_the_gpu_bounds(trajectory):
    name, steps = trajectory
    for rec in steps:
        print(f"{name} step {rec['k']}: fp32 restatement logits {rec['logits']:.3e}, "
              f"gradients {rec['grads']:.3e} of the largest entry")
        assert rec["logits"] <= LOGIT_TOL / 10
        assert rec["grads"] <= GRAD_TOL / 10


def test_wrong_compositions_are_far_outside_the_gpu_bounds(trajectory):
    name, steps = trajectory
    for rec in steps:
        assert len(rec["wrong"]) == (5 if rec["k"] else 4)
        for what, (dl, dg) in rec["wrong"].items():
            print(f"{name} step {rec['k']}: {what}: logits move {dl:.3e}, worst gradient entry {dg:.3e}")
            # at the dropout seeds model_ref.SEEDS records
            assert dl > 100 * LOGIT_TOL, (what, dl)
            assert dg > 100 * GRAD_TOL, (what, dg)
