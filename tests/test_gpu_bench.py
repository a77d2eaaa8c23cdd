"""bench.py's secondary end-to-end line: one whole train.py iteration (HSumGraph /
HSumDocGraph forward with the sentence encoder, cross entropy, backward, Adam) runs
on a small synthetic batch and returns a positive step time."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("config", ["cfg2", "cfg4"])
def test_e2e_train_step_runs(config):
    import bench
    from hetersumgraph_amd import graph as hg
    from hetersumgraph_amd import synth
    docs = synth.make_batch_docs(config, seed=3, n_docs=3)
    G = hg.batch([synth.to_graph(d, hg.DGLGraph) for d in docs])
    dev = torch.device("cuda", 0)
    G.to(dev)
    dt = bench.time_train_step(G, config, 2, steps=2, warmup=1, dev=dev)
    assert np.isfinite(dt) and dt > 0


def test_bench_json_contract(tmp_path):
    """`python bench.py --full` prints ONE JSON line with the driver's keys, the roofline
    and cpu_baseline objects, and a value consistent with its own step time (short run,
    bounded CPU sample)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1",
                          "--full", "--no-e2e", "--cpu-docs", "1", "--cpu-steps", "1", "--kernel-reps", "5",
                          "--kernel-steps", "2"],
                         cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert abs(d["value"] - d["config"]["graph_edges_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["algorithmic_bytes_per_launch"] < r["algorithmic_bytes_per_launch"] + r["epilogue_bytes_per_launch"]
    e = d["edge_aggregate"]
    assert 0 < e["frac"] < 1 and set(e["kernels"]) == {"gat_fwd_W2S", "gat_fwd_S2W", "gat_bwd_W2S", "gat_bwd_S2W"}
    assert e["kernels"]["gat_fwd_S2W"]["launches_per_step"] == 2 and e["kernels"]["gat_fwd_W2S"]["launches_per_step"] == 3
    f = d["full_stack"]
    assert 0 < f["frac"] < 1 and f["floor_us"] > f["dense_floor_us"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["host_cores_visible"] >= c["cores"]


def test_bench_plain_run_and_dump(tmp_path):
    """A plain `python bench.py` times its steps and nothing else: the result line has
    the headline keys and none of the --full objects.  `--dump-outputs` writes the last
    timed step's stack output and gradients as finite fp32 arrays of the step's shapes."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(dump)],
                         cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    for k in ("roofline", "edge_aggregate", "full_stack", "roofline_dense", "e2e_train_step", "cpu_baseline"):
        assert k not in d, k
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["config"]["hip_graph"] is True
    assert abs(d["value"] - d["config"]["graph_edges_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    arrs = {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump))}
    assert {"stack_out", "grad_Xs", "grad__TFembed.weight"} <= set(arrs)
    for layer in ("word2sent", "sent2word"):
        assert any(n.startswith(f"grad_{layer}.") for n in arrs), layer
    assert arrs["stack_out"].shape == arrs["grad_Xs"].shape == (32 * 35, 64)       # cfg2: 32 docs x 35 sentences
    assert arrs["grad__TFembed.weight"].shape == (10, 50)
    for name, a in arrs.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    for name in ("stack_out", "grad_Xs", "grad__TFembed.weight"):
        assert np.abs(arrs[name]).max() > 0, name
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
