"""Dev tool (GPU): where the secondary end-to-end train step (bench.time_train_step)
spends its time on cfg2 -- synchronised wall time per phase, then the same step
under torch.profiler for the host/device split.

    python tools/e2e_profile.py [cfg] [--sent-lstm 0|1|2|ab|ab2] [--tail 0|1|ab] [--glue 0|1|ab]
                                [--embed-train 0|1|ab] [--sent-cnn 0|dw|tokens|ab] [--no-profile]

--sent-lstm selects the sentence LSTM path (path_options(HSG_SENT_LSTM=...): 0 = the
vendor nn.LSTM, 1 = the native recurrence kernels of hetersumgraph_amd.lstm).  ``ab``
alternates the two three times in this one process and prints, per leg, one JSON line
with the phase times plus the LSTM piece's forward and backward timed alone.  2 = the
native kernels with the parameters packed by one launch and one weight-gradient kernel
per layer (hetersumgraph_amd.lstm.sent_lstm(..., fused=True)); ``ab2`` alternates 1 and 2
the same way, with --tail, --glue, --embed-train and --sent-cnn (each 0 / 1 / a path name,
not ab) applied to both legs.

--tail selects the step's tail (train.py:115-135 with --grad_clip at max_grad_norm = 1.0,
phases ``loss``, ``clip``, ``adam``): 0 = torch cross entropy + sum_nodes,
clip_grad_norm_, torch.optim.Adam with its defaults; 1 = the native tail
(hetersumgraph_amd.loss.sentence_loss, hetersumgraph_amd.optim.Adam with the clip folded
in, so its ``clip`` phase is empty); ``ab`` alternates leg 0, leg 1 and -- where this torch
accepts it -- leg ``fused`` (leg 0 with torch.optim.Adam(fused=True)) three times in this
one process, one JSON line per leg.  Without --tail the step is the one this tool always
timed (no clipping).

--glue selects the model glue (path_options(HSG_MODEL_GLUE=...): 0 = the torch ops of
HiGraph.py, 1 = the native kernels of hetersumgraph_amd.head).  With --glue the forward is
timed as ``model(G)`` in ONE phase, ``forward``, so both legs measure the same thing;
``ab`` alternates leg 0 and leg 1 three times in this one process, one JSON line per leg,
with --sent-lstm and --tail (0 or 1) applied to both.

--embed-train trains the word embedding (train.py:342 ``--embed_train``): the embedding's
``requires_grad`` is set and it joins the optimizer's parameters.  0 = the torch path
(nn.Embedding's dense backward, the CNN's index_add_ scatter, autograd's sum of the two
[V, 300] buffers), 1 = path_options(HSG_WORD_EMBED="1"), the native node and reduce of
hetersumgraph_amd.wordembed; ``ab`` alternates leg 0 and leg 1 three times in this one
process, one JSON line per leg, with --sent-lstm, --tail and --glue (0 or 1) applied to
both.

--sent-cnn selects the sentence CNN path (path_options(HSG_SENT_CNN=...), frozen embedding:
0 = today's gather / GEMM / pool and dY^T X, dw = the sparse weight gradient, tokens = also
the forward on the batch's distinct tokens).  ``ab`` alternates the three legs three times
in this one process, one JSON line per leg -- forward, backward and the whole iteration,
plus the encoder's forward and backward timed alone and the batch's distinct-token count U
against the row count of today's GEMM -- with --sent-lstm, --tail and --glue (0 or 1)
applied to all."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from hetersumgraph_amd import HiGraph  # noqa: E402
from hetersumgraph_amd import _lib  # noqa: E402
from hetersumgraph_amd import graph as hg  # noqa: E402
from hetersumgraph_amd import loss as hloss  # noqa: E402
from hetersumgraph_amd import optim as hoptim  # noqa: E402

ARGS = sys.argv[1:]
SENT_LSTM = ARGS[ARGS.index("--sent-lstm") + 1] if "--sent-lstm" in ARGS else "0"
if SENT_LSTM not in ("0", "1", "2", "ab", "ab2"):
    sys.exit("--sent-lstm takes 0, 1, 2, ab or ab2")
TAIL = ARGS[ARGS.index("--tail") + 1] if "--tail" in ARGS else None
if TAIL not in (None, "0", "1", "ab"):
    sys.exit("--tail takes 0, 1 or ab")
GLUE = ARGS[ARGS.index("--glue") + 1] if "--glue" in ARGS else None
if GLUE not in (None, "0", "1", "ab"):
    sys.exit("--glue takes 0, 1 or ab")
EMBED_TRAIN = ARGS[ARGS.index("--embed-train") + 1] if "--embed-train" in ARGS else None
if EMBED_TRAIN not in (None, "0", "1", "ab"):
    sys.exit("--embed-train takes 0, 1 or ab")
SENT_CNN = ARGS[ARGS.index("--sent-cnn") + 1] if "--sent-cnn" in ARGS else None
if SENT_CNN not in (None, "0", "dw", "tokens", "ab"):
    sys.exit("--sent-cnn takes 0, dw, tokens or ab")
if [TAIL, SENT_LSTM.replace("ab2", "ab"), GLUE, EMBED_TRAIN, SENT_CNN].count("ab") > 1:
    sys.exit("one of --sent-lstm, --tail, --glue, --embed-train and --sent-cnn can be ab")
PROFILE = "--no-profile" not in ARGS and "ab" not in (SENT_LSTM.replace("ab2", "ab"), TAIL, GLUE, EMBED_TRAIN, SENT_CNN)
POS = [a for i, a in enumerate(ARGS)
       if not a.startswith("--") and (i == 0 or ARGS[i - 1] not in ("--sent-lstm", "--tail", "--glue", "--embed-train",
                                                                    "--sent-cnn"))]
MAX_GRAD_NORM = 1.0

dev = torch.device("cuda", 0)
docs, G, _, _ = bench.make_shard(POS[0] if POS else "cfg2", 0, 1, 0)
G.to(dev)
hps = bench._HPS(2)
torch.manual_seed(1)
embed = torch.nn.Embedding(hps.vocab_size, 300, padding_idx=0)
embed.weight.requires_grad = EMBED_TRAIN is not None
model = HiGraph.HSumGraph(hps, embed).to(dev).train()
PARAMS = [p for p in model.parameters() if p.requires_grad]
opt = torch.optim.Adam(PARAMS, lr=hps.lr)
crit = torch.nn.CrossEntropyLoss(reduction="none")
T = {}
TAIL_LEG = None                  # None: the historical step; "0" / "1" / "fused": see --tail
_TAIL_OPTS = {}


def tail_opt(leg):
    """One optimizer per leg over the same parameters (each keeps its own state)."""
    if leg not in _TAIL_OPTS:
        if leg == "1":
            _TAIL_OPTS[leg] = hoptim.Adam(PARAMS, lr=hps.lr, max_grad_norm=MAX_GRAD_NORM)
        else:
            _TAIL_OPTS[leg] = torch.optim.Adam(PARAMS, lr=hps.lr, **({"fused": True} if leg == "fused" else {}))
    return _TAIL_OPTS[leg]


def fused_adam_ok():
    try:
        tail_opt("fused")
        return True
    except (RuntimeError, ValueError, TypeError) as e:
        print(json.dumps({"fused_leg": "skipped", "reason": str(e)[:200]}), flush=True)
        return False


def tick(name, t0):
    torch.cuda.synchronize()
    t = time.perf_counter()
    T[name] = T.get(name, 0.0) + (t - t0) * 1e3
    return t


def forward_phases(t):
    if GLUE is not None:
        out = model(G)
        return out, tick("forward", t)
    w = model.set_wnfeature(G)
    t = tick("set_wnfeature", t)
    snode_id = HiGraph.node_ids(G, "dtype", 1.0)
    ngram, cnn = model._sent_cnn_feature(G, snode_id)
    t = tick("cnn", t)
    glen = HiGraph.sentence_counts(G)
    lstm = model._sent_lstm_rows(ngram, glen)
    t = tick("lstm", t)
    s = model.n_feature_proj(torch.cat([cnn, lstm], dim=1))
    st = model.gat_stack(G, w, s)
    out = model.wh(st)
    return out, tick("gat_stack", t)


def step(n):
    out, t = forward_phases(time.perf_counter())
    o = opt if TAIL_LEG is None else tail_opt(TAIL_LEG)
    if TAIL_LEG == "1":
        loss = hloss.sentence_loss(G, out)
    else:
        sid = G.filter_nodes(lambda nodes: nodes.data["dtype"] == 1)
        label = G.ndata["label"][sid].sum(-1)
        G.nodes[sid].data["loss"] = crit(out, label).unsqueeze(-1)
        loss = hg.sum_nodes(G, "loss").mean()
    ok = bool(torch.isfinite(loss).item())
    t = tick("loss", t)
    o.zero_grad()
    loss.backward()
    t = tick("backward", t)
    if TAIL_LEG in ("0", "fused"):
        torch.nn.utils.clip_grad_norm_(PARAMS, MAX_GRAD_NORM)
    if TAIL_LEG is not None:
        t = tick("clip", t)              # leg 1: empty, the clip is folded into the optimizer
    o.step()
    t = tick("adam", t)
    if TAIL_LEG != "1":
        G.ndata.pop("loss")


N = 10


def lstm_alone():
    """(forward ms, backward ms) of the LSTM piece alone, synchronised wall time."""
    snode_id = HiGraph.node_ids(G, "dtype", 1.0)
    with torch.no_grad():
        ngram, _ = model._sent_cnn_feature(G, snode_id)
    glen = HiGraph.sentence_counts(G)
    params = list(model.lstm.parameters()) + list(model.lstm_proj.parameters())
    up = torch.randn(ngram.shape[0], model.lstm_proj.out_features, device=dev)
    tf = tb = 0.0
    for i in range(3 + N):
        x = ngram.clone().requires_grad_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model._sent_lstm_rows(x, glen)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        torch.autograd.grad(out, [x] + params, up)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= 3:
            tf, tb = tf + (t1 - t0) * 1e3, tb + (t2 - t1) * 1e3
    return tf / N, tb / N


def cnn_alone():
    """(forward ms, backward ms) of the sentence CNN encoder alone, synchronised wall time."""
    words = G.ndata["words"][HiGraph.node_ids(G, "dtype", 1.0)]
    params = [p for p in model.ngram_enc.convs.parameters()]
    up = torch.randn(words.shape[0], 300, device=dev)
    tf = tb = 0.0
    for i in range(3 + N):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.ngram_enc(words)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        torch.autograd.grad(out, params, up)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= 3:
            tf, tb = tf + (t1 - t0) * 1e3, tb + (t2 - t1) * 1e3
    return tf / N, tb / N


def token_counts():
    """(distinct tokens U with PAD, rows of today's GEMM, sentences) of the batch."""
    words = G.ndata["words"][HiGraph.node_ids(G, "dtype", 1.0)]
    u = torch.unique(torch.cat([words.reshape(-1), words.new_zeros(1)])).numel()
    return u, int((words != 0).sum()) + words.shape[0], words.shape[0]


def leg(mode, **others):
    with _lib.path_options(HSG_SENT_LSTM=mode, **others):
        for _ in range(3):
            step(0)
        T.clear()
        for _ in range(N):
            step(0)
        res = {k: round(v / N, 3) for k, v in T.items()}
        res["total"] = round(sum(T.values()) / N, 3)
        res["lstm_fwd_alone"], res["lstm_bwd_alone"] = (round(v, 3) for v in lstm_alone())
    return res


def tail_leg(mode):
    global TAIL_LEG
    TAIL_LEG = mode
    with _lib.path_options(HSG_SENT_LSTM=SENT_LSTM):
        for _ in range(3):
            step(0)
        T.clear()
        for _ in range(N):
            step(0)
    res = {k: round(v / N, 3) for k, v in T.items()}
    res["tail"] = round(sum(T[k] for k in ("loss", "clip", "adam")) / N, 3)
    res["total"] = round(sum(T.values()) / N, 3)
    return res


if TAIL == "ab":
    legs = ["0", "1"] + (["fused"] if fused_adam_ok() else [])
    for rep_ in range(3):
        for mode in legs:
            print(json.dumps({"rep": rep_, "tail_leg": mode, "HSG_SENT_LSTM": SENT_LSTM, **tail_leg(mode)}), flush=True)
    sys.exit(0)
TAIL_LEG = TAIL
if GLUE == "ab":
    for rep in range(3):
        for mode in ("0", "1"):
            with _lib.path_options(HSG_SENT_LSTM=SENT_LSTM, HSG_MODEL_GLUE=mode):
                for _ in range(3):
                    step(0)
                T.clear()
                for _ in range(N):
                    step(0)
            res = {k: round(v / N, 3) for k, v in T.items()}
            res["total"] = round(sum(T.values()) / N, 3)
            print(json.dumps({"rep": rep, "HSG_MODEL_GLUE": mode, "HSG_SENT_LSTM": SENT_LSTM, "tail_leg": TAIL, **res}),
                  flush=True)
    sys.exit(0)
if EMBED_TRAIN == "ab":
    for rep in range(3):
        for mode in ("0", "1"):
            with _lib.path_options(HSG_SENT_LSTM=SENT_LSTM, HSG_WORD_EMBED=mode,
                                   **({} if GLUE is None else {"HSG_MODEL_GLUE": GLUE})):
                for _ in range(3):
                    step(0)
                T.clear()
                for _ in range(N):
                    step(0)
            res = {k: round(v / N, 3) for k, v in T.items()}
            res["total"] = round(sum(T.values()) / N, 3)
            print(json.dumps({"rep": rep, "HSG_WORD_EMBED": mode, "HSG_SENT_LSTM": SENT_LSTM, "HSG_MODEL_GLUE": GLUE,
                              "tail_leg": TAIL, **res}), flush=True)
    sys.exit(0)
if SENT_CNN == "ab":
    U_, rows_, n_ = token_counts()
    print(json.dumps({"distinct_tokens_U": U_, "gemm_rows_today": rows_, "sentences": n_,
                      "gemm_rows_tokens": U_ + G.ndata["words"].shape[1] + 1}), flush=True)
    for rep in range(3):
        for mode in ("0", "dw", "tokens"):
            with _lib.path_options(HSG_SENT_LSTM=SENT_LSTM, HSG_SENT_CNN=mode,
                                   **({} if GLUE is None else {"HSG_MODEL_GLUE": GLUE}),
                                   **({} if EMBED_TRAIN is None else {"HSG_WORD_EMBED": EMBED_TRAIN})):
                for _ in range(3):
                    step(0)
                T.clear()
                for _ in range(N):
                    step(0)
                res = {k: round(v / N, 3) for k, v in T.items()}
                res["total"] = round(sum(T.values()) / N, 3)
                res["cnn_fwd_alone"], res["cnn_bwd_alone"] = (round(v, 3) for v in cnn_alone())
            print(json.dumps({"rep": rep, "HSG_SENT_CNN": mode, "HSG_SENT_LSTM": SENT_LSTM, "HSG_MODEL_GLUE": GLUE,
                              "tail_leg": TAIL, **res}), flush=True)
    sys.exit(0)
if SENT_LSTM == "ab":
    for rep in range(3):
        for mode in ("0", "1"):
            print(json.dumps({"rep": rep, "HSG_SENT_LSTM": mode, **leg(mode)}), flush=True)
    sys.exit(0)
if SENT_LSTM == "ab2":
    others = dict(**({} if GLUE is None else {"HSG_MODEL_GLUE": GLUE}),
                  **({} if EMBED_TRAIN is None else {"HSG_WORD_EMBED": EMBED_TRAIN}),
                  **({} if SENT_CNN is None else {"HSG_SENT_CNN": SENT_CNN}))
    for rep in range(3):
        for mode in ("1", "2"):
            print(json.dumps({"rep": rep, "HSG_SENT_LSTM": mode, "tail_leg": TAIL, **others, **leg(mode, **others)}),
                  flush=True)
    sys.exit(0)
_mode = _lib.path_options(HSG_SENT_LSTM=SENT_LSTM, **({} if GLUE is None else {"HSG_MODEL_GLUE": GLUE}),
                          **({} if EMBED_TRAIN is None else {"HSG_WORD_EMBED": EMBED_TRAIN}),
                          **({} if SENT_CNN is None else {"HSG_SENT_CNN": SENT_CNN}))
_mode.__enter__()
for _ in range(3):
    step(0)
T.clear()
for _ in range(N):
    step(0)
print({k: round(v / N, 3) for k, v in T.items()}, "total", round(sum(T.values()) / N, 3), flush=True)
if not PROFILE:
    sys.exit(0)
from torch.profiler import ProfilerActivity, profile  # noqa: E402
with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], with_stack=True) as prof:
    for _ in range(3):
        step(0)
print(prof.key_averages().table(sort_by="self_cuda_time_total", row_limit=25))
print(prof.key_averages().table(sort_by="self_cpu_time_total", row_limit=25))
for name in ("aten::copy_", "aten::fill_", "hipDeviceSynchronize", "aten::nonzero", "aten::item"):
    print("=====", name)
    rows = [e for e in prof.key_averages(group_by_stack_n=6) if e.key == name]
    for e in sorted(rows, key=lambda e: -e.count)[:6]:
        print(e.count, "calls;", " <- ".join(fr.split("/")[-1] for fr in e.stack[:6]))
