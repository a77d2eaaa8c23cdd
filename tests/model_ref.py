"""The fp64 oracle of the WHOLE model -- HSumGraph / HSumDocGraph -- at a model's CURRENT
parameters, in eval mode or in train mode with every dropout mask restated on the host.

tests/step_ref.py follows the fused stack alone through a trajectory; here the same is
done for the model a training step runs: word embedding, sentence CNN
(oracle.cnn.sent_encoder), the sentence LSTM (single-layer ``nn.LSTM``s with the
inter-layer keep-mask between them), the three projections, HDSG's doc nodes, the WSWGAT
stack (oracle.fused.wswgat_layer), ``wh``, and train.py:115-119's loss: per-document sum
of the sentence cross entropies, mean over the documents.  ``snapshot`` takes the
parameters from the model as they are now, so a test can snapshot, run the GPU step, run
the oracle at the snapshot, compare, update and go on (test_gpu_model_train.py; pinned on
the CPU by test_model_ref.py).

The draws of one train-mode step, all from the one stream of hetersumgraph_amd/rng.py and
all masks from oracle/masks.py: with ``off0`` the stream's offset before the forward, the
LSTM's inter-layer keep-mask is (seed, off0 + 1) over [n_sentences, 2 * hidden] when the
LSTM's dropout is on; then, per stack application in the order W2S, n_iter x (S2W, W2S),
the head mask one offset on and the FFN mask one more (test_gpu_stack_parity.train_masks).

No GPU code of its own; the product is imported lazily, and only to build a model.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.nn.utils.rnn as rnn

from helpers import concat_arrays

LR, MAX_NORM = 5e-4, 1.0                 # train.py's tail: clip 1.0, Adam lr 5e-4
FROZEN = ("sent_pos_embed.weight", "ngram_enc.position_embedding.weight")   # fixed sinusoid tables
SHARED = {"ngram_enc.embed.weight": "_embed.weight"}                        # one parameter, two names
P_STACK = 0.1                            # atten_dropout_prob = ffn_dropout_prob of every test model
P_LSTM = 0.1                             # the model's own nn.LSTM(dropout=0.1), HiGraph.py:117
# (fixture, model class, weight seed): the two smallest goldens of test_gpu_model.py -- 2 documents,
# 9-10 sentences, under 60 nodes
CASES = [("model_hsg", "HSumGraph", 4), ("model_hdsg", "HSumDocGraph", 5)]
# the dropout seed S of each case's three-step trajectory (step k draws from S + k + 1).  The GPU test
# uses them too, so the sensitivity test_model_ref.py asserts at every step is the one it relies on; how
# far a wrong draw moves the logits depends on the seed: a changed seed has to pass those assertions
SEEDS = {"model_hsg": 4242, "model_hdsg": 4242}


# ------------------------------------------------------------------ packed-LSTM helpers
def run_packed(mod, x, lens):
    """mod over rows x laid end to end (documents of lens > 0) -> rows [n, ndir*hid]."""
    lens = [g for g in lens if g > 0]                     # packing takes no empty sequence
    n_doc, max_len = len(lens), max(lens)
    doc = torch.repeat_interleave(torch.arange(n_doc), torch.tensor(lens))
    pos = torch.cat([torch.arange(g) for g in lens])
    flat = doc * max_len + pos
    pad = x.new_zeros(n_doc * max_len, x.shape[1]).index_copy(0, flat, x).view(n_doc, max_len, -1)
    out, _ = mod(rnn.pack_padded_sequence(pad, lens, batch_first=True, enforce_sorted=False))
    unp, _ = rnn.pad_packed_sequence(out, batch_first=True, total_length=max_len)
    return unp.reshape(n_doc * max_len, -1).index_select(0, flat)


def lstm_names(layer, ndir):
    """Per direction the (w_ih, w_hh, b_ih, b_hh) parameter names of a layer."""
    for d in range(ndir):
        sfx = f"_l{layer}" + ("_reverse" if d else "")
        yield tuple(n + sfx for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def single_layers(lstm, dtype):
    """An ``nn.LSTM`` -- or a name -> tensor mapping of its parameters -- restated as
    single-layer LSTMs holding the same weights, so a mask can go between the layers."""
    w = dict(lstm.named_parameters()) if isinstance(lstm, nn.Module) else lstm
    ndir = 2 if "weight_ih_l0_reverse" in w else 1
    hid = w["weight_hh_l0"].shape[1]
    mods, layer = [], 0
    while f"weight_ih_l{layer}" in w:
        m = nn.LSTM(w[f"weight_ih_l{layer}"].shape[1], hid, num_layers=1, batch_first=True,
                    bidirectional=ndir == 2).to(dtype)
        with torch.no_grad():
            for names in lstm_names(layer, ndir):
                for nm in names:
                    getattr(m, nm.replace(f"_l{layer}", "_l0")).copy_(w[nm].detach().to(dtype))
        mods.append(m)
        layer += 1
    return mods


# ----------------------------------------------------------------------------- the model
def make_model(cls_name, seed, z):
    """test_gpu_model.build_model's model (same hyper-parameters, same seeded weights) with a
    trainable embedding over the fixture's own vocabulary, left on the CPU in eval mode."""
    import weights
    from hetersumgraph_amd import HiGraph
    from test_gpu_model import HPS
    hps = HPS(vocab_size=int(z.get("vocab_size", 500)), n_iter=int(z.get("n_iter", 2)),
              doc_max_timesteps=int(z.get("doc_max_timesteps", 50)))
    torch.manual_seed(seed)
    model = getattr(HiGraph, cls_name)(hps, nn.Embedding(hps.vocab_size, 300, padding_idx=0))
    weights.seed_module(model, seed)
    assert model._embed.weight.requires_grad
    return model.eval()


def short_sentence(z):
    """The fixture's sentence token ids with sentence 1 cut to a single token: the CNN's
    all-padding windows and the embedding's run of one are then inside the step."""
    words = z["sent_words"].astype(np.int64)
    words[1, 1:] = 0
    lens = (words != 0).sum(1)
    assert lens[1] == 1 and len(set(lens.tolist())) > 2 and len(z["g_n_nodes"]) >= 2
    return words


def snapshot(model, dtype=torch.float64):
    """name -> fresh CPU leaf of ``dtype`` for every state-dict tensor (reference key
    names).  Nothing shares storage with the model, so a later in-place update cannot reach
    the snapshot; the two names of the word embedding hold ONE leaf, as in the model."""
    from oracle import fused
    snap = fused.as_params(model, dtype=dtype)
    for alias, name in SHARED.items():
        if alias in snap:
            snap[alias] = snap[name]
    for k in FROZEN:
        snap[k].requires_grad_(False)
    return snap


def recast(snap, dtype):
    """A snapshot's values as fresh leaves of another dtype (the fp32 restatement)."""
    out = {k: v.detach().to(dtype).clone().requires_grad_(v.requires_grad) for k, v in snap.items()}
    for alias, name in SHARED.items():
        if alias in out:
            out[alias] = out[name]
    return out


def trainable(snap):
    """name -> leaf of everything an optimizer moves (each parameter once)."""
    return {k: v for k, v in snap.items() if v.requires_grad and k not in SHARED}


def hdsg_layout(z):
    """HSumDocGraph.forward's bookkeeping (HiGraph.py:191-244) from a fixture's arrays:
    the sentence -> doc pairs, the rows of [sentences | docs] in supernode order, and per
    sentence the supernode rows of itself and of its doc."""
    a = concat_arrays(z)
    unit, nd, src, dst = a["unit"], a["ndtype"], a["src"], a["dst"]
    snodes, dnodes, supers = (np.nonzero(m)[0] for m in (nd == 1, nd == 2, unit == 1))
    rank = lambda ids: dict(zip(ids.tolist(), range(len(ids))))
    s_rank, d_rank, super_rank = rank(snodes), rank(dnodes), rank(supers)
    pairs = [(s_rank[int(s)], d_rank[int(d)]) for s, d in zip(src, dst) if nd[s] == 1 and nd[d] == 2]
    doc_of = dict(pairs)                                  # the last pair of a sentence wins
    assert len(doc_of) == len(snodes)
    pos = [s_rank[v] if v in s_rank else len(snodes) + d_rank[v] for v in supers.tolist()]
    t = lambda v: torch.as_tensor(np.asarray(v, np.int64))
    return dict(pair_s=t([p[0] for p in pairs]), pair_d=t([p[1] for p in pairs]), n_docs=len(dnodes),
                super_pos=t(pos), sent_super=t([super_rank[int(v)] for v in snodes]),
                doc_super=t([super_rank[int(dnodes[doc_of[i]])] for i in range(len(snodes))]))


def sentence_counts(z):
    """Sentences per member graph, in batch order."""
    off = np.cumsum(np.concatenate([[0], z["g_n_nodes"]]))
    return [int((z["g_ndtype"][a:b] == 1).sum()) for a, b in zip(off[:-1], off[1:])]


def n_draws(n_iter, lstm_draws):
    """Offsets one train-mode forward takes: the LSTM's, then two per stack application."""
    return lstm_draws + 2 * (1 + 2 * n_iter)


def step_masks(z, draws, lstm_shift=0, stack_shift=0):
    """(LSTM keep-mask or None, [(head keep, scale, FFN keep, scale) per application]) of
    ``draws = (seed, off0, p, lstm_dropout)``.  ``lstm_shift`` / ``stack_shift`` move the
    LSTM's offset / every offset of the stack: the wrong draws of test_model_ref.py."""
    from oracle import masks
    from test_gpu_stack_parity import train_masks
    seed, off0, p, p_lstm = draws
    n_w, n_super, n_sent = int((z["g_unit"] == 0).sum()), int((z["g_unit"] == 1).sum()), sum(sentence_counts(z))
    off, keep = off0, None
    if p_lstm > 0:
        keep = (masks.ffn_keep(seed, off0 + 1 + lstm_shift, n_sent, 256, p_lstm), masks.ffn_scale(p_lstm))
        off += 1
    return keep, train_masks(seed, off + stack_shift, n_w, n_super, p=p, n_iter=int(z.get("n_iter", 2)))


def oracle_at(z, words, snap, cls, draws=None, masks=None):
    """Forward, loss and backward of ``cls`` ("HSumGraph" / "HSumDocGraph") on the fixture
    ``z`` with the sentence token ids ``words``, at the snapshot's parameters and in its
    dtype.  ``draws = (seed, off0, p, lstm_dropout)``: train mode with the masks of
    ``step_masks``; ``masks``: that pair given outright.  Returns the logits, the loss and
    ``grads``, the gradients keyed by the reference parameter names."""
    from oracle import cnn as ocnn
    from oracle import fused
    dt = snap["wh.weight"].dtype
    for t in snap.values():
        t.grad = None
    if masks is None and draws is not None:
        masks = step_masks(z, draws)
    lstm_keep, stack_masks = masks if masks is not None else (None, None)
    a = concat_arrays(z)
    n_iter = int(z.get("n_iter", 2))
    lin = lambda x, name: F.linear(x, snap[name + ".weight"], snap.get(name + ".bias"))
    # word nodes and sentence encoders (HiGraph.py:127-152)
    E = snap["_embed.weight"]
    wid = torch.from_numpy(z["g_wid"][a["unit"] == 0].astype(np.int64))
    Xw = F.embedding(wid, E, padding_idx=0)
    conv = [(snap[f"ngram_enc.convs.{i}.weight"], snap[f"ngram_enc.convs.{i}.bias"]) for i in range(6)]
    ngram = ocnn.sent_encoder(torch.as_tensor(np.asarray(words, np.int64)), E, snap["ngram_enc.position_embedding.weight"],
                              [c[0] for c in conv], [c[1] for c in conv], padding_idx=0)
    glen = sentence_counts(z)
    pos = torch.cat([torch.arange(1, g + 1) for g in glen])
    cnn_feature = lin(ngram + snap["sent_pos_embed.weight"][pos], "cnn_proj")
    mods = single_layers({k[5:]: v for k, v in snap.items() if k.startswith("lstm.")}, dt)
    out = ngram
    for layer, m in enumerate(mods):
        out = run_packed(m, out, glen)
        if lstm_keep is not None and layer < len(mods) - 1:
            out = out * (torch.from_numpy(lstm_keep[0]).to(dt) * lstm_keep[1])
    sent = lin(torch.cat([cnn_feature, lin(out, "lstm_proj")], 1), "n_feature_proj")
    lay = hdsg_layout(z) if cls == "HSumDocGraph" else None
    if lay is None:
        s0 = sent
    else:
        cnt = torch.bincount(lay["pair_d"], minlength=lay["n_docs"]).to(dt)
        acc = torch.zeros(lay["n_docs"], sent.shape[1], dtype=dt).index_add(0, lay["pair_d"], sent[lay["pair_s"]])
        s0 = torch.cat([sent, lin(acc / cnt.unsqueeze(1), "dn_feature_proj")], 0)[lay["super_pos"]]
    # the stack (HiGraph.py:99-106)
    rws = fused.typed_relation("W2S", a["src"], a["dst"], a["unit"], a["tffrac"], a["edtype"])
    rsw = fused.typed_relation("S2W", a["src"], a["dst"], a["unit"], a["tffrac"], a["edtype"])
    T = snap["_TFembed.weight"]
    m = iter(stack_masks) if stack_masks is not None else None
    nxt = (lambda: next(m)) if m is not None else (lambda: None)
    w, s = Xw, fused.wswgat_layer("W2S", rws, Xw, s0, snap, T, "word2sent.", masks=nxt())
    for _ in range(n_iter):
        w = fused.wswgat_layer("S2W", rsw, w, s, snap, T, "sent2word.", masks=nxt())
        s = fused.wswgat_layer("W2S", rws, w, s, snap, T, "word2sent.", masks=nxt())
    if lay is not None:
        s = torch.cat([s[lay["sent_super"]], s[lay["doc_super"]]], 1)
    logits = lin(s, "wh")
    # train.py:115-119
    label = torch.from_numpy(z["sent_label"].astype(np.int64).sum(-1))
    doc = torch.repeat_interleave(torch.arange(len(glen)), torch.tensor(glen))
    ce = F.cross_entropy(logits, label, reduction="none")
    loss = torch.zeros(len(glen), dtype=dt).index_add(0, doc, ce).mean()
    loss.backward()
    grads = {k: v.grad for k, v in trainable(snap).items() if not k.startswith("lstm.") and v.grad is not None}
    for layer, mod in enumerate(mods):
        for nm, q in mod.named_parameters():
            grads["lstm." + nm.replace("_l0", f"_l{layer}")] = q.grad
    return dict(logits=logits.detach(), loss=loss.detach(), grads=grads)


def worst_grad_error(got, ref, rel):
    """max over the gradients of ``ref`` of max|got - ref| / (rel * max(max|ref|, 1e-3)):
    test_gpu_model.py's rule for a parameter gradient, as error over allowed."""
    worst = 0.0
    for k, r in ref.items():
        r = r.double()
        worst = max(worst, (got[k].detach().cpu().double() - r).abs().max().item() / (rel * max(r.abs().max().item(), 1e-3)))
    return worst
