"""The models on a resident batch: ``HSumGraph`` and ``HSumDocGraph`` on toy sizes, in train
mode with the paths documented bitwise reproducible on (HSG_SENT_LSTM, HSG_MODEL_GLUE,
HSG_WORD_EMBED, loss.sentence_loss) and the same dropout seed, give BITWISE the same logits,
loss and parameter gradients on ``DocumentStore.batch`` as on today's batch of the same
members (``graph.batch`` then ``.to(device)``): the inputs are identical and those kernels are
deterministic, so there is no tolerance.  One ``SLTester.evaluation`` batch (default mode)
gives the same extracts and counters on both."""
import numpy as np
import pytest
import torch

import model_ref as M
import resident_ref as R
from hetersumgraph_amd import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SWITCHES = dict(HSG_SENT_LSTM="1", HSG_MODEL_GLUE="1", HSG_WORD_EMBED="1")
CASES = [("HSumGraph", 4), ("HSumDocGraph", 5)]
SEED = 977
_cache = {}


def documents(cls):
    rng = np.random.default_rng(31)
    small = dict(vocab_size=500, sent_max_len=12, doc_max_timesteps=50)
    if cls == "HSumGraph":
        return [synth.make_hsg_doc(rng, N, W, k, k_jitter=2, **small)
                for N, W, k in ((5, 30, 6), (3, 20, 4), (7, 40, 6), (3, 25, 5), (4, 30, 5))]
    return [synth.make_hdsg_example(rng, ds, W, k, dw, **small)
            for ds, W, k, dw in (((3, 2), 30, 5, 12), ((2, 2, 1), 25, 4, 10), ((4, 3), 40, 6, 14), ((2, 1), 20, 4, 8))]


def batches(cls):
    """(model, resident batch, today's batch of the same members in the same order, index)."""
    from hetersumgraph_amd.resident import DocumentStore
    if cls not in _cache:
        docs = documents(cls)
        store = DocumentStore.from_doc_arrays(docs, DEV, chunk=2)
        pick = [3, 0, 2, 1]
        G, index = store.batch(pick)
        T = R.todays_batch([docs[i] for i in index]).to(DEV)
        seed = dict(CASES)[cls]
        model = M.make_model(cls, seed, {"vocab_size": 500, "n_iter": 2, "doc_max_timesteps": 50}).to(DEV)
        _cache[cls] = (model, G, T, index, docs)
    return _cache[cls]


def _bits(t):
    return t.contiguous().view(torch.int32)


def train_step(model, G):
    from hetersumgraph_amd import loss as hloss, rng
    from hetersumgraph_amd._lib import path_options
    from hetersumgraph_amd.module.GATStackLayer import reference_named_grads
    model.train()
    model.zero_grad(set_to_none=True)
    rng.manual_seed(SEED)
    rng.advance_all()
    with path_options(**SWITCHES):
        logits = model(G)
        loss = hloss.sentence_loss(G, logits)
        loss.backward()
    grads = {k: g.detach().clone() for k, g in reference_named_grads(model) if g is not None}
    return logits.detach().clone(), loss.detach().clone(), grads


@pytest.mark.parametrize("cls", [c[0] for c in CASES])
def test_train_step_is_bitwise_todays(cls):
    model, G, T, index, docs = batches(cls)
    want = train_step(model, T)
    got = train_step(model, G)
    assert want[0].shape[0] == sum(len(docs[i].sent_nodes) for i in index) and bool(torch.isfinite(want[0]).all())
    assert torch.equal(_bits(got[0]), _bits(want[0])), "logits"
    assert torch.equal(_bits(got[1]), _bits(want[1])), "loss"
    assert got[2].keys() == want[2].keys() and len(want[2]) > 20
    assert any(bool(g.any()) for g in want[2].values())
    for k, g in want[2].items():
        assert torch.equal(_bits(got[2][k]), _bits(g)), k
    # dropout is on: another seed gives other logits, so the equality above is not vacuous
    from hetersumgraph_amd import rng
    from hetersumgraph_amd._lib import path_options
    rng.manual_seed(SEED + 1)
    rng.advance_all()
    with path_options(**SWITCHES), torch.no_grad():
        assert not torch.equal(model(G), want[0])


class _Example:
    def __init__(self, n):
        self.original_article_sents = [f"sentence {i} of a document ." for i in range(n)]
        self.original_abstract = "an abstract ."


class _Set:
    def __init__(self, docs):
        self.docs = docs

    def get_example(self, i):
        return _Example(len(self.docs[i].sent_nodes))


@pytest.mark.parametrize("cls", [c[0] for c in CASES])
def test_evaluation_batch_is_todays(cls):
    from hetersumgraph_amd.Tester import SLTester
    model, G, T, index, docs = batches(cls)
    model.eval()
    state = []
    for g in (T, G):
        t = SLTester(model, 2, limited=True)
        with torch.no_grad():
            t.evaluation(g, index, _Set(docs))
        state.append((t.extracts, t._hyps, int(t.pred), int(t.true), int(t.match), int(t.match_true),
                      t.total_sentence_num, t.example_num, t.batch_number, float(t.running_loss)))
    assert state[0] == state[1]
    assert len(state[0][0]) == len(index) and all(len(e) == 2 for e in state[0][0])
