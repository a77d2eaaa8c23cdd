"""The host side of the sentence CNN's vocabulary path (path_options(HSG_SENT_CNN_VOCAB="1"),
hetersumgraph_amd.cnn.vocab_path_ok / VocabTable, module/Encoder.py), without a GPU: the switch
refuses values it does not know, the eligibility rule declines CPU tensors, a call that records a
gradient and a table over the budget, the table's key moves with every version counter, and the
encoder drops its table at every train() / eval()."""
import types

import pytest
import torch

V, D, L = 30, 8, 11


class Stub:
    """What vocab_path_ok reads of a tensor, claiming to live on the device."""

    def __init__(self, *shape, dtype=torch.float32, requires_grad=False, is_cuda=True, contiguous=True):
        self.shape, self.dtype, self.requires_grad, self.is_cuda = torch.Size(shape), dtype, requires_grad, is_cuda
        self._contiguous = contiguous

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous


def stubs(V=V, Pn=L + 1, **kw):
    return (Stub(5, L, dtype=torch.int64), Stub(V, D, **kw), Stub(Pn, D), [Stub(50, 1, h, D) for h in range(2, 8)],
            [Stub(50) for _ in range(6)])


def encoder():
    from hetersumgraph_amd.module.Encoder import sentEncoder
    hps = types.SimpleNamespace(sent_max_len=L, word_emb_dim=D)
    return sentEncoder(hps, torch.nn.Embedding(V, D, padding_idx=0))


def test_switch_values():
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.cnn import MODES, sent_cnn_vocab_on
    assert MODES == ("0", "dw", "tokens")                          # the other switch is as it was
    assert sent_cnn_vocab_on() is False                            # off by default
    for value, want in (("0", False), ("1", True)):
        with _lib.path_options(HSG_SENT_CNN_VOCAB=value):
            assert sent_cnn_vocab_on() is want
    enc = encoder().eval()
    for bad in ("2", "", "on", "tokens"):
        with _lib.path_options(HSG_SENT_CNN_VOCAB=bad):
            with pytest.raises(ValueError, match="HSG_SENT_CNN_VOCAB"):
                sent_cnn_vocab_on()
            with pytest.raises(ValueError, match="HSG_SENT_CNN_VOCAB"):
                enc.takes_token_path(torch.zeros(2, L, dtype=torch.long))


def test_path_is_declined():
    from hetersumgraph_amd import _lib
    from hetersumgraph_amd.cnn import LDY, vocab_path_ok, vocab_table_bytes
    enc = encoder().eval()
    ids = torch.zeros(2, L, dtype=torch.long)
    with torch.no_grad():
        assert not vocab_path_ok(ids, *enc._vocab_args())          # CPU tensors
    with _lib.path_options(HSG_SENT_CNN_VOCAB="1"), torch.no_grad():
        assert not enc.takes_token_path(ids)
    with torch.enable_grad():
        ok = stubs()
        assert vocab_path_ok(*ok)                                  # nothing requires grad
        ok[3][2].requires_grad = True
        assert not vocab_path_ok(*ok)                              # a trainable conv weight, grad enabled
        with torch.no_grad():
            assert vocab_path_ok(*ok)
        ok = stubs()
        ok[4][5].requires_grad = True
        assert not vocab_path_ok(*ok)                              # ... or bias
        assert not vocab_path_ok(*stubs(requires_grad=True))       # ... or embedding
    with torch.no_grad():
        # the budget: (V + Pn) * LDY * 4 bytes against HSG_SENT_CNN_VOCAB_MB MiB
        assert vocab_table_bytes(50000, 101) == 50101 * LDY * 4 <= 1024 << 20
        assert vocab_path_ok(*stubs(V=50000, Pn=101))
        assert not vocab_path_ok(*stubs(V=400000, Pn=101))
        with _lib.path_options(HSG_SENT_CNN_VOCAB_MB="4096"):
            assert vocab_path_ok(*stubs(V=400000, Pn=101))
        with _lib.path_options(HSG_SENT_CNN_VOCAB_MB="0.1"):
            assert not vocab_path_ok(*stubs())
        assert (V + L + 1) * LDY * 4 > 0.1 * (1 << 20)


def test_path_is_eligible_under_no_grad():
    from hetersumgraph_amd.cnn import vocab_path_ok
    with torch.no_grad():
        assert vocab_path_ok(*stubs())
        assert vocab_path_ok(*stubs(requires_grad=True))           # a trainable embedding is no obstacle
        for breaker in (lambda a: setattr(a[1], "dtype", torch.float64),
                        lambda a: setattr(a[2], "_contiguous", False),
                        lambda a: setattr(a[1], "_contiguous", False),
                        lambda a: setattr(a[0], "is_cuda", False),
                        lambda a: setattr(a[3][0], "is_cuda", False),
                        lambda a: setattr(a[0], "shape", torch.Size((5, 6))),        # L < 7
                        lambda a: setattr(a[0], "shape", torch.Size((5, L + 1))),    # more tokens than positions
                        lambda a: setattr(a[0], "shape", torch.Size((5 * L,))),
                        lambda a: setattr(a[3][1], "shape", torch.Size((50, 1, 4, D))),
                        lambda a: setattr(a[2], "shape", torch.Size((L + 1, D + 4))),
                        lambda a: a[3].pop()):
            args = stubs()
            breaker(args)
            assert not vocab_path_ok(*args)
        a = stubs(Pn=402)
        a[0].shape = torch.Size((5, 401))                           # hsg_cnn_vocab_supported declines
        assert not vocab_path_ok(*a)
        a[0].shape = torch.Size((5, 400))
        assert vocab_path_ok(*a)


def test_table_key_follows_the_version_counters():
    from hetersumgraph_amd import dense
    from hetersumgraph_amd.cnn import VocabTable
    enc = encoder()
    emb, pos, cw, _ = enc._vocab_args()
    key = VocabTable.key_of(emb, pos, cw)
    assert key == VocabTable.key_of(emb, pos, cw)
    assert not any(isinstance(x, torch.Tensor) for part in key[:-1] for x in part)     # numbers only
    with torch.no_grad():
        cw[3].add_(1.0)
    key2 = VocabTable.key_of(emb, pos, cw)
    assert key2 != key
    torch.autograd.graph.increment_version(cw[0])
    key3 = VocabTable.key_of(emb, pos, cw)
    assert key3 != key2
    torch.autograd.graph.increment_version(emb)
    assert VocabTable.key_of(emb, pos, cw) != key3
    with dense.gemm_dtype("bf16" if dense.get_gemm_dtype() != "bf16" else "f32"):
        assert VocabTable.key_of(emb, pos, cw)[:-1] == VocabTable.key_of(emb, pos, cw)[:-1]
        assert VocabTable.key_of(emb, pos, cw) != key
    # a stale key means a rebuild; a dropped table has none
    t = VocabTable()
    assert t.key is None and t.TW is None and t.nbytes() == 0


def test_train_and_eval_drop_the_table():
    enc = encoder()
    assert "_vocab_table" not in dict(enc.named_buffers()) and not any("vocab" in k for k in enc.state_dict())
    for call in (enc.eval, enc.train, lambda: enc.train(False), enc.drop_vocab_table):
        enc._vocab_table.key, enc._vocab_table.TW, enc._vocab_table.V = ("stale",), torch.zeros(1), 1
        call()
        assert enc._vocab_table.key is None and enc._vocab_table.TW is None
    # a parent's eval() reaches the encoder
    holder = torch.nn.Sequential(enc)
    enc._vocab_table.key, enc._vocab_table.TW = ("stale",), torch.zeros(1)
    holder.eval()
    assert enc._vocab_table.TW is None and not enc.training
