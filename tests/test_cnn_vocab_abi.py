"""What is specific to the C ABI of the sentence CNN's vocabulary path (include/hsg_cnn_vocab.h):
its source is built, the host query answers as documented, refusals return HSG_EINVAL before any
launch, and every entry point of the header that writes through a pointer has a guard-band case
in tests/test_gpu_cnn_vocab_guard.py.  Names, exports, signatures and the header's place among
the build's dependencies are tests/test_abi_conformance.py's.  No GPU needed."""
import ctypes
import os

import abi

HEADER = "hsg_cnn_vocab.h"


def test_the_source_is_built():
    from hetersumgraph_amd import _lib, build
    assert any(os.path.basename(s) == "hsg_cnn_vocab.hip" for s in build.SOURCES)
    assert build.FILE_FLAGS["hsg_cnn_vocab.hip"] == ["-ffp-contract=off"] == build.FILE_FLAGS["hsg_cnn_tokens.hip"]
    assert _lib.exports(HEADER) == ("hsg_cnn_vocab_supported", "hsg_cnn_vocab_pool")


def test_supported_set():
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    for L in (7, 20, 100, 400):
        assert lib.hsg_cnn_vocab_supported(L), L
    for L in (6, 401, 0, -1):
        assert not lib.hsg_cnn_vocab_supported(L), L
    assert lib.hsg_cnn_taps() == 1350


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands for
    a non-NULL, 16-byte aligned device pointer that is never dereferenced.  Everything
    hsg_cnn_tok_pool refuses, and what whole-row 16-byte loads add: a pitch that is no multiple
    of 4, a TW base that is not 16-byte aligned."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p = _lib.load(), _lib.HSG_EINVAL, 16
    bias = (ctypes.c_void_p * 6)(*[p] * 6)
    nobias = (ctypes.c_void_p * 6)(p, p, None, p, p, p)

    def pool(n=3, L=9, V=37, ids=p, rowoff=p, TW=p, ldtw=1352, b=bias, feat=p, arg=p):
        return lib.hsg_cnn_vocab_pool(n, L, V, ids, rowoff, TW, ldtw, b, feat, arg, None)
    for kw in (dict(n=-1), dict(L=6), dict(L=401), dict(V=0), dict(rowoff=None), dict(b=None), dict(ldtw=1349),
               dict(ldtw=1350), dict(ldtw=1354), dict(ids=None), dict(TW=None), dict(feat=None), dict(arg=None),
               dict(b=nobias), dict(TW=20), dict(TW=8)):
        assert pool(**kw) == EINVAL, kw
    assert pool(n=0, ids=None, TW=None, feat=None, arg=None) == 0          # nothing to do
    assert pool(n=0, rowoff=None) == EINVAL and pool(n=0, L=6) == EINVAL    # ... but still a valid call


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_cnn_vocab_guard import CASES
    w = abi.writable_entry_points([HEADER])
    assert "float *feat" in w["hsg_cnn_vocab_pool"] and "int32_t *arg" in w["hsg_cnn_vocab_pool"]
    assert "hsg_cnn_vocab_supported" not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
