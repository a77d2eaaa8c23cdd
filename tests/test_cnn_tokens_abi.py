"""What is specific to the C ABI of the sentence CNN's token paths (include/hsg_cnn_tokens.h):
its source is built, the host queries answer as documented, refusals return HSG_EINVAL before
any launch, and every entry point of the header that writes through a pointer has a guard-band
case in tests/test_gpu_cnn_tokens_guard.py.  Names, exports, signatures and the header's place
among the build's dependencies are tests/test_abi_conformance.py's.  No GPU needed."""
import ctypes
import os

import abi

HEADER = "hsg_cnn_tokens.h"


def test_the_source_is_built():
    from hetersumgraph_amd import build
    assert any(os.path.basename(s) == "hsg_cnn_tokens.hip" for s in build.SOURCES)


def test_supported_sets_and_host_queries():
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    C = lib.hsg_cnn_tok_chunk()
    assert C == 64 == lib.hsg_cnn_tok_chunk()
    for L, D in ((7, 4), (100, 300), (400, 4096), (20, 300)):
        assert lib.hsg_cnn_tok_supported(L, D), (L, D)
    for L, D in ((6, 300), (401, 300), (100, 302), (100, 0), (100, -4), (100, 4100), (0, 4)):
        assert not lib.hsg_cnn_tok_supported(L, D), (L, D)
    per = 1350 * 300 + 300
    sizes = [lib.hsg_cnn_tok_dw_ws_floats(n, 300) for n in (-1, 0, 1, C - 1, C, C + 1, 3 * C + 1, 5000)]
    assert sizes == [0, 0, per, per, per, 2 * per, 4 * per, -(-5000 // C) * per]
    assert lib.hsg_cnn_tok_dw_ws_floats(10, 4) == 1350 * 4 + 300
    assert lib.hsg_cnn_tok_dw_ws_floats(10, 302) == 0
    assert lib.hsg_cnn_taps() == 1350


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands for
    a non-NULL, 16-byte aligned device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p = _lib.load(), _lib.HSG_EINVAL, 16
    bias = (ctypes.c_void_p * 6)(*[p] * 6)
    nobias = (ctypes.c_void_p * 6)(p, p, None, p, p, p)

    def mark(n=3, L=9, V=37, ids=p, present=p, bad=p):
        return lib.hsg_cnn_tok_mark(n, L, V, ids, present, bad, None)
    for kw in (dict(n=-1), dict(L=0), dict(V=0), dict(ids=None), dict(present=None), dict(bad=None)):
        assert mark(**kw) == EINVAL, kw

    def table(V=37, D=300, U=5, L=9, present=p, slot=p, E=p, P=p, Tb=p, ldt=304):
        return lib.hsg_cnn_tok_table(V, D, U, L, present, slot, E, P, Tb, ldt, None)
    for kw in (dict(V=0), dict(D=302), dict(D=0), dict(U=0), dict(U=38), dict(L=-1), dict(ldt=296), dict(ldt=302),
               dict(present=None), dict(slot=None), dict(E=None), dict(P=None), dict(Tb=None), dict(E=20), dict(P=8),
               dict(Tb=24)):
        assert table(**kw) == EINVAL, kw

    def pool(n=3, L=9, V=37, U=5, ids=p, rowoff=p, slot=p, TW=p, ldtw=1352, b=bias, feat=p, arg=p):
        return lib.hsg_cnn_tok_pool(n, L, V, U, ids, rowoff, slot, TW, ldtw, b, feat, arg, None)
    for kw in (dict(n=-1), dict(L=6), dict(L=401), dict(V=0), dict(U=0), dict(U=38), dict(rowoff=None), dict(b=None),
               dict(ldtw=1349), dict(ids=None), dict(slot=None), dict(TW=None), dict(feat=None), dict(arg=None),
               dict(b=nobias)):
        assert pool(**kw) == EINVAL, kw
    assert pool(n=0, ids=None, slot=None, TW=None, feat=None, arg=None) == 0          # nothing to do

    def dw(n=3, L=9, V=37, D=300, ids=p, rowoff=p, E=p, P=p, feat=p, arg=p, dfeat=p, ws=p, dWall=p, lddw=304, db=p):
        return lib.hsg_cnn_tok_dw(n, L, V, D, ids, rowoff, E, P, feat, arg, dfeat, ws, dWall, lddw, db, None)
    for kw in (dict(n=-1), dict(L=6), dict(L=401), dict(V=0), dict(D=302), dict(D=0), dict(lddw=296), dict(lddw=302),
               dict(dWall=None), dict(db=None), dict(dWall=24), dict(ids=None), dict(rowoff=None), dict(E=None),
               dict(P=None), dict(feat=None), dict(arg=None), dict(dfeat=None), dict(ws=None), dict(E=20), dict(P=8),
               dict(ws=4)):
        assert dw(**kw) == EINVAL, kw


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_cnn_tokens_guard import CASES
    w = abi.writable_entry_points([HEADER])
    assert "int32_t *present" in w["hsg_cnn_tok_mark"] and "int32_t *bad" in w["hsg_cnn_tok_mark"]
    assert "float *Tb" in w["hsg_cnn_tok_table"]
    assert "float *feat" in w["hsg_cnn_tok_pool"] and "int32_t *arg" in w["hsg_cnn_tok_pool"]
    assert {"float *ws", "float *dWall", "float *dbias"} <= set(w["hsg_cnn_tok_dw"])
    for name in ("hsg_cnn_tok_supported", "hsg_cnn_tok_chunk", "hsg_cnn_tok_dw_ws_floats"):
        assert name not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
