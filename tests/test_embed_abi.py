"""The C ABI of the trainable word embedding (include/hsg_embed.h): libhsg.so exports what
the header declares, the binding's EMBED_EXPORTS equals it and is bound from a table of its
own (EMBED_SIGS, not _SIGS), it is disjoint from the other three export lists, the host
queries answer as documented, refusals return HSG_EINVAL before any launch, and every entry
point of the header that writes through a pointer has a guard-band case in
tests/test_gpu_embed_guard.py.  No GPU needed."""
import ctypes
import os

import pytest

from test_model_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hsg_embed.h")


def writable_entry_points():
    """test_guard_coverage's parser rule, pointed at hsg_embed.h."""
    import test_guard_coverage as cov
    saved = cov.HEADERS
    cov.HEADERS = [HEADER]
    try:
        return cov.writable_entry_points()
    finally:
        cov.HEADERS = saved


def test_header_declares_the_bound_symbols():
    from hetersumgraph_amd import _lib
    assert declared_functions(HEADER) == sorted(_lib.EMBED_EXPORTS)
    assert set(_lib.EMBED_EXPORTS) == set(_lib.EMBED_SIGS)


def test_export_list_is_disjoint_from_the_others():
    from hetersumgraph_amd import _lib
    e = set(_lib.EMBED_EXPORTS)
    for other in (_lib.EXPORTS, _lib.TRAIN_EXPORTS, _lib.MODEL_EXPORTS):
        assert not e & set(other)
    assert not e & set(_lib._SIGS)


def test_library_exports_every_declared_symbol():
    from hetersumgraph_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libhsg.so is not built (run python -m hetersumgraph_amd.build)")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_functions(HEADER):
        assert hasattr(lib, name), name
    bound = _lib.load()
    for name, args in _lib.EMBED_SIGS.items():
        assert getattr(bound, name).argtypes == args, name


def test_supported_sets_and_host_queries():
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    P = lib.hsg_embed_piece_rows()
    assert P >= 2 and P == lib.hsg_embed_piece_rows()
    assert lib.hsg_embed_supported(300) and lib.hsg_embed_supported(4)
    for bad in (302, 0, -4, 2, 301):
        assert not lib.hsg_embed_supported(bad), bad
    sizes = [lib.hsg_embed_ws_floats(n, 300) for n in (-1, 0, 1, P - 1, P, P + 1, 3 * P + 1, 5000, 50000)]
    assert sizes == sorted(sizes) and sizes[:3] == [0, 0, 2 * 300]
    assert sizes[4] == 2 * 300 and sizes[5] == 4 * 300 and sizes[6] == 8 * 300
    assert lib.hsg_embed_ws_floats(100, 302) == 0


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands
    for a non-NULL, 16-byte aligned device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p = _lib.load(), _lib.HSG_EINVAL, 16

    def rows(n_w=5, V=37, D=300, wid=p, E=p, Xw=p, ldx=300):
        return lib.hsg_embed_rows(n_w, V, D, wid, E, Xw, ldx, None)
    for kw in (dict(n_w=-1), dict(V=-1), dict(D=302), dict(D=0), dict(ldx=296), dict(ldx=302), dict(wid=None),
               dict(E=None), dict(Xw=None), dict(E=20), dict(Xw=24)):
        assert rows(**kw) == EINVAL, kw
    assert rows(n_w=0, wid=None, E=None, Xw=None) == 0                            # nothing to do

    def keys(n_w=5, n=2, L=9, rows=7, wid=p, ids=p, rowoff=p, pad=0, out=p):
        return lib.hsg_embed_keys(n_w, n, L, rows, wid, ids, rowoff, pad, out, None)
    for kw in (dict(n_w=-1), dict(n=-1), dict(L=0), dict(rows=1), dict(rows=-1), dict(wid=None), dict(ids=None),
               dict(rowoff=None), dict(out=None), dict(n=0), dict(rows=2 ** 32)):
        assert keys(**kw) == EINVAL, kw
    assert keys(n_w=0, n=0, rows=0, wid=None, ids=None, rowoff=None, out=None) == 0

    def grad(V=37, D=300, n_occ=12, occ=p, n_w=5, dW=p, ldw=300, rows=7, dX=p, ldx=304, dE=p, ws=p):
        return lib.hsg_embed_grad(V, D, n_occ, occ, n_w, dW, ldw, rows, dX, ldx, dE, ws, None)
    for kw in (dict(V=-1), dict(D=302), dict(D=0), dict(n_occ=-1), dict(n_w=-1), dict(rows=-1), dict(occ=None),
               dict(dW=None), dict(dX=None), dict(dE=None), dict(ws=None), dict(ldw=296), dict(ldx=299), dict(ldw=302),
               dict(dW=20), dict(dX=24), dict(dE=8), dict(ws=4)):
        assert grad(**kw) == EINVAL, kw
    assert grad(V=0, n_occ=0, occ=None, n_w=0, dW=None, rows=0, dX=None, dE=None, ws=None) == 0   # no table: nothing to do


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_embed_guard import CASES
    w = writable_entry_points()
    assert "float *Xw" in w["hsg_embed_rows"] and "int64_t *keys" in w["hsg_embed_keys"]
    assert "float *dE" in w["hsg_embed_grad"] and "float *ws" in w["hsg_embed_grad"]
    for name in ("hsg_embed_supported", "hsg_embed_piece_rows", "hsg_embed_ws_floats"):
        assert name not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
