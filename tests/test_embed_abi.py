"""What is specific to the C ABI of the trainable word embedding (include/hsg_embed.h): the
host queries answer as documented, refusals return HSG_EINVAL before any launch, and every
entry point of the header that writes through a pointer has a guard-band case in
tests/test_gpu_embed_guard.py.  Names, exports and signatures are
tests/test_abi_conformance.py's.  No GPU needed."""
import abi

HEADER = "hsg_embed.h"


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
    w = abi.writable_entry_points([HEADER])
    assert "float *Xw" in w["hsg_embed_rows"] and "int64_t *keys" in w["hsg_embed_keys"]
    assert "float *dE" in w["hsg_embed_grad"] and "float *ws" in w["hsg_embed_grad"]
    for name in ("hsg_embed_supported", "hsg_embed_piece_rows", "hsg_embed_ws_floats"):
        assert name not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
