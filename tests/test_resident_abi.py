"""What is specific to the C ABI of the resident document store (include/hsg_resident.h): the
relation's arrays are the reference's, the family constants are the header's, the host query
answers as documented, refusals return HSG_EINVAL before any launch, and every entry point of
the header that writes through a pointer has a guard-band case in
tests/test_gpu_resident_guard.py.  Names, exports, signatures and the two structures' fields
are tests/test_abi_conformance.py's.  No GPU needed."""
import ctypes
import os
import re

import abi

HEADER = "hsg_resident.h"


def test_structures_mirror_the_header():
    """The mirrors' fields are the conformance test's; here: the relation's arrays are, in
    order, the ones the reference store keeps, and the store embeds two relations."""
    from hetersumgraph_amd import _lib
    assert [f for _, f in abi.struct_fields(HEADER, "hsg_res_rel")] == list(__import__("resident_ref").REL_ARRAYS)
    assert [f for f, _ in _lib.HsgResRel._fields_] == list(__import__("resident_ref").REL_ARRAYS)
    assert abi.struct_fields(HEADER, "hsg_res_store")[-1] == ("hsg_res_rel", "rel[2]")


def test_family_constants_match_the_header():
    from hetersumgraph_amd import _lib
    src = open(os.path.join(abi.INCLUDE, HEADER)).read()
    val = lambda n: int(re.search(r"#define %s (\d+)" % n, src).group(1))
    assert (_lib.HSG_RES_NODE, _lib.HSG_RES_EDGE, _lib.HSG_RES_SENT, _lib.HSG_RES_NFAM) == \
        (val("HSG_RES_NODE"), val("HSG_RES_EDGE"), val("HSG_RES_SENT"), val("HSG_RES_NFAM"))
    for fn, off in ((_lib.HSG_RES_SRC, 3), (_lib.HSG_RES_DST, 4), (_lib.HSG_RES_TYP, 5)):
        assert [fn(0), fn(1)] == [off, off + 3]
    assert "#define HSG_RES_SRC(q) (3 + 3 * (q))" in src and "#define HSG_RES_DST(q) (4 + 3 * (q))" in src
    assert "#define HSG_RES_TYP(q) (5 + 3 * (q))" in src


def test_supported_limits():
    from hetersumgraph_amd import _lib
    lib, top = _lib.load(), 2 ** 31 - 1
    for args, want in (((1, 0, 0, 0), 1), ((1 << 20, top, top, top), 1), ((0, 1, 1, 1), 0), ((-1, 1, 1, 1), 0),
                       (((1 << 20) + 1, 1, 1, 1), 0), ((1, top + 1, 0, 0), 0), ((1, 0, top + 1, 0), 0),
                       ((1, 0, 0, top + 1), 0), ((1, -1, 0, 0), 0), ((1, 0, -1, 0), 0), ((1, 0, 0, -1), 0),
                       ((32, 20320, 159040, 80640), 1)):
        assert bool(lib.hsg_res_supported(*args)) == bool(want), args


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands for
    a non-NULL device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p, top = _lib.load(), _lib.HSG_EINVAL, 16, 2 ** 31 - 1

    def store(**kw):
        f = dict(n_docs=4, starts=p, bases=p, sent_len=8, label_len=5)
        f.update(kw)
        return ctypes.byref(_lib.HsgResStore(**f))

    assert lib.hsg_res_offsets(None, 2, p, p, None) == EINVAL
    for st, B, pick, offs in ((store(), 0, p, p), (store(), -1, p, p), (store(), (1 << 20) + 1, p, p),
                              (store(), 2, None, p), (store(), 2, p, None), (store(starts=None), 2, p, p),
                              (store(bases=None), 2, p, p), (store(n_docs=0), 2, p, p), (store(n_docs=top + 1), 2, p, p)):
        assert lib.hsg_res_offsets(st, B, pick, offs, None) == EINVAL

    def graph(st=None, B=2, pick=p, offs=p, n=5, E=7, outs=None):
        outs = [p] * 10 if outs is None else outs
        return lib.hsg_res_graph(store() if st is None else st, B, pick, offs, n, E, *outs, None)
    drop = lambda i: [None if j == i else p for j in range(10)]
    for kw in [dict(B=0), dict(pick=None), dict(offs=None), dict(n=-1), dict(E=-1), dict(n=top + 1), dict(E=top + 1),
               dict(st=store(sent_len=0)), dict(st=store(label_len=0)), dict(st=store(starts=None))] + \
              [dict(outs=drop(i)) for i in range(10)]:
        assert graph(**kw) == EINVAL, kw

    def rel(st=None, kind=0, B=2, pick=p, offs=p, ns=3, nd=4, nt=6, outs=None):
        outs = [p] * 10 if outs is None else outs
        return lib.hsg_res_relation(store() if st is None else st, kind, B, pick, offs, ns, nd, nt, *outs, None)
    for kw in [dict(kind=2), dict(kind=-1), dict(B=0), dict(pick=None), dict(offs=None), dict(ns=-1), dict(nd=-1),
               dict(nt=-1), dict(nt=top + 1), dict(st=store(bases=None))] + [dict(outs=drop(i)) for i in range(10)]:
        assert rel(**kw) == EINVAL, kw
    # indptr and cindptr hold a closing element even when everything else is empty
    assert rel(ns=0, nd=0, nt=0, outs=drop(0)) == EINVAL and rel(ns=0, nd=0, nt=0, outs=drop(5)) == EINVAL


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_resident_guard import CASES
    w = abi.writable_entry_points([HEADER])
    assert w["hsg_res_offsets"] == ["int64_t *offs"]
    for prm in ("float *unit", "int64_t *words", "int64_t *position", "int64_t *label", "int64_t *src", "float *edtype"):
        assert prm in w["hsg_res_graph"], prm
    assert len(w["hsg_res_graph"]) == 10 and len(w["hsg_res_relation"]) == 10
    assert "hsg_res_supported" not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
