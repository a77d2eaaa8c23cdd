"""The ctypes bindings against the C headers, for every header and every entry point.

``_lib.ABI`` (header -> {name: argtypes}) and ``_lib.RESTYPE`` are written by hand, and so
are include/*.h; this file is where the two witnesses meet.  Per header: the declared names
are the registry's, libhsg.so exports them, ``load()`` binds what the registry says, and
every argument list and return type equals the header's declaration parameter by
parameter -- a miscounted ``_I`` / ``_P`` fails here, by name, not on the GPU.  Across
headers: no name is listed twice, the build depends on exactly these headers, and the
struct mirrors equal their C definitions field by field.  The host library's two functions
(include/hsg_graph.h, bound in datapipe.py) get the same treatment.  No GPU needed."""
import ctypes
import os

import pytest

import abi
from hetersumgraph_amd import _lib

HEADERS = sorted(_lib.ABI)


def test_the_registry_names_every_device_header():
    assert HEADERS == sorted(h for h in os.listdir(abi.INCLUDE) if h != "hsg_graph.h")
    for h in HEADERS:
        assert _lib.exports(h) == tuple(_lib.ABI[h]) and _lib.exports(h), h


@pytest.mark.parametrize("header", HEADERS)
def test_header_and_registry_declare_the_same_names(header):
    listed = set(_lib.ABI[header])
    for declared in (set(abi.declared_functions(header)), set(abi.declarations(header))):
        assert declared == listed, (f"{header}: declared but not listed {sorted(declared - listed)}, "
                                    f"listed but not declared {sorted(listed - declared)}")


@pytest.mark.parametrize("header", HEADERS)
def test_library_exports_and_binds_every_name(header):
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libhsg.so is not built (run python -m hetersumgraph_amd.build)")
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name, args in _lib.ABI[header].items():
        assert hasattr(raw, name), name
        assert getattr(bound, name).argtypes == args, name
        assert getattr(bound, name).restype == _lib.RESTYPE.get(name, ctypes.c_int), name


@pytest.mark.parametrize("header", HEADERS)
def test_signatures_match_the_header(header):
    """Parameter by parameter: a pointer is c_void_p (the three struct pointers: a pointer to
    the mirror), a scalar is its ctypes twin; the return type likewise, int unless RESTYPE
    says otherwise."""
    declared = abi.declarations(header)
    for name, args in _lib.ABI[header].items():
        assert name in declared, f"{name} is listed under {header}, which does not declare it"
        restype, argtypes = abi.signature(header, name)
        params = declared[name][1]
        assert len(args) == len(params), f"{name}: {len(args)} argtypes, {len(params)} parameters in {header}"
        for i, (got, want) in enumerate(zip(args, argtypes)):
            assert got == want, f"{name}: argument {i} ({params[i]}) is bound as {got}"
        assert _lib.RESTYPE.get(name, ctypes.c_int) == restype, f"{name}: return type"


def test_no_name_is_listed_under_two_headers():
    seen = {}
    for header in HEADERS:
        for name in _lib.ABI[header]:
            assert name not in seen, f"{name} is listed under {seen[name]} and {header}"
            seen[name] = header
    assert set(_lib.RESTYPE) <= set(seen), sorted(set(_lib.RESTYPE) - set(seen))
    # the headers agree: no function is declared in two of them either
    declared = [n for h in HEADERS for n in abi.declared_functions(h)]
    assert len(declared) == len(set(declared)) == len(seen)


def test_the_build_depends_on_exactly_the_registry_headers():
    from hetersumgraph_amd import build
    inc = [os.path.basename(h) for h in build.HEADERS if os.path.dirname(h) == abi.INCLUDE]
    assert sorted(inc) == HEADERS and len(set(inc)) == len(inc)
    assert [os.path.basename(h) for h in build.HOST_HEADERS] == ["hsg_graph.h"]
    assert sorted(os.path.basename(h) for h in build.HEADERS if os.path.dirname(h) != abi.INCLUDE) == \
        ["hsg_dev.h", "hsg_rng.h", "hsg_wave.h", "hsg_wsplit.h"]
    assert all(os.path.exists(h) for h in build.HEADERS + build.HOST_HEADERS)


def test_struct_mirrors_equal_their_c_definitions():
    for header, cname, cls, nested in (("hsg.h", "hsg_rel", _lib.HsgRel, {}),
                                       ("hsg_train.h", "hsg_mt_tensor", _lib.HsgMtTensor, {}),
                                       ("hsg_resident.h", "hsg_res_rel", _lib.HsgResRel, {}),
                                       ("hsg_resident.h", "hsg_res_store", _lib.HsgResStore,
                                        {"hsg_res_rel": _lib.HsgResRel})):
        assert list(cls._fields_) == abi.mirror_fields(header, cname, nested), cname
    # the layout numbers stay with their headers' tests (tests/test_abi.py, test_train_abi.py)


def test_host_library_matches_its_header():
    """libhsg_host.so (g++, no HIP runtime): include/hsg_graph.h's two functions and hsg_docs,
    as datapipe.py binds them."""
    from hetersumgraph_amd import build, datapipe
    build.build_host(verbose=False)
    assert abi.declared_functions("hsg_graph.h") == sorted(abi.declarations("hsg_graph.h")) == \
        ["hsg_graph_count", "hsg_graph_fill"]
    raw, bound = ctypes.CDLL(datapipe.HOST_LIB), datapipe.host_lib()
    for name in abi.declarations("hsg_graph.h"):
        restype, argtypes = abi.signature("hsg_graph.h", name)
        assert hasattr(raw, name), name
        assert getattr(bound, name).argtypes == argtypes, name
        assert getattr(bound, name).restype == restype == ctypes.c_int, name
    assert list(datapipe.HsgDocs._fields_) == abi.mirror_fields("hsg_graph.h", "hsg_docs")
    assert ctypes.sizeof(datapipe.HsgDocs) == 8 + 12 * 8
