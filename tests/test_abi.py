"""What is specific to include/hsg.h's part of the C ABI: the layout numbers of hsg_rel, the
gfx950 code object and version string, and the host mirror of hsg_gemm_dw_tiles.  Names,
exports, signatures and the struct's fields are tests/test_abi_conformance.py's, for every
header alike.  (No compute calls here -- those need a GPU and live in the -m gpu tests.)"""
import ctypes

def test_struct_layout():
    from hetersumgraph_amd._lib import HsgRel
    # 3 x int32 + pad to 8 + 7 pointers, then the work lists (round 6): 2 x int32 + 2
    # pointers (x86-64 SysV)
    assert ctypes.sizeof(HsgRel) == 16 + 7 * 8 + 8 + 2 * 8
    assert HsgRel.indptr.offset == 16
    assert HsgRel.n_dwork.offset == 72 and HsgRel.dwork.offset == 80 and HsgRel.swork.offset == 88


def test_code_object_is_gfx950():
    from hetersumgraph_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data
    assert _lib.load() is not None
    assert "gfx950" in _lib.version()


def test_host_mirror_of_dw_tiles():
    """bench.dw_tiles (the byte count's host mirror, no HIP call) equals the library's
    hsg_gemm_dw_tiles (a host-only query: no GPU needed) on the FFN shapes and a sweep."""
    import bench
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    shapes = [(300, 512), (512, 300), (64, 512), (512, 64), (4, 4), (160, 128), (161, 129), (1024, 768)]
    shapes += [(m, n) for m in range(4, 700, 36) for n in range(4, 700, 52)]
    for m, n in shapes:
        assert bench.dw_tiles(m, n) == lib.hsg_gemm_dw_tiles(m, n), (m, n)
