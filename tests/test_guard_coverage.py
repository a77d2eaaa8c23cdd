"""Every entry point of the C ABI that writes through a pointer has a guard-band case
(tests/test_gpu_guard_bands.py, CASES) or an explicit reason not to (NOT_COVERED).  A new
entry point fails this test until someone decides where it goes.  No GPU needed."""
import abi

HEADERS = ["hsg.h", "hsg_graph.h"]

DEV_ONLY = "dev / A-B variant: no Python caller on the product path under default options"
NOT_COVERED = {
    # variants the product path does not call
    "hsg_gemm_f32_mfma": DEV_ONLY + " (the exact-f32 MFMA GEMM; gemm(dtype='f32mfma') in tests and tools only)",
    "hsg_gemm_psw_ln": DEV_ONLY + " (the product library declines every call: HSG_EINVAL before any launch)",
    "hsg_hproj_fwd_mf": DEV_ONLY + " (the MFMA narrow-head projection; hproj.py calls hsg_hproj_fwd_t8)",
    # host-side code: nothing is written on the device
    "hsg_wsplit_dims": "host-only query: writes two ints through host pointers (asserted equal to ceil128 / ceil32 in "
                       "every hsg_wsplit case)",
    "hsg_graph_count": "host graph builder (libhsg_host.so, no HIP): host arrays; tests/test_graphbuild.py",
    "hsg_graph_fill": "host graph builder (libhsg_host.so, no HIP): host arrays; tests/test_graphbuild.py",
    # probes
    "hsg_kclock_arm": "measurement hook: its pointers are a stream and two hipEvent_t handles, no buffer is written",
}


def test_parser_sees_the_abi():
    w = abi.writable_entry_points(HEADERS)
    assert set(w) - {"hsg_graph_count", "hsg_graph_fill"} <= set(abi.declared_functions("hsg.h"))
    # spot checks: outputs, arrays of output pointers, const-only and pointer-free functions
    assert "float *out" in w["hsg_gat_fwd"] and "void *out16" in w["hsg_gat_fwd_ws16"]
    assert "float *const *ws" in w["hsg_gemm_dw_slabs"] and "void *const *planes" in w["hsg_wsplit"]
    assert "int64_t *seed" in w["hsg_seed_advance"] and "uint32_t *const *bits" in w["hsg_dropmask_multi"]
    for name in ("hsg_gat_bwd_blocks", "hsg_gemm_workspace_floats", "hsg_dropmask_words", "hsg_version",
                 "hsg_gat_fwd_ws_floats", "hsg_gemm_f32_psw_route"):
        assert name not in w
    assert len(w) >= 60


def test_every_writing_entry_point_has_a_case_or_a_reason():
    from test_gpu_guard_bands import CASES
    w = abi.writable_entry_points(HEADERS)
    missing = sorted(n for n in w if n not in CASES and n not in NOT_COVERED)
    assert not missing, f"no guard-band case and no NOT_COVERED reason: {missing}"
    for name, reason in NOT_COVERED.items():
        assert isinstance(reason, str) and len(reason) > 20, name
        assert name in w, f"NOT_COVERED names {name}, which the headers do not declare as writing"
        assert name not in CASES, f"{name} has a case and a NOT_COVERED reason"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
