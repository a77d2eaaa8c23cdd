"""What is specific to the C ABI of the training-step tail (include/hsg_train.h):
include/hsg.h's own set is untouched, the layout numbers and host queries, refusals before
any launch, and every entry point of the header that writes through a pointer has a
guard-band case in tests/test_gpu_train_guard.py.  Names, exports and signatures are
tests/test_abi_conformance.py's.  No GPU needed."""
import ctypes

import abi

HEADER = "hsg_train.h"


def test_hsg_h_is_unchanged():
    """The training tail adds nothing to include/hsg.h: its declarations are still
    exactly the registry's for hsg.h, and none of the new names is among them."""
    from hetersumgraph_amd import _lib
    old = abi.declared_functions("hsg.h")
    assert old == sorted(_lib.exports("hsg.h"))
    assert not set(old) & set(abi.declared_functions(HEADER))
    assert not set(old) & set(_lib.exports(HEADER))


def test_struct_layout_and_host_queries():
    from hetersumgraph_amd import _lib
    from train_ref import CHUNK
    assert ctypes.sizeof(_lib.HsgMtTensor) == 40 and _lib.HsgMtTensor.n.offset == 32
    lib = _lib.load()
    K = lib.hsg_mt_tensors_per_launch()
    assert K == 64 and lib.hsg_mt_chunk() == CHUNK
    # the table goes into the kernel arguments by value: descriptors + block offsets + count
    assert K * 40 + (K + 1) * 4 + 4 == 2824 < 4096 - 256
    mk = lambda ns: (_lib.HsgMtTensor * len(ns))(*[_lib.HsgMtTensor(16, 16, 16, 16, n) for n in ns])
    ns = [1, 0, CHUNK, CHUNK + 1, 3 * CHUNK - 1]
    assert lib.hsg_mt_blocks(mk(ns), len(ns)) == 1 + 0 + 1 + 2 + 3
    assert lib.hsg_mt_blocks(None, 0) == 0
    bad = ctypes.c_size_t(-1).value
    assert lib.hsg_mt_blocks(mk([4, -1]), 2) == bad
    assert lib.hsg_mt_blocks((_lib.HsgMtTensor * 1)(_lib.HsgMtTensor(16, None, 16, 16, 4)), 1) == bad


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU)."""
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    one = (_lib.HsgMtTensor * 1)(_lib.HsgMtTensor(16, 16, 16, 16, 4))
    assert lib.hsg_doc_ce(4, 3, 1, 16, 16, 1, 4, None, 16, 16, 16, 16, 16, None) == _lib.HSG_EINVAL     # C != 2
    assert lib.hsg_doc_ce(4, 2, 0, 16, 16, 1, 4, None, 16, 16, 16, 16, 16, None) == _lib.HSG_EINVAL     # B < 1
    assert lib.hsg_mt_sqnorm(one, 1, None, None, None) == _lib.HSG_EINVAL                               # no partials
    assert lib.hsg_mt_adam(one, 1, 16, None, 0, None, None) == _lib.HSG_EINVAL                          # no hyper
    nostate = (_lib.HsgMtTensor * 1)(_lib.HsgMtTensor(16, 16, None, None, 4))
    assert lib.hsg_mt_adam(nostate, 1, 16, 16, 0, None, None) == _lib.HSG_EINVAL                        # no m, v


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_train_guard import CASES
    w = abi.writable_entry_points([HEADER])
    assert "float *partials" in w["hsg_mt_sqnorm"] and "double *hyper" in w["hsg_mt_sqnorm"]
    assert "float *norm_out" in w["hsg_mt_adam"] and "float *dlogits" in w["hsg_doc_ce"]
    for name in ("hsg_mt_blocks", "hsg_mt_chunk", "hsg_mt_tensors_per_launch"):
        assert name not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
