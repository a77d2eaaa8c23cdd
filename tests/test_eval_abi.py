"""What is specific to the C ABI of the evaluation step's selection (include/hsg_eval.h): the
host query answers as documented, refusals return HSG_EINVAL before any launch, the Python
wrapper refuses what it must, and every entry point of the header that writes through a
pointer has a guard-band case in tests/test_gpu_eval_guard.py.  Names, exports and
signatures are tests/test_abi_conformance.py's.  No GPU needed."""
import pytest

import abi

HEADER = "hsg_eval.h"


def test_supported_limits():
    from hetersumgraph_amd import _lib, evalsel
    lib = _lib.load()
    for n_max, gram_max, want in ((1, 0, 1), (1024, 262144, 1), (1025, 0, 0), (1024, 262145, 0), (0, 0, 0),
                                  (-1, 0, 0), (50, -1, 0), (50, 1, 1), (1024, 0, 1), (1, 262144, 1)):
        assert bool(lib.hsg_eval_select_supported(n_max, gram_max)) == bool(want), (n_max, gram_max)
        assert evalsel.supported(n_max, gram_max) == bool(want)


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands
    for a non-NULL device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p = _lib.load(), _lib.HSG_EINVAL, 16

    def sel(n=9, B=3, logits=p, labels=p, doc_off=p, m=3, n_max=5, gram_ptr=p, gram_ids=p, gram_cnt=p, gram_max=40,
            sel=p, sel_ld=3, nsel=p, doc_counts=p, totals=p):
        return lib.hsg_eval_select(n, B, logits, labels, doc_off, m, n_max, gram_ptr, gram_ids, gram_cnt, gram_max,
                                   sel, sel_ld, nsel, doc_counts, totals, None)
    for kw in (dict(n=-1), dict(B=0), dict(B=-2), dict(m=-1),
               dict(n_max=0), dict(n_max=1025), dict(gram_max=-1), dict(gram_max=262145),     # unsupported
               dict(sel_ld=2), dict(m=0, sel_ld=4), dict(m=9, sel_ld=4), dict(sel_ld=0), dict(sel_ld=-1),
               dict(logits=None), dict(labels=None), dict(doc_off=None), dict(sel=None), dict(nsel=None),
               dict(doc_counts=None), dict(totals=None),
               dict(gram_ids=None), dict(gram_cnt=None), dict(gram_ids=None, gram_cnt=None),
               dict(gram_ptr=None, gram_ids=None, gram_cnt=None, gram_max=262145),          # checked without blocking too
               dict(m=0, n_max=1025, sel_ld=1025)):
        assert sel(**kw) == EINVAL, kw


def test_python_wrapper_refuses_cpu_tensors_and_unsupported_limits():
    import torch

    from hetersumgraph_amd import evalsel
    logits, labels = torch.zeros(3, 2), torch.zeros(3, dtype=torch.int64)
    off, totals = torch.tensor([0, 3], dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        evalsel.select(logits, labels, off, 3, 3, totals)
    with pytest.raises(RuntimeError, match="ROCm device"):
        evalsel.select(logits.double(), labels, off, 3, 3, totals)


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_eval_guard import CASES
    w = abi.writable_entry_points([HEADER])
    for prm in ("int32_t *sel", "int32_t *nsel", "int32_t *doc_counts", "int64_t *totals"):
        assert prm in w["hsg_eval_select"], prm
    assert "hsg_eval_select_supported" not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
