"""What is specific to the C ABI of the word ids from article bytes (include/hsg_eval_text.h):
the host queries answer as documented at each edge (their 64-bit return types included),
refusals return HSG_EINVAL before any launch, and every entry point of the header that writes
through a pointer has a guard-band case in tests/test_gpu_eval_text_guard.py.  Names, exports
and signatures are tests/test_abi_conformance.py's.  No GPU needed."""
import abi

HEADER = "hsg_eval_text.h"


def test_host_queries():
    from hetersumgraph_amd import _lib, evalsel
    lib = _lib.load()
    for n, B, nbytes, want in ((0, 1, 0, 1), (1120, 32, 184000, 1), (2 ** 20, 2 ** 20, 2 ** 30, 1),
                               (-1, 1, 0, 0), (2 ** 20 + 1, 1, 0, 0),                      # n
                               (5, 0, 10, 0), (5, -1, 10, 0), (5, 2 ** 20 + 1, 10, 0),     # B
                               (5, 1, -1, 0), (5, 1, 2 ** 30 + 1, 0), (5, 1, 2 ** 40, 0)):  # nbytes
        assert bool(lib.hsg_eval_text_supported(n, B, nbytes)) == bool(want), (n, B, nbytes)
        assert evalsel.text_supported(n, B, nbytes) == bool(want)
        bound = (nbytes + n) // 2 if want else 0
        assert lib.hsg_eval_text_workspace_bytes(n, B, nbytes) == (4 * (4 * bound + B + 1) if want else 0)
    for n, nbytes, want in ((0, 0, 0), (1, 0, 0), (1, 1, 1), (3, 4, 3), (3, 5, 4), (1120, 184000, 92560),
                            (2 ** 20, 2 ** 30, 2 ** 29 + 2 ** 19), (-1, 8, 0), (4, -2, 0), (4, 2 ** 30 + 1, 0)):
        assert lib.hsg_eval_text_word_bound(n, nbytes) == want, (n, nbytes)


def test_the_bound_covers_every_row_split():
    """sum over rows of ceil(L_i / 2) <= (nbytes + n) / 2 when the rows share nbytes bytes."""
    import numpy as np
    rng = np.random.default_rng(0)
    for _ in range(200):
        lens = rng.integers(0, 7, int(rng.integers(0, 9)))
        assert int(((lens + 1) // 2).sum()) <= (int(lens.sum()) + len(lens)) // 2


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands
    for a non-NULL device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p = _lib.load(), _lib.HSG_EINVAL, 16

    def words(n=9, B=3, text=p, nbytes=40, byte_ptr=p, doc_off=p, word_cap=24, word_ptr=p, word_ids=p, ws=p):
        return lib.hsg_eval_text_words(n, B, text, nbytes, byte_ptr, doc_off, word_cap, word_ptr, word_ids, ws, None)
    for kw in (dict(n=-1), dict(n=2 ** 20 + 1, word_cap=2 ** 21), dict(B=0), dict(B=-2), dict(B=2 ** 20 + 1),
               dict(nbytes=-1), dict(nbytes=2 ** 30 + 1, word_cap=2 ** 31),
               dict(word_cap=23), dict(word_cap=0), dict(word_cap=-1),          # the bound is (40 + 9) / 2 = 24
               dict(text=None), dict(byte_ptr=None), dict(doc_off=None), dict(word_ptr=None), dict(word_ids=None),
               dict(ws=None)):
        assert words(**kw) == EINVAL, kw


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_eval_text_guard import CASES
    w = abi.writable_entry_points([HEADER])
    for prm in ("int32_t *word_ptr", "int32_t *word_ids", "void *ws"):
        assert prm in w["hsg_eval_text_words"], prm
    for name in ("hsg_eval_text_supported", "hsg_eval_text_word_bound", "hsg_eval_text_workspace_bytes"):
        assert name not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
