"""What is specific to the C ABI of the selection on word ids (include/hsg_eval_words.h): the
host query answers as documented at each edge, refusals return HSG_EINVAL before any launch,
and every entry point of the header that writes through a pointer has a guard-band case in
tests/test_gpu_eval_words_guard.py.  Names, exports and signatures are
tests/test_abi_conformance.py's.  No GPU needed."""
import abi

HEADER = "hsg_eval_words.h"


def test_supported_limits():
    from hetersumgraph_amd import _lib, evalsel
    lib = _lib.load()
    for n_max, n_win, tab_cap, want in ((1, 1, 64, 1), (1024, 8, 8192, 1), (50, 3, 1024, 1),
                                        (0, 3, 64, 0), (-1, 3, 64, 0), (1025, 3, 64, 0),          # n_max
                                        (50, 0, 64, 0), (50, -1, 64, 0), (50, 9, 64, 0), (50, 8, 64, 1),   # n_win
                                        (50, 3, 32, 0), (50, 3, 63, 0), (50, 3, 65, 0), (50, 3, 96, 0), (50, 3, 128, 1),
                                        (50, 3, 8191, 0), (50, 3, 8192, 1), (50, 3, 8193, 0), (50, 3, 16384, 0),
                                        (50, 3, 0, 0), (50, 3, -64, 0), (50, 3, -2 ** 31, 0)):
        assert bool(lib.hsg_eval_words_supported(n_max, n_win, tab_cap)) == bool(want), (n_max, n_win, tab_cap)
        assert evalsel.words_supported(n_max, n_win, tab_cap) == bool(want)


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands
    for a non-NULL device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p = _lib.load(), _lib.HSG_EINVAL, 16

    def sel(n=9, B=3, logits=p, labels=p, doc_off=p, m=3, n_max=5, n_win=3, word_ptr=p, word_ids=p, tab_cap=64,
            sel=p, sel_ld=3, nsel=p, doc_counts=p, totals=p):
        return lib.hsg_eval_select_words(n, B, logits, labels, doc_off, m, n_max, n_win, word_ptr, word_ids, tab_cap,
                                         sel, sel_ld, nsel, doc_counts, totals, None)
    for kw in (dict(n=-1), dict(B=0), dict(B=-2), dict(m=-1),
               dict(n_max=0), dict(n_max=1025), dict(n_win=0), dict(n_win=9), dict(tab_cap=32), dict(tab_cap=96),
               dict(tab_cap=16384), dict(tab_cap=0), dict(tab_cap=-64),                    # unsupported
               dict(sel_ld=2), dict(m=0, sel_ld=4), dict(m=9, sel_ld=4), dict(sel_ld=0), dict(sel_ld=-1),
               dict(logits=None), dict(labels=None), dict(doc_off=None), dict(sel=None), dict(nsel=None),
               dict(doc_counts=None), dict(totals=None),
               dict(word_ids=None),                                                        # word_ptr without word_ids
               dict(word_ptr=None, word_ids=None, tab_cap=96), dict(word_ptr=None, word_ids=None, n_win=9),
               dict(m=0, n_max=1025, sel_ld=1025)):                                        # checked without blocking too
        assert sel(**kw) == EINVAL, kw


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_eval_words_guard import CASES
    w = abi.writable_entry_points([HEADER])
    for prm in ("int32_t *sel", "int32_t *nsel", "int32_t *doc_counts", "int64_t *totals"):
        assert prm in w["hsg_eval_select_words"], prm
    assert "hsg_eval_words_supported" not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
