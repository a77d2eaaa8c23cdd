"""What is specific to the C ABI of the model glue (include/hsg_model.h): the supported
sets and host queries, refusals that return HSG_EINVAL before any launch, and every entry
point of the header that writes through a pointer has a guard-band case in
tests/test_gpu_model_guard.py.  Names, exports and signatures are
tests/test_abi_conformance.py's.  No GPU needed."""
import abi

HEADER = "hsg_model.h"


def test_supported_sets_and_host_queries():
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    assert lib.hsg_sentfeat_supported(300, 128, 256, 64) and lib.hsg_sentfeat_supported(300, 128, 128, 64)
    for bad in ((300, 64, 256, 64), (300, 128, 256, 32), (302, 128, 256, 64), (300, 128, 130, 64), (516, 128, 256, 64),
                (0, 128, 256, 64)):
        assert not lib.hsg_sentfeat_supported(*bad), bad
    assert lib.hsg_docinit_supported(64) and not lib.hsg_docinit_supported(128)
    assert lib.hsg_logits_supported(64) and lib.hsg_logits_supported(128) and not lib.hsg_logits_supported(66)
    rows = lib.hsg_sentfeat_rows()
    assert rows >= 1 and -(-1120 // rows) >= 256          # a config-2 batch: at least one block per CU
    assert [lib.hsg_logits_bwd_blocks(n) for n in (-1, 0, 1, 64, 65)] == [0, 0, 1, 1, 2]


def test_refusals_before_any_launch():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands
    for a non-NULL, 16-byte aligned device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p = _lib.load(), _lib.HSG_EINVAL, 16
    D = (300, 128, 256, 64)

    def fwd(n=4, dims=D, n_pos=51, ngram=p, ldn=300, pos=p, P=p, L=p, ldl=256, Wc=p, bc=p, Wl=p, bl=p, Wn=p, X=p, ldx=300,
            F=p, ldf=256, S=p, lds=64):
        return lib.hsg_sentfeat_fwd(n, *dims, n_pos, ngram, ldn, pos, P, L, ldl, Wc, bc, Wl, bl, Wn, X, ldx, F, ldf, S, lds,
                                    None)
    for kw in (dict(n=-1), dict(dims=(300, 64, 256, 64)), dict(dims=(302, 128, 256, 64)), dict(ldn=299), dict(ldl=255),
               dict(ldx=299), dict(ldf=255), dict(lds=63), dict(ngram=None), dict(pos=None), dict(P=None), dict(L=None),
               dict(Wc=None), dict(bc=None), dict(Wl=None), dict(bl=None), dict(Wn=None), dict(F=None), dict(S=None),
               dict(Wc=20)):
        assert fwd(**kw) == EINVAL, kw
    assert fwd(n=0, ngram=None, S=None) == 0                                     # n == 0: nothing to do

    def bwd(n=4, dims=D, dS=p, ldds=64, Wc=p, Wl=p, Wn=p, dF=p, lddf=256, dng=p, lddn=300, dL=p, lddl=256):
        return lib.hsg_sentfeat_bwd(n, *dims, dS, ldds, Wc, Wl, Wn, dF, lddf, dng, lddn, dL, lddl, None)
    for kw in (dict(n=-1), dict(dims=(300, 128, 256, 128)), dict(ldds=63), dict(lddf=255), dict(lddn=299), dict(lddl=255),
               dict(dS=None), dict(Wc=None), dict(Wl=None), dict(Wn=None), dict(dF=None)):
        assert bwd(**kw) == EINVAL, kw
    assert bwd(n=0, dS=None) == 0

    def dfwd(n_s=3, n_docs=1, n_super=4, Hs=64, S=p, lds=64, src=p, dptr=p, dsent=p, inv=p, Wd=p, mean=p, init=p, ldi=64):
        return lib.hsg_docinit_fwd(n_s, n_docs, n_super, Hs, S, lds, src, dptr, dsent, inv, Wd, mean, init, ldi, None)
    for kw in (dict(n_s=-1), dict(n_docs=-1), dict(n_super=-1), dict(Hs=32), dict(lds=63), dict(ldi=63), dict(S=None),
               dict(src=None), dict(dptr=None), dict(dsent=None), dict(inv=None), dict(Wd=None), dict(mean=None),
               dict(init=None)):
        assert dfwd(**kw) == EINVAL, kw
    assert dfwd(n_super=0, init=None) == 0

    def dbwd(n_s=3, n_docs=1, n_super=4, Hs=64, dI=p, ldd=64, srow=p, drow=p, sptr=p, sdoc=p, inv=p, Wd=p, mean=p, dS=p,
             ldds=64, dWd=p):
        return lib.hsg_docinit_bwd(n_s, n_docs, n_super, Hs, dI, ldd, srow, drow, sptr, sdoc, inv, Wd, mean, dS, ldds, dWd,
                                   None)
    for kw in (dict(n_s=-1), dict(Hs=128), dict(ldd=63), dict(ldds=63), dict(dI=None), dict(srow=None), dict(drow=None),
               dict(sptr=None), dict(sdoc=None), dict(inv=None), dict(Wd=None), dict(mean=None)):
        assert dbwd(**kw) == EINVAL, kw
    assert dbwd(dS=None, dWd=None) == 0                                          # nothing wanted

    def lfwd(n=4, Hs=64, n_super=4, state=p, ldst=64, ss=None, dsup=None, Wh=p, bh=p, out=p):
        return lib.hsg_logits_fwd(n, Hs, n_super, state, ldst, ss, dsup, Wh, bh, out, None)
    for kw in (dict(n=-1), dict(Hs=66), dict(ldst=63), dict(ss=p), dict(dsup=p), dict(n_super=5), dict(state=None),
               dict(Wh=None), dict(bh=None), dict(out=None)):
        assert lfwd(**kw) == EINVAL, kw
    assert lfwd(n=0, n_super=0, out=None) == 0

    def lbwd(n=4, Hs=64, n_super=4, dl=p, state=p, ldst=64, ss=None, dsup=None, sups=None, supp=None, supl=None, Wh=p,
             dstate=p, ldd=64, ws=p, dWh=p, dbh=p):
        return lib.hsg_logits_bwd(n, Hs, n_super, dl, state, ldst, ss, dsup, sups, supp, supl, Wh, dstate, ldd, ws, dWh, dbh,
                                  None)
    for kw in (dict(n=-1), dict(Hs=2), dict(ldst=63), dict(ldd=63), dict(ss=p), dict(n_super=3), dict(dl=None),
               dict(Wh=None), dict(ws=None), dict(dWh=None), dict(dbh=None), dict(state=None),
               dict(ss=p, dsup=p, n_super=6)):                                    # HDSG without the inverse lists
        assert lbwd(**kw) == EINVAL, kw
    assert lbwd(n=0, n_super=0) == 0


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_model_guard import CASES
    w = abi.writable_entry_points([HEADER])
    assert "float *S" in w["hsg_sentfeat_fwd"] and "float *X" in w["hsg_sentfeat_fwd"]
    assert "float *dngram" in w["hsg_sentfeat_bwd"] and "float *mean" in w["hsg_docinit_fwd"]
    assert "float *dWd" in w["hsg_docinit_bwd"] and "float *logits" in w["hsg_logits_fwd"]
    assert "float *ws" in w["hsg_logits_bwd"] and "float *dbh" in w["hsg_logits_bwd"]
    for name in ("hsg_sentfeat_supported", "hsg_sentfeat_rows", "hsg_docinit_supported", "hsg_logits_supported",
                 "hsg_logits_bwd_blocks"):
        assert name not in w
    missing = sorted(n for n in w if n not in CASES)
    assert not missing, f"no guard-band case: {missing}"
    assert set(CASES) <= set(w), sorted(set(CASES) - set(w))
    for name, cs in CASES.items():
        assert cs, name
