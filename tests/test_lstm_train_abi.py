"""What is specific to the C ABI of the sentence LSTM's training path
(include/hsg_lstm_train.h): its source is built, the host queries answer as documented,
refusals return HSG_EINVAL before any HIP call, and every entry point of the header that
writes through a pointer has a guard-band case in tests/test_gpu_lstm_train_guard.py.  Names,
exports, signatures and the header's place among the build's dependencies are
tests/test_abi_conformance.py's.  No GPU needed."""
import ctypes
import os

import abi
import lstm_train_ref as R

HEADER = "hsg_lstm_train.h"


def test_the_source_is_built():
    from hetersumgraph_amd import build
    assert any(os.path.basename(s) == "hsg_lstm_train.hip" for s in build.SOURCES)


def test_supported_set():
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    for hid, ndir, inp in ((128, 1, 4), (128, 2, 300), (128, 2, 256), (128, 1, 4096)):
        assert lib.hsg_lstm_train_supported(hid, ndir, inp), (hid, ndir, inp)
    for hid, ndir, inp in ((64, 2, 300), (256, 2, 300), (128, 0, 300), (128, 3, 300), (128, 2, 302), (128, 2, 0),
                           (128, 2, -4), (0, 2, 300)):
        assert not lib.hsg_lstm_train_supported(hid, ndir, inp), (hid, ndir, inp)


def test_size_queries():
    from hetersumgraph_amd import _lib
    lib = _lib.load()
    C = lib.hsg_lstm_dw_chunk()
    assert C == R.CHUNK == 192
    per = 1024 * (300 + 128 + 1)
    sizes = [lib.hsg_lstm_dw_ws_floats(n, 2, 300) for n in (-1, 0, 1, C - 1, C, C + 1, 1120)]
    assert sizes == [0, 0, per, per, per, 2 * per, 6 * per] == [R.ws_floats(n, 2, 300) for n in (-1, 0, 1, C - 1, C,
                                                                                                   C + 1, 1120)]
    assert lib.hsg_lstm_dw_ws_floats(10, 1, 4) == 512 * 133
    assert lib.hsg_lstm_dw_ws_floats(10, 2, 302) == 0 and lib.hsg_lstm_dw_ws_floats(10, 3, 300) == 0
    # the cfg2 shape puts at least 256 blocks on the device (grid: column tiles x M / 128 x chunks)
    for inp in (300, 256):
        assert -(-((inp + 15) // 16 * 16 + 128) // 64) * (1024 // 128) * -(-1120 // C) >= 256

    for layers, ndir, inp in ((2, 2, 300), (1, 1, 4), (4, 2, 256), (3, 1, 300)):
        off = R.pack_offsets(layers, ndir, inp)
        assert [lib.hsg_lstm_pack_layer_offset(l, 128, ndir, inp) for l in range(layers + 1)] == off
        assert lib.hsg_lstm_pack_floats(layers, 128, ndir, inp) == off[-1]
        assert all(o % 4 == 0 for o in off)
    assert lib.hsg_lstm_pack_floats(2, 128, 2, 300) == 1024 * 429 + 1024 * 385
    for args in ((0, 128, 2, 300), (-1, 128, 2, 300), (5, 128, 2, 300), (2, 64, 2, 300), (2, 128, 2, 302),
                 (2, 128, 3, 300)):
        assert lib.hsg_lstm_pack_floats(*args) == 0, args
    assert lib.hsg_lstm_pack_layer_offset(-1, 128, 2, 300) == 0 == lib.hsg_lstm_pack_layer_offset(5, 128, 2, 300)
    assert lib.hsg_lstm_pack_layer_offset(1, 64, 2, 300) == 0


def test_refusals_before_any_hip_call():
    """HSG_EINVAL paths that return before a launch (so they run without a GPU); 16 stands for
    a non-NULL, 16-byte aligned device pointer that is never dereferenced."""
    from hetersumgraph_amd import _lib
    lib, EINVAL, p = _lib.load(), _lib.HSG_EINVAL, 16

    def table(n, hole=None, odd=None):
        t = [p] * n
        if hole is not None:
            t[hole] = None
        if odd is not None:
            t[odd] = 24
        return (ctypes.c_void_p * n)(*t)

    def pack(n_layers=2, hid=128, ndir=2, inp=300, params=table(16), out=p):
        return lib.hsg_lstm_pack(n_layers, hid, ndir, inp, params, out, None)
    for kw in (dict(n_layers=0), dict(n_layers=-1), dict(n_layers=5), dict(hid=64), dict(hid=-128), dict(ndir=0),
               dict(ndir=3), dict(inp=302), dict(inp=0), dict(inp=-4), dict(params=None), dict(out=None), dict(out=24),
               dict(params=table(16, hole=0)), dict(params=table(16, hole=15)), dict(params=table(16, odd=9))):
        assert pack(**kw) == EINVAL, kw

    def dw(n_docs=3, n_rows=9, hid=128, ndir=2, inp=300, doc_off=p, dg=p, x=p, ld_x=300, h=p, ld_h=256, ws=p, dwih=p,
           dwhh=p, db=p):
        return lib.hsg_lstm_dw(n_docs, n_rows, hid, ndir, inp, doc_off, dg, x, ld_x, h, ld_h, ws, dwih, dwhh, db, None)
    for kw in (dict(n_docs=-1), dict(n_rows=-1), dict(hid=64), dict(hid=0), dict(ndir=0), dict(ndir=3), dict(inp=302),
               dict(inp=0), dict(inp=-4), dict(doc_off=None), dict(dg=None), dict(x=None), dict(h=None), dict(ws=None),
               dict(dwih=None), dict(dwhh=None), dict(db=None), dict(ld_x=299), dict(ld_x=-300), dict(ld_h=255),
               dict(ndir=1, ld_h=127), dict(ws=8), dict(dwih=24), dict(dwhh=4), dict(db=20),
               dict(n_rows=65535 * 192 + 1),
               # the outputs are checked even where there is nothing to sum
               dict(n_rows=0, dwih=None), dict(n_docs=0, db=None), dict(n_rows=0, dwhh=24)):
        assert dw(**kw) == EINVAL, kw


def test_every_writing_entry_point_has_a_guard_case():
    from test_gpu_lstm_train_guard import CASES
    w = abi.writable_entry_points([HEADER])
    assert w["hsg_lstm_pack"] == ["float *out"]
    assert w["hsg_lstm_dw"] == ["float *ws", "float *dW_ih", "float *dW_hh", "float *db"]
    for name in ("hsg_lstm_train_supported", "hsg_lstm_pack_layer_offset", "hsg_lstm_pack_floats", "hsg_lstm_dw_chunk",
                 "hsg_lstm_dw_ws_floats"):
        assert name not in w
    assert sorted(CASES) == sorted(w)
    for name, cs in CASES.items():
        assert cs, name
