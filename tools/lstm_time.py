"""Dev tool (GPU): the sentence LSTM's recurrence launches alone (hsg_lstm_fwd /
hsg_lstm_bwd, one layer, both directions), HIP-event time per launch over REPS
back-to-back launches, for batches of equal-length documents.

    python tools/lstm_time.py [docs x len ...]      (default: 32x35 32x50 32x80 1x80 256x35)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hetersumgraph_amd import lstm as hl  # noqa: E402
from hetersumgraph_amd._lib import check, load, ptr, stream_of  # noqa: E402

REPS = 50
dev = torch.device("cuda", 0)
lib = load()
shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(32, 35), (32, 50), (32, 80), (1, 80),
                                                                         (256, 35)]


def timed(fn):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


for n_docs, length in shapes:
    torch.manual_seed(0)
    lay = hl.doc_layout([length] * n_docs, dev)
    n, hid, ndir = lay.n_rows, 128, 2
    pre = torch.randn(n, ndir * 4 * hid, device=dev)
    whh = torch.empty(ndir, 4 * hid, hid, device=dev).uniform_(-hid ** -0.5, hid ** -0.5)
    h, c = torch.empty(n, ndir * hid, device=dev), torch.empty(n, ndir * hid, device=dev)
    gates, dg = torch.empty_like(pre), torch.empty_like(pre)
    dy = torch.randn(n, ndir * hid, device=dev)
    st = stream_of(pre)

    def fwd():
        check(lib.hsg_lstm_fwd(n_docs, n, hid, ndir, ptr(lay.doc_off), ptr(pre), pre.stride(0), ptr(whh), ptr(h),
                               h.stride(0), ptr(gates), ptr(c), 0.0, None, 0, None, 0, st), "hsg_lstm_fwd")

    def bwd():
        check(lib.hsg_lstm_bwd(n_docs, n, hid, ndir, ptr(lay.doc_off), ptr(dy), dy.stride(0), ptr(gates), ptr(c),
                               ptr(whh), 0.0, None, 0, ptr(dg), st), "hsg_lstm_bwd")

    tf, tb = timed(fwd), timed(bwd)
    print(json.dumps({"docs": n_docs, "len": length, "fwd_us": round(tf, 1), "bwd_us": round(tb, 1),
                      "fwd_us_per_step": round(tf / length, 3), "bwd_us_per_step": round(tb / length, 3)}), flush=True)
