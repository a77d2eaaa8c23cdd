"""Dev tool: hsg_gemm_f32_psw_plan plans back to back on the cfg2 N = 512 FFN shapes
(ffn1: bias + relu; dH: relu mask + column partials), interleaved rounds in one process,
with a bitwise check of every plan against plan 7.

usage: python tools/gemm13_ab.py [M] [plan,plan,...]     (default 19200 7,13)
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from hetersumgraph_amd.dense import gemm_psw, psw_row_tiles, split_weights
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 19200
    plans = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [7, 13]
    N, K = 512, 300
    torch.manual_seed(0)
    X = torch.randn(M, K, device="cuda")
    G = torch.randn(M, K, device="cuda")
    W1 = torch.randn(N, K, device="cuda") * 0.05
    W2 = torch.randn(K, N, device="cuda") * 0.05
    b = torch.randn(N, device="cuda")
    s1, s2t = split_weights((W1, False), (W2, True))
    H = gemm_psw(X, s1, bias=b, relu=True, plan=7)
    part = torch.zeros(psw_row_tiles(M, N, K), N, device="cuda")
    out = torch.empty(M, N, device="cuda")
    calls = {"ffn1": lambda p: gemm_psw(X, s1, bias=b, relu=True, out=out, plan=p),
             "dH": lambda p: gemm_psw(G, s2t, relu_mask=H, colsum_part=part, out=out, plan=p)}
    for name, f in calls.items():
        ref, pref = f(7).clone(), part.clone()
        for p in plans:
            same = torch.equal(f(p), ref) and (name == "ffn1" or torch.equal(part, pref))
            print(f"{name} plan {p}: bitwise plan 7's: {same}", flush=True)
    res = {}
    for name, f in calls.items():
        for p in plans:
            for _ in range(5):
                f(p)
        for _ in range(7):
            for p in plans:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    f(p)
                e1.record()
                torch.cuda.synchronize()
                res.setdefault((name, p), []).append(e0.elapsed_time(e1) * 1000 / 20)
    for (name, p), v in res.items():
        print(f"M={M} {name} plan {p}: median {statistics.median(v):.1f} us  min {min(v):.1f}  max {max(v):.1f}")


if __name__ == "__main__":
    main()
