// hsg_embed.hip -- the trainable word embedding (include/hsg_embed.h) for gfx950: the
// word-node row lookup and the dense gradient over both uses of the shared nn.Embedding
// (word nodes, HiGraph.py:144-152; sentence CNN rows, module/Encoder.py:56-68).
//
// The gradient is a segmented sum over a SORTED occurrence list (token, source row), the
// store-and-sum form of a scatter-add: no float atomics, one fixed order.  A batch's
// tokens are heavily skewed (function words and punctuation occur thousands of times, the
// median token a handful), so the list is cut by POSITION, not by token: one wave owns an
// aligned chunk of kPiece entries whatever tokens they hold, which bounds every wave's
// work; a run that crosses chunk boundaries leaves one partial row per chunk in a
// workspace and a second launch adds those in chunk order.  The order (hsg_embed.h
// "Summation order") is a function of list positions alone, so it is the same on every
// device and for every grid.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hsg_embed.h"

namespace {

constexpr int kPiece = 32;      // list entries per chunk (hsg_embed_piece_rows): <= 64, one key per lane
constexpr int kWaves = 4;       // waves per block
constexpr int kMaxD = 4096;
constexpr int kAhead = 4;       // source rows in flight per wave in the chunk walk
constexpr int kMergeAhead = 8;  // head slots in flight per wave in the merge

static_assert(kPiece >= 2 && kPiece <= 64 && kPiece % kAhead == 0, "one key per lane");

__device__ inline int tok_of(int64_t key) { return (int)(key >> 32); }

struct Src {
    const float *dW, *dX;
    long ldw, ldx, n_w, n_src;
};

// columns [4*c4, 4*c4 + 4) of source row s; a source outside both matrices is NaN
__device__ inline float4 src_row(const Src &S, long s, int c4) {
    const float *p;
    if (s < S.n_w) p = S.dW + s * S.ldw;
    else if (s < S.n_src) p = S.dX + (s - S.n_w) * S.ldx;
    else return make_float4(NAN, NAN, NAN, NAN);
    return *reinterpret_cast<const float4 *>(p + 4 * c4);
}

__device__ inline void add4(float4 &a, const float4 &b) {
    a.x = a.x + b.x;
    a.y = a.y + b.y;
    a.z = a.z + b.z;
    a.w = a.w + b.w;
}

// One wave per (chunk k, column group cg of 64 float4).  Lane l holds the key of list
// position k*kPiece + l; the walk reads token and source of position i from lane i, so
// every branch below is wave-uniform.
__global__ __launch_bounds__(64 * kWaves) void k_embed_chunks(int V, int D, long n_occ, long n_chunks, int n_cg,
                                                             const int64_t *__restrict__ occ, Src S,
                                                             float *__restrict__ dE, float *__restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (wave >= n_chunks * n_cg) return;
    const long k = wave / n_cg;
    const int c4 = (int)(wave - k * n_cg) * 64 + lane;
    const bool on = c4 < (D >> 2);
    const long p0 = k * kPiece;
    const int cnt = n_occ - p0 < kPiece ? (int)(n_occ - p0) : kPiece;
    const int64_t key = lane < cnt ? occ[p0 + lane] : (int64_t)-1;
    const int my_tok = tok_of(key);
    const int my_src = (int)(uint32_t)(key & 0xffffffffLL);
    const int tok_left = p0 > 0 ? tok_of(occ[p0 - 1]) : -1;
    const int tok_right = p0 + kPiece < n_occ ? tok_of(occ[p0 + kPiece]) : -1;

    int cur = -1;               // token of the open run (-1: none)
    bool from_left = false;     // the open run continues one of the previous chunk
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto flush = [&](bool to_right) {
        if (cur < 0 || !on) return;
        float *dst = from_left ? ws + (2 * k) * D : to_right ? ws + (2 * k + 1) * D : dE + (long)cur * D;
        *reinterpret_cast<float4 *>(dst + 4 * c4) = acc;
    };
    for (int i0 = 0; i0 < cnt; i0 += kAhead) {
        int t[kAhead];
        float4 v[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {       // issue the loads of kAhead positions, then add in order
            t[j] = __shfl(my_tok, i0 + j, 64);
            const long s = (long)(uint32_t)__shfl(my_src, i0 + j, 64);
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (on && t[j] >= 0 && t[j] < V) v[j] = src_row(S, s, c4);
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            if (i0 + j >= cnt) break;
            if (t[j] < 0 || t[j] >= V) {         // dropped entry: ends the run, adds nothing
                flush(false);
                cur = -1;
            } else if (t[j] != cur) {
                flush(false);
                cur = t[j];
                from_left = i0 + j == 0 && tok_left == cur;
                acc = v[j];                      // a piece starts from its first element
            } else {
                add4(acc, v[j]);
            }
        }
    }
    flush(tok_right == cur);
}

// The wave of the chunk in which a crossing run STARTS owns that run: tail slot of its
// chunk, then the head slots of the following chunks while they begin with the token.
__global__ __launch_bounds__(64 * kWaves) void k_embed_merge(int V, int D, long n_occ, long n_chunks, int n_cg,
                                                            const int64_t *__restrict__ occ,
                                                            float *__restrict__ dE, const float *__restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (wave >= n_chunks * n_cg) return;
    const long k = wave / n_cg;
    const int c4 = (int)(wave - k * n_cg) * 64 + lane;
    const bool on = c4 < (D >> 2);
    const long p0 = k * kPiece;
    if (p0 + kPiece >= n_occ) return;                                    // nothing to the right
    const int tk = tok_of(occ[p0 + kPiece - 1]);
    if (tk < 0 || tk >= V || tok_of(occ[p0 + kPiece]) != tk) return;      // the last run ends here
    if (p0 > 0 && tok_of(occ[p0]) == tk && tok_of(occ[p0 - 1]) == tk) return;   // it started further left
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) acc = *reinterpret_cast<const float4 *>(ws + (2 * k + 1) * D + 4 * c4);
    for (long j = k + 1; j < n_chunks; j += 64) {
        const long c = j + lane;                                         // 64 chunks' first tokens at once
        const bool same = c < n_chunks && tok_of(occ[c * kPiece]) == tk;
        const unsigned long long b = __ballot(same);
        const int n = b == ~0ull ? 64 : __ffsll(~b) - 1;                 // the chunks that continue the run
        for (int i0 = 0; i0 < n; i0 += kMergeAhead) {
            float4 v[kMergeAhead];
#pragma unroll
            for (int u = 0; u < kMergeAhead; ++u) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (on && i0 + u < n) v[u] = *reinterpret_cast<const float4 *>(ws + (2 * (j + i0 + u)) * D + 4 * c4);
            }
#pragma unroll
            for (int u = 0; u < kMergeAhead; ++u)
                if (i0 + u < n) add4(acc, v[u]);
        }
        if (n < 64) break;
    }
    if (on) *reinterpret_cast<float4 *>(dE + (long)tk * D + 4 * c4) = acc;
}

// keys[i] = token(i) << 32 | i for source i (word rows, then the CNN rows in hsg_cnn_gather's
// layout: the sentence of a row by binary search over rowoff, as k_cnn_gather); the
// padding token and tokens that do not fit 31 bits get the dropped key.
__global__ __launch_bounds__(256) void k_embed_keys(long n_w, int n, int L, long n_src, const int64_t *__restrict__ wid,
                                                    const int64_t *__restrict__ ids,
                                                    const int32_t *__restrict__ rowoff, long padding_idx,
                                                    int64_t *__restrict__ keys) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_src) return;
    int64_t tok;
    if (i < n_w) {
        tok = wid[i];
    } else {
        const long r = i - n_w;
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rowoff[mid] <= r) lo = mid;
            else hi = mid - 1;
        }
        const int t = (int)(r - rowoff[lo]);
        const int len = rowoff[lo + 1] - rowoff[lo] - 1;
        tok = t < len && t < L ? ids[(long)lo * L + t] : 0;
    }
    const bool drop = tok == padding_idx || tok < 0 || tok >= INT32_MAX;
    keys[i] = drop ? INT64_MAX : (tok << 32) | i;
}

// Xw[i] = E[wid[i]]; one wave per row, grid-stride.
__global__ __launch_bounds__(64 * kWaves) void k_embed_rows(int n_w, int V, int D, const int64_t *__restrict__ wid,
                                                           const float *__restrict__ E, float *__restrict__ Xw,
                                                           long ldx) {
    const int lane = threadIdx.x & 63;
    for (long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); r < n_w; r += (long)gridDim.x * kWaves) {
        const int64_t w = wid[r];
        const bool ok = w >= 0 && w < V;
        const float *er = E + (ok ? w : 0) * D;
        float *xr = Xw + r * ldx;
        for (int c = lane * 4; c < D; c += 256) {
            const float4 v = ok ? *reinterpret_cast<const float4 *>(er + c) : make_float4(NAN, NAN, NAN, NAN);
            *reinterpret_cast<float4 *>(xr + c) = v;
        }
    }
}

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

bool misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

bool bad_pitch(int ld, int D) { return ld < D || (ld & 3); }

}  // namespace

extern "C" {

int hsg_embed_supported(int D) { return D >= 4 && D <= kMaxD && D % 4 == 0; }

int hsg_embed_piece_rows(void) { return kPiece; }

size_t hsg_embed_ws_floats(long n_occ, int D) {
    if (n_occ <= 0 || !hsg_embed_supported(D)) return 0;
    return (size_t)2 * D * (size_t)((n_occ + kPiece - 1) / kPiece);
}

int hsg_embed_rows(int n_w, int V, int D, const int64_t *wid, const float *E, float *Xw, int ldx, void *stream) {
    if (n_w < 0 || V < 0 || !hsg_embed_supported(D) || bad_pitch(ldx, D)) return HSG_EINVAL;
    if (n_w && (!wid || !E || !Xw || misaligned(E) || misaligned(Xw))) return HSG_EINVAL;
    if (n_w == 0) return 0;
    int blocks = (n_w + kWaves - 1) / kWaves;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_embed_rows, dim3((unsigned)blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, n_w, V, D, wid,
                       E, Xw, (long)ldx);
    return status();
}

int hsg_embed_keys(int n_w, int n, int L, long rows, const int64_t *wid, const int64_t *ids, const int32_t *rowoff,
                   long padding_idx, int64_t *keys, void *stream) {
    if (n_w < 0 || n < 0 || L < 1 || rows < n || rows > (long)UINT32_MAX - n_w) return HSG_EINVAL;
    if ((n_w && !wid) || (rows && (!ids || !rowoff || n == 0)) || ((n_w || rows) && !keys)) return HSG_EINVAL;
    const long n_src = (long)n_w + rows;
    if (n_src == 0) return 0;
    hipLaunchKernelGGL(k_embed_keys, dim3((unsigned)((n_src + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long)n_w,
                       n, L, n_src, wid, ids, rowoff, padding_idx, keys);
    return status();
}

int hsg_embed_grad(int V, int D, long n_occ, const int64_t *occ, int n_w, const float *dW, int ldw, long rows,
                   const float *dX, int ldx, float *dE, float *ws, void *stream) {
    if (V < 0 || !hsg_embed_supported(D) || n_occ < 0 || n_w < 0 || rows < 0) return HSG_EINVAL;
    if (V && (!dE || misaligned(dE))) return HSG_EINVAL;
    if (n_w && (!dW || misaligned(dW) || bad_pitch(ldw, D))) return HSG_EINVAL;
    if (rows && (!dX || misaligned(dX) || bad_pitch(ldx, D))) return HSG_EINVAL;
    if (n_occ && (!occ || !ws || misaligned(ws))) return HSG_EINVAL;
    const long n_chunks = (n_occ + kPiece - 1) / kPiece;
    const int n_cg = (D / 4 + 63) / 64;
    const long blocks = (n_chunks * n_cg + kWaves - 1) / kWaves;
    if (blocks > INT_MAX) return HSG_EINVAL;
    if (V == 0) return 0;
    hipError_t e = hipMemsetAsync(dE, 0, (size_t)V * D * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (n_occ == 0) return 0;
    Src S{dW, dX, (long)ldw, (long)ldx, (long)n_w, (long)n_w + rows};
    hipLaunchKernelGGL(k_embed_chunks, dim3((unsigned)blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, V, D, n_occ,
                       n_chunks, n_cg, occ, S, dE, ws);
    hipLaunchKernelGGL(k_embed_merge, dim3((unsigned)blocks), dim3(64 * kWaves), 0, (hipStream_t)stream, V, D, n_occ,
                       n_chunks, n_cg, occ, dE, (const float *)ws);
    return status();
}

}  // extern "C"
