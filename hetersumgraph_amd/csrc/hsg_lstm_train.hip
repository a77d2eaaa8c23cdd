// hsg_lstm_train.hip -- the sentence LSTM's training path around the recurrence kernels of
// hsg_lstm.hip (include/hsg_lstm_train.h): k_lstm_pack stacks the nn.LSTM parameters of all
// layers into the operands the projection GEMM and the recurrence read, in one launch per
// step; k_lstm_dw forms the three weight gradients of a layer as one product
//     [dW_ih | dW_hh | db] = dgates^T [x | h_prev | 1]
// chunk by chunk over the rows, and k_lstm_dw_reduce adds the chunks in ascending order.
//
// k_lstm_dw.  The reduction runs over rows, so both MFMA operands are read "down" a column:
// v_mfma_f32_16x16x4_f32 takes A[i][k] from lane (i = l & 15, k = l >> 4) and B[k][j] from
// lane (j = l & 15, k = l >> 4), i.e. every lane reads one float of row r0 + (l >> 4), 16
// consecutive floats per row: 64-byte segments of dgates, x and h straight from L2, no LDS
// tile.  A wave keeps a 32 x 64 tile (2 x 4 accumulators of 16 x 16, 32 VGPRs) and per four
// rows issues 2 + 4 loads for 8 MFMAs (32 cycles each: 256 cycles of matrix work per 6
// loads); the next 16 rows' operands are in flight while the current 16 multiply.  h_prev is
// h one row up (direction 0) or down (direction 1) and zero at a document edge: the block
// writes one flag word per row of its chunk into LDS (a binary search of doc_off per row),
// and a masked lane loads nothing and feeds +0.0.  The operand columns are laid out as
// ceil16(in) columns of x, then hid columns of h_prev, so a 16-column tile never straddles
// the two sources (in = 300 is not a multiple of 16; its last x tile masks four columns).
// The bias gradient is the column sum of the A operand, kept by the blocks of column tile 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg_lstm_train.h"

namespace {

constexpr int kHid = 128;                    // hidden units per direction
constexpr int kG = 4 * kHid;                 // gate rows per direction
constexpr int kC = HSG_LSTM_DW_CHUNK;        // rows per chunk
constexpr int kBM = 128, kBN = 64;           // block tile: gate rows x operand columns
constexpr int kThreads = 256;                // four waves, 32 gate rows each
constexpr int kU = 4;                        // MFMA k steps (of 4 rows) per pipeline stage
constexpr int kMaxPtr = 4 * HSG_LSTM_PACK_MAX_LAYERS * 2;

static_assert(kC % (4 * kU) == 0 && kC <= kThreads, "chunk: whole pipeline stages, one flag thread per row");
static_assert(kG % kBM == 0, "a block's gate rows lie in one direction");

typedef float f32x4v __attribute__((ext_vector_type(4)));

struct PackArgs {
    const float *p[kMaxPtr];
};

// out, per layer: W_ih [M][in_l] | W_hh [ndir][G][hid] | bias [M]; one float4 per thread.
__global__ __launch_bounds__(256) void k_lstm_pack(PackArgs a, int n_layers, int ndir, int in, long total4,
                                                   float *__restrict__ out) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int M = ndir * kG;
    long e = i * 4;                                              // float index in out
    int layer = 0, in_l = in;
    for (;; ++layer) {
        const long len = (long)M * in_l + (long)M * kHid + M;
        if (e < len || layer == n_layers - 1) break;
        e -= len;
        in_l = ndir * kHid;
    }
    const float *const *q = a.p + (size_t)layer * ndir * 4;
    float4 v;
    if (e < (long)M * in_l) {                                    // W_ih: rows d*G.. of direction d
        const int d = (int)(e / ((long)kG * in_l));
        v = *reinterpret_cast<const float4 *>(q[d * 4] + (e - (long)d * kG * in_l));
    } else if ((e -= (long)M * in_l) < (long)M * kHid) {         // W_hh
        const int d = (int)(e / (kG * kHid));
        v = *reinterpret_cast<const float4 *>(q[d * 4 + 1] + (e - (long)d * kG * kHid));
    } else {                                                     // bias_ih + bias_hh
        e -= (long)M * kHid;
        const int d = (int)(e / kG);
        const float4 b0 = *reinterpret_cast<const float4 *>(q[d * 4 + 2] + (e - d * kG));
        const float4 b1 = *reinterpret_cast<const float4 *>(q[d * 4 + 3] + (e - d * kG));
        v = make_float4(b0.x + b1.x, b0.y + b1.y, b0.z + b1.z, b0.w + b1.w);
    }
    *reinterpret_cast<float4 *>(out + i * 4) = v;
}

// Flags of one row: bit 0 = the row exists, bit 1 = it has an h_prev in this block's direction.
__device__ __forceinline__ int row_flags(int r, int n_rows, int n_docs, int dir, const int32_t *__restrict__ doc_off) {
    if (r >= n_rows) return 0;
    int lo = 0, hi = n_docs + 1;                                 // first index with doc_off[idx] > r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (doc_off[mid] > r) hi = mid; else lo = mid + 1;
    }
    bool has = false;
    if (lo >= 1 && lo <= n_docs) {                               // document lo - 1 holds row r
        has = dir ? (doc_off[lo] != r + 1 && r + 1 < n_rows) : (doc_off[lo - 1] != r && r > 0);
    }
    return has ? 3 : 1;
}

__global__ __launch_bounds__(kThreads) void k_lstm_dw(int n_docs, int n_rows, int ndir, int in,
                                                      const int32_t *__restrict__ doc_off,
                                                      const float *__restrict__ dg, const float *__restrict__ x,
                                                      int ld_x, const float *__restrict__ h, int ld_h,
                                                      float *__restrict__ ws) {
    __shared__ int fl_s[kC];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int M = ndir * kG, NW = in + kHid, inP = (in + 15) & ~15;
    const int chunk = (int)blockIdx.z, c0 = chunk * kC;
    const int m0 = (int)blockIdx.y * kBM + wave * 32;            // this wave's 32 gate rows
    const int dir = ((int)blockIdx.y * kBM) / kG;
    const int nb0 = (int)blockIdx.x * kBN;

    if (tid < kC) fl_s[tid] = row_flags(c0 + tid, n_rows, n_docs, dir, doc_off);
    __syncthreads();

    // the four 16-column B tiles of this block: source, column, row shift, flag bit needed
    const float *bp[4];
    int bld[4], need[4], wcol[4];                                // wcol: first ws column, -1 = no such tile
    bool colok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n0 = nb0 + t * 16;
        if (n0 < inP) {
            bp[t] = x + n0 + li; bld[t] = ld_x; need[t] = 1;
            colok[t] = n0 + li < in; wcol[t] = n0;
        } else if (n0 - inP < kHid) {
            bld[t] = ld_h; need[t] = 2; colok[t] = true; wcol[t] = in + (n0 - inP);
            bp[t] = h + dir * kHid + (n0 - inP) + li + (dir ? (long)ld_h : -(long)ld_h);
        } else {
            bp[t] = x; bld[t] = 0; need[t] = 1; colok[t] = false; wcol[t] = -1;
        }
    }
    const float *ap = dg + m0 + li;
    const bool want_db = blockIdx.x == 0;

    f32x4v acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = f32x4v{0.f, 0.f, 0.f, 0.f};
    float dbs[2] = {0.f, 0.f};

    float av[2][kU][2], bv[2][kU][4];                            // [stage][k step][tile]
    auto load = [&](int buf, int it) {
#pragma unroll
        for (int s = 0; s < kU; ++s) {
            const int rl = it * (4 * kU) + s * 4 + lk;           // row within the chunk
            const int f = fl_s[rl];
            const long r = c0 + rl;
#pragma unroll
            for (int i = 0; i < 2; ++i) av[buf][s][i] = (f & 1) ? ap[r * M + i * 16] : 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) bv[buf][s][t] = (colok[t] && (f & need[t])) ? bp[t][r * bld[t]] : 0.f;
        }
    };
    const int rows_here = min(kC, n_rows - c0);
    const int n_it = (rows_here + 4 * kU - 1) / (4 * kU);       // block-uniform
    load(0, 0);
#pragma unroll 1
    for (int it = 0; it < n_it; it += 2) {
        // two stages per trip so that the buffers are indexed by constants
        if (it + 1 < n_it) load(1, it + 1);
#pragma unroll
        for (int s = 0; s < kU; ++s) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                dbs[i] += av[0][s][i];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0][s][i], bv[0][s][t], acc[i][t], 0, 0, 0);
            }
        }
        if (it + 1 >= n_it) break;
        if (it + 2 < n_it) load(0, it + 2);
#pragma unroll
        for (int s = 0; s < kU; ++s) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                dbs[i] += av[1][s][i];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1][s][i], bv[1][s][t], acc[i][t], 0, 0, 0);
            }
        }
    }

    // D layout: lane (li, lk) holds column li of the tile, rows 4 lk .. 4 lk + 3
    float *wsc = ws + (size_t)chunk * ((size_t)M * NW + M);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (wcol[t] < 0 || !colok[t]) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                wsc[(size_t)(m0 + i * 16 + 4 * lk + e) * NW + wcol[t] + li] = acc[i][t][e];
    }
    if (want_db) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float v = dbs[i];
            v = v + __shfl_xor(v, 16);                           // s0 + s1 | s2 + s3
            v = v + __shfl_xor(v, 32);                           // (s0 + s1) + (s2 + s3)
            if (lk == 0) wsc[(size_t)M * NW + m0 + i * 16 + li] = v;
        }
    }
}

// One float4 of [dW_ih | dW_hh] (or of db) per thread: the chunks' partials in ascending order.
__global__ __launch_bounds__(256) void k_lstm_dw_reduce(int n_chunks, int ndir, int in, const float *__restrict__ ws,
                                                        float *__restrict__ dwih, float *__restrict__ dwhh,
                                                        float *__restrict__ db) {
    const int M = ndir * kG, NW = in + kHid, NW4 = NW / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n_w = (long)M * NW4;
    if (i >= n_w + M / 4) return;
    const size_t stride = (size_t)M * NW + M;
    const size_t src = i < n_w ? (size_t)i * 4 : (size_t)M * NW + (size_t)(i - n_w) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n_chunks > 0) s = *reinterpret_cast<const float4 *>(ws + src);
    for (int c = 1; c < n_chunks; ++c) {
        const float4 p = *reinterpret_cast<const float4 *>(ws + (size_t)c * stride + src);
        s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
    float *dst;
    if (i < n_w) {
        const int m = (int)(i / NW4), n = (int)(i - (long)m * NW4) * 4;
        dst = n < in ? dwih + (size_t)m * in + n : dwhh + (size_t)m * kHid + (n - in);
    } else {
        dst = db + (size_t)(i - n_w) * 4;
    }
    *reinterpret_cast<float4 *>(dst) = s;
}

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

size_t layer_floats(int ndir, int in_l) { return (size_t)ndir * kG * ((size_t)in_l + kHid + 1); }

}  // namespace

extern "C" {

int hsg_lstm_train_supported(int hid, int ndir, int in) {
    return hid == kHid && (ndir == 1 || ndir == 2) && in > 0 && in % 4 == 0;
}

size_t hsg_lstm_pack_layer_offset(int layer, int hid, int ndir, int in) {
    if (!hsg_lstm_train_supported(hid, ndir, in) || layer < 0 || layer > HSG_LSTM_PACK_MAX_LAYERS) return 0;
    size_t off = 0;
    for (int l = 0; l < layer; ++l) off += layer_floats(ndir, l ? ndir * kHid : in);
    return off;
}

size_t hsg_lstm_pack_floats(int n_layers, int hid, int ndir, int in) {
    return n_layers < 1 ? 0 : hsg_lstm_pack_layer_offset(n_layers, hid, ndir, in);
}

int hsg_lstm_pack(int n_layers, int hid, int ndir, int in, const float *const *params, float *out, void *stream) {
    if (!hsg_lstm_train_supported(hid, ndir, in) || n_layers < 1 || n_layers > HSG_LSTM_PACK_MAX_LAYERS || !params ||
        !out || !aligned16(out))
        return HSG_EINVAL;
    PackArgs a = {};
    for (int i = 0; i < 4 * n_layers * ndir; ++i) {
        if (!params[i] || !aligned16(params[i])) return HSG_EINVAL;
        a.p[i] = params[i];
    }
    const long total4 = (long)(hsg_lstm_pack_floats(n_layers, hid, ndir, in) / 4);
    hipLaunchKernelGGL(k_lstm_pack, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a,
                       n_layers, ndir, in, total4, out);
    return status();
}

int hsg_lstm_dw_chunk(void) { return kC; }

size_t hsg_lstm_dw_ws_floats(int n_rows, int ndir, int in) {
    if (n_rows <= 0 || !hsg_lstm_train_supported(kHid, ndir, in)) return 0;
    return (size_t)((n_rows + kC - 1) / kC) * layer_floats(ndir, in);
}

int hsg_lstm_dw(int n_docs, int n_rows, int hid, int ndir, int in, const int32_t *doc_off, const float *dgates,
                const float *x, int ld_x, const float *h, int ld_h, float *ws, float *dW_ih, float *dW_hh,
                float *db, void *stream) {
    if (!hsg_lstm_train_supported(hid, ndir, in) || n_docs < 0 || n_rows < 0 || !dW_ih || !dW_hh || !db ||
        !aligned16(dW_ih) || !aligned16(dW_hh) || !aligned16(db))
        return HSG_EINVAL;
    const int M = ndir * kG;
    int n_chunks = 0;
    if (n_docs > 0 && n_rows > 0) {
        if (!doc_off || !dgates || !x || !h || !ws || !aligned16(ws) || ld_x < in || ld_h < ndir * kHid ||
            n_rows > 65535L * kC)
            return HSG_EINVAL;
        n_chunks = (n_rows + kC - 1) / kC;
        const int inP = (in + 15) & ~15;
        const dim3 grid((unsigned)((inP + kHid + kBN - 1) / kBN), (unsigned)(M / kBM), (unsigned)n_chunks);
        hipLaunchKernelGGL(k_lstm_dw, grid, dim3(kThreads), 0, (hipStream_t)stream, n_docs, n_rows, ndir, in, doc_off,
                           dgates, x, ld_x, h, ld_h, ws);
        const int rc = status();
        if (rc) return rc;
    }
    const long items = (long)M * ((in + kHid) / 4) + M / 4;
    hipLaunchKernelGGL(k_lstm_dw_reduce, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       n_chunks, ndir, in, ws, dW_ih, dW_hh, db);
    return status();
}

}  // extern "C"
