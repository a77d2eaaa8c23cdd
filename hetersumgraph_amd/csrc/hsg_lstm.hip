// hsg_lstm.hip -- the sentence encoder's LSTM recurrence (HiGraph.py:117-123, 135-142:
// nn.LSTM(300, 128, num_layers=2, bidirectional=True) over each document's sentence
// sequence) for gfx950.
//
// The input projection x W_ih^T + b_ih + b_hh of all steps and directions is one GEMM
// (hsg_gemm_f32) done by the caller; what is left is the recurrence
//   a_t = pre_t + W_hh h_{t-1},  (i, f, o) = sigmoid(a), g = tanh(a)   (torch order i, f, g, o)
//   c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)
// which a vendor RNN runs as one small GEMM and one pointwise kernel per time step.
// Documents are independent and so are the directions, and one direction's W_hh
// (512 x 128 fp32 = 256 KiB) fits the VGPR file of one CU: a 512-thread block at two
// waves per SIMD holds 128 floats per thread.  So ONE block runs the whole recurrence
// of a (document, direction) pair: the weights are read once, a step costs 128 FMAs
// per thread, two barriers and no launch.
//
// Rows: document d owns rows doc_off[d] .. doc_off[d+1]-1 of every [n_rows][.] array,
// in time order, no padding; direction 1 walks them backwards.
//
// Forward: thread j keeps row j of W_hh (gate j / 128, unit j % 128).  Per step it
// reads h_{t-1} from LDS (every lane the same address: broadcast ds_read_b128), sums
// four interleaved FMA chains in a fixed order, adds pre, applies its gate's
// nonlinearity (wave-uniform: a gate is two whole waves) and publishes the gate in
// LDS; after a barrier the first 128 threads update c and h.
// Backward (reverse time): the first 128 threads turn dh_t + dh_rec and dc into the
// four gate gradients (= dgates, the gradient of pre); thread (k, q) keeps the quarter
// j = 128 q .. 128 q + 127 of column k of W_hh and reduces its quarter of
// dh_rec[k] = sum_j W_hh[j][k] dgates[j]; the four quarters meet in LDS and are summed
// in a fixed order.  No atomics, no cross-block traffic: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hsg.h"
#include "hsg_rng.h"

namespace {

constexpr int kHid = 128;            // hidden units per direction
constexpr int kG = 4 * kHid;         // gate rows per direction = threads per block

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(kG) void k_lstm_fwd(int n_rows, int ndir, const int32_t *__restrict__ doc_off,
                                                 const float *__restrict__ pre, int ld_pre,
                                                 const float *__restrict__ w_hh, float *__restrict__ h, int ld_h,
                                                 float *__restrict__ gates, float *__restrict__ c, float p_drop,
                                                 const int64_t *__restrict__ seed, uint32_t offset,
                                                 float *__restrict__ y, int ld_y) {
    __shared__ float4 h_s[kHid / 4];
    __shared__ float g_s[kG];
    const int doc = (int)blockIdx.x / ndir, dir = (int)blockIdx.x - doc * ndir;
    const int off = doc_off[doc], L = doc_off[doc + 1] - off;
    if (L <= 0 || off < 0 || off + L > n_rows) return;           // block-uniform
    const int j = (int)threadIdx.x;
    const int gate = j >> 7;

    float w[kHid];
    {
        const float4 *wr = reinterpret_cast<const float4 *>(w_hh + ((size_t)dir * kG + j) * kHid);
#pragma unroll
        for (int k = 0; k < kHid / 4; ++k) {
            const float4 v = wr[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    }
    const bool drop = p_drop > 0.f;
    uint32_t key = 0, thr = 0;
    float scale = 1.f;
    if (drop) {
        key = hsg_drop_key((uint64_t)seed[0], offset);
        thr = hsg_drop_threshold(p_drop);
        scale = 1.f / (1.f - p_drop);
    }
    float cst = 0.f;
    if (j < kHid) reinterpret_cast<float *>(h_s)[j] = 0.f;
    __syncthreads();

    const int gcol = dir * kG + j;                               // column in pre / gates
    const int hcol = dir * kHid + j;                             // column in h / c / y (j < kHid)
    const int GW = ndir * kG, HW = ndir * kHid;
    int r = dir ? off + L - 1 : off;
    const int step = dir ? -1 : 1;
    float pcur = pre[(size_t)r * ld_pre + gcol];
    for (int s = 0; s < L; ++s, r += step) {
        const float pnext = s + 1 < L ? pre[(size_t)(r + step) * ld_pre + gcol] : 0.f;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int k = 0; k < kHid / 4; ++k) {
            const float4 hv = h_s[k];
            a0 = fmaf(w[4 * k], hv.x, a0);
            a1 = fmaf(w[4 * k + 1], hv.y, a1);
            a2 = fmaf(w[4 * k + 2], hv.z, a2);
            a3 = fmaf(w[4 * k + 3], hv.w, a3);
        }
        const float a = pcur + ((a0 + a1) + (a2 + a3));
        const float act = gate == 2 ? tanhf(a) : sigmoidf_(a);
        g_s[j] = act;
        gates[(size_t)r * GW + gcol] = act;
        __syncthreads();
        if (j < kHid) {
            const float gi = g_s[j], gf = g_s[kHid + j], gg = g_s[2 * kHid + j], go = g_s[3 * kHid + j];
            cst = gf * cst + gi * gg;
            const float hv = go * tanhf(cst);
            c[(size_t)r * HW + hcol] = cst;
            h[(size_t)r * ld_h + hcol] = hv;
            if (drop) {
                const uint32_t idx = (uint32_t)r * (uint32_t)HW + (uint32_t)hcol;
                y[(size_t)r * ld_y + hcol] = hsg_keep32(key, idx, thr) ? hv * scale : 0.f;
            }
            reinterpret_cast<float *>(h_s)[j] = hv;
        }
        __syncthreads();
        pcur = pnext;
    }
}

__global__ __launch_bounds__(kG) void k_lstm_bwd(int n_rows, int ndir, const int32_t *__restrict__ doc_off,
                                                 const float *__restrict__ dy, int ld,
                                                 const float *__restrict__ gates, const float *__restrict__ c,
                                                 const float *__restrict__ w_hh, float p_drop,
                                                 const int64_t *__restrict__ seed, uint32_t offset,
                                                 float *__restrict__ dgates) {
    __shared__ float4 dg_s[kG / 4];
    __shared__ float part_s[4][kHid];
    const int doc = (int)blockIdx.x / ndir, dir = (int)blockIdx.x - doc * ndir;
    const int off = doc_off[doc], L = doc_off[doc + 1] - off;
    if (L <= 0 || off < 0 || off + L > n_rows) return;           // block-uniform
    const int tid = (int)threadIdx.x;
    const int k = tid & (kHid - 1), q = tid >> 7;

    float w[kHid];                                               // W_hh[128 q + jj][k]
    {
        const float *wc = w_hh + ((size_t)dir * kG + (size_t)q * kHid) * kHid + k;
#pragma unroll
        for (int jj = 0; jj < kHid; ++jj) w[jj] = wc[(size_t)jj * kHid];
    }
    const bool drop = p_drop > 0.f;
    uint32_t key = 0, thr = 0;
    float scale = 1.f;
    if (drop) {
        key = hsg_drop_key((uint64_t)seed[0], offset);
        thr = hsg_drop_threshold(p_drop);
        scale = 1.f / (1.f - p_drop);
    }
    const int GW = ndir * kG, HW = ndir * kHid;
    const int hcol = dir * kHid + k;
    const int step = dir ? -1 : 1;
    const bool ew = tid < kHid;                                  // the pointwise threads (waves 0, 1)
    float *dgf = reinterpret_cast<float *>(dg_s);
    float dh_rec = 0.f, dc = 0.f;
    // the walk is the forward's in reverse: forward step s is row r(s); s = L-1 .. 0
    int r = dir ? off : off + L - 1;
    float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, dyv = 0.f, ccur = 0.f, cprev = 0.f;
    if (ew) {
        const float *gr = gates + (size_t)r * GW + dir * kG + k;
        gi = gr[0]; gf = gr[kHid]; gg = gr[2 * kHid]; go = gr[3 * kHid];
        dyv = dy[(size_t)r * ld + hcol];
        ccur = c[(size_t)r * HW + hcol];
        cprev = L > 1 ? c[(size_t)(r - step) * HW + hcol] : 0.f;
    }
    for (int s = L - 1; s >= 0; --s, r -= step) {
        if (ew) {
            // the next iteration's operands (step s - 1; its c_prev is step s - 2's c)
            float ni = 0.f, nf = 0.f, ng = 0.f, no = 0.f, ndy = 0.f, ncp = 0.f;
            if (s > 0) {
                const int rn = r - step;
                const float *gr = gates + (size_t)rn * GW + dir * kG + k;
                ni = gr[0]; nf = gr[kHid]; ng = gr[2 * kHid]; no = gr[3 * kHid];
                ndy = dy[(size_t)rn * ld + hcol];
                if (s > 1) ncp = c[(size_t)(rn - step) * HW + hcol];
            }
            float dh = dyv;
            if (drop) {
                const uint32_t idx = (uint32_t)r * (uint32_t)HW + (uint32_t)hcol;
                dh = hsg_keep32(key, idx, thr) ? dh * scale : 0.f;
            }
            dh += dh_rec;
            const float tc = tanhf(ccur);
            const float dct = dc + dh * go * (1.f - tc * tc);
            const float p_i = dct * gg * gi * (1.f - gi);
            const float p_f = dct * cprev * gf * (1.f - gf);
            const float p_g = dct * gi * (1.f - gg * gg);
            const float p_o = dh * tc * go * (1.f - go);
            dc = dct * gf;
            float *dr = dgates + (size_t)r * GW + dir * kG + k;
            dr[0] = p_i; dr[kHid] = p_f; dr[2 * kHid] = p_g; dr[3 * kHid] = p_o;
            dgf[k] = p_i; dgf[kHid + k] = p_f; dgf[2 * kHid + k] = p_g; dgf[3 * kHid + k] = p_o;
            gi = ni; gf = nf; gg = ng; go = no; dyv = ndy; ccur = cprev; cprev = ncp;
        }
        if (s == 0) break;                                       // block-uniform: no dh_rec needed
        __syncthreads();
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int jj = 0; jj < kHid / 4; ++jj) {
            const float4 dv = dg_s[q * (kHid / 4) + jj];         // wave-uniform address: broadcast
            a0 = fmaf(w[4 * jj], dv.x, a0);
            a1 = fmaf(w[4 * jj + 1], dv.y, a1);
            a2 = fmaf(w[4 * jj + 2], dv.z, a2);
            a3 = fmaf(w[4 * jj + 3], dv.w, a3);
        }
        part_s[q][k] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (ew) dh_rec = (part_s[0][k] + part_s[1][k]) + (part_s[2][k] + part_s[3][k]);
    }
}

int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int hsg_lstm_supported(int hid, int ndir) { return hid == kHid && (ndir == 1 || ndir == 2); }

int hsg_lstm_fwd(int n_docs, int n_rows, int hid, int ndir, const int32_t *doc_off, const float *pre, int ld_pre,
                 const float *w_hh, float *h, int ld_h, float *gates, float *c, float p_drop, const int64_t *seed,
                 uint32_t offset, float *y, int ld_y, void *stream) {
    if (!hsg_lstm_supported(hid, ndir) || n_docs < 0 || n_rows < 0 || !(p_drop >= 0.f && p_drop < 1.f))
        return HSG_EINVAL;
    if (n_docs == 0 || n_rows == 0) return 0;
    if (!doc_off || !pre || !w_hh || !h || !gates || !c || ld_pre < ndir * kG || ld_h < ndir * kHid ||
        !aligned16(w_hh) || (long)n_docs * ndir > 0x7FFFFFFFL)
        return HSG_EINVAL;
    if (p_drop > 0.f && (!seed || !y || ld_y < ndir * kHid || (long)n_rows * ndir * kHid > 0xFFFFFFFFL))
        return HSG_EINVAL;
    hipLaunchKernelGGL(k_lstm_fwd, dim3((unsigned)(n_docs * ndir)), dim3(kG), 0, (hipStream_t)stream, n_rows, ndir,
                       doc_off, pre, ld_pre, w_hh, h, ld_h, gates, c, p_drop, seed, offset, y, ld_y);
    return status();
}

int hsg_lstm_bwd(int n_docs, int n_rows, int hid, int ndir, const int32_t *doc_off, const float *dh_out, int ld,
                 const float *gates, const float *c, const float *w_hh, float p_drop, const int64_t *seed,
                 uint32_t offset, float *dgates, void *stream) {
    if (!hsg_lstm_supported(hid, ndir) || n_docs < 0 || n_rows < 0 || !(p_drop >= 0.f && p_drop < 1.f))
        return HSG_EINVAL;
    if (n_docs == 0 || n_rows == 0) return 0;
    if (!doc_off || !dh_out || !gates || !c || !w_hh || !dgates || ld < ndir * kHid ||
        (long)n_docs * ndir > 0x7FFFFFFFL)
        return HSG_EINVAL;
    if (p_drop > 0.f && (!seed || (long)n_rows * ndir * kHid > 0xFFFFFFFFL)) return HSG_EINVAL;
    hipLaunchKernelGGL(k_lstm_bwd, dim3((unsigned)(n_docs * ndir)), dim3(kG), 0, (hipStream_t)stream, n_rows, ndir,
                       doc_off, dh_out, ld, gates, c, w_hh, p_drop, seed, offset, dgates);
    return status();
}

}  // extern "C"
