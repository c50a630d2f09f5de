// train_step.h — kernels of the stage-2 training step: the reference's p_losses (transformer_cond_diffusion_model.py:574-605)
// forward with saves, its loss, and the gradient of every trainable tensor, on split-bf16 MFMAs.
//
// Every contraction runs as three v_mfma_f32_32x32x16_bf16 per 16-deep k step (hi*hi + lo*hi + hi*lo, fp32 accumulate).  Both
// operands are fp32 rows in memory — activations, saved tensors and the caller's LIVE parameter tensors alike — and a lane splits
// the 8 values it feeds the MFMA as it loads them (the pattern of stage1.h), so a call never reads a packed copy of a weight that
// an optimizer step could have made stale.  LayerNorm, softmax, GELU, the residuals and the loss stay fp32; the loss sums in fp64.
//
// Rows: window b owns rows [b * L, (b + 1) * L), L = T + 1.  Row b * L is the time token, row b * L + 1 + t is frame t.  There is no
// padding to tiles: the contraction kernel checks every row, column and k index against its bounds and feeds zeros past them.
//
// One contraction kernel serves every product of the step: C(i, j) = alpha * sum_k A(i, k) B(j, k) with free strides on both
// operands, so that Y = X W^T (forward), dX = dY W (data gradient) and dW = dY^T X (weight gradient) differ in their strides only.
// A sum over the B * L rows (weight gradients, bias gradients, LayerNorm gains) is cut into fixed chunks of rows; every chunk
// writes its partial and fold_kernel adds the partials in chunk order: no float atomics, the same bits on every run.
#pragma once
#include "common.h"

namespace tr {

static constexpr int DM = 512;    // d_model = FFN width
static constexpr int HD = 1024;   // n_head * d_k = n_head * d_v
static constexpr int NH = 4;
static constexpr int DK = 256;
static constexpr int TE = 64;     // sinusoidal time embedding
static constexpr int TH = 256;    // hidden width of the time MLP
static constexpr int CHUNK = 512;   // rows per partial of a weight / bias gradient
static constexpr int LN_ROWS = 8;   // rows per partial of a LayerNorm gain / bias gradient (one wave)
static constexpr int COL_ROWS = 64; // rows per partial of a bias gradient (one thread per column: short strips keep the grid full)
static constexpr int MAX_L = 197;   // the sampler's longest window + 1

// Dropout site of a layer: the attention probabilities, the fc output, the FFN output (TM:63, 68, 108).
enum { SITE_ATTN = 0, SITE_FC = 1, SITE_FFN = 2 };

// A dropout mask is a pure function of (seed, layer, site, window id, element index within the window): nothing about the tiling
// or the other windows of the batch enters, and the backward pass regenerates it.  thr = 0 switches it off.
struct Drop {
    uint64_t seed;
    const int64_t* wids;  // [B] window ids
    uint32_t thr;         // keep when a 32-bit draw >= thr: thr = p * 2^32
    float scale;          // 1 / (1 - p)
    int layer, site;
};

EG_D Philox4 drop_draw4(const Drop& d, int64_t wid, uint32_t e4) {
    return philox4x32_10(e4, (uint32_t)wid, (uint32_t)((uint64_t)wid >> 32), (uint32_t)(d.layer * 4 + d.site), (uint32_t)d.seed,
                         (uint32_t)(d.seed >> 32));
}

// keep (1) or drop (0) element e of window wid
EG_D bool drop_keep(const Drop& d, int64_t wid, uint32_t e) {
    const Philox4 r = drop_draw4(d, wid, e >> 2);
    const uint32_t c = e & 3;
    const uint32_t v = c == 0 ? r.c[0] : c == 1 ? r.c[1] : c == 2 ? r.c[2] : r.c[3];
    return v >= d.thr;
}

// ------------------------------------------------------------------------------------------------ contraction
struct Gemm {
    const float* A; long sai, sak, bsA0, bsA1;  // A(i, k) = A[i * sai + k * sak]; batch z: + (z / zdiv) * bsA0 + (z % zdiv) * bsA1
    const float* B; long sbj, sbk, bsB0, bsB1;
    float* C; long ldc, bsC0, bsC1;
    const float* bias;  // [N] or nullptr
    const float* gate;  // laid out like C, or nullptr: the result is kept where gate > 0 (ReLU backward)
    const float* pos;   // [..][N] or nullptr: += pos[(i % posL + 1) * N + j] (the position table of the embed)
    int posL;
    int M, N, K, zdiv;
    int kchunk;         // > 0: blockIdx.z is a chunk of k (rows of a gradient sum): k in [z * kchunk, ..), C + z * bsC0
    float alpha;
    int relu, accum;    // accum: C += result
};

// 8 values of operand row `p` from k (stride sk), zeros past kend or when the row is out of range
EG_D void ld8(const float* p, long sk, int k, int kend, bool ok, float v[8]) {
    if (ok && sk == 1 && k + 8 <= kend && (((uintptr_t)(p + k)) & 15) == 0) {
        const float4 x = *(const float4*)(p + k), y = *(const float4*)(p + k + 4);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (ok && k + i < kend) ? p[(long)(k + i) * sk] : 0.f;
    }
}

// One wave per 32 x 32 tile of C, four tiles (128 columns) per workgroup.  Accumulator register r of lane l holds
// (row mfma32_row(r, l >> 5), column l & 31).  KIND only names the use (a kernel trace then tells the four apart): the code is one.
enum { GEMM_FWD = 0, GEMM_DGRAD = 1, GEMM_WGRAD = 2, GEMM_ATTN = 3 };
template <int KIND>
__global__ __launch_bounds__(256) void gemm_kernel(Gemm g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5, l31 = lane & 31;
    const int n0 = (blockIdx.y * 4 + wave) * 32;
    if (n0 >= g.N) return;
    const int m0 = blockIdx.x * 32;
    const int z = blockIdx.z;
    const float* A = g.A;
    const float* B = g.B;
    float* C = g.C;
    const float* gate = g.gate;
    int k0 = 0, k1 = g.K;
    if (g.kchunk > 0) {
        k0 = z * g.kchunk;
        k1 = min(g.K, k0 + g.kchunk);
        C += (size_t)z * g.bsC0;
    } else {
        const long zb = z / g.zdiv, zh = z % g.zdiv;
        A += zb * g.bsA0 + zh * g.bsA1;
        B += zb * g.bsB0 + zh * g.bsB1;
        C += zb * g.bsC0 + zh * g.bsC1;
        if (gate) gate += zb * g.bsC0 + zh * g.bsC1;
    }
    const int i = m0 + l31, j = n0 + l31;
    const bool aok = i < g.M, bok = j < g.N;
    const float* ap = A + (long)(aok ? i : 0) * g.sai;
    const float* bp = B + (long)(bok ? j : 0) * g.sbj;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k = k0; k < k1; k += 16) {
        float a[8], b[8];
        ld8(ap, g.sak, k + hf * 8, k1, aok, a);
        ld8(bp, g.sbk, k + hf * 8, k1, bok, b);
        u32x4 ah, al, bh, bl;
        split8(a, ah, al);
        split8(b, bh, bl);
        acc = mfma3(ah, al, bh, bl, acc);
    }
    if (!bok) return;
    const float bias = g.bias ? g.bias[j] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ii = m0 + mfma32_row(r, hf);
        if (ii >= g.M) continue;
        const size_t idx = (size_t)ii * g.ldc + j;
        float v = acc[r] * g.alpha;
        v = v + bias;
        if (g.pos) v = v + g.pos[(size_t)(ii % g.posL + 1) * g.N + j];
        if (g.relu) v = fmaxf(v, 0.f);
        if (gate) v = gate[idx] > 0.f ? v : 0.f;
        if (g.accum) v = C[idx] + v;
        C[idx] = v;
    }
}

// out[i] = part[0][i] + part[1][i] + ... in chunk order (chunk c at part + c * stride), added in fp64 and rounded once
template <typename T>
__global__ void fold_kernel(const T* part, long stride, int nch, long n, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = (double)part[i];
#pragma unroll 8
    for (int c = 1; c < nch; ++c) s += (double)part[(long)c * stride + i];  // (the loads run ahead; the additions stay in order)
    out[i] = (float)s;
}

// part[z][j] = sum over the COL_ROWS rows m of strip z, in row order, of Y[m * ld + j]; skipL > 0 leaves out the rows m % skipL == 0.
// A bias gradient is a bare sum — under l1, linear_out's is a sum of +-c with c the same for a whole window — so nothing hides
// the rounding of its additions: they run in fp64 (the partials too), and the result is rounded once.
__global__ void colsum_kernel(const float* Y, long ld, int R, int N, int skipL, double* part) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int m0 = blockIdx.y * COL_ROWS, m1 = min(R, m0 + COL_ROWS);
    double s = 0.0;
    for (int m = m0; m < m1; ++m)
        if (skipL == 0 || m % skipL != 0) s += (double)Y[(size_t)m * ld + j];
    part[(size_t)blockIdx.y * N + j] = s;
}

// ------------------------------------------------------------------------------------------------ prep
// x = sqrt_ac[t] x_start + sqrt_1mac[t] noise; x_cond = x_start (1 - m) + m cond_noise; xin row b * L + 1 + t = [x | x_cond],
// row b * L (the time token's) = 0; target = x_start (pred_x0) or noise.  Also copies the row mask and the window ids into the saves.
struct Prep {
    const float *x_start, *noise, *cond_noise, *cond_mask;
    const int64_t* t;
    const float *row_mask, *sqrt_ac, *sqrt_1mac;
    const int64_t* wids;
    float *xin, *target, *maskR;
    int64_t* wids_out;
    int B, T, D, S, pred_x0;
};

__global__ void prep_kernel(Prep a) {
    const int L = a.T + 1;
    const long n = (long)a.B * L * a.D;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int d = (int)(i % a.D);
    const long row = i / a.D;
    const int b = (int)(row / L), tt = (int)(row % L);
    float* xr = a.xin + (size_t)row * (2 * a.D);
    if (d == 0) a.maskR[row] = a.row_mask ? a.row_mask[row] : 1.f;
    if (tt == 0) {
        xr[d] = 0.f;
        xr[a.D + d] = 0.f;
        if (d == 0) a.wids_out[b] = a.wids ? a.wids[b] : (int64_t)b;
        return;
    }
    int64_t ts = a.t[b];
    ts = ts < 0 ? 0 : (ts >= a.S ? a.S - 1 : ts);
    const size_t src = ((size_t)b * a.T + (tt - 1)) * a.D + d;
    const float xs = a.x_start[src], nz = a.noise[src], m = a.cond_mask[src];
    const float p1 = a.sqrt_ac[ts] * xs, p2 = a.sqrt_1mac[ts] * nz;
    xr[d] = p1 + p2;
    const float q1 = xs * (1.0f - m), q2 = m * a.cond_noise[src];
    xr[a.D + d] = q1 + q2;
    a.target[src] = a.pred_x0 ? xs : nz;
}

// ------------------------------------------------------------------------------------------------ time token
// SinusoidalPosEmb(64) -> Linear(64, 256) -> GELU(erf) -> Linear(256, 512), + position row 1; one workgroup per window, fp32 FMA.
struct TimeFwd {
    const int64_t* t;
    const float *w1, *b1, *w3, *b3, *pos;
    float *emb, *h1, *gact, *X;  // saves [B][64], [B][256], [B][256]; X row b * L
    int L, S;
};

__global__ __launch_bounds__(256) void time_fwd_kernel(TimeFwd a) {
    __shared__ float e[TE];
    __shared__ float gl[TH];
    const int b = blockIdx.x, j = threadIdx.x;
    int64_t ts = a.t[b];
    ts = ts < 0 ? 0 : (ts >= a.S ? a.S - 1 : ts);
    if (j < TE / 2) {
        // freq = fp32 exp(j * -(log(10000) / 31)), angle = t * freq in fp32, then a correctly rounded sine / cosine
        const float c = (float)(-(9.210340371976184 / (double)(TE / 2 - 1)));
        const float arg = (float)j * c;
        const float freq = (float)exp((double)arg);
        const float ang = (float)ts * freq;
        const float sn = (float)sin((double)ang), cs = (float)cos((double)ang);
        e[j] = sn;
        e[TE / 2 + j] = cs;
        a.emb[(size_t)b * TE + j] = sn;
        a.emb[(size_t)b * TE + TE / 2 + j] = cs;
    }
    __syncthreads();
    {
        float s = a.b1[j];
        const float* w = a.w1 + (size_t)j * TE;
        for (int k = 0; k < TE; ++k) s = fmaf(w[k], e[k], s);
        a.h1[(size_t)b * TH + j] = s;
        const float gv = 0.5f * s * (1.0f + erff(s * 0.70710678118654752f));
        gl[j] = gv;
        a.gact[(size_t)b * TH + j] = gv;
    }
    __syncthreads();
    for (int n = j; n < DM; n += 256) {
        float s = a.b3[n];
        const float* w = a.w3 + (size_t)n * TH;
        for (int k = 0; k < TH; ++k) s = fmaf(w[k], gl[k], s);
        a.X[(size_t)b * a.L * DM + n] = s + a.pos[DM + n];
    }
}

// dh1[b][k] = gelu'(h1[b][k]) * sum_n dtok[b][n] w3[n][k], dtok[b] = dX row b * L; one workgroup per window
__global__ __launch_bounds__(256) void time_bwd_hidden_kernel(const float* dX, int L, const float* w3, const float* h1, float* dtok, float* dh1) {
    __shared__ float d[DM];
    const int b = blockIdx.x, k = threadIdx.x;
    for (int n = k; n < DM; n += 256) {
        const float v = dX[(size_t)b * L * DM + n];
        d[n] = v;
        dtok[(size_t)b * DM + n] = v;
    }
    __syncthreads();
    float s = 0.f;
    for (int n = 0; n < DM; ++n) s = fmaf(d[n], w3[(size_t)n * TH + k], s);
    const float x = h1[(size_t)b * TH + k];
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * x * x);
    dh1[(size_t)b * TH + k] = s * (cdf + x * pdf);
}

// dW[n][k] = sum_b U[b][n] V[b][k] and db[n] = sum_b U[b][n], windows in order
__global__ void outer_sum_kernel(const float* U, const float* V, int B, int N, int K, float* dW, float* db) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * K) return;
    const int n = (int)(i / K), k = (int)(i % K);
    float s = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
        const float u = U[(size_t)b * N + n];
        s = fmaf(u, V[(size_t)b * K + k], s);
        sb += u;
    }
    dW[i] = s;
    if (k == 0) db[n] = sb;
}

// ------------------------------------------------------------------------------------------------ softmax
// One wave per row of S [B * 4][L][L]: P = softmax(S) in place (saved); Pd = dropout(P) when the site is on.
struct Softmax {
    float* S;
    float* Pd;  // or nullptr
    int L, rows;  // rows = B * 4 * L
    Drop d;
};

__global__ __launch_bounds__(256) void softmax_kernel(Softmax a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= a.rows) return;
    float* s = a.S + (size_t)row * a.L;
    float v[4];
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = lane + 64 * c;
        v[c] = k < a.L ? s[k] : -INFINITY;
        mx = fmaxf(mx, v[c]);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        v[c] = lane + 64 * c < a.L ? expf(v[c] - mx) : 0.f;
        sum += v[c];
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
    const long zb = row / ((long)NH * a.L);           // window
    const uint32_t e0 = (uint32_t)(row % ((long)NH * a.L)) * (uint32_t)a.L;  // (head * L + query) * L
    const int64_t wid = a.d.thr ? a.d.wids[zb] : 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = lane + 64 * c;
        if (k >= a.L) continue;
        const float p = v[c] * inv;
        s[k] = p;
        if (a.Pd) a.Pd[(size_t)row * a.L + k] = (a.d.thr == 0 || drop_keep(a.d, wid, e0 + k)) ? p * a.d.scale : 0.f;
    }
}

// Pd = dropout(P) again, for the backward pass
__global__ void redrop_kernel(const float* P, float* Pd, int L, long n, Drop d) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long per = (long)NH * L * L;
    const long zb = i / per;
    const uint32_t e = (uint32_t)(i % per);
    Pd[i] = drop_keep(d, d.wids[zb], e) ? P[i] * d.scale : 0.f;
}

// dS = P o (dP - rowsum(dP o P)) / 16 in place over dPd, dP = dropout'(dPd); one wave per row
struct SoftmaxBwd {
    float* dP;
    const float* P;
    int L, rows;
    Drop d;
};

__global__ __launch_bounds__(256) void softmax_bwd_kernel(SoftmaxBwd a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= a.rows) return;
    float* g = a.dP + (size_t)row * a.L;
    const float* p = a.P + (size_t)row * a.L;
    const long zb = row / ((long)NH * a.L);
    const uint32_t e0 = (uint32_t)(row % ((long)NH * a.L)) * (uint32_t)a.L;
    const int64_t wid = a.d.thr ? a.d.wids[zb] : 0;
    float dv[4], pv[4];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = lane + 64 * c;
        dv[c] = 0.f;
        pv[c] = 0.f;
        if (k < a.L) {
            pv[c] = p[k];
            const float gg = g[k];
            dv[c] = (a.d.thr == 0 || drop_keep(a.d, wid, e0 + k)) ? gg * a.d.scale : 0.f;
        }
        const float t = dv[c] * pv[c];
        sum += t;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = lane + 64 * c;
        if (k < a.L) g[k] = pv[c] * (dv[c] - sum) * 0.0625f;
    }
}

// ------------------------------------------------------------------------------------------------ LayerNorm
// z = dropout(Y) + resid (saved); out = (LN(z) gamma + beta) * mask.  One wave per row, 8 columns per lane.
struct LnFwd {
    const float *Y, *resid;
    float *Z, *out;
    const float *g, *b, *mask;  // mask [R]
    int R, L;
    Drop d;
};

EG_D void ld8v(const float* p, float v[8]) {
    const float4 x = *(const float4*)p, y = *(const float4*)(p + 4);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
}
EG_D void st8v(float* p, const float v[8]) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
EG_D float wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}
// keep flags of the 8 elements from e (a multiple of 8) of window wid
EG_D void drop_keep8(const Drop& d, int64_t wid, uint32_t e, bool keep[8]) {
    const Philox4 r0 = drop_draw4(d, wid, e >> 2), r1 = drop_draw4(d, wid, (e >> 2) + 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        keep[i] = r0.c[i] >= d.thr;
        keep[4 + i] = r1.c[i] >= d.thr;
    }
}
EG_D void ln_stats(const float z[8], float& mean, float& rstd) {
    float s = ((z[0] + z[1]) + (z[2] + z[3])) + ((z[4] + z[5]) + (z[6] + z[7]));
    mean = wave_sum(s) * (1.0f / DM);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float c = z[i] - mean;
        q += c * c;
    }
    rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / DM) + 1e-5f);
}

__global__ __launch_bounds__(256) void ln_fwd_kernel(LnFwd a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= a.R) return;
    const int c0 = lane * 8;
    const size_t off = (size_t)row * DM + c0;
    float y[8], x[8], z[8], gg[8], bb[8], o[8];
    ld8v(a.Y + off, y);
    ld8v(a.resid + off, x);
    if (a.d.thr) {
        bool keep[8];
        drop_keep8(a.d, a.d.wids[row / a.L], (uint32_t)(row % a.L) * DM + c0, keep);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = keep[i] ? y[i] * a.d.scale : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = y[i] + x[i];
    st8v(a.Z + off, z);
    float mean, rstd;
    ln_stats(z, mean, rstd);
    ld8v(a.g + c0, gg);
    ld8v(a.b + c0, bb);
    const float m = a.mask[row];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float xh = (z[i] - mean) * rstd;
        const float t = xh * gg[i] + bb[i];
        o[i] = t * m;
    }
    st8v(a.out + off, o);
}

// Backward of the above.  dZ: the gradient of z (the residual's share); dY = dropout'(dZ): the sublayer output's share.  A wave
// walks its LN_ROWS rows in order and writes its partial of the gain / bias gradient to part[wave][0..511 | 512..1023].
struct LnBwd {
    const float *dOut, *Z, *g, *mask;
    float *dZ, *dY, *part;
    int R, L;
    Drop d;
};

__global__ __launch_bounds__(256) void ln_bwd_kernel(LnBwd a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long chunk = (long)blockIdx.x * 4 + wave;
    const long r0 = chunk * LN_ROWS;
    if (r0 >= a.R) return;
    const long r1 = r0 + LN_ROWS < a.R ? r0 + LN_ROWS : a.R;
    const int c0 = lane * 8;
    float gg[8], ag[8], ab[8];
    ld8v(a.g + c0, gg);
#pragma unroll
    for (int i = 0; i < 8; ++i) ag[i] = ab[i] = 0.f;
    for (long row = r0; row < r1; ++row) {
        const size_t off = (size_t)row * DM + c0;
        float z[8], d[8], dz[8], dy[8];
        ld8v(a.Z + off, z);
        ld8v(a.dOut + off, d);
        float mean, rstd;
        ln_stats(z, mean, rstd);
        const float m = a.mask[row];
        float s1 = 0.f, s2 = 0.f;
        float xh[8], dx[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            d[i] = d[i] * m;
            xh[i] = (z[i] - mean) * rstd;
            const float t = d[i] * xh[i];
            ag[i] += t;
            ab[i] += d[i];
            dx[i] = d[i] * gg[i];
            s1 += dx[i];
            const float u = dx[i] * xh[i];
            s2 += u;
        }
        const float m1 = wave_sum(s1) * (1.0f / DM), m2 = wave_sum(s2) * (1.0f / DM);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float u = xh[i] * m2;
            dz[i] = rstd * ((dx[i] - m1) - u);
            dy[i] = dz[i];
        }
        if (a.d.thr) {
            bool keep[8];
            drop_keep8(a.d, a.d.wids[row / a.L], (uint32_t)(row % a.L) * DM + c0, keep);
#pragma unroll
            for (int i = 0; i < 8; ++i) dy[i] = keep[i] ? dz[i] * a.d.scale : 0.f;
        }
        st8v(a.dZ + off, dz);
        st8v(a.dY + off, dy);
    }
    st8v(a.part + (size_t)chunk * (2 * DM) + c0, ag);
    st8v(a.part + (size_t)chunk * (2 * DM) + DM + c0, ab);
}

// ------------------------------------------------------------------------------------------------ loss
// Per window, over its T * D elements in a fixed order, in fp64: sum |out - target| (l1) or (out - target)^2 (l2), times the row
// mask.  Also writes model_out (optional) and d(loss)/d(out) into the [B * L][D] row layout (zero on the time token's row).
struct Loss {
    const float *outL, *target, *maskR, *p2w;
    const int64_t* t;
    float *model_out, *dout;
    double* winsum;
    int B, T, D, S, l2;
};

__global__ __launch_bounds__(256) void loss_window_kernel(Loss a) {
    __shared__ double red[256];
    const int b = blockIdx.x, L = a.T + 1;
    int64_t ts = a.t[b];
    ts = ts < 0 ? 0 : (ts >= a.S ? a.S - 1 : ts);
    // d(loss)/d(elem) = w[t_b] / (T D B): the mean over T * D (padded positions included), the weight, the mean over B
    const float coef = (float)((double)a.p2w[ts] / ((double)a.T * a.D * a.B));
    double acc = 0.0;
    const int n = a.T * a.D;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int tt = i / a.D, d = i % a.D;
        const size_t rl = (size_t)b * L + 1 + tt;
        const float o = a.outL[rl * a.D + d];
        const float diff = o - a.target[((size_t)b * a.T + tt) * a.D + d];
        const float m = a.maskR[rl];
        float gr;
        if (a.l2) {
            acc += (double)diff * (double)diff * (double)m;
            gr = 2.0f * diff * (m * coef);
        } else {
            acc += (double)fabsf(diff) * (double)m;
            gr = (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * (m * coef);
        }
        a.dout[rl * a.D + d] = gr;
        if (a.model_out) a.model_out[((size_t)b * a.T + tt) * a.D + d] = o;
    }
    for (int d = threadIdx.x; d < a.D; d += 256) a.dout[(size_t)b * L * a.D + d] = 0.f;
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.winsum[b] = red[0];
}

__global__ void loss_final_kernel(const double* winsum, const int64_t* t, const float* p2w, int B, int T, int D, int S, float* loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        int64_t ts = t[b];
        ts = ts < 0 ? 0 : (ts >= S ? S - 1 : ts);
        s += winsum[b] / ((double)T * D) * (double)p2w[ts];
    }
    *loss = (float)(s / B);
}

// out = in * scale[0] (the upstream gradient, a device scalar)
__global__ void scale_kernel(const float* in, const float* scale, long n, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] * scale[0];
}

// the bytes of a dropout mask: site 0 [B][4][L][L], sites 1, 2 [B][L][512]
__global__ void drop_mask_kernel(Drop d, long per, long n, uint8_t* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (d.thr == 0 || drop_keep(d, d.wids[i / per], (uint32_t)(i % per))) ? 1 : 0;
}

__global__ void iota_kernel(int64_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

}  // namespace tr
