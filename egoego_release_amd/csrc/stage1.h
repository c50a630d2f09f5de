// stage1.h — kernels of the stage-1 head-pose estimators (HeadFormer / HeadNormalFormer, d_model 256) on split-bf16 MFMAs.
//
// Every contraction runs as three v_mfma_f32_32x32x16_bf16 per 16-deep k step (hi*hi + lo*hi + hi*lo, fp32 accumulate), like
// stage 2's precision 3.  Weights are packed once (egoego_s1_load_weights) into fragment-tiled hi / lo planes (common.h,
// tiled_index); activations stay fp32 rows in the workspace and a consumer splits the 8 values a lane feeds the MFMA as it
// loads them.  At d_model 256 a 32-row tile of the residual stream is 32 KiB, so the whole layer tail (fc, residual, LayerNorm,
// mask, FFN, residual, LayerNorm, mask) runs in one workgroup per 32 rows out of LDS.
//
// Rows: window w of a call owns rows [w * Lp, (w + 1) * Lp), Lp = window rounded up to 32.  Row t < window is token t (pos_vec
// t + 1); rows window .. Lp - 1 only pad the tile: they are zero, never attended to and never written out.  Token t is "valid"
// when t < valid[w]; the reference (TM:126-141, use_full_attention=True) does NOT mask the other tokens as keys — it only
// multiplies each sublayer's output by the padding mask — and neither do these kernels.
#pragma once
#include "common.h"

namespace s1 {

static constexpr int DM = 256;    // d_model
static constexpr int HD = 1024;   // n_head * d_k = n_head * d_v
static constexpr int NH = 4;
static constexpr int DK = 256;
static constexpr int LN_STRIDE = DM + 4;  // fp32 LDS row stride of the tail's tiles (breaks the 1 KiB row alignment)

// A packed linear layer: W [N][K] as fragment-tiled hi / lo bf16 planes of Np x Kp (zero padded), bias [N] fp32.
struct Lin {
    const __bf16* hi;
    const __bf16* lo;
    const float* b;
    int N, K16;
};

// 8 consecutive fp32 of row `p` from column k (zero when !ok; columns >= K zero when !VEC).
template <bool VEC>
EG_D void load8(const float* p, int k, int K, bool ok, float v[8]) {
    if (VEC) {
        if (ok) {
            const float4 x = *(const float4*)(p + k), y = *(const float4*)(p + k + 4);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0.f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (ok && k + i < K) ? p[k + i] : 0.f;
    }
}

// One wave: the 32 x 32 block  A[32 rows][K] . W[nb*32 .. nb*32+31][K]^T.  Lane l feeds row l & 31 of A from `arow` (its own row
// pointer; `aok` = false reads zeros) and column l & 31 of the weight block.  Accumulator register r of lane l holds
// (row mfma32_row(r, l >> 5), column l & 31).
template <bool VEC>
EG_D f32x16 mm_rows_w(const float* arow, bool aok, int K, const Lin& w, int nb, int lane) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int hf = lane >> 5;
    const size_t base = (size_t)nb * w.K16 * 512 + (size_t)hf * 256 + (size_t)(lane & 31) * 8;
    for (int k16 = 0; k16 < w.K16; ++k16) {
        float a[8];
        load8<VEC>(arow, k16 * 16 + hf * 8, K, aok, a);
        u32x4 ah, al;
        split8(a, ah, al);
        const size_t off = base + (size_t)k16 * 512;
        const u32x4 bh = *(const u32x4*)(w.hi + off), bl = *(const u32x4*)(w.lo + off);
        acc = mfma3(ah, al, bh, bl, acc);
    }
    return acc;
}

// ------------------------------------------------------------------------------------------------ generic linear
// out = act(A . W^T + b) for up to two weight groups (grid.z): group g reads A's columns from a_goff * g and writes out's
// columns from o_goff * g.  Row m of A is A + m * lda.  With `window` > 0 the output rows follow the window layout: row m is
// token m % Lp of window m / Lp, written to out + ((m / Lp) * window + m % Lp) * ldo and skipped when m % Lp >= window.
struct GemmArgs {
    const float* A;
    long lda;
    int a_goff, K;
    float* out;
    long ldo;
    int o_goff;
    Lin w[2];
    int M, relu, Lp, window;
};

template <bool VEC>
__global__ __launch_bounds__(256) void s1_linear_kernel(GemmArgs g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = blockIdx.z;
    const Lin& w = g.w[grp];
    const int nb = blockIdx.y * 4 + wave;
    if (nb * 32 >= w.N) return;
    const int m = blockIdx.x * 32 + (lane & 31);
    const float* arow = g.A + (size_t)(m < g.M ? m : 0) * g.lda + (size_t)grp * g.a_goff;
    f32x16 acc = mm_rows_w<VEC>(arow, m < g.M, g.K, w, nb, lane);
    const int n = nb * 32 + (lane & 31);
    if (n >= w.N) return;
    const float bias = w.b[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mr = blockIdx.x * 32 + mfma32_row(r, lane >> 5);
        if (mr >= g.M) continue;
        float v = acc[r] + bias;
        if (g.relu) v = fmaxf(v, 0.f);
        size_t orow;
        if (g.window > 0) {
            const int t = mr % g.Lp;
            if (t >= g.window) continue;
            orow = (size_t)(mr / g.Lp) * g.window + t;
        } else {
            orow = mr;
        }
        g.out[orow * g.ldo + (size_t)grp * g.o_goff + n] = v;
    }
}

// ------------------------------------------------------------------------------------------------ embed
// X[row] = start_conv(feat) + position_vec[t + 1] for t < window (a token past valid[w] reads a zero feature row: bias + position,
// as the reference's zero-padded input gives); rows window .. Lp - 1 are zero.
struct EmbedArgs {
    const float* feat;    // [W][window][F]
    const int* valid;     // [W]
    const float* pos;     // [window + 1][256]
    float* X;             // [W * Lp][256]
    Lin w;
    int F, window, Lp, M;
};

template <bool VEC>
__global__ __launch_bounds__(256) void s1_embed_kernel(EmbedArgs e) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = blockIdx.y * 4 + wave;
    const int m = blockIdx.x * 32 + (lane & 31);
    const int win = m / e.Lp, t = m % e.Lp;
    const bool ok = t < min(e.valid[win], e.window);
    const float* arow = e.feat + ((size_t)win * e.window + (ok ? t : 0)) * e.F;
    f32x16 acc = mm_rows_w<VEC>(arow, ok, e.F, e.w, nb, lane);
    const int n = nb * 32 + (lane & 31);
    const float bias = e.w.b[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mr = blockIdx.x * 32 + mfma32_row(r, lane >> 5);
        const int tr = mr % e.Lp;
        const float v = tr < e.window ? (acc[r] + bias) + e.pos[(size_t)(tr + 1) * DM + n] : 0.f;
        e.X[(size_t)mr * DM + n] = v;
    }
}

// ------------------------------------------------------------------------------------------------ attention
// One workgroup per (window, head, 32-query tile): S = Q K^T / 16 over every key row t < window (padded tokens included),
// softmax in fp32, O = P V.  Q | K | V are the three 1024-column blocks of a [rows][3072] fp32 buffer; O is [rows][1024].
struct AttnArgs {
    const float* qkv;
    float* O;
    int window, Lp;
};

static constexpr int ATT_SROW = 128 + 4;

__global__ __launch_bounds__(256) void s1_attn_kernel(AttnArgs a) {
    __shared__ float S[32 * ATT_SROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
    const int win = blockIdx.x / NH, h = blockIdx.x % NH, qt = blockIdx.y;
    const size_t row0 = (size_t)win * a.Lp;
    const int nkb = a.Lp / 32;
    // S block (queries qt*32.., keys wave*32..)
    if (wave < nkb) {
        const float* qrow = a.qkv + (row0 + qt * 32 + (lane & 31)) * (3 * HD) + h * DK;
        const float* krow = a.qkv + (row0 + wave * 32 + (lane & 31)) * (3 * HD) + HD + h * DK;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k16 = 0; k16 < DK / 16; ++k16) {
            float x[8], y[8];
            load8<true>(qrow, k16 * 16 + hf * 8, DK, true, x);
            load8<true>(krow, k16 * 16 + hf * 8, DK, true, y);
            u32x4 ah, al, bh, bl;
            split8(x, ah, al);
            split8(y, bh, bl);
            acc = mfma3(ah, al, bh, bl, acc);
        }
        const int key = wave * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            S[mfma32_row(r, hf) * ATT_SROW + key] = key < a.window ? acc[r] / 16.0f : -INFINITY;
    }
    __syncthreads();
    // softmax: 8 rows per wave, keys lane and lane + 64
    for (int rr = 0; rr < 8; ++rr) {
        float* s = S + (wave * 8 + rr) * ATT_SROW;
        const float v0 = lane < a.Lp ? s[lane] : -INFINITY;
        const float v1 = lane + 64 < a.Lp ? s[lane + 64] : -INFINITY;
        float mx = fmaxf(v0, v1);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        const float e0 = lane < a.Lp ? __expf(v0 - mx) : 0.f;
        const float e1 = lane + 64 < a.Lp ? __expf(v1 - mx) : 0.f;
        float sum = e0 + e1;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const float inv = 1.0f / sum;
        if (lane < a.Lp) s[lane] = e0 * inv;
        if (lane + 64 < a.Lp) s[lane + 64] = e1 * inv;
    }
    __syncthreads();
    // O = P V: wave owns output columns wave*64 .. +63 (two 32-column blocks), k = key
    const float* prow = S + (lane & 31) * ATT_SROW;
    for (int cb = 0; cb < 2; ++cb) {
        const int d = wave * 64 + cb * 32 + (lane & 31);
        const float* vcol = a.qkv + row0 * (3 * HD) + 2 * HD + h * DK + d;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k16 = 0; k16 < a.Lp / 16; ++k16) {
            const int kb = k16 * 16 + hf * 8;
            float x[8], y[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                x[i] = prow[kb + i];
                y[i] = vcol[(size_t)(kb + i) * (3 * HD)];
            }
            u32x4 ah, al, bh, bl;
            split8(x, ah, al);
            split8(y, bh, bl);
            acc = mfma3(ah, al, bh, bl, acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            a.O[(row0 + qt * 32 + mfma32_row(r, hf)) * HD + h * DK + d] = acc[r];
    }
}

// ------------------------------------------------------------------------------------------------ layer tail
// One workgroup (8 waves, wave j = output columns 32j..32j+31) per 32 rows:
//   Y = LN1(O fc^T + b_fc + X) * mask;  X' = LN2(relu(Y w1^T + b1) w2^T + b2 + Y) * mask
// X is read (residual) and overwritten in place; dbg (optional) receives X' of every token t < window as [W][window][256].
struct TailArgs {
    const float* O;
    float* X;
    float* dbg;
    const int* valid;
    Lin fc, w1, w2;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    int window, Lp;
};

// LayerNorm (eps 1e-5, biased variance) of 4 rows per wave over the LDS tile, then the row mask.
EG_D void tail_ln(float* Y, const float* g, const float* b, const int* valid, int window, int Lp, int row0, int wave, int lane) {
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        float* y = Y + r * LN_STRIDE;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = y[lane + 64 * i];
        float s = (v[0] + v[1]) + (v[2] + v[3]);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s * (1.0f / DM);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) q += (v[i] - mean) * (v[i] - mean);
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
        const float rstd = 1.0f / sqrtf(q * (1.0f / DM) + 1e-5f);
        const int m = row0 + r;
        const float mask = (m % Lp) < min(valid[m / Lp], window) ? 1.f : 0.f;  // valid > window counts as window
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = lane + 64 * i;
            y[n] = ((v[i] - mean) * rstd * g[n] + b[n]) * mask;
        }
    }
}

__global__ __launch_bounds__(512) void s1_tail_kernel(TailArgs a) {
    extern __shared__ float smem[];
    float* Y = smem;                    // [32][LN_STRIDE]
    float* Hs = smem + 32 * LN_STRIDE;  // [32][LN_STRIDE]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5;
    const int row0 = blockIdx.x * 32;
    const int n = wave * 32 + (lane & 31);
    // fc + bias + residual
    {
        const float* arow = a.O + (size_t)(row0 + (lane & 31)) * HD;
        f32x16 acc = mm_rows_w<true>(arow, true, HD, a.fc, wave, lane);
        const float bias = a.fc.b[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = mfma32_row(r, hf);
            Y[rr * LN_STRIDE + n] = (acc[r] + bias) + a.X[(size_t)(row0 + rr) * DM + n];
        }
    }
    __syncthreads();
    tail_ln(Y, a.ln1_g, a.ln1_b, a.valid, a.window, a.Lp, row0, wave, lane);
    __syncthreads();
    {
        f32x16 acc = mm_rows_w<true>(Y + (lane & 31) * LN_STRIDE, true, DM, a.w1, wave, lane);
        const float bias = a.w1.b[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) Hs[mfma32_row(r, hf) * LN_STRIDE + n] = fmaxf(acc[r] + bias, 0.f);
    }
    __syncthreads();
    {
        f32x16 acc = mm_rows_w<true>(Hs + (lane & 31) * LN_STRIDE, true, DM, a.w2, wave, lane);
        const float bias = a.w2.b[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = mfma32_row(r, hf);
            Y[rr * LN_STRIDE + n] = (acc[r] + bias) + Y[rr * LN_STRIDE + n];
        }
    }
    __syncthreads();
    tail_ln(Y, a.ln2_g, a.ln2_b, a.valid, a.window, a.Lp, row0, wave, lane);
    __syncthreads();
    // write back: 32 rows x 256 fp32, 512 threads x 16 values
    for (int i = threadIdx.x; i < 32 * DM; i += 512) {
        const int rr = i / DM, c = i % DM;
        const int m = row0 + rr, t = m % a.Lp;
        // rows window .. Lp-1 stay zero (their mask is 0 as valid <= window)
        const float v = Y[rr * LN_STRIDE + c];
        a.X[(size_t)m * DM + c] = v;
        if (a.dbg && t < a.window) a.dbg[((size_t)(m / a.Lp) * a.window + t) * DM + c] = v;
    }
}

// ------------------------------------------------------------------------------------------------ per-frame geometry (fp64)
EG_D void qmul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// rotation matrix (row-major) -> unit quaternion (w, x, y, z) with w >= 0
EG_D void mat2quat(const double m[9], double q[4]) {
    const double tr = m[0] + m[4] + m[8];
    double w, x, y, z;
    if (tr > m[0] && tr > m[4] && tr > m[8]) {
        const double s = 2.0 * sqrt(1.0 + tr);
        w = 0.25 * s; x = (m[7] - m[5]) / s; y = (m[2] - m[6]) / s; z = (m[3] - m[1]) / s;
    } else if (m[0] > m[4] && m[0] > m[8]) {
        const double s = 2.0 * sqrt(1.0 + m[0] - m[4] - m[8]);
        w = (m[7] - m[5]) / s; x = 0.25 * s; y = (m[1] + m[3]) / s; z = (m[2] + m[6]) / s;
    } else if (m[4] > m[8]) {
        const double s = 2.0 * sqrt(1.0 + m[4] - m[0] - m[8]);
        w = (m[2] - m[6]) / s; x = (m[1] + m[3]) / s; y = 0.25 * s; z = (m[5] + m[7]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + m[8] - m[0] - m[4]);
        w = (m[3] - m[1]) / s; x = (m[2] + m[6]) / s; y = (m[5] + m[7]) / s; z = 0.25 * s;
    }
    const double nrm = sqrt(w * w + x * x + y * y + z * z), sg = w < 0 ? -1.0 : 1.0;
    q[0] = sg * w / nrm; q[1] = sg * x / nrm; q[2] = sg * y / nrm; q[3] = sg * z / nrm;
}

EG_D void mat3mul(const double a[9], const double b[9], double o[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

EG_D void mat3vec(const double a[9], const double v[3], double o[3]) {
    for (int i = 0; i < 3; ++i) o[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}

// GravityNet's input (head_normal_estimation_transformer.py:118-145): per frame t < n = min(len, window + 1) - 1 of a sequence,
// [rot6d(R_t), p_t, rot6d(R_{t+1} R_t^T), p_{t+1} - p_t] (18 fp32); frames n .. window - 1 are zero; valid[s] = max(n, 0).
__global__ void s1_gravity_features_kernel(const float* rot, const float* trans, const int* len, int Lmax, int window, float* feat,
                                           int* valid, int S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * window) return;
    const int s = i / window, t = i % window;
    const int n = min(len[s], window + 1) - 1;
    float* f = feat + (size_t)i * 18;
    if (t == 0) valid[s] = n > 0 ? n : 0;
    if (t >= n) {
        for (int j = 0; j < 18; ++j) f[j] = 0.f;
        return;
    }
    const float* R0 = rot + ((size_t)s * Lmax + t) * 9;
    const float* R1 = R0 + 9;
    const float* p0 = trans + ((size_t)s * Lmax + t) * 3;
    const float* p1 = p0 + 3;
    for (int j = 0; j < 6; ++j) f[j] = R0[j];
    for (int j = 0; j < 3; ++j) f[6 + j] = p0[j];
    // rows 0, 1 of R1 R0^T: (R1 R0^T)[a][b] = sum_c R1[a][c] R0[b][c]
    for (int aa = 0; aa < 2; ++aa)
        for (int b = 0; b < 3; ++b)
            f[9 + 3 * aa + b] = R1[3 * aa] * R0[3 * b] + R1[3 * aa + 1] * R0[3 * b + 1] + R1[3 * aa + 2] * R0[3 * b + 2];
    for (int j = 0; j < 3; ++j) f[15 + j] = p1[j] - p0[j];
}

// HeadNet's integration, one thread per sequence (head_estimation_transformer.py:97-119, 180-212, 214-308), fp64:
// quaternions q_0 = q0, q_{t+1} = normalize(standardize(aa2quat(dt * rotate(q_t, va_t)) * q_t)) over the T frames of the
// sequence's consecutive windows win0 .. (one chain: each block starts from the last rotation of the previous one);
// scale = mean(dist / dist_scale) / mean |slam_{i+1} - slam_i| over the first min(T, len - 1) steps; trans_0 = slam_0,
// trans_{i+1} = trans_i + scale (slam_{i+1} - slam_i) over all len - 1 steps.
__global__ void s1_integrate_kernel(const float* heads, int window, const int* T, const int* win0, const double* q0,
                                    const double* slam, const int* len, int Lmax, int Qmax, float dist_scale, double* quat,
                                    double* trans, double* scale, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int Ts = T[s], L = len[s];
    double q[4] = {q0[4 * s], q0[4 * s + 1], q0[4 * s + 2], q0[4 * s + 3]};
    double* qo = quat + (size_t)s * Qmax * 4;
    for (int j = 0; j < 4; ++j) qo[j] = q[j];
    const double dt = 1.0 / 30.0;
    double dsum = 0.0;
    const int m = min(Ts, L - 1);
    for (int t = 0; t < Ts; ++t) {
        const float* hrow = heads + ((size_t)(win0[s] + t / window) * window + t % window) * 4;
        const double v[3] = {hrow[0], hrow[1], hrow[2]};
        if (t < m) dsum += (double)(hrow[3] / dist_scale);  // fp32 division, as the reference's tensor / float
        // angv = q v q^-1
        const double u[3] = {q[1], q[2], q[3]}, w = q[0];
        const double c1[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const double c2[3] = {u[1] * c1[2] - u[2] * c1[1], u[2] * c1[0] - u[0] * c1[2], u[0] * c1[1] - u[1] * c1[0]};
        double a[3];
        for (int j = 0; j < 3; ++j) a[j] = (v[j] + 2.0 * (w * c1[j] + c2[j])) * dt;
        const double ang = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double half = 0.5 * ang;
        const double sh = ang < 1e-6 ? 0.5 - ang * ang / 48.0 : sin(half) / ang;
        const double qa[4] = {cos(half), a[0] * sh, a[1] * sh, a[2] * sh};
        double nq[4];
        qmul(qa, q, nq);
        const double sg = nq[0] < 0 ? -1.0 : 1.0;
        const double nrm = sqrt(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
        for (int j = 0; j < 4; ++j) q[j] = sg * nq[j] / nrm;
        if (t + 1 < Qmax)
            for (int j = 0; j < 4; ++j) qo[4 * (t + 1) + j] = q[j];
    }
    const double* sl = slam + (size_t)s * Lmax * 3;
    double lsum = 0.0;
    for (int i = 0; i < m; ++i) {
        const double d0 = sl[3 * i + 3] - sl[3 * i], d1 = sl[3 * i + 4] - sl[3 * i + 1], d2 = sl[3 * i + 5] - sl[3 * i + 2];
        lsum += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    }
    const double sc = m > 0 ? (dsum / m) / (lsum / m) : 1.0;
    scale[s] = sc;
    double* to = trans + (size_t)s * Lmax * 3;
    double p[3] = {sl[0], sl[1], sl[2]};
    for (int j = 0; j < 3; ++j) to[j] = p[j];
    for (int i = 0; i + 1 < L; ++i) {
        for (int j = 0; j < 3; ++j) {
            p[j] += sc * (sl[3 * i + 3 + j] - sl[3 * i + j]);
            to[3 * (i + 1) + j] = p[j];
        }
    }
}

// GravityNet's trajectory (head_normal_estimation_transformer.py:214-294), one thread per sequence, fp64:
// a_0 = p_0, a_{i+1} = a_i + scale Rn (p_{i+1} - p_i); out_i = [Ralign (a_i - a_0) + origin, quat(Ralign Rn R_i)].
// With Ralign = I and origin = p_0 this is the trajectory the Umeyama alignment reads; with the alignment's r and the
// ground-truth start it is the de-headed head pose.
__global__ void s1_gravity_apply_kernel(const float* rot, const float* trans, const int* len, int Lmax, const double* Rn,
                                        const double* scl, const double* Ral, const double* origin, double* pose, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double rn[9], ra[9], rar[9];
    for (int j = 0; j < 9; ++j) { rn[j] = Rn[9 * s + j]; ra[j] = Ral[9 * s + j]; }
    mat3mul(ra, rn, rar);
    const double sc = scl[s];
    const float* P = trans + (size_t)s * Lmax * 3;
    double a[3] = {0, 0, 0};
    for (int i = 0; i < len[s]; ++i) {
        if (i > 0) {
            const double d[3] = {(double)P[3 * i] - P[3 * i - 3], (double)P[3 * i + 1] - P[3 * i - 2], (double)P[3 * i + 2] - P[3 * i - 1]};
            double rd[3];
            mat3vec(rn, d, rd);
            for (int j = 0; j < 3; ++j) a[j] += sc * rd[j];
        }
        double o[3];
        mat3vec(ra, a, o);
        double* po = pose + ((size_t)s * Lmax + i) * 7;
        for (int j = 0; j < 3; ++j) po[j] = o[j] + origin[3 * s + j];
        double R[9], M[9];
        for (int j = 0; j < 9; ++j) R[j] = rot[((size_t)s * Lmax + i) * 9 + j];
        mat3mul(rar, R, M);
        mat2quat(M, po + 3);
    }
}

// ------------------------------------------------------------------------------------------------ Rodrigues + planar Umeyama
static constexpr int ALIGN_CHUNK = 512;  // frames of the trajectory held in LDS at a time

EG_D double round_f32(double x) { return (double)(float)x; }

// One wave per sequence.  Rn: head_normal_estimation_transformer.py:47-63 in fp64, rounded through fp32.  Ralign: the r of evo's
// umeyama_alignment on est_i = p_0 + a_i (a as in s1_gravity_apply_kernel) and ref_i, both with z = 1, over n = min(len, ref_len)
// frames.  With z constant the 3 x 3 covariance is the 2 x 2 matrix A = (1/n) sum (ref_i - mean_ref)(est_i - mean_est)^T bordered
// by zeros, and u s v with evo's determinant fix is blockdiag(Q, det Q), Q the orthogonal polar factor of A:
//   det A >= 0:  Q = [[e, -f], [f, e]] / hypot(e, f),  e = A00 + A11, f = A10 - A01   (rotation)
//   det A <  0:  Q = [[e, f], [f, -e]] / hypot(e, f),  e = A00 - A11, f = A01 + A10   (reflection)
// Order: per chunk of ALIGN_CHUNK frames the lanes compute Rn (p_i - p_{i-1}) into LDS, lane 0 runs the serial chain over it, and
// lane l sums frames l, l + 64, ... in fp64; pass 0 gives the means, pass 1 the covariance; the 64 partials are folded in lane
// order.  Nothing depends on S, Lmax or Rmax.
__global__ __launch_bounds__(64) void s1_gravity_align_kernel(const float* trans, const int* len, int Lmax, const float* normal,
                                                              const double* scl, const double* ref, const int* ref_len, int Rmax,
                                                              double* Rn_out, double* Ral_out) {
    __shared__ double axy[ALIGN_CHUNK][2];
    __shared__ double part[64][4];
    __shared__ double carry[2];
    __shared__ double tot[4];
    const int s = blockIdx.x, lane = threadIdx.x;
    double rn[9];
    {
        const double n0 = normal[3 * s], n1 = normal[3 * s + 1], n2 = normal[3 * s + 2];
        const double nn = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        const double a0 = n0 / nn, a1 = n1 / nn, a2 = n2 / nn;
        const double v0 = a1, v1 = -a0, v2 = 0.0;  // a x (0, 0, 1)
        const double c = a2, sn = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
        const double k[9] = {0.0, -v2, v1, v2, 0.0, -v0, -v1, v0, 0.0};
        double kk[9];
        mat3mul(k, k, kk);
        const double g = (1.0 - c) / (sn * sn);
        for (int j = 0; j < 9; ++j) rn[j] = round_f32((j % 4 == 0 ? 1.0 : 0.0) + k[j] + kk[j] * g);
    }
    if (lane < 9) Rn_out[9 * s + lane] = rn[lane];
    const int n = max(0, min(min(len[s], Lmax), min(ref_len[s], Rmax)));
    const double sc = scl[s];
    const float* P = trans + (size_t)s * Lmax * 3;
    const double* Rf = ref + (size_t)s * Rmax * 7;
    const double p0x = n > 0 ? (double)P[0] : 0.0, p0y = n > 0 ? (double)P[1] : 0.0;
    double mean[4] = {0, 0, 0, 0};  // est x, est y, ref x, ref y
    double A[4] = {0, 0, 0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        double acc[4] = {0, 0, 0, 0};
        if (lane == 0) carry[0] = carry[1] = 0.0;
        for (int c0 = 0; c0 < n; c0 += ALIGN_CHUNK) {
            const int m = min(ALIGN_CHUNK, n - c0);
            __syncthreads();
            for (int j = lane; j < m; j += 64) {
                const int i = c0 + j;
                double dx = 0.0, dy = 0.0;
                if (i > 0) {
                    const double d[3] = {(double)P[3 * i] - P[3 * i - 3], (double)P[3 * i + 1] - P[3 * i - 2], (double)P[3 * i + 2] - P[3 * i - 1]};
                    dx = rn[0] * d[0] + rn[1] * d[1] + rn[2] * d[2];
                    dy = rn[3] * d[0] + rn[4] * d[1] + rn[5] * d[2];
                }
                axy[j][0] = dx;
                axy[j][1] = dy;
            }
            __syncthreads();
            if (lane == 0) {
                double ax = carry[0], ay = carry[1];
                for (int j = 0; j < m; ++j) {
                    if (c0 + j > 0) {
                        ax += sc * axy[j][0];
                        ay += sc * axy[j][1];
                    }
                    axy[j][0] = ax;
                    axy[j][1] = ay;
                }
                carry[0] = ax;
                carry[1] = ay;
            }
            __syncthreads();
            for (int j = lane; j < m; j += 64) {
                const int i = c0 + j;
                const double ex = axy[j][0] + p0x, ey = axy[j][1] + p0y;
                const double rx = Rf[(size_t)i * 7], ry = Rf[(size_t)i * 7 + 1];
                if (pass == 0) {
                    acc[0] += ex; acc[1] += ey; acc[2] += rx; acc[3] += ry;
                } else {
                    const double qx = ex - mean[0], qy = ey - mean[1], wx = rx - mean[2], wy = ry - mean[3];
                    acc[0] += wx * qx; acc[1] += wx * qy; acc[2] += wy * qx; acc[3] += wy * qy;
                }
            }
        }
        __syncthreads();
        for (int j = 0; j < 4; ++j) part[lane][j] = acc[j];
        __syncthreads();
        if (lane == 0) {
            for (int j = 0; j < 4; ++j) {
                double t = 0.0;
                for (int l = 0; l < 64; ++l) t += part[l][j];
                tot[j] = n > 0 ? t / n : 0.0;
            }
        }
        __syncthreads();
        for (int j = 0; j < 4; ++j) (pass == 0 ? mean : A)[j] = tot[j];
    }
    if (lane == 0) {
        const bool rot = A[0] * A[3] - A[1] * A[2] >= 0.0;
        const double e = rot ? A[0] + A[3] : A[0] - A[3];
        const double f = rot ? A[2] - A[1] : A[1] + A[2];
        const double h = hypot(e, f);
        double q[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (h != 0.0) {  // (h == 0: a zero covariance, n <= 1 — the SVD path's answer for a zero matrix; NaN input stays NaN)
            const double ce = round_f32(e / h), sf = round_f32(f / h);
            q[0] = ce;
            q[1] = rot ? -sf : sf;
            q[3] = sf;
            q[4] = rot ? ce : -ce;
            q[8] = rot ? 1.0 : -1.0;
        }
        for (int j = 0; j < 9; ++j) Ral_out[9 * s + j] = q[j];
    }
}

// ------------------------------------------------------------------------------------------------ stage-1 head-pose metrics
// pytorch3d's quaternion_to_matrix (w, x, y, z; any norm), row-major
EG_D void quat2mat_p3d(const double* q, double m[9]) {
    const double r = q[0], i = q[1], j = q[2], k = q[3];
    const double two_s = 2.0 / (r * r + i * i + j * j + k * k);
    m[0] = 1 - two_s * (j * j + k * k); m[1] = two_s * (i * j - k * r);     m[2] = two_s * (i * k + j * r);
    m[3] = two_s * (i * j + k * r);     m[4] = 1 - two_s * (i * i + k * k); m[5] = two_s * (j * k - i * r);
    m[6] = two_s * (i * k - j * r);     m[7] = two_s * (j * k + i * r);     m[8] = 1 - two_s * (i * i + j * j);
}

// egoego/eval/head_pose_metrics.py:26-44, one wave per sequence: lane l sums frames l, l + 64, ... in fp64, the 64 partials are
// folded in lane order and divided by the length.  out[b] = (head_dist, head_dist_rot_only, head_trans_err * 1000).
__global__ __launch_bounds__(64) void s1_head_pose_metrics_kernel(const double* pred, const double* gt, const int* lengths, int Tmax,
                                                                  double* out) {
    __shared__ double part[64][3];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = max(0, min(lengths[b], Tmax));
    double acc[3] = {0, 0, 0};
    for (int t = lane; t < n; t += 64) {
        const double* p = pred + ((size_t)b * Tmax + t) * 7;
        const double* g = gt + ((size_t)b * Tmax + t) * 7;
        double Rp[9], Rg[9], inv[9], E[9];
        quat2mat_p3d(p + 3, Rp);
        quat2mat_p3d(g + 3, Rg);
        // Rg^-1 = adj(Rg) / det(Rg)
        inv[0] = Rg[4] * Rg[8] - Rg[5] * Rg[7]; inv[1] = Rg[2] * Rg[7] - Rg[1] * Rg[8]; inv[2] = Rg[1] * Rg[5] - Rg[2] * Rg[4];
        inv[3] = Rg[5] * Rg[6] - Rg[3] * Rg[8]; inv[4] = Rg[0] * Rg[8] - Rg[2] * Rg[6]; inv[5] = Rg[2] * Rg[3] - Rg[0] * Rg[5];
        inv[6] = Rg[3] * Rg[7] - Rg[4] * Rg[6]; inv[7] = Rg[1] * Rg[6] - Rg[0] * Rg[7]; inv[8] = Rg[0] * Rg[4] - Rg[1] * Rg[3];
        const double det = Rg[0] * inv[0] + Rg[1] * inv[3] + Rg[2] * inv[6];
        for (int j = 0; j < 9; ++j) inv[j] /= det;
        mat3mul(Rp, inv, E);
        double fr = 0.0;
        for (int j = 0; j < 9; ++j) {
            const double d = (j % 4 == 0 ? 1.0 : 0.0) - E[j];
            fr += d * d;
        }
        double Et[3];
        mat3vec(E, g, Et);
        double ft = 0.0, tt = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double d = p[j] - Et[j], u = p[j] - g[j];
            ft += d * d;
            tt += u * u;
        }
        acc[0] += sqrt(fr + ft);
        acc[1] += sqrt(fr);
        acc[2] += sqrt(tt);
    }
    for (int j = 0; j < 3; ++j) part[lane][j] = acc[j];
    __syncthreads();
    if (lane < 3) {
        double t = 0.0;
        for (int l = 0; l < 64; ++l) t += part[l][lane];
        t /= n;  // a length of 0 gives NaN: the mean of no frames
        out[3 * b + lane] = lane == 2 ? t * 1000.0 : t;
    }
}

}  // namespace s1
