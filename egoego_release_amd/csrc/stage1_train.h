// stage1_train.h — kernels of stage-1 training that train_step.h does not already have: HeadNet's loss with its gradient with
// respect to the heads (head_estimation_transformer.py:97-119 and 310-345 in one launch sequence, fp64), and LayerNorm forward /
// backward at stage 1's width of 256.  Everything else of the training encode (the contraction, the ordered folds, the fp64 bias
// strips, softmax and the Philox dropout) is train_step.h's, included below and used as it is.
#pragma once
#include "common.h"

namespace s1t {
// train_step.hip is a translation unit of the same library and defines the kernels of train_step.h under tr::.  This unit takes
// its own copy of them as s1t::tr:: (common.h is already in, so the nested include adds train_step.h's own text only): no kernel
// is defined twice under one name, and a kernel trace tells stage 1's launches from stage 2's.
#include "train_step.h"

static constexpr int DM = 256;        // d_model = FFN width of stage 1
static constexpr int MAX_WINDOW = 128;

// ------------------------------------------------------------------------------------------------ HeadNet's loss
// va2rot detaches the running rotation, so the rotation of frame t + 1 is a function of q_t (a constant) and of va_t alone:
//   q_{t+1} = normalize(standardize(aa2quat(dt * apply(q_t, va_t)) (x) q_t)),
// and the orientation term of frame t, sum((|standardize(gt_{t+1} (x) conj(q_{t+1}))| - [1,0,0,0])^2), has a gradient with respect
// to va_t only.  One thread walks the chain of a sequence with plain doubles; then thread t evaluates frame t once more on numbers
// that carry their derivative along the three components of va_t (forward mode), which yields the term and its 3-vector gradient
// from the same code that produced the chain.

// a value and its derivative along va_t's three components
struct D3 {
    double v, d[3];
    EG_D D3() {}
    EG_D D3(double x) : v(x) { d[0] = d[1] = d[2] = 0.0; }
};
EG_D D3 operator+(const D3& a, const D3& b) { D3 r; r.v = a.v + b.v; for (int i = 0; i < 3; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
EG_D D3 operator-(const D3& a, const D3& b) { D3 r; r.v = a.v - b.v; for (int i = 0; i < 3; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
EG_D D3 operator-(const D3& a) { D3 r; r.v = -a.v; for (int i = 0; i < 3; ++i) r.d[i] = -a.d[i]; return r; }
EG_D D3 operator*(const D3& a, const D3& b) {
    D3 r; r.v = a.v * b.v;
    for (int i = 0; i < 3; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
    return r;
}
EG_D D3 operator/(const D3& a, const D3& b) {
    D3 r; r.v = a.v / b.v;
    for (int i = 0; i < 3; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
    return r;
}
EG_D double val(double x) { return x; }
EG_D double val(const D3& x) { return x.v; }
EG_D double xsqrt(double x) { return sqrt(x); }
EG_D D3 xsqrt(const D3& x) {  // the derivative of a norm at zero is taken as zero, as autograd takes it
    D3 r; r.v = sqrt(x.v);
    for (int i = 0; i < 3; ++i) r.d[i] = x.v > 0.0 ? x.d[i] / (2.0 * r.v) : 0.0;
    return r;
}
EG_D double xsin(double x) { return sin(x); }
EG_D D3 xsin(const D3& x) { D3 r; r.v = sin(x.v); const double c = cos(x.v); for (int i = 0; i < 3; ++i) r.d[i] = c * x.d[i]; return r; }
EG_D double xcos(double x) { return cos(x); }
EG_D D3 xcos(const D3& x) { D3 r; r.v = cos(x.v); const double s = -sin(x.v); for (int i = 0; i < 3; ++i) r.d[i] = s * x.d[i]; return r; }
EG_D double xabs(double x) { return fabs(x); }
EG_D D3 xabs(const D3& x) {
    const double s = x.v > 0.0 ? 1.0 : (x.v < 0.0 ? -1.0 : 0.0);
    D3 r; r.v = fabs(x.v);
    for (int i = 0; i < 3; ++i) r.d[i] = s * x.d[i];
    return r;
}

// pytorch3d's quaternion_raw_multiply
template <class S>
EG_D void qraw(const S a[4], const S b[4], S o[4]) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// One step of va2rot (HE:108-113) from the constant rotation q with pytorch3d's formulas: quaternion_apply by raw products (no
// normalisation of q), axis_angle_to_quaternion with its Taylor branch below 1e-6, quaternion_multiply with w >= 0, the norm.
template <class S>
EG_D void chain_step(const double q[4], const S va[3], S out[4]) {
    const S Q[4] = {S(q[0]), S(q[1]), S(q[2]), S(q[3])};
    const S Qc[4] = {S(q[0]), S(-q[1]), S(-q[2]), S(-q[3])};
    const S P[4] = {S(0.0), va[0], va[1], va[2]};
    S t1[4], r[4];
    qraw(Q, P, t1);
    qraw(t1, Qc, r);
    const S dt(1.0 / 30.0);
    const S a[3] = {r[1] * dt, r[2] * dt, r[3] * dt};
    const S ang = xsqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const S half = ang * S(0.5);
    const S sh = val(ang) < 1e-6 ? S(0.5) - ang * ang / S(48.0) : xsin(half) / ang;
    const S qa[4] = {xcos(half), a[0] * sh, a[1] * sh, a[2] * sh};
    S nq[4];
    qraw(qa, Q, nq);
    if (val(nq[0]) < 0.0)
        for (int j = 0; j < 4; ++j) nq[j] = -nq[j];
    const S nrm = xsqrt(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
    for (int j = 0; j < 4; ++j) out[j] = nq[j] / nrm;
}

// orientation_loss (HE:40-48) of one frame
template <class S>
EG_D S orient_term(const double gt[4], const S pred[4]) {
    const S G[4] = {S(gt[0]), S(gt[1]), S(gt[2]), S(gt[3])};
    const S Pc[4] = {pred[0], -pred[1], -pred[2], -pred[3]};
    S d[4];
    qraw(G, Pc, d);
    if (val(d[0]) < 0.0)
        for (int j = 0; j < 4; ++j) d[j] = -d[j];
    const S e0 = xabs(d[0]) - S(1.0), e1 = xabs(d[1]), e2 = xabs(d[2]), e3 = xabs(d[3]);
    return ((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3;
}

struct HeadLoss {
    const float* heads;  // [B][window][4]: va | dist
    const float* pose;   // [B][T + 1][7]
    const float* vels;   // [B][T][6]
    int window, B, T;
    double dist_scale, w_rot, w_va, w_dist;
    double* part;        // [B][3]: a sequence's sums of the three terms
    double* d64;         // [B][window][4] or nullptr
    float* d32;          // [B][window][4] or nullptr
};

// One workgroup of MAX_WINDOW threads per sequence; thread t owns frame t (and row t of the gradient, zero for t >= T).
__global__ __launch_bounds__(MAX_WINDOW) void headnet_loss_kernel(HeadLoss a) {
    __shared__ double qs[MAX_WINDOW][4];  // q_t, the rotation frame t starts from
    __shared__ double red[3][MAX_WINDOW];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* hb = a.heads + (size_t)b * a.window * 4;
    const float* pb = a.pose + (size_t)b * (a.T + 1) * 7;
    if (t == 0) {
        double q[4] = {pb[3], pb[4], pb[5], pb[6]};
        for (int i = 0; i < a.T; ++i) {
            for (int j = 0; j < 4; ++j) qs[i][j] = q[j];
            const double va[3] = {hb[4 * i], hb[4 * i + 1], hb[4 * i + 2]};
            double nq[4];
            chain_step<double>(q, va, nq);
            for (int j = 0; j < 4; ++j) q[j] = nq[j];
        }
    }
    __syncthreads();
    double lo = 0.0, lv = 0.0, ld = 0.0;
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    if (t < a.T) {
        const double coef = 1.0 / ((double)a.B * (double)a.T);  // every mean is over all B * T frames
        const double q[4] = {qs[t][0], qs[t][1], qs[t][2], qs[t][3]};
        D3 va[3], pred[4];
        for (int k = 0; k < 3; ++k) {
            va[k] = D3((double)hb[4 * t + k]);
            va[k].d[k] = 1.0;
        }
        chain_step<D3>(q, va, pred);
        const float* gp = pb + (size_t)(t + 1) * 7;
        const double gt[4] = {gp[3], gp[4], gp[5], gp[6]};
        const D3 o = orient_term<D3>(gt, pred);
        lo = o.v;
        const float* gv = a.vels + ((size_t)b * a.T + t) * 6 + 3;
        for (int k = 0; k < 3; ++k) {
            const double e = (double)gv[k] - va[k].v;
            lv += e * e;
            g[k] = coef * (a.w_rot * o.d[k] - a.w_va * 2.0 * e);
        }
        const float* p0 = pb + (size_t)t * 7;
        const double s0 = (double)gp[0] - (double)p0[0], s1 = (double)gp[1] - (double)p0[1], s2 = (double)gp[2] - (double)p0[2];
        const double gd = a.dist_scale * sqrt(s0 * s0 + s1 * s1 + s2 * s2);
        const double e = (double)hb[4 * t + 3] - gd;
        ld = e * e;
        g[3] = coef * a.w_dist * 2.0 * e;
    }
    if (t < a.window) {
        const size_t o = ((size_t)b * a.window + t) * 4;
        for (int k = 0; k < 4; ++k) {
            if (a.d64) a.d64[o + k] = g[k];
            if (a.d32) a.d32[o + k] = (float)g[k];
        }
    }
    red[0][t] = lo;
    red[1][t] = lv;
    red[2][t] = ld;
    __syncthreads();
    for (int s = MAX_WINDOW / 2; s > 0; s >>= 1) {  // a fixed tree: the same bits on every run
        if (t < s)
            for (int k = 0; k < 3; ++k) red[k][t] += red[k][t + s];
        __syncthreads();
    }
    if (t < 3) a.part[(size_t)b * 3 + t] = red[t][0];
}

// loss[4] = (total, orient, va, dist): the sequences' sums added in order, each mean over B * T frames
__global__ void headnet_loss_final_kernel(const double* part, int B, int T, double w_rot, double w_va, double w_dist, double* loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 3; ++k) s[k] += part[(size_t)b * 3 + k];
    const double n = (double)B * (double)T;
    const double o = s[0] / n, v = s[1] / n, d = s[2] / n;
    loss[0] = (w_rot * o + w_va * v) + w_dist * d;
    loss[1] = o;
    loss[2] = v;
    loss[3] = d;
}

// ------------------------------------------------------------------------------------------------ training encode: prep
// xin = feats with the rows t >= valid[w] as zero rows (whatever they hold), the row mask and the window ids, all into the saves
struct Prep {
    const float* feats;
    const int* valid;
    const int64_t* wids;
    float *xin, *maskR;
    int64_t* wids_out;
    int W, L, D;
};

__global__ void prep_kernel(Prep a) {
    const long n = (long)a.W * a.L * a.D;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int d = (int)(i % a.D);
    const long row = i / a.D;
    const int w = (int)(row / a.L), t = (int)(row % a.L);
    const bool ok = t < a.valid[w];
    a.xin[i] = ok ? a.feats[i] : 0.f;
    if (d == 0) {
        a.maskR[row] = ok ? 1.f : 0.f;
        if (t == 0) a.wids_out[w] = a.wids ? a.wids[w] : (int64_t)w;
    }
}

// ------------------------------------------------------------------------------------------------ LayerNorm at width 256
// tr::ln_fwd_kernel / tr::ln_bwd_kernel with 4 columns per lane: z = dropout(Y) + resid (saved); out = (LN(z) gamma + beta) * mask.
EG_D void ld4v(const float* p, float v[4]) {
    const float4 x = *(const float4*)p;
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
EG_D void st4v(float* p, const float v[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
// keep flags of the 4 elements from e (a multiple of 4) of window wid: one Philox draw
EG_D void drop_keep4(const tr::Drop& d, int64_t wid, uint32_t e, bool keep[4]) {
    const Philox4 r = tr::drop_draw4(d, wid, e >> 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) keep[i] = r.c[i] >= d.thr;
}
EG_D void ln_stats(const float z[4], float& mean, float& rstd) {
    const float s = (z[0] + z[1]) + (z[2] + z[3]);
    mean = tr::wave_sum(s) * (1.0f / DM);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float c = z[i] - mean;
        q += c * c;
    }
    rstd = 1.0f / sqrtf(tr::wave_sum(q) * (1.0f / DM) + 1e-5f);
}

__global__ __launch_bounds__(256) void ln_fwd_kernel(tr::LnFwd a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= a.R) return;
    const int c0 = lane * 4;
    const size_t off = (size_t)row * DM + c0;
    float y[4], x[4], z[4], gg[4], bb[4], o[4];
    ld4v(a.Y + off, y);
    ld4v(a.resid + off, x);
    if (a.d.thr) {
        bool keep[4];
        drop_keep4(a.d, a.d.wids[row / a.L], (uint32_t)(row % a.L) * DM + c0, keep);
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = keep[i] ? y[i] * a.d.scale : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = y[i] + x[i];
    st4v(a.Z + off, z);
    float mean, rstd;
    ln_stats(z, mean, rstd);
    ld4v(a.g + c0, gg);
    ld4v(a.b + c0, bb);
    const float m = a.mask[row];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float xh = (z[i] - mean) * rstd;
        const float t = xh * gg[i] + bb[i];
        o[i] = t * m;
    }
    st4v(a.out + off, o);
}

// A wave walks its tr::LN_ROWS rows in order and writes its partial of the gain / bias gradient to part[chunk][0..255 | 256..511].
__global__ __launch_bounds__(256) void ln_bwd_kernel(tr::LnBwd a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long chunk = (long)blockIdx.x * 4 + wave;
    const long r0 = chunk * tr::LN_ROWS;
    if (r0 >= a.R) return;
    const long r1 = r0 + tr::LN_ROWS < a.R ? r0 + tr::LN_ROWS : a.R;
    const int c0 = lane * 4;
    float gg[4], ag[4], ab[4];
    ld4v(a.g + c0, gg);
#pragma unroll
    for (int i = 0; i < 4; ++i) ag[i] = ab[i] = 0.f;
    for (long row = r0; row < r1; ++row) {
        const size_t off = (size_t)row * DM + c0;
        float z[4], d[4], dz[4], dy[4];
        ld4v(a.Z + off, z);
        ld4v(a.dOut + off, d);
        float mean, rstd;
        ln_stats(z, mean, rstd);
        const float m = a.mask[row];
        float s1 = 0.f, s2 = 0.f;
        float xh[4], dx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
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
        const float m1 = tr::wave_sum(s1) * (1.0f / DM), m2 = tr::wave_sum(s2) * (1.0f / DM);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float u = xh[i] * m2;
            dz[i] = rstd * ((dx[i] - m1) - u);
            dy[i] = dz[i];
        }
        if (a.d.thr) {
            bool keep[4];
            drop_keep4(a.d, a.d.wids[row / a.L], (uint32_t)(row % a.L) * DM + c0, keep);
#pragma unroll
            for (int i = 0; i < 4; ++i) dy[i] = keep[i] ? dz[i] * a.d.scale : 0.f;
        }
        st4v(a.dZ + off, dz);
        st4v(a.dY + off, dy);
    }
    st4v(a.part + (size_t)chunk * (2 * DM) + c0, ag);
    st4v(a.part + (size_t)chunk * (2 * DM) + DM + c0, ab);
}

}  // namespace s1t
