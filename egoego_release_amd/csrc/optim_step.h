// optim_step.h — the kernels of the fused parameter update (egoego_optim_*): the gradient norm, the skip decision with the
// device-resident counters, and Adam + EMA + gradient clearing in one pass over a list of fp32 tensors.
//
//   table_kernel / chunks_kernel   the descriptor tables inside the caller's state block: one Tensor entry per tensor (the five
//                                  pointers, the element count, the first chunk), one Chunk entry per CHUNK elements of a tensor
//   norm_kernel                    one workgroup per chunk: sum of (g * inv_scale)^2 in fp64, in a fixed order -> one partial
//   decide_kernel                  one workgroup: the partials in a fixed order -> total_norm; the skip rule; the counters; this
//                                  step's scalars (step size, sqrt of the second bias correction, the EMA action, 1 - decay, and
//                                  with clipping on clip_coef = min(1, max_norm / (total_norm + clip_eps)))
//   apply_kernel                   grid-stride over the chunk table: Adam (L2 or decoupled weight decay; the gradient unscaled,
//                                  then clipped, in registers only), then the EMA, then the gradient's zeros
//
// No float atomics and no cross-workgroup communication inside a kernel: the three launches are ordered by the stream.  Every
// value that goes to memory is written by an ordinary vector store from plain C++.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/egoego_hip.h"

namespace op {

constexpr int CHUNK = 4096;  // elements of one tensor per chunk: a multiple of 4, so a chunk keeps its tensor's 16-byte phase
constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;  // of apply_kernel
constexpr int MAX_LOSSES = EGOEGO_OPTIM_MAX_LOSSES;
constexpr int TABLE_BATCH = 16;  // Tensor entries one table_kernel launch carries in its arguments
constexpr size_t HEADER_BYTES = 256;  // egoego_optim_state, padded: the tables start here

struct Tensor {
    float* p;
    float* g;
    float* m;
    float* v;
    float* ema;
    int64_t count;
    int64_t first_chunk;
};
struct Chunk {
    int32_t tensor;
    int32_t count;
    int64_t off;
};

struct TableArgs {
    Tensor t[TABLE_BATCH];
    int first, n;
};

__global__ void table_kernel(TableArgs a, Tensor* table) {
    const int i = threadIdx.x;
    if (i < a.n) table[a.first + i] = a.t[i];
}

__global__ void chunks_kernel(const Tensor* table, int n_tensors, Chunk* chunks, int n_chunks) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    int lo = 0, hi = n_tensors - 1;  // the last tensor whose first chunk is <= c
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
    }
    const int64_t off = ((int64_t)c - table[lo].first_chunk) * CHUNK;
    const int64_t left = table[lo].count - off;
    Chunk ch;
    ch.tensor = lo;
    ch.count = (int32_t)(left < CHUNK ? left : CHUNK);
    ch.off = off;
    chunks[c] = ch;
}

// ---------------------------------------------------------------------------------------------------------------- the norm
// Lane: its elements in ascending order; wave: a fixed shuffle tree; workgroup: the four wave sums in wave order.
__global__ __launch_bounds__(THREADS) void norm_kernel(const Tensor* table, const Chunk* chunks, const float* inv_scale, double* partial) {
    __shared__ double wave_sum[THREADS / 64];
    const Chunk ch = chunks[blockIdx.x];
    const float* g = table[ch.tensor].g + ch.off;
    const float inv = inv_scale ? *inv_scale : 1.0f;
    double s = 0.0;
    for (int i = threadIdx.x; i < ch.count; i += THREADS) {
        const double x = (double)(g[i] * inv);
        s += x * x;
    }
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wave_sum[0];
        for (int w = 1; w < THREADS / 64; ++w) t += wave_sum[w];
        partial[blockIdx.x] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the decision
struct Decide {
    const double* partial;
    int n_chunks;
    const float* losses[MAX_LOSSES];
    int n_losses;
    const float* found_inf;
    int skip_nonfinite, do_adam, do_ema;
    double lr, beta1, beta2;
    double max_norm, clip_eps;  // max_norm <= 0: no clipping
    egoego_optim_ema ema;
    egoego_optim_state* st;
};

// Thread t adds the partials of chunks [t * per, (t + 1) * per) in chunk order; thread 0 adds the 256 sums in thread order.
__global__ __launch_bounds__(THREADS) void decide_kernel(Decide a) {
    __shared__ double seg[THREADS];
    if (a.do_adam) {
        const int per = (a.n_chunks + THREADS - 1) / THREADS;
        const int lo = threadIdx.x * per;
        const int hi = lo + per < a.n_chunks ? lo + per : a.n_chunks;
        double s = 0.0;
        for (int c = lo; c < hi; ++c) s += a.partial[c];
        seg[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    egoego_optim_state st = *a.st;
    bool skip = false;
    if (a.do_adam) {
        double sum = 0.0;
        for (int t = 0; t < THREADS; ++t) sum += seg[t];
        const double norm = sqrt(sum);
        st.total_norm = norm;
        st.total_norm_f32 = (float)norm;
        skip = isnan(norm) || (a.skip_nonfinite && isinf(norm));
    }
    for (int i = 0; i < a.n_losses; ++i) {
        const float l = *a.losses[i];
        skip = skip || isnan(l) || (a.skip_nonfinite && isinf(l));
    }
    if (a.found_inf && *a.found_inf != 0.0f) skip = true;
    st.last_skip = skip ? 1 : 0;
    st.ema_action = EGOEGO_OPTIM_EMA_NONE;
    st.clip_coef = 1.0f;
    if (skip) {
        st.skipped += 1;
    } else {
        st.applied += 1;
        if (a.do_adam) {
            st.adam_step += 1;
            const double k = (double)st.adam_step;
            st.step_size = (float)(a.lr / (1.0 - pow(a.beta1, k)));
            st.bc2_sqrt = (float)sqrt(1.0 - pow(a.beta2, k));
            if (a.max_norm > 0.0) {  // clip_grad_norm_'s coefficient, in fp64 from the fp64 norm, rounded once
                const double coef = a.max_norm / (st.total_norm + a.clip_eps);
                st.clip_coef = (float)(coef < 1.0 ? coef : 1.0);
            }
        }
        if (a.do_ema) {  // ema-pytorch's update(): the decay is read after the step counter has advanced
            const int64_t step = *a.ema.d_step;
            *a.ema.d_step = step + 1;
            if (step % a.ema.update_every == 0) {
                if (step <= a.ema.update_after_step) {
                    st.ema_action = EGOEGO_OPTIM_EMA_COPY;
                } else if (*a.ema.d_initted == 0.0f) {
                    st.ema_action = EGOEGO_OPTIM_EMA_COPY;  // (the lerp that follows a copy moves nothing)
                    *a.ema.d_initted = 1.0f;
                } else {
                    const double e = (double)(step + 1 - a.ema.update_after_step - 1);
                    double decay = 0.0;
                    if (e > 0.0) {
                        decay = 1.0 - pow(1.0 + e / a.ema.inv_gamma, -a.ema.power);
                        decay = decay < a.ema.min_value ? a.ema.min_value : decay;
                        decay = decay > a.ema.beta ? a.ema.beta : decay;
                    }
                    st.ema_action = EGOEGO_OPTIM_EMA_LERP;
                    st.one_minus_decay = (float)(1.0 - decay);
                }
            }
        }
    }
    *a.st = st;
}

// ---------------------------------------------------------------------------------------------------------------- the update
struct Apply {
    const Tensor* table;
    const Chunk* chunks;
    int n_chunks;
    const egoego_optim_state* st;
    const float* inv_scale;
    float w1, beta2, w2, eps, wd;  // 1 - beta1, beta2, 1 - beta2, eps, weight decay: each rounded once from the caller's doubles
    int zero_grads;
    float wmul;  // decoupled: (float)(1 - lr * weight_decay), formed in double
    int decoupled, clip;
};

struct Scalars {
    float inv, step_size, bc2_sqrt, omd, clip;
    bool adam, zero;
    int action;
};

template <int W>
__device__ __forceinline__ void ldv(const float* p, float (&r)[W]) {
    if constexpr (W == 4) {
        const float4 x = *reinterpret_cast<const float4*>(p);
        r[0] = x.x; r[1] = x.y; r[2] = x.z; r[3] = x.w;
    } else {
        r[0] = *p;
    }
}
template <int W>
__device__ __forceinline__ void stv(float* p, const float (&r)[W]) {
    if constexpr (W == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
        *p = r[0];
    }
}

// W elements at index i of a chunk.  torch.optim.Adam (amsgrad off; weight decay in its L2 form) or, with a.decoupled,
// torch.optim.AdamW (p *= 1 - lr * wd first, no L2 term); then ema-pytorch's update.  With a.clip the unscaled gradient is
// multiplied by clip_coef: a second fp32 product in a statement of its own, in torch's order (unscale, then clip).  The clipped
// value lives in registers only: the gradient in memory keeps its bits (or becomes zero).
template <bool ADAM, bool EMA, int W>
__device__ __forceinline__ void update(const Apply& a, const Scalars& s, float* p, float* g, float* m, float* v, float* e, long i) {
    float P[W];
    if (s.adam || s.action) ldv<W>(p + i, P);
    if constexpr (ADAM) {
        if (s.adam) {
            float G[W], M[W], V[W];
            ldv<W>(g + i, G);
            ldv<W>(m + i, M);
            ldv<W>(v + i, V);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                float gg = G[k] * s.inv;
                if (a.clip) gg = gg * s.clip;
                if (a.decoupled) P[k] = P[k] * a.wmul;
                else if (a.wd != 0.f) gg = gg + a.wd * P[k];
                // torch's lerp_(grad, 1 - beta1): the weight decides the form, and a weight of 1 (beta1 = 0) returns gg itself
                const float dm = gg - M[k];
                M[k] = a.w1 < 0.5f ? M[k] + a.w1 * dm : gg - dm * (1.0f - a.w1);
                const float vb = V[k] * a.beta2;
                const float g2 = a.w2 * gg;
                V[k] = vb + g2 * gg;
                const float denom = sqrtf(V[k]) / s.bc2_sqrt + a.eps;
                const float q = M[k] / denom;
                P[k] = P[k] - s.step_size * q;
            }
            stv<W>(m + i, M);
            stv<W>(v + i, V);
            stv<W>(p + i, P);
        }
        if (s.zero) {
            float Z[W];
#pragma unroll
            for (int k = 0; k < W; ++k) Z[k] = 0.f;
            stv<W>(g + i, Z);
        }
    }
    if constexpr (EMA) {
        if (s.action == EGOEGO_OPTIM_EMA_COPY) {
            stv<W>(e + i, P);
        } else if (s.action == EGOEGO_OPTIM_EMA_LERP) {
            float E[W];
            ldv<W>(e + i, E);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float d = E[k] - P[k];
                E[k] = E[k] - d * s.omd;
            }
            stv<W>(e + i, E);
        }
    }
}

__device__ __forceinline__ int phase16(const float* p) { return (int)(((uintptr_t)p >> 2) & 3); }

template <bool ADAM, bool EMA>
__global__ __launch_bounds__(THREADS) void apply_kernel(Apply a) {
    Scalars s;
    const int skip = a.st->last_skip;
    s.adam = ADAM && !skip;
    s.zero = ADAM && a.zero_grads;
    s.action = (EMA && !skip) ? a.st->ema_action : EGOEGO_OPTIM_EMA_NONE;
    if (!s.adam && !s.zero && !s.action) return;  // a skipped step writes nothing
    s.inv = a.inv_scale ? *a.inv_scale : 1.0f;
    s.step_size = a.st->step_size;
    s.bc2_sqrt = a.st->bc2_sqrt;
    s.omd = a.st->one_minus_decay;
    s.clip = a.st->clip_coef;
    for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const Chunk ch = a.chunks[c];
        const Tensor t = a.table[ch.tensor];
        float* p = t.p + ch.off;
        float* g = ADAM ? t.g + ch.off : nullptr;
        float* m = ADAM ? t.m + ch.off : nullptr;
        float* v = ADAM ? t.v + ch.off : nullptr;
        float* e = EMA ? t.ema + ch.off : nullptr;
        // 16-byte accesses where every tensor this launch touches has the same phase: a scalar head up to the boundary, the
        // vector body, a scalar tail.  Different phases (a view at an odd offset next to an aligned moment): scalars throughout.
        const int ph = phase16(p);
        bool same = true;
        if (ADAM) same = same && phase16(g) == ph && phase16(m) == ph && phase16(v) == ph;
        if (EMA) same = same && phase16(e) == ph;
        const int count = ch.count;
        int head = same ? ((4 - ph) & 3) : count;
        if (head > count) head = count;
        const int nvec = (count - head) >> 2;
        const int tail0 = head + 4 * nvec;
        for (int i = threadIdx.x; i < head; i += THREADS) update<ADAM, EMA, 1>(a, s, p, g, m, v, e, i);
        for (int i = threadIdx.x; i < nvec; i += THREADS) update<ADAM, EMA, 4>(a, s, p, g, m, v, e, head + 4L * i);
        for (int i = tail0 + threadIdx.x; i < count; i += THREADS) update<ADAM, EMA, 1>(a, s, p, g, m, v, e, i);
    }
}

}  // namespace op
