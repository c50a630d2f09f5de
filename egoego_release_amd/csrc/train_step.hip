// train_step.hip — host side of the stage-2 training step (egoego_train_*): the launch sequences of the forward pass with saves,
// the loss, and the backward pass over train_step.h's kernels.  A call only enqueues work on the caller's stream: no allocation,
// no copy through the host and no synchronisation.  The weights are the caller's live fp32 tensors, read in place.
#include "host_util.h"
#include "train_step.h"

struct egoego_train_ctx {
    egoego_config cfg;
    int device;
    DevMem mem;
};

namespace {

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// Byte offsets of the saved tensors of a (B, T) call.  X[l] is the input of layer l, X[n_layers] the decoder output.
struct Saves {
    size_t xin, target, dout, emb, h1, gact, maskR, wids, X0, layer0, per_layer, total;
    size_t qkv, P, O, Z1, Y1, H, Z2;  // inside a layer's block
    size_t Xbytes;
};

Saves saves_map(const egoego_config& c, int B, int T) {
    const size_t L = (size_t)T + 1, R = (size_t)B * L, D = (size_t)c.d_feats, f = sizeof(float);
    Saves s;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    s.xin = take(R * 2 * D * f);
    s.target = take((size_t)B * T * D * f);
    s.dout = take(R * D * f);
    s.emb = take((size_t)B * tr::TE * f);
    s.h1 = take((size_t)B * tr::TH * f);
    s.gact = take((size_t)B * tr::TH * f);
    s.maskR = take(R * f);
    s.wids = take((size_t)B * sizeof(int64_t));
    s.Xbytes = up256(R * tr::DM * f);
    s.X0 = take((size_t)(c.n_dec_layers + 1) * s.Xbytes);
    s.layer0 = o;
    size_t p = 0;
    auto in_layer = [&](size_t bytes) { const size_t at = p; p += up256(bytes); return at; };
    s.qkv = in_layer(R * 3 * tr::HD * f);
    s.P = in_layer((size_t)B * tr::NH * L * L * f);
    s.O = in_layer(R * tr::HD * f);
    s.Z1 = in_layer(R * tr::DM * f);
    s.Y1 = in_layer(R * tr::DM * f);
    s.H = in_layer(R * tr::DM * f);
    s.Z2 = in_layer(R * tr::DM * f);
    s.per_layer = p;
    s.total = o + (size_t)c.n_dec_layers * p;
    return s;
}

// Byte offsets inside the workspace (one layout for both passes).
struct Work {
    size_t outL, F, Pd, winsum;                       // forward
    size_t GA, GB, GF, GH, GO, GQKV, GP, dYs, part, dtok, dh1;  // backward
    size_t total;
};

int n_chunks(size_t R) { return (int)((R + tr::CHUNK - 1) / tr::CHUNK); }
int n_ln_chunks(size_t R) { return (int)((R + tr::LN_ROWS - 1) / tr::LN_ROWS); }

Work work_map(const egoego_config& c, int B, int T) {
    const size_t L = (size_t)T + 1, R = (size_t)B * L, D = (size_t)c.d_feats, f = sizeof(float);
    Work w;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    w.outL = take(R * D * f);
    w.F = take(R * tr::DM * f);
    w.Pd = take((size_t)B * tr::NH * L * L * f);
    w.winsum = take((size_t)B * sizeof(double));
    w.GA = take(R * tr::DM * f);
    w.GB = take(R * tr::DM * f);
    w.GF = take(R * tr::DM * f);
    w.GH = take(R * tr::DM * f);
    w.GO = take(R * tr::HD * f);
    w.GQKV = take(R * 3 * tr::HD * f);
    w.GP = take((size_t)B * tr::NH * L * L * f);
    w.dYs = take(R * D * f);
    const size_t part_w = (size_t)n_chunks(R) * tr::HD * tr::DM;  // the largest weight: [1024][512]
    const size_t part_ln = (size_t)n_ln_chunks(R) * 2 * tr::DM;
    w.part = take((part_w > part_ln ? part_w : part_ln) * f);
    w.dtok = take((size_t)B * tr::DM * f);
    w.dh1 = take((size_t)B * tr::TH * f);
    w.total = o;
    return w;
}

int check_shape(const egoego_train_ctx* c, int B, int T) {
    if (!c) return fail(EGOEGO_E_INVALID, "train context is NULL");
    if (B < 1 || T < 1) return fail(EGOEGO_E_INVALID, "B = %d, T = %d: both must be positive", B, T);
    if (T + 1 > tr::MAX_L || T + 1 > c->cfg.max_timesteps)
        return fail(EGOEGO_E_INVALID, "T + 1 = %d exceeds the longest window (%d, max_timesteps %d)", T + 1, tr::MAX_L, c->cfg.max_timesteps);
    if ((size_t)B * (T + 1) > ((size_t)1 << 20) || B * tr::NH > 65535)
        return fail(EGOEGO_E_INVALID, "B = %d at T = %d: more than 2^20 rows or 16383 windows per call; split the batch", B, T);
    return 0;
}

int check_weights(const egoego_weights* w, int n_layers) {
    if (!w || !w->layers) return fail(EGOEGO_E_INVALID, "weights are NULL");
    const void* top[] = {w->start_conv_w, w->start_conv_b, w->position_vec, w->linear_out_w, w->linear_out_b,
                         w->time_mlp1_w, w->time_mlp1_b, w->time_mlp3_w, w->time_mlp3_b};
    for (const void* p : top)
        if (!p) return fail(EGOEGO_E_INVALID, "a weight pointer is NULL");
    for (int l = 0; l < n_layers; ++l) {
        const egoego_layer_weights& lw = w->layers[l];
        const void* ps[] = {lw.w_q, lw.b_q, lw.w_k, lw.b_k, lw.w_v, lw.b_v, lw.w_fc, lw.b_fc, lw.ln1_g, lw.ln1_b,
                            lw.w_1, lw.b_1, lw.w_2, lw.b_2, lw.ln2_g, lw.ln2_b};
        for (const void* p : ps)
            if (!p) return fail(EGOEGO_E_INVALID, "a weight pointer of layer %d is NULL", l);
    }
    return 0;
}

tr::Drop make_drop(float p, uint64_t seed, const int64_t* wids, int layer, int site) {
    tr::Drop d;
    d.seed = seed;
    d.wids = wids;
    d.layer = layer;
    d.site = site;
    if (p > 0.f) {
        const double thr = (double)p * 4294967296.0;
        d.thr = thr >= 4294967295.0 ? 4294967295u : (uint32_t)thr;
        if (d.thr == 0) d.thr = 1;
        d.scale = 1.0f / (1.0f - p);
    } else {
        d.thr = 0;
        d.scale = 1.0f;
    }
    return d;
}

tr::Gemm gemm_base(int M, int N, int K) {
    tr::Gemm g;
    memset(&g, 0, sizeof g);
    g.M = M; g.N = N; g.K = K;
    g.zdiv = 1;
    g.alpha = 1.0f;
    return g;
}

template <int KIND>
void launch_gemm(hipStream_t s, const tr::Gemm& g, int nz = 1) {
    dim3 grid((g.M + 31) / 32, (g.N + 127) / 128, nz);
    hipLaunchKernelGGL(tr::gemm_kernel<KIND>, grid, dim3(256), 0, s, g);
}

// C[M][N] (ldc) = act(A[M][K] (lda) . W[N][K]^T + bias)
void linear_fwd(hipStream_t s, const float* A, long lda, int M, int K, const float* W, const float* bias, int N, float* C, long ldc,
                int relu = 0, const float* pos = nullptr, int posL = 0) {
    tr::Gemm g = gemm_base(M, N, K);
    g.A = A; g.sai = lda; g.sak = 1;
    g.B = W; g.sbj = K; g.sbk = 1;
    g.C = C; g.ldc = ldc;
    g.bias = bias; g.relu = relu; g.pos = pos; g.posL = posL;
    launch_gemm<tr::GEMM_FWD>(s, g);
}

// dX[M][K] (ldx) (+)= dY[M][N] (ldy) . W[N][K], kept where gate > 0
void linear_bwd_data(hipStream_t s, const float* dY, long ldy, int M, int N, const float* W, int K, float* dX, long ldx, int accum,
                     const float* gate = nullptr) {
    tr::Gemm g = gemm_base(M, K, N);
    g.A = dY; g.sai = ldy; g.sak = 1;
    g.B = W; g.sbj = 1; g.sbk = K;
    g.C = dX; g.ldc = ldx;
    g.accum = accum; g.gate = gate;
    launch_gemm<tr::GEMM_DGRAD>(s, g);
}

template <typename T>
void fold(hipStream_t s, const T* part, long stride, int nch, long n, float* out) {
    hipLaunchKernelGGL(tr::fold_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, stride, nch, n, out);
}

// dW[N][K] = dY[R][N]^T (ldy) . X[R][K] (ldx) and db[N] = column sums of dY, both over the rows in fixed chunks, folded in order
void linear_bwd_weight(hipStream_t s, const float* dY, long ldy, int R, int N, const float* X, long ldx, int K, float* part, float* dW,
                       float* db, int skipL = 0) {
    const int nch = n_chunks(R);
    tr::Gemm g = gemm_base(N, K, R);
    g.A = dY; g.sai = 1; g.sak = ldy;
    g.B = X; g.sbj = 1; g.sbk = ldx;
    g.C = part; g.ldc = K; g.bsC0 = (long)N * K;
    g.kchunk = tr::CHUNK;
    launch_gemm<tr::GEMM_WGRAD>(s, g, nch);
    fold(s, (const float*)part, (long)N * K, nch, (long)N * K, dW);
    const int ncol = (R + tr::COL_ROWS - 1) / tr::COL_ROWS;  // (R / 64 * N doubles: far inside the weight partials' buffer)
    hipLaunchKernelGGL(tr::colsum_kernel, dim3((N + 255) / 256, ncol), dim3(256), 0, s, dY, ldy, R, N, skipL, (double*)part);
    fold(s, (const double*)part, N, ncol, N, db);
}

}  // namespace

extern "C" {

const char* egoego_train_last_error(void) { return last_err.c_str(); }

int egoego_train_ctx_create(const egoego_config* cfg, int device, egoego_train_ctx** out) {
    if (!cfg || !out) return fail(EGOEGO_E_INVALID, "cfg / out is NULL");
    if (cfg->d_model != tr::DM || cfg->n_head != tr::NH || cfg->d_k != tr::DK || cfg->d_v != tr::DK)
        return fail(EGOEGO_E_INVALID, "the training step serves d_model 512, 4 heads, d_k = d_v = 256 only");
    if (cfg->d_feats < 1 || cfg->d_feats > 512 || cfg->n_dec_layers < 1 || cfg->n_dec_layers > 16 || cfg->num_timesteps < 1 ||
        cfg->max_timesteps < 2)
        return fail(EGOEGO_E_INVALID, "d_feats %d, n_dec_layers %d, num_timesteps %d, max_timesteps %d: not supported", cfg->d_feats,
                    cfg->n_dec_layers, cfg->num_timesteps, cfg->max_timesteps);
    if (int rc = check_device(device)) return rc;
    egoego_train_ctx* c = new egoego_train_ctx();
    c->cfg = *cfg;
    c->device = device;
    *out = c;
    return 0;
}

void egoego_train_ctx_destroy(egoego_train_ctx* ctx) { destroy_ctx(ctx); }

size_t egoego_train_workspace_bytes(const egoego_train_ctx* ctx, int B, int T) {
    if (check_shape(ctx, B, T)) return 0;
    return work_map(ctx->cfg, B, T).total;
}

size_t egoego_train_saves_bytes(const egoego_train_ctx* ctx, int B, int T) {
    if (check_shape(ctx, B, T)) return 0;
    return saves_map(ctx->cfg, B, T).total;
}

int egoego_train_forward(egoego_train_ctx* ctx, const egoego_weights* w, const float* d_x_start, const float* d_noise,
                         const float* d_cond_noise, const float* d_cond_mask, const int64_t* d_t, const float* d_row_mask,
                         const float* d_sqrt_alphas_cumprod, const float* d_sqrt_one_minus_alphas_cumprod, const float* d_p2_loss_weight,
                         int objective, int loss_type, float p_drop, uint64_t dropout_seed, const int64_t* d_window_ids, int B, int T,
                         void* d_saves, size_t saves_bytes, void* d_workspace, size_t workspace_bytes, float* d_loss, float* d_model_out,
                         void* stream) {
    if (int rc = check_shape(ctx, B, T)) return rc;
    const egoego_config& c = ctx->cfg;
    if (int rc = check_weights(w, c.n_dec_layers)) return rc;
    if (!d_x_start || !d_noise || !d_cond_noise || !d_cond_mask || !d_t || !d_sqrt_alphas_cumprod || !d_sqrt_one_minus_alphas_cumprod ||
        !d_p2_loss_weight || !d_loss)
        return fail(EGOEGO_E_INVALID, "an input pointer is NULL");
    if (objective != EGOEGO_PRED_NOISE && objective != EGOEGO_PRED_X0) return fail(EGOEGO_E_INVALID, "unknown objective %d", objective);
    if (loss_type != EGOEGO_LOSS_L1 && loss_type != EGOEGO_LOSS_L2) return fail(EGOEGO_E_INVALID, "unknown loss type %d", loss_type);
    if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(EGOEGO_E_INVALID, "p_drop %g outside [0, 1)", (double)p_drop);
    const Saves sm = saves_map(c, B, T);
    const Work wm = work_map(c, B, T);
    if (int rc = check_workspace(d_workspace, workspace_bytes, wm.total)) return rc;
    if (!d_saves || ((uintptr_t)d_saves & 255) || saves_bytes < sm.total)
        return fail(EGOEGO_E_WORKSPACE, "saves: %zu bytes at %p, need %zu (256-byte aligned)", saves_bytes, d_saves, sm.total);
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    hipStream_t s = as_stream(stream);
    char* sv = (char*)d_saves;
    char* ws = (char*)d_workspace;
    const int L = T + 1, R = B * L, D = c.d_feats, NL = c.n_dec_layers;
    auto SF = [&](size_t off) { return (float*)(sv + off); };
    auto WF = [&](size_t off) { return (float*)(ws + off); };
    const int64_t* wids = (const int64_t*)(sv + sm.wids);
    float* maskR = SF(sm.maskR);

    {
        tr::Prep p;
        p.x_start = d_x_start; p.noise = d_noise; p.cond_noise = d_cond_noise; p.cond_mask = d_cond_mask;
        p.t = d_t; p.row_mask = d_row_mask; p.sqrt_ac = d_sqrt_alphas_cumprod; p.sqrt_1mac = d_sqrt_one_minus_alphas_cumprod;
        p.wids = d_window_ids;
        p.xin = SF(sm.xin); p.target = SF(sm.target); p.maskR = maskR; p.wids_out = (int64_t*)(sv + sm.wids);
        p.B = B; p.T = T; p.D = D; p.S = c.num_timesteps; p.pred_x0 = objective == EGOEGO_PRED_X0;
        const long n = (long)R * D;
        hipLaunchKernelGGL(tr::prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    }
    float* X = SF(sm.X0);
    // embed: every row gets start_conv(xin) + bias + position; the time token's rows are then overwritten
    linear_fwd(s, SF(sm.xin), 2 * D, R, 2 * D, w->start_conv_w, w->start_conv_b, tr::DM, X, tr::DM, 0, w->position_vec, L);
    {
        tr::TimeFwd a;
        a.t = d_t; a.w1 = w->time_mlp1_w; a.b1 = w->time_mlp1_b; a.w3 = w->time_mlp3_w; a.b3 = w->time_mlp3_b; a.pos = w->position_vec;
        a.emb = SF(sm.emb); a.h1 = SF(sm.h1); a.gact = SF(sm.gact); a.X = X; a.L = L; a.S = c.num_timesteps;
        hipLaunchKernelGGL(tr::time_fwd_kernel, dim3(B), dim3(256), 0, s, a);
    }
    const size_t PP = (size_t)L * L;  // one (window, head) block of probabilities
    for (int l = 0; l < NL; ++l) {
        const egoego_layer_weights& lw = w->layers[l];
        char* lb = sv + sm.layer0 + (size_t)l * sm.per_layer;
        float* qkv = (float*)(lb + sm.qkv);
        float* P = (float*)(lb + sm.P);
        float* O = (float*)(lb + sm.O);
        float* Xn = (float*)(sv + sm.X0 + (size_t)(l + 1) * sm.Xbytes);
        linear_fwd(s, X, tr::DM, R, tr::DM, lw.w_q, lw.b_q, tr::HD, qkv, 3 * tr::HD);
        linear_fwd(s, X, tr::DM, R, tr::DM, lw.w_k, lw.b_k, tr::HD, qkv + tr::HD, 3 * tr::HD);
        linear_fwd(s, X, tr::DM, R, tr::DM, lw.w_v, lw.b_v, tr::HD, qkv + 2 * tr::HD, 3 * tr::HD);
        {   // S = Q K^T / 16 per (window, head), over all L keys
            tr::Gemm g = gemm_base(L, L, tr::DK);
            g.zdiv = tr::NH;
            g.A = qkv; g.sai = 3 * tr::HD; g.sak = 1; g.bsA0 = (long)L * 3 * tr::HD; g.bsA1 = tr::DK;
            g.B = qkv + tr::HD; g.sbj = 3 * tr::HD; g.sbk = 1; g.bsB0 = g.bsA0; g.bsB1 = tr::DK;
            g.C = P; g.ldc = L; g.bsC0 = (long)tr::NH * PP; g.bsC1 = (long)PP;
            g.alpha = 0.0625f;
            launch_gemm<tr::GEMM_ATTN>(s, g, B * tr::NH);
        }
        const float* Pd = P;
        {
            tr::Softmax a;
            a.S = P; a.Pd = p_drop > 0.f ? WF(wm.Pd) : nullptr; a.L = L; a.rows = B * tr::NH * L;
            a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_ATTN);
            hipLaunchKernelGGL(tr::softmax_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
            if (a.Pd) Pd = a.Pd;
        }
        {   // O = dropout(P) V
            tr::Gemm g = gemm_base(L, tr::DK, L);
            g.zdiv = tr::NH;
            g.A = Pd; g.sai = L; g.sak = 1; g.bsA0 = (long)tr::NH * PP; g.bsA1 = (long)PP;
            g.B = qkv + 2 * tr::HD; g.sbj = 1; g.sbk = 3 * tr::HD; g.bsB0 = (long)L * 3 * tr::HD; g.bsB1 = tr::DK;
            g.C = O; g.ldc = tr::HD; g.bsC0 = (long)L * tr::HD; g.bsC1 = tr::DK;
            launch_gemm<tr::GEMM_ATTN>(s, g, B * tr::NH);
        }
        linear_fwd(s, O, tr::HD, R, tr::HD, lw.w_fc, lw.b_fc, tr::DM, WF(wm.F), tr::DM);
        {
            tr::LnFwd a;
            a.Y = WF(wm.F); a.resid = X; a.Z = (float*)(lb + sm.Z1); a.out = (float*)(lb + sm.Y1);
            a.g = lw.ln1_g; a.b = lw.ln1_b; a.mask = maskR; a.R = R; a.L = L;
            a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_FC);
            hipLaunchKernelGGL(tr::ln_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, s, a);
        }
        linear_fwd(s, (float*)(lb + sm.Y1), tr::DM, R, tr::DM, lw.w_1, lw.b_1, tr::DM, (float*)(lb + sm.H), tr::DM, 1);
        linear_fwd(s, (float*)(lb + sm.H), tr::DM, R, tr::DM, lw.w_2, lw.b_2, tr::DM, WF(wm.F), tr::DM);
        {
            tr::LnFwd a;
            a.Y = WF(wm.F); a.resid = (float*)(lb + sm.Y1); a.Z = (float*)(lb + sm.Z2); a.out = Xn;
            a.g = lw.ln2_g; a.b = lw.ln2_b; a.mask = maskR; a.R = R; a.L = L;
            a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_FFN);
            hipLaunchKernelGGL(tr::ln_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, s, a);
        }
        X = Xn;
    }
    // linear_out on every row (the time token's result is never read)
    linear_fwd(s, X, tr::DM, R, tr::DM, w->linear_out_w, w->linear_out_b, D, WF(wm.outL), D);
    {
        tr::Loss a;
        a.outL = WF(wm.outL); a.target = SF(sm.target); a.maskR = maskR; a.p2w = d_p2_loss_weight; a.t = d_t;
        a.model_out = d_model_out; a.dout = SF(sm.dout); a.winsum = (double*)(ws + wm.winsum);
        a.B = B; a.T = T; a.D = D; a.S = c.num_timesteps; a.l2 = loss_type == EGOEGO_LOSS_L2;
        hipLaunchKernelGGL(tr::loss_window_kernel, dim3(B), dim3(256), 0, s, a);
        hipLaunchKernelGGL(tr::loss_final_kernel, dim3(1), dim3(64), 0, s, (const double*)a.winsum, d_t, d_p2_loss_weight, B, T, D,
                           c.num_timesteps, d_loss);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_train_backward(egoego_train_ctx* ctx, const egoego_weights* w, const void* d_saves, size_t saves_bytes,
                          const float* d_upstream, const egoego_train_grads* grads, float p_drop, uint64_t dropout_seed, int B, int T,
                          void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_shape(ctx, B, T)) return rc;
    const egoego_config& c = ctx->cfg;
    if (int rc = check_weights(w, c.n_dec_layers)) return rc;
    if (!d_upstream || !grads || !grads->layers) return fail(EGOEGO_E_INVALID, "the upstream gradient / the gradient buffers are NULL");
    {
        float* top[] = {grads->start_conv_w, grads->start_conv_b, grads->linear_out_w, grads->linear_out_b, grads->time_mlp1_w,
                        grads->time_mlp1_b, grads->time_mlp3_w, grads->time_mlp3_b};
        for (float* p : top)
            if (!p) return fail(EGOEGO_E_INVALID, "a gradient buffer is NULL");
        for (int l = 0; l < c.n_dec_layers; ++l) {
            const egoego_train_layer_grads& g = grads->layers[l];
            float* ps[] = {g.w_q, g.b_q, g.w_k, g.b_k, g.w_v, g.b_v, g.w_fc, g.b_fc, g.ln1_g, g.ln1_b, g.w_1, g.b_1, g.w_2, g.b_2, g.ln2_g, g.ln2_b};
            for (float* p : ps)
                if (!p) return fail(EGOEGO_E_INVALID, "a gradient buffer of layer %d is NULL", l);
        }
    }
    if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(EGOEGO_E_INVALID, "p_drop %g outside [0, 1)", (double)p_drop);
    const Saves sm = saves_map(c, B, T);
    const Work wm = work_map(c, B, T);
    if (int rc = check_workspace(d_workspace, workspace_bytes, wm.total)) return rc;
    if (!d_saves || ((uintptr_t)d_saves & 255) || saves_bytes < sm.total)
        return fail(EGOEGO_E_WORKSPACE, "saves: %zu bytes at %p, need %zu (256-byte aligned)", saves_bytes, d_saves, sm.total);
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    hipStream_t s = as_stream(stream);
    const char* sv = (const char*)d_saves;
    char* ws = (char*)d_workspace;
    const int L = T + 1, R = B * L, D = c.d_feats, NL = c.n_dec_layers;
    auto SF = [&](size_t off) { return (const float*)(sv + off); };
    auto WF = [&](size_t off) { return (float*)(ws + off); };
    const int64_t* wids = (const int64_t*)(sv + sm.wids);
    const float* maskR = SF(sm.maskR);
    float *GA = WF(wm.GA), *GB = WF(wm.GB), *GF = WF(wm.GF), *GH = WF(wm.GH), *GO = WF(wm.GO), *GQKV = WF(wm.GQKV), *GP = WF(wm.GP);
    float *dYs = WF(wm.dYs), *part = WF(wm.part);
    const size_t PP = (size_t)L * L;
    const int nln = n_ln_chunks(R);

    // d(loss)/d(out) times the upstream gradient (a power of two scales every gradient exactly)
    {
        const long n = (long)R * D;
        hipLaunchKernelGGL(tr::scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, SF(sm.dout), d_upstream, n, dYs);
    }
    const float* Xf = (const float*)(sv + sm.X0 + (size_t)NL * sm.Xbytes);
    linear_bwd_weight(s, dYs, D, R, D, Xf, tr::DM, tr::DM, part, grads->linear_out_w, grads->linear_out_b);
    linear_bwd_data(s, dYs, D, R, D, w->linear_out_w, tr::DM, GA, tr::DM, 0);

    for (int l = NL - 1; l >= 0; --l) {
        const egoego_layer_weights& lw = w->layers[l];
        const egoego_train_layer_grads& lg = grads->layers[l];
        const char* lb = sv + sm.layer0 + (size_t)l * sm.per_layer;
        const float* qkv = (const float*)(lb + sm.qkv);
        const float* P = (const float*)(lb + sm.P);
        const float* O = (const float*)(lb + sm.O);
        const float* Y1 = (const float*)(lb + sm.Y1);
        const float* H = (const float*)(lb + sm.H);
        const float* Xl = (const float*)(sv + sm.X0 + (size_t)l * sm.Xbytes);
        {   // LayerNorm 2: GA = d(layer out) -> GB = d z2 (the residual's share, to Y1), GF = d(FFN out)
            tr::LnBwd a;
            a.dOut = GA; a.Z = (const float*)(lb + sm.Z2); a.g = lw.ln2_g; a.mask = maskR; a.dZ = GB; a.dY = GF; a.part = part;
            a.R = R; a.L = L; a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_FFN);
            hipLaunchKernelGGL(tr::ln_bwd_kernel, dim3((nln + 3) / 4), dim3(256), 0, s, a);
            fold(s, (const float*)part, 2 * tr::DM, nln, tr::DM, lg.ln2_g);
            fold(s, (const float*)(part + tr::DM), 2 * tr::DM, nln, tr::DM, lg.ln2_b);
        }
        linear_bwd_weight(s, GF, tr::DM, R, tr::DM, H, tr::DM, tr::DM, part, lg.w_2, lg.b_2);
        linear_bwd_data(s, GF, tr::DM, R, tr::DM, lw.w_2, tr::DM, GH, tr::DM, 0, H);  // through the ReLU: kept where H > 0
        linear_bwd_weight(s, GH, tr::DM, R, tr::DM, Y1, tr::DM, tr::DM, part, lg.w_1, lg.b_1);
        linear_bwd_data(s, GH, tr::DM, R, tr::DM, lw.w_1, tr::DM, GB, tr::DM, 1);
        {   // LayerNorm 1: GB = d Y1 -> GA = d z1 (the residual's share, to X), GF = d(fc out)
            tr::LnBwd a;
            a.dOut = GB; a.Z = (const float*)(lb + sm.Z1); a.g = lw.ln1_g; a.mask = maskR; a.dZ = GA; a.dY = GF; a.part = part;
            a.R = R; a.L = L; a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_FC);
            hipLaunchKernelGGL(tr::ln_bwd_kernel, dim3((nln + 3) / 4), dim3(256), 0, s, a);
            fold(s, (const float*)part, 2 * tr::DM, nln, tr::DM, lg.ln1_g);
            fold(s, (const float*)(part + tr::DM), 2 * tr::DM, nln, tr::DM, lg.ln1_b);
        }
        linear_bwd_weight(s, GF, tr::DM, R, tr::DM, O, tr::HD, tr::HD, part, lg.w_fc, lg.b_fc);
        linear_bwd_data(s, GF, tr::DM, R, tr::DM, lw.w_fc, tr::HD, GO, tr::HD, 0);
        // attention backward per (window, head); one wave sums over all keys / queries of its tile: no sum across workgroups
        const tr::Drop da = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_ATTN);
        const float* Pd = P;
        if (da.thr) {
            const long n = (long)B * tr::NH * (long)PP;
            hipLaunchKernelGGL(tr::redrop_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, WF(wm.Pd), L, n, da);
            Pd = WF(wm.Pd);
        }
        {   // dV = Pd^T dO
            tr::Gemm g = gemm_base(L, tr::DK, L);
            g.zdiv = tr::NH;
            g.A = Pd; g.sai = 1; g.sak = L; g.bsA0 = (long)tr::NH * PP; g.bsA1 = (long)PP;
            g.B = GO; g.sbj = 1; g.sbk = tr::HD; g.bsB0 = (long)L * tr::HD; g.bsB1 = tr::DK;
            g.C = GQKV + 2 * tr::HD; g.ldc = 3 * tr::HD; g.bsC0 = (long)L * 3 * tr::HD; g.bsC1 = tr::DK;
            launch_gemm<tr::GEMM_ATTN>(s, g, B * tr::NH);
        }
        {   // dPd = dO V^T
            tr::Gemm g = gemm_base(L, L, tr::DK);
            g.zdiv = tr::NH;
            g.A = GO; g.sai = tr::HD; g.sak = 1; g.bsA0 = (long)L * tr::HD; g.bsA1 = tr::DK;
            g.B = qkv + 2 * tr::HD; g.sbj = 3 * tr::HD; g.sbk = 1; g.bsB0 = (long)L * 3 * tr::HD; g.bsB1 = tr::DK;
            g.C = GP; g.ldc = L; g.bsC0 = (long)tr::NH * PP; g.bsC1 = (long)PP;
            launch_gemm<tr::GEMM_ATTN>(s, g, B * tr::NH);
        }
        {
            tr::SoftmaxBwd a;
            a.dP = GP; a.P = P; a.L = L; a.rows = B * tr::NH * L; a.d = da;
            hipLaunchKernelGGL(tr::softmax_bwd_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
        }
        {   // dQ = dS K
            tr::Gemm g = gemm_base(L, tr::DK, L);
            g.zdiv = tr::NH;
            g.A = GP; g.sai = L; g.sak = 1; g.bsA0 = (long)tr::NH * PP; g.bsA1 = (long)PP;
            g.B = qkv + tr::HD; g.sbj = 1; g.sbk = 3 * tr::HD; g.bsB0 = (long)L * 3 * tr::HD; g.bsB1 = tr::DK;
            g.C = GQKV; g.ldc = 3 * tr::HD; g.bsC0 = (long)L * 3 * tr::HD; g.bsC1 = tr::DK;
            launch_gemm<tr::GEMM_ATTN>(s, g, B * tr::NH);
        }
        {   // dK = dS^T Q
            tr::Gemm g = gemm_base(L, tr::DK, L);
            g.zdiv = tr::NH;
            g.A = GP; g.sai = 1; g.sak = L; g.bsA0 = (long)tr::NH * PP; g.bsA1 = (long)PP;
            g.B = qkv; g.sbj = 1; g.sbk = 3 * tr::HD; g.bsB0 = (long)L * 3 * tr::HD; g.bsB1 = tr::DK;
            g.C = GQKV + tr::HD; g.ldc = 3 * tr::HD; g.bsC0 = (long)L * 3 * tr::HD; g.bsC1 = tr::DK;
            launch_gemm<tr::GEMM_ATTN>(s, g, B * tr::NH);
        }
        const float* pw[3] = {lw.w_q, lw.w_k, lw.w_v};
        float* gw[3] = {lg.w_q, lg.w_k, lg.w_v};
        float* gb[3] = {lg.b_q, lg.b_k, lg.b_v};
        for (int k = 0; k < 3; ++k) {
            linear_bwd_weight(s, GQKV + k * tr::HD, 3 * tr::HD, R, tr::HD, Xl, tr::DM, tr::DM, part, gw[k], gb[k]);
            linear_bwd_data(s, GQKV + k * tr::HD, 3 * tr::HD, R, tr::HD, pw[k], tr::DM, GA, tr::DM, 1);
        }
        // GA = d(layer input)
    }
    // the time MLP (from the time token's rows of d X0), then start_conv (its bias sum leaves those rows out; xin is zero there)
    hipLaunchKernelGGL(tr::time_bwd_hidden_kernel, dim3(B), dim3(256), 0, s, (const float*)GA, L, w->time_mlp3_w, SF(sm.h1), WF(wm.dtok),
                       WF(wm.dh1));
    hipLaunchKernelGGL(tr::outer_sum_kernel, dim3((tr::DM * tr::TH + 255) / 256), dim3(256), 0, s, (const float*)WF(wm.dtok), SF(sm.gact), B,
                       tr::DM, tr::TH, grads->time_mlp3_w, grads->time_mlp3_b);
    hipLaunchKernelGGL(tr::outer_sum_kernel, dim3((tr::TH * tr::TE + 255) / 256), dim3(256), 0, s, (const float*)WF(wm.dh1), SF(sm.emb), B,
                       tr::TH, tr::TE, grads->time_mlp1_w, grads->time_mlp1_b);
    linear_bwd_weight(s, GA, tr::DM, R, tr::DM, SF(sm.xin), 2 * D, 2 * D, part, grads->start_conv_w, grads->start_conv_b, L);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_train_dropout_mask(egoego_train_ctx* ctx, float p_drop, uint64_t dropout_seed, int layer, int site, const int64_t* d_window_ids,
                              int B, int T, uint8_t* d_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_shape(ctx, B, T)) return rc;
    if (!d_out) return fail(EGOEGO_E_INVALID, "d_out is NULL");
    if (site < 0 || site > 2 || layer < 0 || layer >= ctx->cfg.n_dec_layers) return fail(EGOEGO_E_INVALID, "layer %d / site %d out of range", layer, site);
    if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(EGOEGO_E_INVALID, "p_drop %g outside [0, 1)", (double)p_drop);
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    hipStream_t s = as_stream(stream);
    const int64_t* wids = d_window_ids;
    if (!wids) {  // window b draws the stream of id b
        if (int rc = check_workspace(d_workspace, workspace_bytes, (size_t)B * sizeof(int64_t))) return rc;
        hipLaunchKernelGGL(tr::iota_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (int64_t*)d_workspace, B);
        wids = (const int64_t*)d_workspace;
    }
    const long L = T + 1;
    const long per = site == tr::SITE_ATTN ? (long)tr::NH * L * L : L * tr::DM;
    const long n = per * B;
    const tr::Drop d = make_drop(p_drop, dropout_seed, wids, layer, site);
    hipLaunchKernelGGL(tr::drop_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, per, n, d_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_train_saved(egoego_train_ctx* ctx, const void* d_saves, size_t saves_bytes, int B, int T, int layer, int which, float* d_out,
                       void* stream) {
    if (int rc = check_shape(ctx, B, T)) return rc;
    if (!d_out) return fail(EGOEGO_E_INVALID, "d_out is NULL");
    const egoego_config& c = ctx->cfg;
    if (layer < 0 || layer >= c.n_dec_layers) return fail(EGOEGO_E_INVALID, "layer %d out of range", layer);
    const Saves sm = saves_map(c, B, T);
    if (!d_saves || saves_bytes < sm.total) return fail(EGOEGO_E_WORKSPACE, "saves: %zu bytes, need %zu", saves_bytes, sm.total);
    const size_t L = (size_t)T + 1, R = (size_t)B * L, f = sizeof(float);
    const char* lb = (const char*)d_saves + sm.layer0 + (size_t)layer * sm.per_layer;
    const char* src;
    size_t bytes;
    switch (which) {
        case EGOEGO_TRAIN_SAVED_FFN_HIDDEN: src = lb + sm.H; bytes = R * tr::DM * f; break;
        case EGOEGO_TRAIN_SAVED_ATTN_PROB: src = lb + sm.P; bytes = (size_t)B * tr::NH * L * L * f; break;
        case EGOEGO_TRAIN_SAVED_ATTN_OUT: src = lb + sm.O; bytes = R * tr::HD * f; break;
        case EGOEGO_TRAIN_SAVED_ATTN_LN: src = lb + sm.Y1; bytes = R * tr::DM * f; break;
        case EGOEGO_TRAIN_SAVED_LAYER_OUT: src = (const char*)d_saves + sm.X0 + (size_t)(layer + 1) * sm.Xbytes; bytes = R * tr::DM * f; break;
        case EGOEGO_TRAIN_SAVED_LAYER_IN: src = (const char*)d_saves + sm.X0 + (size_t)layer * sm.Xbytes; bytes = R * tr::DM * f; break;
        default: return fail(EGOEGO_E_INVALID, "unknown saved tensor %d", which);
    }
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    HIP_TRY(hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return 0;
}

}  // extern "C"
