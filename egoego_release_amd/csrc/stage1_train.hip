// stage1_train.hip — host side of stage-1 training (egoego_s1_train_*, egoego_s1_headnet_loss): launch sequences over
// stage1_train.h's and train_step.h's kernels.  A call only enqueues work on the caller's stream: no allocation, no copy through
// the host and no synchronisation.
#include "host_util.h"
#include "stage1_train.h"

using s1t::tr::DK;
using s1t::tr::HD;
using s1t::tr::NH;
static constexpr int DM = s1t::DM;
namespace tr = s1t::tr;

// One MLP head: Linear dims[0] -> dims[1] -> ... -> dims[n], ReLU behind all but the last; its result goes to column `col` of the output.
struct HeadDesc {
    int n, dims[5], col, w0;  // w0: index of its first Linear in egoego_s1_weights.head_w
};

struct egoego_s1_train_ctx {
    egoego_s1_config cfg;
    int device;
    DevMem mem;
    int n_heads, out_stride;
    HeadDesc heads[2];
};

namespace {

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
int n_chunks(size_t R) { return (int)((R + tr::CHUNK - 1) / tr::CHUNK); }
int n_ln_chunks(size_t R) { return (int)((R + tr::LN_ROWS - 1) / tr::LN_ROWS); }
bool is_headnet(const egoego_s1_train_ctx* c) { return c->cfg.kind == EGOEGO_S1_HEADNET; }
// rows the heads run on: every token (HeadNet) or token 0 of every window (GravityNet)
size_t head_rows(const egoego_s1_train_ctx* c, int W) { return is_headnet(c) ? (size_t)W * c->cfg.window : (size_t)W; }

// Byte offsets of the saved tensors of a call of W windows.  X[l] is the input of layer l, X[n_layers] the decoder output.
struct Saves {
    size_t xin, maskR, wids, X0, Xbytes, layer0, per_layer, total;
    size_t qkv, P, O, Z1, Y1, H, Z2;  // inside a layer's block
    size_t hid[2][4];                 // hid[h][j]: the output of Linear j (1-based) of head h, j = 1 .. n - 1
};

Saves saves_map(const egoego_s1_train_ctx* c, int W) {
    const size_t L = (size_t)c->cfg.window, R = (size_t)W * L, D = (size_t)c->cfg.d_feats, f = sizeof(float);
    Saves s;
    memset(&s, 0, sizeof s);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    s.xin = take(R * D * f);
    s.maskR = take(R * f);
    s.wids = take((size_t)W * sizeof(int64_t));
    s.Xbytes = up256(R * DM * f);
    s.X0 = take((size_t)(c->cfg.n_dec_layers + 1) * s.Xbytes);
    const size_t Rh = head_rows(c, W);
    for (int h = 0; h < c->n_heads; ++h)
        for (int j = 1; j < c->heads[h].n; ++j) s.hid[h][j] = take(Rh * c->heads[h].dims[j] * f);
    s.layer0 = o;
    size_t p = 0;
    auto in_layer = [&](size_t bytes) { const size_t at = p; p += up256(bytes); return at; };
    s.qkv = in_layer(R * 3 * HD * f);
    s.P = in_layer((size_t)W * NH * L * L * f);
    s.O = in_layer(R * HD * f);
    s.Z1 = in_layer(R * DM * f);
    s.Y1 = in_layer(R * DM * f);
    s.H = in_layer(R * DM * f);
    s.Z2 = in_layer(R * DM * f);
    s.per_layer = p;
    s.total = o + (size_t)c->cfg.n_dec_layers * p;
    return s;
}

// Byte offsets inside the workspace (one layout for both passes).
struct Work {
    size_t F, Pd;                                              // forward
    size_t GA, GB, GF, GH, GO, GQKV, GP, part, HG0, HG1;       // backward
    size_t total;
};

Work work_map(const egoego_s1_train_ctx* c, int W) {
    const size_t L = (size_t)c->cfg.window, R = (size_t)W * L, f = sizeof(float);
    Work w;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    w.F = take(R * DM * f);
    w.Pd = take((size_t)W * NH * L * L * f);
    w.GA = take(R * DM * f);
    w.GB = take(R * DM * f);
    w.GF = take(R * DM * f);
    w.GH = take(R * DM * f);
    w.GO = take(R * HD * f);
    w.GQKV = take(R * 3 * HD * f);
    w.GP = take((size_t)W * NH * L * L * f);
    const size_t part_w = (size_t)n_chunks(R) * 1024 * 512;  // the largest weight: a head's [512][1024]
    const size_t part_ln = (size_t)n_ln_chunks(R) * 2 * DM;
    w.part = take((part_w > part_ln ? part_w : part_ln) * f);
    const size_t Rh = head_rows(c, W);
    w.HG0 = take(Rh * 1024 * f);
    w.HG1 = take(Rh * 1024 * f);
    w.total = o;
    return w;
}

int check_shape(const egoego_s1_train_ctx* c, int W) {
    if (!c) return fail(EGOEGO_E_INVALID, "stage-1 training context is NULL");
    if (W < 1) return fail(EGOEGO_E_INVALID, "n_windows = %d: must be positive", W);
    if ((size_t)W * c->cfg.window > ((size_t)1 << 20) || W * NH > 65535)
        return fail(EGOEGO_E_INVALID, "n_windows = %d at window %d: more than 2^20 rows or 16383 windows per call; split the batch", W,
                    c->cfg.window);
    return 0;
}

int n_head_linears(const egoego_s1_train_ctx* c) {
    int n = 0;
    for (int h = 0; h < c->n_heads; ++h) n += c->heads[h].n;
    return n;
}

int check_weights(const egoego_s1_train_ctx* c, const egoego_s1_weights* w) {
    if (!w || !w->layers) return fail(EGOEGO_E_INVALID, "weights are NULL");
    if (!w->start_conv_w || !w->start_conv_b || !w->position_vec) return fail(EGOEGO_E_INVALID, "a weight pointer is NULL");
    for (int l = 0; l < c->cfg.n_dec_layers; ++l) {
        const egoego_layer_weights& lw = w->layers[l];
        const void* ps[] = {lw.w_q, lw.b_q, lw.w_k, lw.b_k, lw.w_v, lw.b_v, lw.w_fc, lw.b_fc, lw.ln1_g, lw.ln1_b,
                            lw.w_1, lw.b_1, lw.w_2, lw.b_2, lw.ln2_g, lw.ln2_b};
        for (const void* p : ps)
            if (!p) return fail(EGOEGO_E_INVALID, "a weight pointer of layer %d is NULL", l);
    }
    for (int j = 0; j < n_head_linears(c); ++j)
        if (!w->head_w[j] || !w->head_b[j]) return fail(EGOEGO_E_INVALID, "a weight pointer of the heads is NULL");
    return 0;
}

int check_saves(const void* d_saves, size_t saves_bytes, size_t need) {
    if (!d_saves || ((uintptr_t)d_saves & 255) || saves_bytes < need)
        return fail(EGOEGO_E_WORKSPACE, "saves: %zu bytes at %p, need %zu (256-byte aligned)", saves_bytes, d_saves, need);
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
                       float* db) {
    const int nch = n_chunks(R);
    tr::Gemm g = gemm_base(N, K, R);
    g.A = dY; g.sai = 1; g.sak = ldy;
    g.B = X; g.sbj = 1; g.sbk = ldx;
    g.C = part; g.ldc = K; g.bsC0 = (long)N * K;
    g.kchunk = tr::CHUNK;
    launch_gemm<tr::GEMM_WGRAD>(s, g, nch);
    fold(s, (const float*)part, (long)N * K, nch, (long)N * K, dW);
    const int ncol = (R + tr::COL_ROWS - 1) / tr::COL_ROWS;  // (R / 64 * N doubles: far inside the weight partials' buffer)
    hipLaunchKernelGGL(tr::colsum_kernel, dim3((N + 255) / 256, ncol), dim3(256), 0, s, dY, ldy, R, N, 0, (double*)part);
    fold(s, (const double*)part, N, ncol, N, db);
}

}  // namespace

extern "C" {

const char* egoego_s1_train_last_error(void) { return last_err.c_str(); }

int egoego_s1_train_ctx_create(const egoego_s1_config* cfg, int device, egoego_s1_train_ctx** out) {
    if (!cfg || !out) return fail(EGOEGO_E_INVALID, "cfg / out is NULL");
    if (cfg->kind != EGOEGO_S1_HEADNET && cfg->kind != EGOEGO_S1_GRAVITYNET) return fail(EGOEGO_E_INVALID, "unknown kind %d", cfg->kind);
    if (cfg->d_model != DM || cfg->n_head != NH || cfg->d_k != DK || cfg->d_v != DK)
        return fail(EGOEGO_E_INVALID, "stage-1 training serves d_model 256, 4 heads, d_k = d_v = 256 only");
    if (cfg->d_feats < 1 || cfg->d_feats > 1024 || cfg->n_dec_layers < 1 || cfg->n_dec_layers > 8 || cfg->window < 1 ||
        cfg->window > s1t::MAX_WINDOW)
        return fail(EGOEGO_E_INVALID, "d_feats %d, n_dec_layers %d, window %d: not supported", cfg->d_feats, cfg->n_dec_layers, cfg->window);
    if (int rc = check_device(device)) return rc;
    egoego_s1_train_ctx* c = new egoego_s1_train_ctx();
    c->cfg = *cfg;
    c->device = device;
    if (cfg->kind == EGOEGO_S1_HEADNET) {
        c->n_heads = 2;
        c->out_stride = 4;
        c->heads[0] = HeadDesc{4, {DM, 1024, 512, 256, 3}, 0, 0};
        c->heads[1] = HeadDesc{4, {DM, 1024, 512, 256, 1}, 3, 4};
    } else {
        c->n_heads = 1;
        c->out_stride = 3;
        c->heads[0] = HeadDesc{3, {DM, 512, 256, 3, 0}, 0, 0};
    }
    *out = c;
    return 0;
}

void egoego_s1_train_ctx_destroy(egoego_s1_train_ctx* ctx) { destroy_ctx(ctx); }

size_t egoego_s1_train_workspace_bytes(const egoego_s1_train_ctx* ctx, int n_windows) {
    if (check_shape(ctx, n_windows)) return 0;
    return work_map(ctx, n_windows).total;
}

size_t egoego_s1_train_saves_bytes(const egoego_s1_train_ctx* ctx, int n_windows) {
    if (check_shape(ctx, n_windows)) return 0;
    return saves_map(ctx, n_windows).total;
}

int egoego_s1_train_forward(egoego_s1_train_ctx* ctx, const egoego_s1_weights* w, const float* d_feats, const int32_t* d_valid,
                            float p_drop, uint64_t dropout_seed, const int64_t* d_window_ids, int W, void* d_saves, size_t saves_bytes,
                            void* d_workspace, size_t workspace_bytes, float* d_heads, void* stream) {
    if (int rc = check_shape(ctx, W)) return rc;
    if (int rc = check_weights(ctx, w)) return rc;
    if (!d_feats || !d_valid || !d_heads) return fail(EGOEGO_E_INVALID, "an input / output pointer is NULL");
    if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(EGOEGO_E_INVALID, "p_drop %g outside [0, 1)", (double)p_drop);
    const Saves sm = saves_map(ctx, W);
    const Work wm = work_map(ctx, W);
    if (int rc = check_workspace(d_workspace, workspace_bytes, wm.total)) return rc;
    if (int rc = check_saves(d_saves, saves_bytes, sm.total)) return rc;
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    hipStream_t s = as_stream(stream);
    char* sv = (char*)d_saves;
    char* ws = (char*)d_workspace;
    const int L = ctx->cfg.window, R = W * L, D = ctx->cfg.d_feats, NL = ctx->cfg.n_dec_layers;
    auto SF = [&](size_t off) { return (float*)(sv + off); };
    auto WF = [&](size_t off) { return (float*)(ws + off); };
    const int64_t* wids = (const int64_t*)(sv + sm.wids);
    float* maskR = SF(sm.maskR);

    {
        s1t::Prep p;
        p.feats = d_feats; p.valid = (const int*)d_valid; p.wids = d_window_ids;
        p.xin = SF(sm.xin); p.maskR = maskR; p.wids_out = (int64_t*)(sv + sm.wids);
        p.W = W; p.L = L; p.D = D;
        const long n = (long)R * D;
        hipLaunchKernelGGL(s1t::prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    }
    float* X = SF(sm.X0);
    // embed: start_conv(xin) + bias + position row t + 1 (TM:180-182, 203-208)
    linear_fwd(s, SF(sm.xin), D, R, D, w->start_conv_w, w->start_conv_b, DM, X, DM, 0, w->position_vec, L);
    const size_t PP = (size_t)L * L;  // one (window, head) block of probabilities
    for (int l = 0; l < NL; ++l) {
        const egoego_layer_weights& lw = w->layers[l];
        char* lb = sv + sm.layer0 + (size_t)l * sm.per_layer;
        float* qkv = (float*)(lb + sm.qkv);
        float* P = (float*)(lb + sm.P);
        float* O = (float*)(lb + sm.O);
        float* Xn = (float*)(sv + sm.X0 + (size_t)(l + 1) * sm.Xbytes);
        linear_fwd(s, X, DM, R, DM, lw.w_q, lw.b_q, HD, qkv, 3 * HD);
        linear_fwd(s, X, DM, R, DM, lw.w_k, lw.b_k, HD, qkv + HD, 3 * HD);
        linear_fwd(s, X, DM, R, DM, lw.w_v, lw.b_v, HD, qkv + 2 * HD, 3 * HD);
        {   // S = Q K^T / 16 per (window, head), over all L keys (a padded token is not masked as a key)
            tr::Gemm g = gemm_base(L, L, DK);
            g.zdiv = NH;
            g.A = qkv; g.sai = 3 * HD; g.sak = 1; g.bsA0 = (long)L * 3 * HD; g.bsA1 = DK;
            g.B = qkv + HD; g.sbj = 3 * HD; g.sbk = 1; g.bsB0 = g.bsA0; g.bsB1 = DK;
            g.C = P; g.ldc = L; g.bsC0 = (long)NH * PP; g.bsC1 = (long)PP;
            g.alpha = 0.0625f;
            launch_gemm<tr::GEMM_ATTN>(s, g, W * NH);
        }
        const float* Pd = P;
        {
            tr::Softmax a;
            a.S = P; a.Pd = p_drop > 0.f ? WF(wm.Pd) : nullptr; a.L = L; a.rows = W * NH * L;
            a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_ATTN);
            hipLaunchKernelGGL(tr::softmax_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
            if (a.Pd) Pd = a.Pd;
        }
        {   // O = dropout(P) V
            tr::Gemm g = gemm_base(L, DK, L);
            g.zdiv = NH;
            g.A = Pd; g.sai = L; g.sak = 1; g.bsA0 = (long)NH * PP; g.bsA1 = (long)PP;
            g.B = qkv + 2 * HD; g.sbj = 1; g.sbk = 3 * HD; g.bsB0 = (long)L * 3 * HD; g.bsB1 = DK;
            g.C = O; g.ldc = HD; g.bsC0 = (long)L * HD; g.bsC1 = DK;
            launch_gemm<tr::GEMM_ATTN>(s, g, W * NH);
        }
        linear_fwd(s, O, HD, R, HD, lw.w_fc, lw.b_fc, DM, WF(wm.F), DM);
        {
            tr::LnFwd a;
            a.Y = WF(wm.F); a.resid = X; a.Z = (float*)(lb + sm.Z1); a.out = (float*)(lb + sm.Y1);
            a.g = lw.ln1_g; a.b = lw.ln1_b; a.mask = maskR; a.R = R; a.L = L;
            a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_FC);
            hipLaunchKernelGGL(s1t::ln_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, s, a);
        }
        linear_fwd(s, (float*)(lb + sm.Y1), DM, R, DM, lw.w_1, lw.b_1, DM, (float*)(lb + sm.H), DM, 1);
        linear_fwd(s, (float*)(lb + sm.H), DM, R, DM, lw.w_2, lw.b_2, DM, WF(wm.F), DM);
        {
            tr::LnFwd a;
            a.Y = WF(wm.F); a.resid = (float*)(lb + sm.Y1); a.Z = (float*)(lb + sm.Z2); a.out = Xn;
            a.g = lw.ln2_g; a.b = lw.ln2_b; a.mask = maskR; a.R = R; a.L = L;
            a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_FFN);
            hipLaunchKernelGGL(s1t::ln_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, s, a);
        }
        X = Xn;
    }
    // the heads: on every token (HeadNet) or on token 0 of every window (GravityNet: rows L * 256 apart)
    const int Rh = (int)head_rows(ctx, W);
    const long ldx = is_headnet(ctx) ? DM : (long)L * DM;
    for (int h = 0; h < ctx->n_heads; ++h) {
        const HeadDesc& hd = ctx->heads[h];
        const float* in = X;
        long ldin = ldx;
        for (int j = 1; j < hd.n; ++j) {
            float* hid = SF(sm.hid[h][j]);
            linear_fwd(s, in, ldin, Rh, hd.dims[j - 1], w->head_w[hd.w0 + j - 1], w->head_b[hd.w0 + j - 1], hd.dims[j], hid, hd.dims[j], 1);
            in = hid;
            ldin = hd.dims[j];
        }
        linear_fwd(s, in, ldin, Rh, hd.dims[hd.n - 1], w->head_w[hd.w0 + hd.n - 1], w->head_b[hd.w0 + hd.n - 1], hd.dims[hd.n],
                   d_heads + hd.col, ctx->out_stride);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_s1_train_backward(egoego_s1_train_ctx* ctx, const egoego_s1_weights* w, const void* d_saves, size_t saves_bytes,
                             const float* d_dheads, const egoego_s1_train_grads* grads, float p_drop, uint64_t dropout_seed, int W,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_shape(ctx, W)) return rc;
    if (int rc = check_weights(ctx, w)) return rc;
    if (!d_dheads || !grads || !grads->layers) return fail(EGOEGO_E_INVALID, "the upstream gradient / the gradient buffers are NULL");
    if (!grads->start_conv_w || !grads->start_conv_b) return fail(EGOEGO_E_INVALID, "a gradient buffer is NULL");
    for (int l = 0; l < ctx->cfg.n_dec_layers; ++l) {
        const egoego_train_layer_grads& g = grads->layers[l];
        float* ps[] = {g.w_q, g.b_q, g.w_k, g.b_k, g.w_v, g.b_v, g.w_fc, g.b_fc, g.ln1_g, g.ln1_b, g.w_1, g.b_1, g.w_2, g.b_2, g.ln2_g, g.ln2_b};
        for (float* p : ps)
            if (!p) return fail(EGOEGO_E_INVALID, "a gradient buffer of layer %d is NULL", l);
    }
    for (int j = 0; j < n_head_linears(ctx); ++j)
        if (!grads->head_w[j] || !grads->head_b[j]) return fail(EGOEGO_E_INVALID, "a gradient buffer of the heads is NULL");
    if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(EGOEGO_E_INVALID, "p_drop %g outside [0, 1)", (double)p_drop);
    const Saves sm = saves_map(ctx, W);
    const Work wm = work_map(ctx, W);
    if (int rc = check_workspace(d_workspace, workspace_bytes, wm.total)) return rc;
    if (int rc = check_saves(d_saves, saves_bytes, sm.total)) return rc;
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    hipStream_t s = as_stream(stream);
    const char* sv = (const char*)d_saves;
    char* ws = (char*)d_workspace;
    const int L = ctx->cfg.window, R = W * L, D = ctx->cfg.d_feats, NL = ctx->cfg.n_dec_layers;
    auto SF = [&](size_t off) { return (const float*)(sv + off); };
    auto WF = [&](size_t off) { return (float*)(ws + off); };
    const int64_t* wids = (const int64_t*)(sv + sm.wids);
    const float* maskR = SF(sm.maskR);
    float *GA = WF(wm.GA), *GB = WF(wm.GB), *GF = WF(wm.GF), *GH = WF(wm.GH), *GO = WF(wm.GO), *GQKV = WF(wm.GQKV), *GP = WF(wm.GP);
    float* part = WF(wm.part);
    const size_t PP = (size_t)L * L;
    const int nln = n_ln_chunks(R);

    // the heads, from the upstream gradient down to GA = d(decoder output); the ReLUs are gates on the saved hidden rows
    const float* Xf = (const float*)(sv + sm.X0 + (size_t)NL * sm.Xbytes);
    const int Rh = (int)head_rows(ctx, W);
    const long ldx = is_headnet(ctx) ? DM : (long)L * DM;
    if (!is_headnet(ctx)) HIP_TRY(hipMemsetAsync(GA, 0, (size_t)R * DM * sizeof(float), s));  // only token 0's rows receive a gradient
    for (int h = 0; h < ctx->n_heads; ++h) {
        const HeadDesc& hd = ctx->heads[h];
        const float* dY = d_dheads + hd.col;
        long ldy = ctx->out_stride;
        float* ping[2] = {WF(wm.HG0), WF(wm.HG1)};
        for (int j = hd.n; j >= 1; --j) {
            const int wi = hd.w0 + j - 1;
            const float* in = j == 1 ? Xf : SF(sm.hid[h][j - 1]);
            const long ldin = j == 1 ? ldx : hd.dims[j - 1];
            linear_bwd_weight(s, dY, ldy, Rh, hd.dims[j], in, ldin, hd.dims[j - 1], part, grads->head_w[wi], grads->head_b[wi]);
            if (j > 1) {
                float* dX = ping[j & 1];
                linear_bwd_data(s, dY, ldy, Rh, hd.dims[j], w->head_w[wi], hd.dims[j - 1], dX, hd.dims[j - 1], 0, in);
                dY = dX;
                ldy = hd.dims[j - 1];
            } else {
                linear_bwd_data(s, dY, ldy, Rh, hd.dims[1], w->head_w[wi], DM, GA, ldx, h > 0 ? 1 : 0);
            }
        }
    }

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
            hipLaunchKernelGGL(s1t::ln_bwd_kernel, dim3((nln + 3) / 4), dim3(256), 0, s, a);
            fold(s, (const float*)part, 2 * DM, nln, DM, lg.ln2_g);
            fold(s, (const float*)(part + DM), 2 * DM, nln, DM, lg.ln2_b);
        }
        linear_bwd_weight(s, GF, DM, R, DM, H, DM, DM, part, lg.w_2, lg.b_2);
        linear_bwd_data(s, GF, DM, R, DM, lw.w_2, DM, GH, DM, 0, H);  // through the ReLU: kept where H > 0
        linear_bwd_weight(s, GH, DM, R, DM, Y1, DM, DM, part, lg.w_1, lg.b_1);
        linear_bwd_data(s, GH, DM, R, DM, lw.w_1, DM, GB, DM, 1);
        {   // LayerNorm 1: GB = d Y1 -> GA = d z1 (the residual's share, to X), GF = d(fc out)
            tr::LnBwd a;
            a.dOut = GB; a.Z = (const float*)(lb + sm.Z1); a.g = lw.ln1_g; a.mask = maskR; a.dZ = GA; a.dY = GF; a.part = part;
            a.R = R; a.L = L; a.d = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_FC);
            hipLaunchKernelGGL(s1t::ln_bwd_kernel, dim3((nln + 3) / 4), dim3(256), 0, s, a);
            fold(s, (const float*)part, 2 * DM, nln, DM, lg.ln1_g);
            fold(s, (const float*)(part + DM), 2 * DM, nln, DM, lg.ln1_b);
        }
        linear_bwd_weight(s, GF, DM, R, DM, O, HD, HD, part, lg.w_fc, lg.b_fc);
        linear_bwd_data(s, GF, DM, R, DM, lw.w_fc, HD, GO, HD, 0);
        // attention backward per (window, head); one wave sums over all keys / queries of its tile: no sum across workgroups
        const tr::Drop da = make_drop(p_drop, dropout_seed, wids, l, tr::SITE_ATTN);
        const float* Pd = P;
        if (da.thr) {
            const long n = (long)W * NH * (long)PP;
            hipLaunchKernelGGL(tr::redrop_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, WF(wm.Pd), L, n, da);
            Pd = WF(wm.Pd);
        }
        {   // dV = Pd^T dO
            tr::Gemm g = gemm_base(L, DK, L);
            g.zdiv = NH;
            g.A = Pd; g.sai = 1; g.sak = L; g.bsA0 = (long)NH * PP; g.bsA1 = (long)PP;
            g.B = GO; g.sbj = 1; g.sbk = HD; g.bsB0 = (long)L * HD; g.bsB1 = DK;
            g.C = GQKV + 2 * HD; g.ldc = 3 * HD; g.bsC0 = (long)L * 3 * HD; g.bsC1 = DK;
            launch_gemm<tr::GEMM_ATTN>(s, g, W * NH);
        }
        {   // dPd = dO V^T
            tr::Gemm g = gemm_base(L, L, DK);
            g.zdiv = NH;
            g.A = GO; g.sai = HD; g.sak = 1; g.bsA0 = (long)L * HD; g.bsA1 = DK;
            g.B = qkv + 2 * HD; g.sbj = 3 * HD; g.sbk = 1; g.bsB0 = (long)L * 3 * HD; g.bsB1 = DK;
            g.C = GP; g.ldc = L; g.bsC0 = (long)NH * PP; g.bsC1 = (long)PP;
            launch_gemm<tr::GEMM_ATTN>(s, g, W * NH);
        }
        {
            tr::SoftmaxBwd a;
            a.dP = GP; a.P = P; a.L = L; a.rows = W * NH * L; a.d = da;
            hipLaunchKernelGGL(tr::softmax_bwd_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
        }
        {   // dQ = dS K
            tr::Gemm g = gemm_base(L, DK, L);
            g.zdiv = NH;
            g.A = GP; g.sai = L; g.sak = 1; g.bsA0 = (long)NH * PP; g.bsA1 = (long)PP;
            g.B = qkv + HD; g.sbj = 1; g.sbk = 3 * HD; g.bsB0 = (long)L * 3 * HD; g.bsB1 = DK;
            g.C = GQKV; g.ldc = 3 * HD; g.bsC0 = (long)L * 3 * HD; g.bsC1 = DK;
            launch_gemm<tr::GEMM_ATTN>(s, g, W * NH);
        }
        {   // dK = dS^T Q
            tr::Gemm g = gemm_base(L, DK, L);
            g.zdiv = NH;
            g.A = GP; g.sai = 1; g.sak = L; g.bsA0 = (long)NH * PP; g.bsA1 = (long)PP;
            g.B = qkv; g.sbj = 1; g.sbk = 3 * HD; g.bsB0 = (long)L * 3 * HD; g.bsB1 = DK;
            g.C = GQKV + HD; g.ldc = 3 * HD; g.bsC0 = (long)L * 3 * HD; g.bsC1 = DK;
            launch_gemm<tr::GEMM_ATTN>(s, g, W * NH);
        }
        const float* pw[3] = {lw.w_q, lw.w_k, lw.w_v};
        float* gw[3] = {lg.w_q, lg.w_k, lg.w_v};
        float* gb[3] = {lg.b_q, lg.b_k, lg.b_v};
        for (int k = 0; k < 3; ++k) {
            linear_bwd_weight(s, GQKV + k * HD, 3 * HD, R, HD, Xl, DM, DM, part, gw[k], gb[k]);
            linear_bwd_data(s, GQKV + k * HD, 3 * HD, R, HD, pw[k], DM, GA, DM, 1);
        }
        // GA = d(layer input)
    }
    linear_bwd_weight(s, GA, DM, R, DM, SF(sm.xin), D, D, part, grads->start_conv_w, grads->start_conv_b);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_s1_train_dropout_mask(egoego_s1_train_ctx* ctx, float p_drop, uint64_t dropout_seed, int layer, int site,
                                 const int64_t* d_window_ids, int W, uint8_t* d_out, void* d_workspace, size_t workspace_bytes,
                                 void* stream) {
    if (int rc = check_shape(ctx, W)) return rc;
    if (!d_out) return fail(EGOEGO_E_INVALID, "d_out is NULL");
    if (site < 0 || site > 2 || layer < 0 || layer >= ctx->cfg.n_dec_layers) return fail(EGOEGO_E_INVALID, "layer %d / site %d out of range", layer, site);
    if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(EGOEGO_E_INVALID, "p_drop %g outside [0, 1)", (double)p_drop);
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    hipStream_t s = as_stream(stream);
    const int64_t* wids = d_window_ids;
    if (!wids) {  // window w draws the stream of id w
        if (int rc = check_workspace(d_workspace, workspace_bytes, (size_t)W * sizeof(int64_t))) return rc;
        hipLaunchKernelGGL(tr::iota_kernel, dim3((W + 255) / 256), dim3(256), 0, s, (int64_t*)d_workspace, W);
        wids = (const int64_t*)d_workspace;
    }
    const long L = ctx->cfg.window;
    const long per = site == tr::SITE_ATTN ? (long)NH * L * L : L * DM;
    const long n = per * W;
    const tr::Drop d = make_drop(p_drop, dropout_seed, wids, layer, site);
    hipLaunchKernelGGL(tr::drop_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, per, n, d_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_s1_train_saved(egoego_s1_train_ctx* ctx, const void* d_saves, size_t saves_bytes, int W, int layer, int which, float* d_out,
                          void* stream) {
    if (int rc = check_shape(ctx, W)) return rc;
    if (!d_out) return fail(EGOEGO_E_INVALID, "d_out is NULL");
    const Saves sm = saves_map(ctx, W);
    if (!d_saves || saves_bytes < sm.total) return fail(EGOEGO_E_WORKSPACE, "saves: %zu bytes, need %zu", saves_bytes, sm.total);
    const size_t L = (size_t)ctx->cfg.window, R = (size_t)W * L, f = sizeof(float);
    const char* src;
    size_t bytes;
    if (which == EGOEGO_S1_TRAIN_SAVED_HEAD_HIDDEN) {  // `layer` counts the heads' Linears as egoego_s1_weights.head_w does
        src = nullptr;
        bytes = 0;
        for (int h = 0; h < ctx->n_heads; ++h) {
            const HeadDesc& hd = ctx->heads[h];
            const int j = layer - hd.w0 + 1;
            if (j >= 1 && j < hd.n) {
                src = (const char*)d_saves + sm.hid[h][j];
                bytes = head_rows(ctx, W) * hd.dims[j] * f;
            }
        }
        if (!src) return fail(EGOEGO_E_INVALID, "head Linear %d has no saved hidden rows", layer);
    } else {
        if (layer < 0 || layer >= ctx->cfg.n_dec_layers) return fail(EGOEGO_E_INVALID, "layer %d out of range", layer);
        const char* lb = (const char*)d_saves + sm.layer0 + (size_t)layer * sm.per_layer;
        switch (which) {
            case EGOEGO_TRAIN_SAVED_FFN_HIDDEN: src = lb + sm.H; bytes = R * DM * f; break;
            case EGOEGO_TRAIN_SAVED_ATTN_PROB: src = lb + sm.P; bytes = (size_t)W * NH * L * L * f; break;
            case EGOEGO_TRAIN_SAVED_ATTN_OUT: src = lb + sm.O; bytes = R * HD * f; break;
            case EGOEGO_TRAIN_SAVED_ATTN_LN: src = lb + sm.Y1; bytes = R * DM * f; break;
            case EGOEGO_TRAIN_SAVED_LAYER_OUT: src = (const char*)d_saves + sm.X0 + (size_t)(layer + 1) * sm.Xbytes; bytes = R * DM * f; break;
            case EGOEGO_TRAIN_SAVED_LAYER_IN: src = (const char*)d_saves + sm.X0 + (size_t)layer * sm.Xbytes; bytes = R * DM * f; break;
            default: return fail(EGOEGO_E_INVALID, "unknown saved tensor %d", which);
        }
    }
    DeviceGuard guard;
    if (int rc = guard.enter(ctx->device)) return rc;
    HIP_TRY(hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return 0;
}

size_t egoego_s1_headnet_loss_workspace_bytes(int B) {
    if (B < 1) return 0;
    return (((size_t)B * 3 * sizeof(double)) + 255) & ~(size_t)255;
}

int egoego_s1_headnet_loss(const float* d_heads, int window, int B, int T, const float* d_head_pose, const float* d_head_vels,
                           double dist_scale, double w_rotation, double w_va, double w_dist, double* d_loss, double* d_dheads64,
                           float* d_dheads, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!d_heads || !d_head_pose || !d_head_vels || !d_loss) return fail(EGOEGO_E_INVALID, "an input pointer is NULL");
    if (B < 1 || B > 65535 || window < 1 || window > s1t::MAX_WINDOW || T < 1 || T > window)
        return fail(EGOEGO_E_INVALID, "B = %d, T = %d, window = %d: 1 <= B <= 65535 and 1 <= T <= window <= %d expected", B, T, window,
                    s1t::MAX_WINDOW);
    if (int rc = check_workspace(d_workspace, workspace_bytes, egoego_s1_headnet_loss_workspace_bytes(B))) return rc;
    s1t::HeadLoss a;
    a.heads = d_heads; a.pose = d_head_pose; a.vels = d_head_vels;
    a.window = window; a.B = B; a.T = T;
    a.dist_scale = dist_scale; a.w_rot = w_rotation; a.w_va = w_va; a.w_dist = w_dist;
    a.part = (double*)d_workspace; a.d64 = d_dheads64; a.d32 = d_dheads;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(s1t::headnet_loss_kernel, dim3(B), dim3(s1t::MAX_WINDOW), 0, s, a);
    hipLaunchKernelGGL(s1t::headnet_loss_final_kernel, dim3(1), dim3(64), 0, s, (const double*)a.part, B, T, w_rotation, w_va, w_dist,
                       d_loss);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
