// stage1.hip — context, weight packing, workspace and the C ABI (include/egoego_hip.h, egoego_s1_*) of the stage-1 head-pose
// estimators.  Kernels: stage1.h.  Nothing here touches a stage-2 code path.
#include <math.h>

#include "host_util.h"
#include "stage1.h"

using namespace s1;

static constexpr int MAX_LAYERS = 8;
static constexpr int MAX_HEAD = 4;  // linears per head (HeadNet: 3 hidden + fc)

struct S1Layer {
    Lin qkv, fc, w1, w2;
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
};

struct egoego_s1_ctx {
    egoego_s1_config cfg;
    int device, Lp;
    bool loaded, tail_attr;
    DevMem mem;
    Lin embed;
    float* pos;
    S1Layer layers[MAX_LAYERS];
    // heads: hl[0] = first hidden layer of every head, concatenated (HeadNet: va | dist, 2048 rows); hl[1..] per head
    Lin h0;
    Lin hid[2][MAX_HEAD];  // [head][layer 1..]: hid[g][i] = layer i + 1 of head g (the last one is the fc)
    int n_lin;             // linears per head
    int n_heads;
};

// Pack the rows of `parts` (each [rows][K] fp32 on the device, stacked) into hi / lo fragment-tiled planes.
static int pack_lin(egoego_s1_ctx* c, const std::vector<std::pair<const float*, int>>& w, const std::vector<const float*>& b, int K,
                    Lin& out) {
    int N = 0;
    for (auto& p : w) N += p.second;
    const int Np = (N + 31) / 32 * 32, Kp = (K + 15) / 16 * 16, K16 = Kp / 16;
    std::vector<uint16_t> hi((size_t)Np * Kp, 0), lo((size_t)Np * Kp, 0);
    std::vector<float> bias(N), tmp;
    int r0 = 0;
    for (size_t i = 0; i < w.size(); ++i) {
        const int rows = w[i].second;
        if (int rc = fetch(w[i].first, (size_t)rows * K, tmp)) return rc;
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < K; ++k)
                split_store(hi, lo, tiled_index(r0 + r, k, K16), tmp[(size_t)r * K + k]);
        if (int rc = fetch(b[i], rows, tmp)) return rc;
        memcpy(bias.data() + r0, tmp.data(), rows * sizeof(float));
        r0 += rows;
    }
    const uint16_t *dh, *dl;
    if (int rc = c->mem.upload(hi, &dh)) return rc;
    if (int rc = c->mem.upload(lo, &dl)) return rc;
    if (int rc = c->mem.upload(bias, &out.b)) return rc;
    out.hi = (const __bf16*)dh;
    out.lo = (const __bf16*)dl;
    out.N = N;
    out.K16 = K16;
    return 0;
}

static int pack_weights(egoego_s1_ctx* c, const egoego_s1_weights* w) {
    const egoego_s1_config& g = c->cfg;
    if (int r = pack_lin(c, {{w->start_conv_w, DM}}, {w->start_conv_b}, g.d_feats, c->embed)) return r;
    if (int r = c->mem.copy_dev(w->position_vec, (size_t)(g.window + 1) * DM, &c->pos)) return r;
    for (int i = 0; i < g.n_dec_layers; ++i) {
        const egoego_layer_weights& L = w->layers[i];
        S1Layer& d = c->layers[i];
        if (int r = pack_lin(c, {{L.w_q, HD}, {L.w_k, HD}, {L.w_v, HD}}, {L.b_q, L.b_k, L.b_v}, DM, d.qkv)) return r;
        if (int r = pack_lin(c, {{L.w_fc, DM}}, {L.b_fc}, HD, d.fc)) return r;
        if (int r = pack_lin(c, {{L.w_1, DM}}, {L.b_1}, DM, d.w1)) return r;
        if (int r = pack_lin(c, {{L.w_2, DM}}, {L.b_2}, DM, d.w2)) return r;
        if (int r = c->mem.copy_dev(L.ln1_g, DM, &d.ln1_g)) return r;
        if (int r = c->mem.copy_dev(L.ln1_b, DM, &d.ln1_b)) return r;
        if (int r = c->mem.copy_dev(L.ln2_g, DM, &d.ln2_g)) return r;
        if (int r = c->mem.copy_dev(L.ln2_b, DM, &d.ln2_b)) return r;
    }
    if (g.kind == EGOEGO_S1_HEADNET) {
        // va: 256 -> 1024 -> 512 -> 256 -> 3; dist: 256 -> 1024 -> 512 -> 256 -> 1
        c->n_heads = 2;
        c->n_lin = 4;
        if (int r = pack_lin(c, {{w->head_w[0], 1024}, {w->head_w[4], 1024}}, {w->head_b[0], w->head_b[4]}, DM, c->h0)) return r;
        const int dims[4][2] = {{1024, 256}, {512, 1024}, {256, 512}, {0, 256}};
        for (int h = 0; h < 2; ++h)
            for (int i = 1; i < 4; ++i) {
                const int N = i < 3 ? dims[i][0] : (h == 0 ? 3 : 1);
                if (int r = pack_lin(c, {{w->head_w[4 * h + i], N}}, {w->head_b[4 * h + i]}, dims[i][1], c->hid[h][i - 1])) return r;
            }
    } else {
        // normal: 256 -> 512 -> 256 -> 3 on token 0
        c->n_heads = 1;
        c->n_lin = 3;
        if (int r = pack_lin(c, {{w->head_w[0], 512}}, {w->head_b[0]}, DM, c->h0)) return r;
        if (int r = pack_lin(c, {{w->head_w[1], 256}}, {w->head_b[1]}, 512, c->hid[0][0])) return r;
        if (int r = pack_lin(c, {{w->head_w[2], 3}}, {w->head_b[2]}, 256, c->hid[0][1])) return r;
    }
    return 0;
}

extern "C" {

const char* egoego_s1_last_error(void) { return last_err.c_str(); }

int egoego_s1_ctx_create(const egoego_s1_config* cfg, int device, egoego_s1_ctx** out) {
    if (!cfg || !out) return fail(EGOEGO_E_INVALID, "NULL argument");
    *out = nullptr;
    if (cfg->kind != EGOEGO_S1_HEADNET && cfg->kind != EGOEGO_S1_GRAVITYNET) return fail(EGOEGO_E_INVALID, "unknown kind %d", cfg->kind);
    if (cfg->d_model != DM) return fail(EGOEGO_E_INVALID, "d_model %d: stage 1 supports 256 only", cfg->d_model);
    if (cfg->n_head * cfg->d_k != HD || cfg->n_head * cfg->d_v != HD || cfg->n_head != NH)
        return fail(EGOEGO_E_INVALID, "n_head %d, d_k %d, d_v %d: stage 1 supports n_head 4, d_k = d_v = 256 only", cfg->n_head,
                       cfg->d_k, cfg->d_v);
    if (cfg->n_dec_layers < 1 || cfg->n_dec_layers > MAX_LAYERS)
        return fail(EGOEGO_E_INVALID, "n_dec_layers %d: 1..%d supported", cfg->n_dec_layers, MAX_LAYERS);
    if (cfg->window < 1 || cfg->window > 128) return fail(EGOEGO_E_INVALID, "window %d: 1..128 supported", cfg->window);
    if (cfg->d_feats < 1 || cfg->d_feats > 1024) return fail(EGOEGO_E_INVALID, "d_feats %d: 1..1024 supported", cfg->d_feats);
    if (int rc = check_device(device)) return rc;
    egoego_s1_ctx* c = new egoego_s1_ctx();
    c->cfg = *cfg;
    c->device = device;
    c->Lp = (cfg->window + 31) / 32 * 32;
    c->loaded = false;
    c->tail_attr = false;
    *out = c;
    return 0;
}

void egoego_s1_ctx_destroy(egoego_s1_ctx* c) { destroy_ctx(c); }

int egoego_s1_load_weights(egoego_s1_ctx* c, const egoego_s1_weights* w, void* stream) {
    if (!c || !w || !w->layers) return fail(EGOEGO_E_INVALID, "NULL argument");
    DeviceGuard dev;
    if (int rc = dev.enter(c->device)) return rc;
    HIP_TRY(hipStreamSynchronize(as_stream(stream)));  // the caller's tensors are written on its stream; old weights may still be read
    c->mem.free_all();
    c->loaded = false;
    const int rc = pack_weights(c, w);
    if (rc == 0) c->loaded = true;
    else c->mem.free_all();
    return rc;
}

// workspace: X [R][256] | QKV [R][3072] | O [R][1024]  (R = W * Lp); the heads reuse QKV / O
static size_t ws_bytes(const egoego_s1_ctx* c, int W) {
    const size_t R = (size_t)W * c->Lp;
    return R * (DM + 3 * HD + HD) * sizeof(float);
}

size_t egoego_s1_workspace_bytes(const egoego_s1_ctx* c, int n_windows) {
    if (!c || n_windows < 1) {
        fail(EGOEGO_E_INVALID, "n_windows must be >= 1");
        return 0;
    }
    if ((size_t)n_windows * c->Lp > (1u << 22)) {
        fail(EGOEGO_E_INVALID, "%d windows: more than 2^22 rows per call", n_windows);
        return 0;
    }
    return ws_bytes(c, n_windows);
}

static void launch_linear(const float* A, long lda, int a_goff, int K, float* out, long ldo, int o_goff, const Lin* w, int ngroups,
                          int M, bool relu, int Lp, int window, hipStream_t s) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.a_goff = a_goff; g.K = K;
    g.out = out; g.ldo = ldo; g.o_goff = o_goff;
    int nmax = 0;
    for (int i = 0; i < ngroups; ++i) {
        g.w[i] = w[i];
        nmax = w[i].N > nmax ? w[i].N : nmax;
    }
    g.M = M; g.relu = relu ? 1 : 0; g.Lp = Lp; g.window = window;
    const dim3 grid((M + 31) / 32, ((nmax + 31) / 32 + 3) / 4, ngroups);
    // the vector loads read whole 16-column k steps: only when K fills them (K % 8 == 8 would read 8 columns past a row's end)
    const bool vec = (K % 16 == 0) && (lda % 4 == 0) && (a_goff % 4 == 0);
    if (vec) s1_linear_kernel<true><<<grid, dim3(256), 0, s>>>(g);
    else s1_linear_kernel<false><<<grid, dim3(256), 0, s>>>(g);
}

int egoego_s1_encode(egoego_s1_ctx* c, const float* d_feats, const int32_t* d_valid, int W, float* d_out, float* d_layers,
                     void* d_ws, size_t ws_n, void* stream) {
    if (!c || !d_feats || !d_valid || !d_out) return fail(EGOEGO_E_INVALID, "NULL argument");
    if (!c->loaded) return fail(EGOEGO_E_STATE, "weights not loaded");
    if (W < 1) return fail(EGOEGO_E_INVALID, "n_windows must be >= 1");
    if ((size_t)W * c->Lp > (1u << 22)) return fail(EGOEGO_E_INVALID, "%d windows: more than 2^22 rows per call", W);
    if (int rc = check_workspace(d_ws, ws_n, ws_bytes(c, W))) return rc;
    DeviceGuard dev;
    if (int rc = dev.enter(c->device)) return rc;
    const egoego_s1_config& g = c->cfg;
    hipStream_t s = as_stream(stream);
    const int Lp = c->Lp, R = W * Lp;
    float* X = (float*)d_ws;
    float* QKV = X + (size_t)R * DM;
    float* O = QKV + (size_t)R * 3 * HD;
    const int* valid = (const int*)d_valid;
    {
        EmbedArgs e{d_feats, valid, c->pos, X, c->embed, g.d_feats, g.window, Lp, R};
        const dim3 grid(R / 32, DM / 128);
        if (g.d_feats % 16 == 0) s1_embed_kernel<true><<<grid, dim3(256), 0, s>>>(e);
        else s1_embed_kernel<false><<<grid, dim3(256), 0, s>>>(e);
    }
    const size_t tail_smem = 2 * 32 * LN_STRIDE * sizeof(float);
    if (!c->tail_attr) {  // 65 KiB of dynamic LDS: opt in once (the context lives on one device)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(s1_tail_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)tail_smem);
        if (e != hipSuccess) return fail(EGOEGO_E_HIP, "hipFuncSetAttribute(s1_tail_kernel) failed: %s", hipGetErrorString(e));
        c->tail_attr = true;
    }
    for (int l = 0; l < g.n_dec_layers; ++l) {
        const S1Layer& L = c->layers[l];
        launch_linear(X, DM, 0, DM, QKV, 3 * HD, 0, &L.qkv, 1, R, false, 0, 0, s);
        s1_attn_kernel<<<dim3(W * NH, Lp / 32), dim3(256), 0, s>>>(AttnArgs{QKV, O, g.window, Lp});
        TailArgs t{O, X, d_layers ? d_layers + (size_t)l * W * g.window * DM : nullptr, valid, L.fc, L.w1, L.w2,
                   L.ln1_g, L.ln1_b, L.ln2_g, L.ln2_b, g.window, Lp};
        s1_tail_kernel<<<dim3(R / 32), dim3(512), tail_smem, s>>>(t);
    }
    float* H1 = QKV;                    // [R][2048] (HeadNet) / [W][512]
    float* H3 = QKV + (size_t)R * 2048; // [R][2 * 256]
    float* H2 = O;                      // [R][2 * 512]
    if (g.kind == EGOEGO_S1_HEADNET) {
        launch_linear(X, DM, 0, DM, H1, 2048, 0, &c->h0, 1, R, true, 0, 0, s);
        const Lin l1[2] = {c->hid[0][0], c->hid[1][0]}, l2[2] = {c->hid[0][1], c->hid[1][1]}, l3[2] = {c->hid[0][2], c->hid[1][2]};
        launch_linear(H1, 2048, 1024, 1024, H2, 1024, 512, l1, 2, R, true, 0, 0, s);
        launch_linear(H2, 1024, 512, 512, H3, 512, 256, l2, 2, R, true, 0, 0, s);
        launch_linear(H3, 512, 256, 256, d_out, 4, 3, l3, 2, R, false, Lp, g.window, s);
    } else {
        // token 0 of every window: row w * Lp
        launch_linear(X, (long)Lp * DM, 0, DM, H1, 512, 0, &c->h0, 1, W, true, 0, 0, s);
        launch_linear(H1, 512, 0, 512, H2, 256, 0, &c->hid[0][0], 1, W, true, 0, 0, s);
        launch_linear(H2, 256, 0, 256, d_out, 3, 0, &c->hid[0][1], 1, W, false, 0, 0, s);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EGOEGO_E_HIP, "stage-1 launch failed: %s", hipGetErrorString(e));
    return 0;
}

int egoego_s1_gravity_features(const float* d_rot, const float* d_trans, const int32_t* d_len, int Sn, int Lmax, int window,
                               float* d_feats, int32_t* d_valid, void* stream) {
    if (!d_rot || !d_trans || !d_len || !d_feats || !d_valid || Sn < 1 || Lmax < 1 || window < 1)
        return fail(EGOEGO_E_INVALID, "bad argument");
    const int n = Sn * window;
    s1_gravity_features_kernel<<<(n + 255) / 256, 256, 0, as_stream(stream)>>>(d_rot, d_trans, (const int*)d_len, Lmax, window,
                                                                               d_feats, (int*)d_valid, Sn);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EGOEGO_E_HIP, "launch failed: %s", hipGetErrorString(e));
    return 0;
}

int egoego_s1_integrate(const float* d_heads, int window, const int32_t* d_T, const int32_t* d_win0, const double* d_q0,
                        const double* d_slam, const int32_t* d_len, int Sn, int Lmax, int Qmax, float dist_scale, double* d_quat,
                        double* d_trans, double* d_scale, void* stream) {
    if (!d_heads || !d_T || !d_win0 || !d_q0 || !d_slam || !d_len || !d_quat || !d_trans || !d_scale || Sn < 1 || window < 1 ||
        Lmax < 1 || Qmax < 1)
        return fail(EGOEGO_E_INVALID, "bad argument");
    s1_integrate_kernel<<<(Sn + 63) / 64, 64, 0, as_stream(stream)>>>(d_heads, window, (const int*)d_T, (const int*)d_win0, d_q0,
                                                                      d_slam, (const int*)d_len, Lmax, Qmax, dist_scale, d_quat,
                                                                      d_trans, d_scale, Sn);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EGOEGO_E_HIP, "launch failed: %s", hipGetErrorString(e));
    return 0;
}

int egoego_s1_gravity_apply(const float* d_rot, const float* d_trans, const int32_t* d_len, int Sn, int Lmax, const double* d_Rn,
                            const double* d_scale, const double* d_Ralign, const double* d_origin, double* d_pose, void* stream) {
    if (!d_rot || !d_trans || !d_len || !d_Rn || !d_scale || !d_Ralign || !d_origin || !d_pose || Sn < 1 || Lmax < 1)
        return fail(EGOEGO_E_INVALID, "bad argument");
    s1_gravity_apply_kernel<<<(Sn + 63) / 64, 64, 0, as_stream(stream)>>>(d_rot, d_trans, (const int*)d_len, Lmax, d_Rn, d_scale,
                                                                          d_Ralign, d_origin, d_pose, Sn);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EGOEGO_E_HIP, "launch failed: %s", hipGetErrorString(e));
    return 0;
}

int egoego_s1_gravity_align(const float* d_rot, const float* d_trans, const int32_t* d_len, int Sn, int Lmax, const float* d_normal,
                            const double* d_scale, const double* d_ref, const int32_t* d_ref_len, int Rmax, double* d_Rn,
                            double* d_Ralign, void* stream) {
    (void)d_rot;  // the alignment reads positions only
    if (!d_trans || !d_len || !d_normal || !d_scale || !d_ref || !d_ref_len || !d_Rn || !d_Ralign || Sn < 1 || Lmax < 1 || Rmax < 1)
        return fail(EGOEGO_E_INVALID, "bad argument");
    s1_gravity_align_kernel<<<Sn, 64, 0, as_stream(stream)>>>(d_trans, (const int*)d_len, Lmax, d_normal, d_scale, d_ref,
                                                              (const int*)d_ref_len, Rmax, d_Rn, d_Ralign);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EGOEGO_E_HIP, "launch failed: %s", hipGetErrorString(e));
    return 0;
}

int egoego_s1_head_pose_metrics(const double* d_pred, const double* d_gt, const int32_t* d_lengths, int Bn, int Tmax, double* d_out,
                                void* stream) {
    if (!d_pred || !d_gt || !d_lengths || !d_out || Bn < 1 || Tmax < 1) return fail(EGOEGO_E_INVALID, "bad argument");
    s1_head_pose_metrics_kernel<<<Bn, 64, 0, as_stream(stream)>>>(d_pred, d_gt, (const int*)d_lengths, Tmax, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EGOEGO_E_HIP, "launch failed: %s", hipGetErrorString(e));
    return 0;
}

}  // extern "C"
