// flow_cnn.hip — context, weight packing, workspace and the C ABI (include/egoego_hip.h, egoego_flow_*) of the optical-flow
// ResNet-18 feature extractor (egoego/model/resnet.py = RN).  Kernels: flow_cnn.h.  Nothing here touches another code path.
#include <math.h>

#include "host_util.h"
#include "flow_cnn.h"

using namespace fcnn;

static constexpr int N_CONV = 20;
static constexpr int IMG = 224;
static constexpr int FEAT = 512;
static constexpr int DEFAULT_CHUNK = 256;
// per-frame floats of one block buffer (the largest block activation, 56 x 56 x 64); the stem's output [112][112][64] is four
static constexpr size_t BUF_FLOATS = (size_t)56 * 56 * 64;
static constexpr int N_BUF = 5;  // buffers 0-3 hold the stem output, 4 the pooled stem; afterwards the blocks use all five
static const int STAGE_HW[5] = {56, 56, 28, 14, 7};
static const int STAGE_C[5] = {64, 64, 128, 256, 512};

// one packed convolution: shape and device planes
struct FConv {
    int Cin, Cout, KH, KW, stride, pad, K16;
    const __bf16* hi;
    const __bf16* lo;
    const float* scale;
    const float* shift;
};

struct egoego_flow_ctx {
    int device, chunk;
    bool loaded;
    DevMem mem;
    FConv conv[N_CONV];
    FConv fc;
};

// The reference's conv weight (Cout, cin_src, KH, KW) -> [Cout][kh][kw][Cin] (only the first Cin input channels) as hi / lo
// fragment-tiled planes with K padded to a multiple of 32; scale / shift from the BatchNorm (or the fc's bias with scale 1).
static int pack_conv(egoego_flow_ctx* c, const float* w, int Cout, int cin_src, int Cin, int KH, int KW, int stride, int pad,
                     const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var, const float* bias, FConv& out) {
    const int K = KH * KW * Cin, Kp = (K + 31) / 32 * 32, K16 = Kp / 16;
    std::vector<float> tmp;
    if (int rc = fetch(w, (size_t)Cout * cin_src * KH * KW, tmp)) return rc;
    std::vector<uint16_t> hi((size_t)Cout * Kp, 0), lo((size_t)Cout * Kp, 0);
    for (int co = 0; co < Cout; ++co)
        for (int kh = 0; kh < KH; ++kh)
            for (int kw = 0; kw < KW; ++kw)
                for (int ci = 0; ci < Cin; ++ci) {
                    const float v = tmp[(((size_t)co * cin_src + ci) * KH + kh) * KW + kw];
                    const int k = (kh * KW + kw) * Cin + ci;
                    split_store(hi, lo, tiled_index(co, k, K16), v);
                }
    std::vector<float> sc(Cout), sh(Cout);
    if (bias) {
        if (int rc = fetch(bias, Cout, tmp)) return rc;
        for (int i = 0; i < Cout; ++i) {
            sc[i] = 1.0f;
            sh[i] = tmp[i];
        }
    } else {
        std::vector<float> g, b, m, v;
        if (int rc = fetch(bn_w, Cout, g)) return rc;
        if (int rc = fetch(bn_b, Cout, b)) return rc;
        if (int rc = fetch(bn_mean, Cout, m)) return rc;
        if (int rc = fetch(bn_var, Cout, v)) return rc;
        for (int i = 0; i < Cout; ++i) {
            const double s = (double)g[i] / sqrt((double)v[i] + 1e-5);
            sc[i] = (float)s;
            sh[i] = (float)((double)b[i] - (double)m[i] * s);
        }
    }
    out.Cin = Cin; out.Cout = Cout; out.KH = KH; out.KW = KW; out.stride = stride; out.pad = pad; out.K16 = K16;
    const uint16_t *dh, *dl;
    if (int rc = c->mem.upload(hi, &dh)) return rc;
    if (int rc = c->mem.upload(lo, &dl)) return rc;
    if (int rc = c->mem.upload(sc, &out.scale)) return rc;
    if (int rc = c->mem.upload(sh, &out.shift)) return rc;
    out.hi = (const __bf16*)dh;
    out.lo = (const __bf16*)dl;
    return 0;
}

static size_t ws_bytes(const egoego_flow_ctx* c, int n) {
    const size_t F = (size_t)(n < c->chunk ? n : c->chunk);
    return F * (N_BUF * BUF_FLOATS + FEAT) * sizeof(float);
}

// y = act(BN(conv(x)) [+ res]) over F frames of H x W; returns the launch's own error
static hipError_t launch_conv(const FConv& cv, const float* x, float* y, const float* res, int F, int H, int W, bool relu, bool stem,
                        hipStream_t s) {
    ConvArgs a;
    a.x = x; a.y = y; a.res = res; a.whi = cv.hi; a.wlo = cv.lo; a.scale = cv.scale; a.shift = cv.shift;
    a.H = H; a.W = W; a.Cin = cv.Cin;
    a.OH = (H + 2 * cv.pad - cv.KH) / cv.stride + 1;
    a.OW = (W + 2 * cv.pad - cv.KW) / cv.stride + 1;
    a.Cout = cv.Cout; a.KH = cv.KH; a.KW = cv.KW; a.stride = cv.stride; a.pad = cv.pad;
    a.M = F * a.OH * a.OW;
    a.K16 = cv.K16;
    a.relu = relu ? 1 : 0;
    const int mt = (a.M + BM - 1) / BM;
    if (stem) flow_conv_kernel<1, true><<<dim3(mt, cv.Cout / 64), dim3(256), 0, s>>>(a);
    else if (cv.Cout % 128 == 0) flow_conv_kernel<2, false><<<dim3(mt, cv.Cout / 128), dim3(256), 0, s>>>(a);
    else flow_conv_kernel<1, false><<<dim3(mt, cv.Cout / 64), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

#define FL_LAUNCH(expr)                                                                                                \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            return fail(EGOEGO_E_HIP, "flow-CNN launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static int pack_weights(egoego_flow_ctx* c, const egoego_flow_weights* w) {
    int i = 0;
    auto conv = [&](int cin_src, int cin, int cout, int k, int stride, int pad) -> int {
        const int j = i++;
        return pack_conv(c, w->conv_w[j], cout, cin_src, cin, k, k, stride, pad, w->bn_w[j], w->bn_b[j], w->bn_mean[j],
                         w->bn_var[j], nullptr, c->conv[j]);
    };
    if (int r = conv(3, 2, 64, 7, 2, 3)) return r;  // the zero third input channel is dropped
    int cin = 64;
    for (int l = 0; l < 4; ++l) {
        const int cout = 64 << l;
        for (int b = 0; b < 2; ++b) {
            const int stride = (l > 0 && b == 0) ? 2 : 1;
            if (int r = conv(b == 0 ? cin : cout, b == 0 ? cin : cout, cout, 3, stride, 1)) return r;
            if (int r = conv(cout, cout, cout, 3, 1, 1)) return r;
            if (l > 0 && b == 0)
                if (int r = conv(cin, cin, cout, 1, 2, 0)) return r;
        }
        cin = cout;
    }
    return pack_conv(c, w->fc_w, FEAT, FEAT, FEAT, 1, 1, 1, 0, nullptr, nullptr, nullptr, nullptr, w->fc_b, c->fc);
}

extern "C" {

const char* egoego_flow_last_error(void) { return last_err.c_str(); }

int egoego_flow_ctx_create(int device, int chunk_frames, egoego_flow_ctx** out) {
    if (!out) return fail(EGOEGO_E_INVALID, "NULL argument");
    *out = nullptr;
    if (chunk_frames < 0 || chunk_frames > 4096) return fail(EGOEGO_E_INVALID, "chunk_frames %d: 0..4096 accepted", chunk_frames);
    if (int rc = check_device(device)) return rc;
    egoego_flow_ctx* c = new egoego_flow_ctx();
    c->device = device;
    c->chunk = chunk_frames ? chunk_frames : DEFAULT_CHUNK;
    c->loaded = false;
    *out = c;
    return 0;
}

void egoego_flow_ctx_destroy(egoego_flow_ctx* c) { destroy_ctx(c); }

int egoego_flow_load_weights(egoego_flow_ctx* c, const egoego_flow_weights* w, void* stream) {
    if (!c || !w) return fail(EGOEGO_E_INVALID, "NULL argument");
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

size_t egoego_flow_workspace_bytes(const egoego_flow_ctx* c, int n_frames) {
    if (!c || n_frames < 1) {
        fail(EGOEGO_E_INVALID, "n_frames must be >= 1");
        return 0;
    }
    return ws_bytes(c, n_frames);
}

int egoego_flow_features(egoego_flow_ctx* c, const float* d_flow, int N, float* d_out, float* d_stages, void* d_ws, size_t ws_n,
                         void* stream) {
    if (!c || !d_flow || !d_out) return fail(EGOEGO_E_INVALID, "NULL argument");
    if (!c->loaded) return fail(EGOEGO_E_STATE, "weights not loaded");
    if (N < 1) return fail(EGOEGO_E_INVALID, "n_frames must be >= 1");
    if (int rc = check_workspace(d_ws, ws_n, ws_bytes(c, N))) return rc;
    if (((uintptr_t)d_flow & 7) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_stages & 15))
        return fail(EGOEGO_E_INVALID, "d_flow must be 8-byte aligned, d_out and d_stages 16-byte aligned");
    DeviceGuard dev;
    if (int rc = dev.enter(c->device)) return rc;
    // every launch below is checked on its own; an error some earlier, unrelated call left pending is not ours to report
    (void)hipGetLastError();
    hipStream_t s = as_stream(stream);
    const int chunk = N < c->chunk ? N : c->chunk;
    float* ws = (float*)d_ws;
    float* buf[N_BUF];
    for (int i = 0; i < N_BUF; ++i) buf[i] = ws + (size_t)i * chunk * BUF_FLOATS;
    float* pooled = ws + (size_t)N_BUF * chunk * BUF_FLOATS;
    size_t stage_off[5], off = 0;
    for (int i = 0; i < 5; ++i) {
        stage_off[i] = off;
        off += (size_t)N * STAGE_HW[i] * STAGE_HW[i] * STAGE_C[i];
    }
    for (int f0 = 0; f0 < N; f0 += chunk) {  // one chunk of F frames from frame f0
        const int F = N - f0 < chunk ? N - f0 : chunk;
        auto stage = [&](int i, const float* src) -> int {
            if (!d_stages) return 0;
            const size_t per = (size_t)STAGE_HW[i] * STAGE_HW[i] * STAGE_C[i];
            HIP_TRY(hipMemcpyAsync(d_stages + stage_off[i] + (size_t)f0 * per, src, (size_t)F * per * sizeof(float),
                                   hipMemcpyDeviceToDevice, s));
            return 0;
        };
        // stem: conv1 + bn1 + ReLU into buffers 0-3 (one [F][112][112][64] array), max-pool into buffer 4
        FL_LAUNCH(launch_conv(c->conv[0], d_flow + (size_t)f0 * IMG * IMG * 2, buf[0], nullptr, F, IMG, IMG, true, true, s));
        {
            const size_t n = (size_t)F * 56 * 56 * 16;
            flow_maxpool_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(buf[0], buf[4], F, 112, 112, 64, 56, 56);
            FL_LAUNCH(hipGetLastError());
        }
        if (int rc = stage(0, buf[4])) return rc;
        int cur = 4, hw = 56, ci = 1;
        for (int l = 0; l < 4; ++l) {
            for (int b = 0; b < 2; ++b) {
                int fr[N_BUF - 1], k = 0;
                for (int i = 0; i < N_BUF; ++i)
                    if (i != cur) fr[k++] = i;
                const FConv& c1 = c->conv[ci++];
                const FConv& c2 = c->conv[ci++];
                const bool ds = l > 0 && b == 0;
                const int ohw = (hw + 2 - 3) / c1.stride + 1;
                float* X = buf[cur];
                float* T = buf[fr[0]];
                float* Y = buf[fr[1]];
                const float* id = X;
                FL_LAUNCH(launch_conv(c1, X, T, nullptr, F, hw, hw, true, false, s));
                if (ds) {
                    FL_LAUNCH(launch_conv(c->conv[ci++], X, buf[fr[2]], nullptr, F, hw, hw, false, false, s));
                    id = buf[fr[2]];
                }
                FL_LAUNCH(launch_conv(c2, T, Y, id, F, ohw, ohw, true, false, s));
                cur = fr[1];
                hw = ohw;
            }
            if (int rc = stage(l + 1, buf[cur])) return rc;
        }
        {
            const int n = F * FEAT;
            flow_avgpool_kernel<<<(n + 255) / 256, 256, 0, s>>>(buf[cur], pooled, F, hw * hw, FEAT);
            FL_LAUNCH(hipGetLastError());
        }
        FL_LAUNCH(launch_conv(c->fc, pooled, d_out + (size_t)f0 * FEAT, nullptr, F, 1, 1, false, false, s));
    }
    return 0;
}

}  // extern "C"
