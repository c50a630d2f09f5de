// flow_cnn.h — kernels of the optical-flow ResNet-18 feature extractor (egoego/model/resnet.py, torchvision resnet18 in eval mode)
// on split-bf16 MFMAs.
//
// Every convolution (and the final fc, as a 1 x 1 convolution of a 1 x 1 image) is one implicit GEMM:
//   M = frames x output pixels (row m = output pixel m % (OH * OW) of frame m / (OH * OW)),  N = output channels,
//   K = taps x input channels, k = (kh * KW + kw) * Cin + c (the weights are packed as [Cout][kh][kw][Cin], K padded to 32).
// Activations are fp32 NHWC: a 32-deep K step is one tap x 32 consecutive channels, 128 contiguous bytes of one input pixel.
// The stem reads the raw flow [N][224][224][2] directly (Cin = 2: the reference's all-zero third channel adds exact zeros and is
// dropped, K = 98 -> 128).
//
// One workgroup (4 waves, 2 x 2) computes a 128 x BN tile (BN = 64 or 128; a wave 64 x BN/2, i.e. 2 x BN/64 MFMA tiles).  Per
// 32-deep K step the A tile (128 rows x 32 k, fp32) and the B tile (BN rows of the packed weights, hi and lo) are staged through
// LDS, double buffered: the global loads of step s + 1 are issued before the MFMAs of step s and written to the other buffer
// after them, one barrier per step.  The A tile is split into hi / lo bf16 planes once, when it is written to LDS, and laid out
// fragment-tiled (common.h): every fragment read is one lane-linear ds_read_b128.
//
// Epilogue (fp32): v = acc * scale[n] + shift[n] (BatchNorm with its running statistics, folded at load into a per-channel
// scale = w / sqrt(var + 1e-5) and shift = b - mean * scale, computed in fp64 and rounded once; fc: scale 1, shift = bias),
// then + residual, then ReLU.  ReLU and the max-pool carry a NaN on, as the reference's F.relu and max_pool2d do (fmaxf
// returns its other operand): a non-finite flow pixel ends as non-finite features of its frame, not as plausible numbers.
// max_nan below is IEEE 754-2019 maximum, one v_maximum3_f32 on gfx950: fmaxf's bits for numbers (+0 above -0), NaN for a NaN.
//
// Bit-identity: an output element is one accumulator lane of one wave; its K loop runs in the same order whatever tile, chunk or
// position its row falls in, and the rows of an MFMA do not interact.  A frame's features therefore do not depend on the others.
#pragma once
#include "common.h"

// Ablation builds only (tools/flow_cnn_ablation.py; the product library is built without it): a bit mask that removes parts of
// flow_conv_kernel's main loop to time what is left.  The results of such a build are wrong by design.
//   1: no MFMAs (one VALU op per product step keeps the fragment reads alive)   2: no global loads (zeros are staged)
//   4: no LDS staging writes   8: no barrier in the K loop
#ifndef EGOEGO_FLOW_ABLATE
#define EGOEGO_FLOW_ABLATE 0
#endif

namespace fcnn {

EG_D float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }

static constexpr int BM = 128;   // rows (output pixels) per workgroup
static constexpr int BK = 32;    // K per staged step
static constexpr int A_PLANE = BM * BK;  // bf16 per plane of one A buffer (8 KiB)

struct ConvArgs {
    const float* x;      // [F][H][W][Cin] fp32 NHWC
    float* y;            // [F][OH][OW][Cout]
    const float* res;    // nullable: added after the BatchNorm affine, same layout as y
    const __bf16* whi;   // [Cout/32][K16][2][32][8] fragment-tiled hi plane
    const __bf16* wlo;
    const float* scale;  // [Cout]
    const float* shift;  // [Cout]
    int H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, M, K16, relu;
};

// 16 consecutive K values of row (f, oh, ow) starting at K index kk (kk % 16 == 0) -> v.  Zero outside the image and past M.
template <bool STEM>
EG_D void load_a16(const ConvArgs& a, int f, int oh, int ow, bool mok, int kk, float v[16]) {
    if (STEM) {
        // Cin = 2, 7 x 7 taps: eight (tap, 2 channels) pairs; taps >= 49 are the K padding
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int tap = (kk >> 1) + i;
            const int kh = tap / 7, kw = tap - 7 * (tap / 7);
            const int ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
            const bool ok = mok && tap < 49 && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
            float2 p = make_float2(0.f, 0.f);
            if (ok) p = *(const float2*)(a.x + (((size_t)f * a.H + ih) * a.W + iw) * 2);
            v[2 * i] = p.x;
            v[2 * i + 1] = p.y;
        }
    } else {
        const int tap = kk / a.Cin, c0 = kk - tap * a.Cin;
        const int kh = tap / a.KW, kw = tap - kh * a.KW;
        const int ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
        const bool ok = mok && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        if (ok) {
            const float4* p = (const float4*)(a.x + (((size_t)f * a.H + ih) * a.W + iw) * a.Cin + c0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 q = p[i];
                v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = 0.f;
        }
    }
}

// LDS per buffer (u32x4 units): A hi | A lo (A_PLANE / 8 each), then B hi | B lo (BN * BK / 8 each).
template <int TN>
struct Smem {
    static constexpr int BN = 64 * TN;
    static constexpr int A16 = A_PLANE / 8;   // 512
    static constexpr int B16 = BN * BK / 8;   // 256 * TN
    static constexpr int BUF = 2 * A16 + 2 * B16;
};

template <int TN, bool STEM>
__global__ __launch_bounds__(256) void flow_conv_kernel(ConvArgs a) {
    using SM = Smem<TN>;
    constexpr int BN = SM::BN;
    constexpr int NB = TN * 2;  // 16-byte B chunks each thread stages per step
    __shared__ u32x4 lds[2 * SM::BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int nsteps = a.K16 / 2;

    // this thread's A row and k half
    const int ar = tid & (BM - 1), aj = tid >> 7;
    const int am = m0 + ar;
    const bool mok = am < a.M;
    const int P = a.OH * a.OW;
    const int amc = mok ? am : 0;
    const int af = amc / P, ap = amc - af * P;
    const int aoh = ap / a.OW, aow = ap - (ap / a.OW) * a.OW;
    const int a_slot = ((ar >> 5) * 2 + aj) * 2 * 32 + (ar & 31);  // + 32 * hf

    // this thread's B chunks: chunk c = tid + 256 i -> plane c / (BN * 4), block (c % (BN * 4)) / 128, 16-byte piece c % 128
    const u32x4* wsrc[NB];
    int bdst[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int c = tid + 256 * i;
        const int plane = c / (BN * 4), rem = c % (BN * 4), blk = rem >> 7, off = rem & 127;
        const __bf16* base = plane ? a.wlo : a.whi;
        wsrc[i] = (const u32x4*)(base + ((size_t)(n0 / 32 + blk) * a.K16) * 512) + off;
        bdst[i] = 2 * SM::A16 + plane * SM::B16 + blk * 128 + off;
    }

    float av[16];
    u32x4 bv[NB];
    auto gload = [&](int s) {
        if (EGOEGO_FLOW_ABLATE & 2) {
#pragma unroll
            for (int i = 0; i < 16; ++i) av[i] = 0.f;
#pragma unroll
            for (int i = 0; i < NB; ++i) bv[i] = u32x4{0u, 0u, 0u, 0u};
            return;
        }
        load_a16<STEM>(a, af, aoh, aow, mok, s * BK + aj * 16, av);
#pragma unroll
        for (int i = 0; i < NB; ++i) bv[i] = wsrc[i][(size_t)s * 128];  // 2 k16 blocks = 1024 bf16 = 128 chunks per step
    };
    auto lstore = [&](int buf) {
        if (EGOEGO_FLOW_ABLATE & 4) return;
        u32x4* L = lds + buf * SM::BUF;
        u32x4 h0, l0, h1, l1;
        split8(av, h0, l0);
        split8(av + 8, h1, l1);
        L[a_slot] = h0;
        L[a_slot + 32] = h1;
        L[SM::A16 + a_slot] = l0;
        L[SM::A16 + a_slot + 32] = l1;
#pragma unroll
        for (int i = 0; i < NB; ++i) L[bdst[i]] = bv[i];
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    gload(0);
    lstore(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) gload(s + 1);
        const u32x4* L = lds + buf * SM::BUF;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            u32x4 ah[2], al[2], bh[TN], bl[TN];
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
                const int idx = ((wm * 2 + tm) * 2 + j) * 64 + hf * 32 + (lane & 31);
                ah[tm] = L[idx];
                al[tm] = L[SM::A16 + idx];
            }
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int idx = 2 * SM::A16 + ((wn * TN + tn) * 2 + j) * 64 + hf * 32 + (lane & 31);
                bh[tn] = L[idx];
                bl[tn] = L[SM::B16 + idx];
            }
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    if (EGOEGO_FLOW_ABLATE & 1)
                        acc[tm][tn][j] += __builtin_bit_cast(float, (ah[tm][0] ^ al[tm][1] ^ bh[tn][2] ^ bl[tn][3]) & 0x3fffffffu);
                    else
                        acc[tm][tn] = mfma3(ah[tm], al[tm], bh[tn], bl[tn], acc[tm][tn]);
                }
        }
        if (s + 1 < nsteps) lstore(buf ^ 1);
        if (!(EGOEGO_FLOW_ABLATE & 8)) __syncthreads();
    }

#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int n = n0 + (wn * TN + tn) * 32 + (lane & 31);
        const float sc = a.scale[n], sh = a.shift[n];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + tm * 32 + mfma32_row(r, hf);
                if (m >= a.M) continue;
                const size_t o = (size_t)m * a.Cout + n;
                float v = acc[tm][tn][r] * sc + sh;
                if (a.res) v = v + a.res[o];
                if (a.relu) v = max_nan(v, 0.f);
                a.y[o] = v;
            }
    }
}

// 3 x 3 / 2 max-pool, pad 1 (out-of-image taps skipped, as PyTorch's -inf padding): [F][H][W][C] -> [F][OH][OW][C], 4 channels
// per thread.
__global__ void flow_maxpool_kernel(const float* x, float* y, int F, int H, int W, int C, int OH, int OW) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int C4 = C / 4;
    const size_t total = (size_t)F * OH * OW * C4;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const size_t pix = i / C4;
    const int ow = (int)(pix % OW), oh = (int)((pix / OW) % OH);
    const int f = (int)(pix / ((size_t)OW * OH));
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = oh * 2 - 1 + kh;
        if (ih < 0 || ih >= H) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int iw = ow * 2 - 1 + kw;
            if (iw < 0 || iw >= W) continue;
            const float4 v = *(const float4*)(x + (((size_t)f * H + ih) * W + iw) * C + 4 * c4);
            m.x = max_nan(m.x, v.x); m.y = max_nan(m.y, v.y); m.z = max_nan(m.z, v.z); m.w = max_nan(m.w, v.w);
        }
    }
    *(float4*)(y + pix * C + 4 * c4) = m;
}

// Global average pool: [F][P][C] -> [F][C], pixels summed in order 0 .. P-1 in fp32, then divided by P.
__global__ void flow_avgpool_kernel(const float* x, float* y, int F, int P, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * C) return;
    const int f = i / C, c = i - f * C;
    const float* p = x + (size_t)f * P * C + c;
    float s = 0.f;
    for (int q = 0; q < P; ++q) s += p[(size_t)q * C];
    y[i] = s / (float)P;
}

}  // namespace fcnn
