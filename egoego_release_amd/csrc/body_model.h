// body_model.h — kernels of the SMPL-H body model (linear-blend skinning): what the reference reaches through
// human_body_prior's BodyModel in run_smpl_model (egoego/data/amass_diffusion_dataset.py:15-81), written from the definition.
//
//   v_shaped = v_template + shapedirs . betas                       per sequence, fp32                   (body_shape_kernel)
//   J        = J_template + J_shapedirs . betas                     per sequence, fp32                   (body_shape_kernel)
//   R_j = Rodrigues(pose_j),  feat = (R_j - I), j = 1..51           per frame, fp64, one thread a frame  (body_frame_kernel)
//   G_0 = [R_0 | J_0],  G_j = G_parent(j) . [R_j | J_j - J_parent(j)];  A_j = G_j . [I | -J_j];  Jtr_j = t(G_j) + trans
//   v = (sum_k w_k A_jk) . (v_shaped + posedirs . feat) + trans     split-bf16 GEMM + fused skinning     (body_skin_kernel)
//
// The GEMM: M = frames, N = 3 V, K = 9 x 51 = 459 -> 480 (k = 9 (j - 1) + 3 row + col of R_j - I; 9 x 21 = 189 -> 192 when the
// caller gives no hand pose: the skipped terms are exact zeros and the K order is otherwise the same, so both calls agree bit
// for bit).  Both operands are fragment-tiled hi / lo bf16 planes (common.h).  The packed N dimension is ordered
// n' = 96 (v / 32) + 32 c + v % 32: the three 32-column blocks of a group of 32 vertices are its x, y and z, so the lane that
// owns column v % 32 holds all three pose offsets of its vertex for the 16 frames of its accumulator rows, and the skinning
// epilogue needs no cross-lane traffic.  A wave computes TM x 3 MFMA tiles (32 TM frames of one vertex group); the four waves
// of a workgroup take four consecutive vertex groups.  No operand is shared between the waves of a workgroup (the features
// are, but they are small and stay in the vector cache), so the fragments go from global memory straight to registers, lane
// linear 16 bytes, one K step ahead of the MFMAs that use them; there is no LDS and no barrier.
//
// The metre-sized v_shaped is added in fp32 in the epilogue (through the split it would cost ~1e-5 m; the centimetre-sized pose
// offsets lose ~1e-7 m).  The pose offsets never go to memory (except into the optional debug output).
//
// Bit-identity: an output vertex is one accumulator lane of one wave; its K loop and its epilogue run in the same order whatever
// tile, chunk or position its frame falls in, and the rows of an MFMA do not interact.
#pragma once
#include "common.h"
#include "quat_f64.h"

namespace bodym {

static constexpr int NJ = 52;             // SMPL-H joints
static constexpr int K_FULL = 9 * (NJ - 1);  // 459
static constexpr int K_BODY = 9 * 21;        // 189: the 21 body joints of a 22-joint pose
static constexpr int PK16 = (K_FULL + 31) / 32 * 2;  // 30: K/16 of the packed posedirs planes

// out[s][n] = base[n] + sum_b dirs[n][b] * betas[s][b], b ascending (n over V * 3 or 52 * 3)
__global__ void body_shape_kernel(const float* base, const float* dirs, const float* betas, int N, int nb, int S, float* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)N * S) return;
    const int s = (int)(i / N), n = (int)(i - (size_t)s * N);
    float acc = base[n];
    for (int b = 0; b < nb; ++b) acc = fmaf(dirs[(size_t)n * nb + b], betas[(size_t)s * nb + b], acc);
    out[i] = acc;
}

struct FrameArgs {
    const float* root;    // [F][3] axis-angle
    const float* body;    // [F][63]
    const float* hand;    // [F][90] or nullptr (identity rotations)
    const float* trans;   // [F][3]
    const int* seq;       // [F] row of J
    const float* J;       // [S][52][3]
    const int* parents;   // [52], parents[j] < j
    __bf16* fhi;          // [ceil(F / 32)][K16][2][32][8] pose features
    __bf16* flo;
    float* A;             // [F][52][12] rows of [R | t]
    float* joints;        // [F][52][3]
    int F, S, K16;
};

__global__ void body_frame_kernel(FrameArgs a) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    // (the rows that pad the last 32-frame tile are not written: the MFMAs of that tile read whatever the workspace holds there,
    // which is harmless because the rows of an MFMA do not interact and those rows are never stored)
    if (f >= a.F) return;
    int s = a.seq[f];
    s = s < 0 ? 0 : (s >= a.S ? a.S - 1 : s);
    const float* Js = a.J + (size_t)s * NJ * 3;
    const double tx = a.trans[3 * (size_t)f], ty = a.trans[3 * (size_t)f + 1], tz = a.trans[3 * (size_t)f + 2];
    const int Kp = a.K16 * 16;
    double G[NJ][12];
    for (int j = 0; j < NJ; ++j) {
        double x = 0.0, y = 0.0, z = 0.0;
        const float* p = j == 0 ? a.root + 3 * (size_t)f
                                : (j < 22 ? a.body + 63 * (size_t)f + 3 * (j - 1) : (a.hand ? a.hand + 90 * (size_t)f + 3 * (j - 22) : nullptr));
        if (p) {
            x = p[0]; y = p[1]; z = p[2];
        }
        double R[9];
        rodrigues(x, y, z, R);
        if (j >= 1 && 9 * j <= Kp) {  // this joint's nine features lie inside the K this call runs
            for (int e = 0; e < 9; ++e) {
                const float v = (float)(R[e] - ((e & 3) == 0 ? 1.0 : 0.0));
                __bf16 h, l;
                split_bf16(v, h, l);
                const size_t idx = tiled_index(f, 9 * (j - 1) + e, a.K16);
                a.fhi[idx] = h;
                a.flo[idx] = l;
            }
        }
        const double jx = Js[3 * j], jy = Js[3 * j + 1], jz = Js[3 * j + 2];
        double* g = G[j];
        if (j == 0) {
            for (int r = 0; r < 3; ++r) {
                g[4 * r] = R[3 * r]; g[4 * r + 1] = R[3 * r + 1]; g[4 * r + 2] = R[3 * r + 2];
            }
            g[3] = jx; g[7] = jy; g[11] = jz;
        } else {
            const int pj = a.parents[j];
            const double* gp = G[pj];
            const double rx = jx - Js[3 * pj], ry = jy - Js[3 * pj + 1], rz = jz - Js[3 * pj + 2];
            for (int r = 0; r < 3; ++r) {
                const double p0 = gp[4 * r], p1 = gp[4 * r + 1], p2 = gp[4 * r + 2];
                g[4 * r] = p0 * R[0] + p1 * R[3] + p2 * R[6];
                g[4 * r + 1] = p0 * R[1] + p1 * R[4] + p2 * R[7];
                g[4 * r + 2] = p0 * R[2] + p1 * R[5] + p2 * R[8];
                g[4 * r + 3] = p0 * rx + p1 * ry + p2 * rz + gp[4 * r + 3];
            }
        }
        float* jo = a.joints + ((size_t)f * NJ + j) * 3;
        jo[0] = (float)(g[3] + tx); jo[1] = (float)(g[7] + ty); jo[2] = (float)(g[11] + tz);
        float* A = a.A + ((size_t)f * NJ + j) * 12;
        for (int r = 0; r < 3; ++r) {
            A[4 * r] = (float)g[4 * r]; A[4 * r + 1] = (float)g[4 * r + 1]; A[4 * r + 2] = (float)g[4 * r + 2];
            A[4 * r + 3] = (float)(g[4 * r + 3] - (g[4 * r] * jx + g[4 * r + 1] * jy + g[4 * r + 2] * jz));
        }
    }
    // the K padding (and, without a hand pose, nothing else) is zero
    const int Kreal = a.hand ? K_FULL : K_BODY;
    for (int k = Kreal; k < Kp; ++k) {
        const size_t idx = tiled_index(f, k, a.K16);
        a.fhi[idx] = (__bf16)0.0f;
        a.flo[idx] = (__bf16)0.0f;
    }
}

struct SkinArgs {
    const u32x4* fhi;        // pose features, [MT][K16][64] 16-byte pieces
    const u32x4* flo;
    const u32x4* phi;        // posedirs, [3 VG][PK16][64]
    const u32x4* plo;
    const float* v_shaped;   // [S][V][3]
    const int* seq;          // [F]
    const float* A;          // [F][52][12]
    const float* trans;      // [F][3]
    const int* skin_joint;   // [nw][V]
    const float* skin_weight;
    float* verts;            // [F][V][3]
    float* offsets;          // [F][V][3] or nullptr: posedirs . feat (debug)
    int F, S, V, VG, MT, K16, nw;
};

template <int TM>
__global__ __launch_bounds__(256) void body_skin_kernel(SkinArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, hf = lane >> 5, col = lane & 31;
    const int vg = blockIdx.y * 4 + (tid >> 6);
    if (vg >= a.VG) return;  // no barrier below
    const int mt0 = blockIdx.x * TM;

    const u32x4 *pa_h[TM], *pa_l[TM], *pb_h[3], *pb_l[3];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int mt = mt0 + tm < a.MT ? mt0 + tm : a.MT - 1;  // a tile past the end repeats the last one; its rows, like the unwritten feature rows that pad the last tile, are not stored
        pa_h[tm] = a.fhi + (size_t)mt * a.K16 * 64 + lane;
        pa_l[tm] = a.flo + (size_t)mt * a.K16 * 64 + lane;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pb_h[c] = a.phi + (size_t)(vg * 3 + c) * PK16 * 64 + lane;
        pb_l[c] = a.plo + (size_t)(vg * 3 + c) * PK16 * 64 + lane;
    }

    f32x16 acc[TM][3];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][c][r] = 0.f;

    u32x4 ah[TM], al[TM], bh[3], bl[3], nah[TM], nal[TM], nbh[3], nbl[3];
    auto gload = [&](int k, u32x4* xah, u32x4* xal, u32x4* xbh, u32x4* xbl) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            xah[tm] = pa_h[tm][(size_t)k * 64];
            xal[tm] = pa_l[tm][(size_t)k * 64];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xbh[c] = pb_h[c][(size_t)k * 64];
            xbl[c] = pb_l[c][(size_t)k * 64];
        }
    };
    gload(0, ah, al, bh, bl);
    for (int k = 0; k < a.K16; ++k) {
        if (k + 1 < a.K16) gload(k + 1, nah, nal, nbh, nbl);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[tm][c] = mfma3(ah[tm], al[tm], bh[c], bl[c], acc[tm][c]);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            ah[tm] = nah[tm];
            al[tm] = nal[tm];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            bh[c] = nbh[c];
            bl[c] = nbl[c];
        }
    }

    // skinning: this lane's vertex, the 16 frames of each of its accumulator tiles
    const int v = vg * 32 + col;
    if (v >= a.V) return;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = (mt0 + tm) * 32 + mfma32_row(r, hf);
            if (m >= a.F) continue;
            const float ox = acc[tm][0][r], oy = acc[tm][1][r], oz = acc[tm][2][r];
            const size_t o = ((size_t)m * a.V + v) * 3;
            if (a.offsets) {
                a.offsets[o] = ox; a.offsets[o + 1] = oy; a.offsets[o + 2] = oz;
            }
            int s = a.seq[m];
            s = s < 0 ? 0 : (s >= a.S ? a.S - 1 : s);
            const float* vs = a.v_shaped + ((size_t)s * a.V + v) * 3;
            const float px = vs[0] + ox, py = vs[1] + oy, pz = vs[2] + oz;
            const float4* Af = (const float4*)(a.A + (size_t)m * NJ * 12);
            float4 t0 = make_float4(0.f, 0.f, 0.f, 0.f), t1 = t0, t2 = t0;
            for (int k = 0; k < a.nw; ++k) {
                const int j = a.skin_joint[(size_t)k * a.V + v];
                const float w = a.skin_weight[(size_t)k * a.V + v];
                const float4 a0 = Af[3 * j], a1 = Af[3 * j + 1], a2 = Af[3 * j + 2];
                t0.x = fmaf(w, a0.x, t0.x); t0.y = fmaf(w, a0.y, t0.y); t0.z = fmaf(w, a0.z, t0.z); t0.w = fmaf(w, a0.w, t0.w);
                t1.x = fmaf(w, a1.x, t1.x); t1.y = fmaf(w, a1.y, t1.y); t1.z = fmaf(w, a1.z, t1.z); t1.w = fmaf(w, a1.w, t1.w);
                t2.x = fmaf(w, a2.x, t2.x); t2.y = fmaf(w, a2.y, t2.y); t2.z = fmaf(w, a2.z, t2.z); t2.w = fmaf(w, a2.w, t2.w);
            }
            const float* tr = a.trans + 3 * (size_t)m;
            a.verts[o] = fmaf(t0.x, px, fmaf(t0.y, py, fmaf(t0.z, pz, t0.w))) + tr[0];
            a.verts[o + 1] = fmaf(t1.x, px, fmaf(t1.y, py, fmaf(t1.z, pz, t1.w))) + tr[1];
            a.verts[o + 2] = fmaf(t2.x, px, fmaf(t2.y, py, fmaf(t2.z, pz, t2.w))) + tr[2];
        }
    }
}

}  // namespace bodym
