// eval_metrics.h — the evaluation step of the reference on the device: forward kinematics (fk_smpl, amass_diffusion_dataset.py
// 265-293), determine_floor_height_and_contacts (utils/data_utils/process_amass_dataset.py:160-338) and compute_metrics_for_smpl
// (kinpoly/scripts/eval_metrics_imu_rec.py:66-107, 222-342 over kinpoly/relive/utils/metrics.py:15-24, 64-82), batched over
// sequences of different lengths.  Joint layout: 22 SMPL joints, z up.
//
//   eval_fk_kernel       one fp64 thread per frame; quaternions (w >= 0) and joints rounded once to fp32 (the fp64
//                        quaternion helpers: quat_f64.h).
//   eval_floor_kernel    one 1024-thread workgroup per sequence; everything between the joint read and the results lives in LDS.
//   eval_metrics_kernel  one 256-thread workgroup per (sample, ground truth) pair; fp64 accumulators, thread t owns frames
//                        t, t + 256, ... and the partial sums meet in a fixed shuffle / LDS order, so a sample's numbers depend
//                        on its own frames and length only: not on the batch, its position in it or the padded T.
//
// The floor kernel's seven steps, its thresholds, the contact joints and the LDS layout live in floor_common.h, which
// amass_prep.h's floor kernel shares.
#pragma once
#include "common.h"
#include "quat_f64.h"
#include "floor_common.h"

namespace evalm {

// ---------------------------------------------------------------- forward kinematics
struct FkArgs {
    const float* root;  // [N][3]
    const float* aa;    // [N][22][3] local axis-angle
    const float* rest;  // [22][3] rest-pose offsets
    float* quat;        // [N][22][4] (w, x, y, z)
    float* jpos;        // [N][22][3]
    int parents[NJ];
    int N;
};

__global__ void eval_fk_kernel(FkArgs a) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.N) return;
    const float* aa = a.aa + (size_t)f * NJ * 3;
    const double rx = a.root[3 * (size_t)f], ry = a.root[3 * (size_t)f + 1], rz = a.root[3 * (size_t)f + 2];
    QuatD gq[NJ];
    double gp[NJ][3];
    gq[0] = qd_from_aa(aa[0], aa[1], aa[2]);
    gp[0][0] = a.rest[0]; gp[0][1] = a.rest[1]; gp[0][2] = a.rest[2];
    for (int j = 1; j < NJ; ++j) {
        const int p = a.parents[j];
        const double off[3] = {a.rest[3 * j], a.rest[3 * j + 1], a.rest[3 * j + 2]};
        double r[3];
        qd_rotate(gq[p], off, r);
        gp[j][0] = r[0] + gp[p][0]; gp[j][1] = r[1] + gp[p][1]; gp[j][2] = r[2] + gp[p][2];
        gq[j] = qd_std(qd_mul(gq[p], qd_from_aa(aa[3 * j], aa[3 * j + 1], aa[3 * j + 2])));
    }
    float* qo = a.quat + (size_t)f * NJ * 4;
    float* po = a.jpos + (size_t)f * NJ * 3;
    for (int j = 0; j < NJ; ++j) {
        qo[4 * j] = (float)gq[j].w; qo[4 * j + 1] = (float)gq[j].x; qo[4 * j + 2] = (float)gq[j].y; qo[4 * j + 3] = (float)gq[j].z;
        po[3 * j] = (float)(gp[j][0] + rx); po[3 * j + 1] = (float)(gp[j][1] + ry); po[3 * j + 2] = (float)(gp[j][2] + rz);
    }
}

// eval_egoego.py:376-383: every joint of a sequence moves by minus the xy of joint `joint` in its first frame
__global__ void eval_shift_xy_kernel(float* jpos, int B, int T, int joint) {
    const size_t n = (size_t)B * T * NJ;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / ((size_t)T * NJ);
        // (the first frame's own `joint` is read by other threads while this one writes: take it last, from a copy)
        const float* h = jpos + (b * T * NJ + joint) * 3;
        const float hx = h[0], hy = h[1];
        if (i == b * T * NJ + joint) continue;
        jpos[3 * i] -= hx;
        jpos[3 * i + 1] -= hy;
    }
}
__global__ void eval_shift_xy_origin_kernel(float* jpos, int B, int T, int joint) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float* h = jpos + ((size_t)b * T * NJ + joint) * 3;
    h[0] -= h[0];
    h[1] -= h[1];
}

// eval_egoego.py:385, 402: root = joint 0 with the floor height taken off z
__global__ void eval_root_to_floor_kernel(const float* jpos, const float* floor_h, int B, int T, float* root) {
    const size_t n = (size_t)B * T;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float* p = jpos + i * NJ * 3;
        root[3 * i] = p[0];
        root[3 * i + 1] = p[1];
        root[3 * i + 2] = p[2] - floor_h[i / T];
    }
}

// eval_egoego.py:434-446: per group the first sample with the smallest value (strict <, as the reference's loop)
__global__ void eval_best_kernel(const double* table, int stride, int col, const int* group, int B, int n_groups, int* best) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += gridDim.x * blockDim.x) {
        int bi = -1;
        double bv = 0.0;
        for (int b = 0; b < B; ++b) {
            if ((group ? group[b] : 0) != g) continue;
            const double v = table[(size_t)b * stride + col];
            if (bi < 0 || v < bv) {
                bi = b;
                bv = v;
            }
        }
        best[g] = bi;
    }
}

// ---------------------------------------------------------------- floor height and contacts
struct FloorArgs {
    const float* jpos;    // [B][T][22][3]
    const int* lengths;   // [B] or nullptr (all T)
    float* floor_h;       // [B]
    float* offset_h;      // [B]
    float* contacts;      // [B][T][22]
    int* discard;         // [B]
    int* labels;          // [B][2 T] in compacted order, -2 past n_static; or nullptr
    int* n_static;        // [B]
    int* n_groups;        // [B]
    int B, T, size_thresh, cap;  // cap: power of two >= max(2 T, 64), fixes the LDS layout
};

// floor_common.h's floor_body on a padded batch: sequence b owns rows b T .. b T + lengths[b], every output is written for all T
__global__ void __launch_bounds__(FC_THREADS) eval_floor_kernel(FloorArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
    __shared__ float s_pair[2];
    __shared__ unsigned long long s_best;
    const int b = blockIdx.x, T = a.T;
    int L = a.lengths ? a.lengths[b] : T;
    L = L < 0 ? 0 : (L > T ? T : L);
    const FloorSeq q{a.jpos + (size_t)b * T * NJ * 3, L, a.size_thresh, a.contacts + (size_t)b * T * NJ, T,
                     a.labels ? a.labels + (size_t)b * 2 * T : nullptr, 2 * T,
                     a.floor_h + b, a.offset_h + b, a.discard + b, a.n_static + b, a.n_groups + b};
    floor_body<false>(q, floor_mem_lds(fc_lds, a.cap), s_pair, &s_best);
}

// ---------------------------------------------------------------- metrics
struct MetricArgs {
    const float* gt_quat;   // [B or 1][T][22][4]
    const float* gt_jpos;   // [B or 1][T][22][3]
    const float* pr_quat;   // [B][T][22][4]
    const float* pr_jpos;   // [B][T][22][3]
    const float* gt_floor;  // [B]
    const float* pr_floor;  // [B]
    const int* lengths;     // [B] or nullptr
    double* out;            // [B][N_METRICS]
    int B, T, gt_shared;
};

// quaternion_matrix (transformation.py:1346-1370): the rotation of q / |q|, identity below |q|^2 = 4 eps
EG_D void quat_matrix(const float* q4, double (&R)[9]) {
    double w = q4[0], x = q4[1], y = q4[2], z = q4[3];
    const double n = w * w + x * x + y * y + z * z;
    if (n < 8.881784197001252e-16) {
        R[0] = R[4] = R[8] = 1.0;
        R[1] = R[2] = R[3] = R[5] = R[6] = R[7] = 0.0;
        return;
    }
    const double s = sqrt(2.0 / n);
    w *= s; x *= s; y *= s; z *= s;
    R[0] = 1.0 - y * y - z * z; R[1] = x * y - z * w;       R[2] = x * z + y * w;
    R[3] = x * y + z * w;       R[4] = 1.0 - x * x - z * z; R[5] = y * z - x * w;
    R[6] = x * z - y * w;       R[7] = y * z + x * w;       R[8] = 1.0 - x * x - y * y;
}
// get_frobenious_norm / _rot_only (metrics.py:64-82) for rigid X, Y: X Y^-1 = [E | tx - E ty], E = Rx Ry^T
EG_D void pose_dist(const float* qp, const float* tp, const float* qg, const float* tg, double& full, double& rot, double& trans) {
    double Rp[9], Rg[9];
    quat_matrix(qp, Rp);
    quat_matrix(qg, Rg);
    double s = 0.0, te[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double acc = (double)tp[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double e = Rp[3 * r] * Rg[3 * c] + Rp[3 * r + 1] * Rg[3 * c + 1] + Rp[3 * r + 2] * Rg[3 * c + 2];
            const double d = (r == c ? 1.0 : 0.0) - e;
            s += d * d;
            acc -= e * (double)tg[c];
        }
        te[r] = acc;
    }
    rot = sqrt(s);
    full = sqrt(s + te[0] * te[0] + te[1] * te[1] + te[2] * te[2]);
    const double dx = (double)tp[0] - (double)tg[0], dy = (double)tp[1] - (double)tg[1], dz = (double)tp[2] - (double)tg[2];
    trans = sqrt(dx * dx + dy * dy + dz * dz);
}
// compute_foot_sliding_for_smpl (:222-262), one frame pair: ankles 7, 8 below 0.08, toes 10, 11 below 0.04
EG_D double foot_slide(const float* p0, const float* p1, double floor_h) {
    const int joint[4] = {7, 10, 8, 11};
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = joint[k];
        const double H = (k & 1) ? 0.04 : 0.08;
        const double z = (double)p0[3 * j + 2] - floor_h;
        if (z < H) {
            const double dx = (double)p1[3 * j] - (double)p0[3 * j], dy = (double)p1[3 * j + 1] - (double)p0[3 * j + 1];
            s += fabs(sqrt(dx * dx + dy * dy) * (2.0 - exp2(z / H)));
        }
    }
    return s;
}

__global__ void __launch_bounds__(MT_THREADS) eval_metrics_kernel(MetricArgs a) {
    __shared__ double red[MT_THREADS / 64][N_ACC];
    const int tid = threadIdx.x, b = blockIdx.x, T = a.T;
    int L = a.lengths ? a.lengths[b] : T;
    L = L < 0 ? 0 : (L > T ? T : L);
    const size_t gb = a.gt_shared ? 0 : (size_t)b * T;
    const float* GQ = a.gt_quat + gb * NJ * 4;
    const float* GP = a.gt_jpos + gb * NJ * 3;
    const float* PQ = a.pr_quat + (size_t)b * T * NJ * 4;
    const float* PP = a.pr_jpos + (size_t)b * T * NJ * 3;
    const double gfl = a.gt_floor[b], pfl = a.pr_floor[b];

    double acc[N_ACC];
#pragma unroll
    for (int q = 0; q < N_ACC; ++q) acc[q] = 0.0;
    for (int t = tid; t < L; t += MT_THREADS) {
        const float* pp = PP + (size_t)t * NJ * 3;
        const float* gp = GP + (size_t)t * NJ * 3;
        double d, r, tr;
        pose_dist(PQ + (size_t)t * NJ * 4, pp, GQ + (size_t)t * NJ * 4, gp, d, r, tr);
        acc[0] += d; acc[1] += r; acc[2] += tr;
        pose_dist(PQ + ((size_t)t * NJ + HEAD) * 4, pp + 3 * HEAD, GQ + ((size_t)t * NJ + HEAD) * 4, gp + 3 * HEAD, d, r, tr);
        acc[3] += d; acc[4] += r; acc[5] += tr;
        // root-relative joint errors
        const double pr0[3] = {pp[0], pp[1], pp[2]}, gr0[3] = {gp[0], gp[1], gp[2]};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double e = ((double)pp[3 * j + c] - pr0[c]) - ((double)gp[3 * j + c] - gr0[c]);
                s += e * e;
            }
            acc[11 + j] += sqrt(s);
        }
        if (t >= 1 && t + 1 < L) {  // accelerations about frame t
            double sp_ = 0.0, sg = 0.0, se = 0.0;
            for (int j = 0; j < NJ; ++j) {
                double np_ = 0.0, ng = 0.0, ne = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int o = 3 * j + c;
                    const double ap = (double)pp[o - NJ * 3] - 2.0 * (double)pp[o] + (double)pp[o + NJ * 3];
                    const double ag = (double)gp[o - NJ * 3] - 2.0 * (double)gp[o] + (double)gp[o + NJ * 3];
                    np_ += ap * ap; ng += ag * ag; ne += (ap - ag) * (ap - ag);
                }
                sp_ += sqrt(np_); sg += sqrt(ng); se += sqrt(ne);
            }
            acc[6] += sp_ / NJ; acc[7] += sg / NJ; acc[8] += se / NJ;
        }
        if (t + 1 < L) {
            acc[9] += foot_slide(pp, pp + NJ * 3, pfl);
            acc[10] += foot_slide(gp, gp + NJ * 3, gfl);
        }
    }
    // fixed-order reduction: within a wave by halving strides, then the waves in order
#pragma unroll
    for (int q = 0; q < N_ACC; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double tot[N_ACC];
        for (int q = 0; q < N_ACC; ++q) {
            double v = red[0][q];
            for (int w = 1; w < MT_THREADS / 64; ++w) v += red[w][q];
            tot[q] = v;
        }
        double* o = a.out + (size_t)b * N_METRICS;
        // below 3 frames no frame has both neighbours: the reference takes np.mean of nothing, NaN (0 / 0 here; L - 2 would
        // give 0 / -1 = -0.0 at L = 1)
        const double n = (double)L, na = L > 2 ? (double)(L - 2) : 0.0;
        o[0] = tot[0] / n; o[1] = tot[1] / n; o[2] = tot[2] / n * 1000.0;   // root_dist, root_rot_dist, root_trans_dist
        o[3] = tot[3] / n; o[4] = tot[4] / n; o[5] = tot[5] / n * 1000.0;   // head_*
        double all = 0.0, body = 0.0;
        for (int j = 0; j < NJ; ++j) {
            const double e = tot[11 + j] / n * 1000.0;
            o[13 + j] = e;                                                    // single_jpe
            all += tot[11 + j];
            if (j < 18) body += e;
        }
        o[6] = all / (n * NJ) * 1000.0;                                       // mpjpe
        o[7] = body / 18.0;                                                   // mpjpe_wo_hand
        o[8] = tot[6] / na * 1000.0; o[9] = tot[7] / na * 1000.0; o[10] = tot[8] / na * 1000.0;  // accel_pred, accel_gt, accel_err
        o[11] = tot[9] / n * 1000.0 / 4.0; o[12] = tot[10] / n * 1000.0 / 4.0;                   // pred_fs, gt_fs
    }
}

}  // namespace evalm
