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
// The floor kernel, step by step (n = number of static toe samples, at most 2 L):
//   1. per frame, eight velocity flags (|p[t + 1] - p[t]| < 0.005 in fp64; the last frame repeats the one before it);
//   2. one block scan over the 2 L virtual entries (left toe frames, then right toe frames) compacts the static heights in the
//      reference's order; a sample carries (compacted index << 12 | frame);
//   3. bitonic sort by (height, compacted index) over the next power of two;
//   4. DBSCAN(eps = 0.005, min_samples = 3) on the sorted line.  A point is core when three points, itself included, lie within
//      eps: h[i + 2] - h[i] <= eps, or h[i] - h[i - 2] <= eps, or both neighbours within eps.  Two cores within eps of each other
//      have only cores between them (any point between them sees both), so a core opens a cluster exactly when its left
//      neighbour is not a core within eps: one more scan numbers the clusters left to right.  sklearn numbers them by first
//      appearance in input order, i.e. by the smallest compacted index among their cores: an LDS atomic min per cluster and a
//      rank count give that order.  A non-core point within eps of a core is a border point; only its two sorted neighbours can
//      be such cores (a core two places away would make the point itself core), and it takes the lower-numbered cluster if both
//      are.  With min_samples = 3 that last case cannot arise (the point would see both cores and be core); the rule is kept
//      as stated.  Everything else is noise (-1).  Clusters are contiguous runs of the sorted line; the noise group is not.
//   5. group medians in fp32 ((a + b) * 0.5f of the two middle samples, numpy's mean of two): runs by position, noise by a scan;
//      floor = the smallest, the first group in label order (-1, 0, 1, ...) on a tie;
//   6. the discard test needs a group's median root height over its unique frames: a frame bit mask (LDS atomic or), a scan to
//      gather the root heights, and a rank count for the middle ones.  It runs for the floor group and for the groups that pass
//      the two cheap tests (median height, size) only;
//   7. contacts from the velocity flags and the heights above floor_height (not the offset height).
// The thresholds, the contact joints and the LDS layout live in floor_common.h, which amass_prep.h's floor kernel shares.
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

// Exclusive prefix sum of flag(i), i < n, over the block: emit(i, prefix, flag(i)) for every i, returns the total.  A thread owns
// a contiguous run of ceil(n / threads) <= 32 entries and evaluates each flag once, before any emit runs.
template <typename F, typename E>
EG_D int block_scan(int n, int* part, F flag, E emit) {
    const int tid = threadIdx.x, chunk = (n + FC_THREADS - 1) / FC_THREADS;
    const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    uint32_t bits = 0;
    for (int i = lo; i < hi; ++i) bits |= (flag(i) ? 1u : 0u) << (i - lo);
    const int cnt = __popc(bits);
    part[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < FC_THREADS; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int pre = part[tid] - cnt;
    const int total = part[FC_THREADS - 1];
    for (int i = lo; i < hi; ++i) {
        const bool f = (bits >> (i - lo)) & 1u;
        emit(i, pre, f);
        pre += f;
    }
    __syncthreads();
    return total;
}

// the median (fp32, numpy's) of the root heights of the unique frames of the samples labelled `label`
EG_D float root_median(int label, int n, int L, const float* P, const uint32_t* sp, const int* lab, uint32_t* mask, float* rootv, int* part,
                       float* s_pair) {
    const int tid = threadIdx.x;
    for (int w = tid; w < (L + 31) / 32; w += FC_THREADS) mask[w] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += FC_THREADS)
        if (lab[i] == label) {
            const uint32_t f = sp[i] & (MAX_T - 1);
            atomicOr(&mask[f >> 5], 1u << (f & 31));
        }
    __syncthreads();
    const int m = block_scan(L, part, [&](int t) { return (mask[t >> 5] >> (t & 31)) & 1u; },
                             [&](int t, int pre, bool f) { if (f) rootv[pre] = P[(size_t)t * NJ * 3 + 2]; });
    for (int i = tid; i < m; i += FC_THREADS) {
        const float v = rootv[i];
        int r = 0;
        for (int j = 0; j < m; ++j) {
            const float u = rootv[j];
            r += (u < v || (u == v && j < i)) ? 1 : 0;
        }
        if (r == (m - 1) / 2) s_pair[0] = v;
        if (r == m / 2) s_pair[1] = v;
    }
    __syncthreads();
    const float med = (s_pair[0] + s_pair[1]) * 0.5f;
    __syncthreads();
    return med;
}

__global__ void __launch_bounds__(FC_THREADS) eval_floor_kernel(FloorArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
    __shared__ float s_pair[2];
    __shared__ unsigned long long s_best;
    const FloorLds lay = floor_lds(a.cap);
    float* sh = (float*)(fc_lds + lay.sh);
    uint32_t* sp = (uint32_t*)(fc_lds + lay.sp);
    int* lab = (int*)(fc_lds + lay.lab);
    float* gmed = (float*)(fc_lds + lay.gmed);
    int* gsz = (int*)(fc_lds + lay.gsz);
    float* rootv = (float*)(fc_lds + lay.rootv);
    uint8_t* vf = fc_lds + lay.vf;
    uint32_t* mask = (uint32_t*)(fc_lds + lay.mask);
    int* part = (int*)(fc_lds + lay.part);

    const int tid = threadIdx.x, b = blockIdx.x, T = a.T;
    int L = a.lengths ? a.lengths[b] : T;
    L = L < 0 ? 0 : (L > T ? T : L);
    const float* P = a.jpos + (size_t)b * T * NJ * 3;

    // 1. velocity flags
    for (int t = tid; t < L; t += FC_THREADS) {
        uint32_t flags = 0;
        if (L >= 2) {
            const int tv = t + 1 < L ? t : L - 2;
            const float* p0 = P + (size_t)tv * NJ * 3;
            const float* p1 = p0 + NJ * 3;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = contact_joint(k);
                const double dx = (double)p1[3 * j] - (double)p0[3 * j], dy = (double)p1[3 * j + 1] - (double)p0[3 * j + 1],
                             dz = (double)p1[3 * j + 2] - (double)p0[3 * j + 2];
                if (sqrt(dx * dx + dy * dy + dz * dz) < VEL_THRESH) flags |= 1u << k;
            }
        }
        vf[t] = (uint8_t)flags;
    }
    __syncthreads();

    // 2. static toe heights, left frames then right frames
    const int n = block_scan(2 * L, part, [&](int e) { return e < L ? (vf[e] & 1u) : ((vf[e - L] >> 1) & 1u); },
                             [&](int e, int pre, bool f) {
                                 if (!f) return;
                                 const int fr = e < L ? e : e - L;
                                 sh[pre] = P[(size_t)fr * NJ * 3 + 3 * (e < L ? 10 : 11) + 2];
                                 sp[pre] = ((uint32_t)pre << FRAME_BITS) | (uint32_t)fr;
                             });

    // 3. sort by (height, compacted index)
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    for (int i = n + tid; i < np2; i += FC_THREADS) {
        sh[i] = __builtin_inff();
        sp[i] = 0xffffffffu;
    }
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += FC_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const float hi_ = sh[i], hl = sh[l];
                    const uint32_t pi = sp[i], pl = sp[l];
                    const bool gt = hi_ > hl || (hi_ == hl && pi > pl);
                    if (gt == ((i & k) == 0)) {
                        sh[i] = hl; sh[l] = hi_;
                        sp[i] = pl; sp[l] = pi;
                    }
                }
            }
            __syncthreads();
        }

    // 4. DBSCAN on the sorted line
    auto is_core = [&](int i) {
        const bool l1 = i >= 1 && within_eps(sh[i], sh[i - 1]), r1 = i + 1 < n && within_eps(sh[i], sh[i + 1]);
        return (l1 && r1) || (i >= 2 && within_eps(sh[i], sh[i - 2])) || (i + 2 < n && within_eps(sh[i], sh[i + 2]));
    };
    for (int i = tid; i < n; i += FC_THREADS) lab[i] = is_core(i) ? 1 : 0;
    __syncthreads();
    // raw cluster ids, left to right: lab[i] = id for a core, -1 otherwise
    const int K = block_scan(n, part, [&](int i) { return lab[i] && !(i >= 1 && lab[i - 1] && within_eps(sh[i], sh[i - 1])); },
                             [&](int i, int pre, bool f) {
                                 // (lab[i] is read by the owner of i and of i + 1 only, both before any emit: block_scan)
                                 lab[i] = lab[i] ? pre + (f ? 1 : 0) - 1 : -1;
                             });
    for (int k = tid; k < K; k += FC_THREADS) gsz[k] = 0x7fffffff;
    __syncthreads();
    for (int i = tid; i < n; i += FC_THREADS)
        if (lab[i] >= 0) atomicMin(&gsz[lab[i]], (int)(sp[i] >> FRAME_BITS));
    __syncthreads();
    {  // a cluster's number = how many clusters appear before it in input order; K <= n / 3 < 3 * FC_THREADS
        int rank[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int k = tid + q * FC_THREADS;
            rank[q] = 0;
            if (k < K) {
                const int mine = gsz[k];
                for (int o = 0; o < K; ++o) rank[q] += gsz[o] < mine ? 1 : 0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int k = tid + q * FC_THREADS;
            if (k < K) gsz[k] = rank[q];
        }
        __syncthreads();
    }
    {
        int fin[FC_ELEMS];
#pragma unroll
        for (int q = 0; q < FC_ELEMS; ++q) {
            const int i = tid + q * FC_THREADS;
            fin[q] = -1;
            if (i < n) {
                if (lab[i] >= 0) {
                    fin[q] = gsz[lab[i]];
                } else {
                    const int cl = i >= 1 && lab[i - 1] >= 0 && within_eps(sh[i], sh[i - 1]) ? gsz[lab[i - 1]] : -1;
                    const int cr = i + 1 < n && lab[i + 1] >= 0 && within_eps(sh[i], sh[i + 1]) ? gsz[lab[i + 1]] : -1;
                    fin[q] = cl < 0 ? cr : (cr < 0 ? cl : min(cl, cr));
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < FC_ELEMS; ++q) {
            const int i = tid + q * FC_THREADS;
            if (i < n) {
                lab[i] = fin[q];
                if (a.labels) a.labels[(size_t)b * 2 * T + (sp[i] >> FRAME_BITS)] = fin[q];
            }
        }
        if (a.labels)
            for (int i = n + tid; i < 2 * T; i += FC_THREADS) a.labels[(size_t)b * 2 * T + i] = -2;
        __syncthreads();
    }

    // 5. group medians; slot g = label + 1 (slot 0: noise)
    for (int i = tid; i < n; i += FC_THREADS) {
        const int l = lab[i];
        if (l < 0) continue;
        if (i == 0 || lab[i - 1] != l) gsz[l + 1] = i;
        if (i == n - 1 || lab[i + 1] != l) ((int*)gmed)[l + 1] = i;
    }
    __syncthreads();
    for (int g = 1 + tid; g <= K; g += FC_THREADS) {
        const int s = gsz[g], m = ((int*)gmed)[g] - s + 1;
        gmed[g] = (sh[s + (m - 1) / 2] + sh[s + m / 2]) * 0.5f;
        gsz[g] = m;
    }
    const int nn = block_scan(n, part, [&](int i) { return lab[i] < 0; }, [&](int, int, bool) {});
    block_scan(n, part, [&](int i) { return lab[i] < 0; },
               [&](int i, int pre, bool f) {
                   if (!f) return;
                   if (pre == (nn - 1) / 2) s_pair[0] = sh[i];
                   if (pre == nn / 2) s_pair[1] = sh[i];
               });
    if (tid == 0) {
        gsz[0] = nn;
        gmed[0] = nn ? (s_pair[0] + s_pair[1]) * 0.5f : __builtin_inff();
        s_best = ~0ull;
    }
    __syncthreads();

    float floor_h = 0.f;
    int discard = 0;
    if (n > 0) {
        for (int g = tid; g <= K; g += FC_THREADS)
            if (gsz[g] > 0) {
                uint32_t u = __float_as_uint(gmed[g]);
                u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving
                atomicMin(&s_best, ((unsigned long long)u << 32) | (uint32_t)g);
            }
        __syncthreads();
        const int gbest = (int)(s_best & 0xffffffffu);
        floor_h = gmed[gbest];
        // 6. DISCARD_TERRAIN_SEQUENCES (:267-277)
        const float min_root = root_median(gbest - 1, n, L, P, sp, lab, mask, rootv, part, s_pair);
        for (int g = 0; g <= K && !discard; ++g) {
            if (gsz[g] == 0 || !(gmed[g] > floor_h + TERRAIN_H) || !(gsz[g] > a.size_thresh)) continue;
            const float rm = root_median(g - 1, n, L, P, sp, lab, mask, rootv, part, s_pair);
            if (rm > min_root + ROOT_H) discard = 1;
        }
    }
    if (tid == 0) {
        a.floor_h[b] = floor_h;
        a.offset_h[b] = n > 0 ? floor_h - FLOOR_OFFSET : 0.f;
        a.discard[b] = discard;
        a.n_static[b] = n;
        a.n_groups[b] = K + (nn > 0 ? 1 : 0);
    }

    // 7. contacts
    float* C = a.contacts + (size_t)b * T * NJ;
    for (int t = tid; t < T; t += FC_THREADS) {
        uint32_t on = 0;
        if (t < L) {
            const uint32_t flags = vf[t];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = contact_joint(k);
                const float hgt = P[(size_t)t * NJ * 3 + 3 * j + 2] - floor_h;
                if (((flags >> k) & 1u) && hgt < (k < 2 ? TOE_H : ANKLE_H)) on |= 1u << j;
            }
        }
        for (int j = 0; j < NJ; ++j) C[(size_t)t * NJ + j] = (float)((on >> j) & 1u);
    }
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
        const double n = (double)L, na = (double)(L - 2);
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
