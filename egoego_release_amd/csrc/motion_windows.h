// motion_windows.h — raw SMPL-H motion (trans, root_orient, body_pose per frame) -> the stage-2 model-space windows of the
// reference's AMASSDataset (egoego/data/amass_diffusion_dataset.py: process_window_data 409-510, extract_min_max_mean_std_from_data
// 355-377, __getitem__ 515-538; rotate_at_frame_smplh, egoego/lafan1/utils.py:111-137).  Joint layout: 22 SMPL joints, z up.
//
//   win_build_kernel      one 64-thread workgroup per window, one thread per frame, 64 frames at a time.  Per frame in fp64:
//                         Rodrigues for the 22 joints, the global rotations down the tree, FK with the rest offsets; the head's
//                         global rotation in the window's first frame gives the heading, whose inverse turns every global
//                         rotation, the root's local one, the skeleton and the root translation; the first frame's head xy is
//                         taken off.  Each output is rounded to fp32 once.
//   win_minmax_kernel     per-coordinate min / max of global_jpos and global_jvel over the real frames of all windows: row r of
//                         the [N * W] rows goes to workgroup r % G, a second launch folds the G partial rows.  No atomics: min and
//                         max do not depend on the order.
//   win_motion_kernel     __getitem__: (jpos - min) / (max - min) * 2 - 1 in fp32, then the global 6D rotations; zero rows past
//                         the length.
//
// Memory: a frame's outputs are rows of 66, 66, 132 and 132 floats; a thread that wrote its own frame's rows would scatter a
// wave's store over 64 lines.  So a chunk's inputs (64 x 69 floats) and its 6D rows (64 x 132, local then global) pass through
// one LDS stage and move to and from HBM as straight dword-linear copies (rows of one window are contiguous: lane i takes dword i).
// The positions of the whole window stay in LDS as the fp32 values that are written, so the velocity is their fp32 difference
// without a second pass over HBM.
//
// LDS: (W * 66 + 64 * 132) * 4 bytes + 48: 65.5 KiB at W = 120 (two workgroups per CU); W <= MAX_W fits the 160 KiB.
#pragma once
#include "common.h"
#include "quat_f64.h"

namespace mwin {

static constexpr int NJ = 22;
static constexpr int HEAD = 15;
static constexpr int JP = NJ * 3;   // 66: a frame's joint positions
static constexpr int R6 = NJ * 6;   // 132: a frame's 6D rotations
static constexpr int FEATS = JP + R6;
static constexpr int CHUNK = 64;    // frames per pass = threads per workgroup
static constexpr int MAX_W = 480;
static constexpr int MM_THREADS = 192;  // 2 tensors x 66 columns, rounded up to whole waves
static constexpr int MM_MAX_BLOCKS = 1024;

struct BuildArgs {
    const float* trans;        // [F][3]
    const float* root_orient;  // [F][3]
    const float* body_pose;    // [F][63]
    const float* rest;         // [22][3]
    const int* first;          // [N] index of each window's first frame in the F concatenated frames
    const int* length;         // [N] real frames, 0..W
    float* jpos;               // [N][W][66]
    float* jvel;               // [N][W][66]
    float* grot6d;             // [N][W][132]
    float* lrot6d;             // [N][W][132]
    float* recover;            // [N][4]
    int parents[NJ];
    int F, N, W, canonicalize;
};

EG_HD size_t build_lds_bytes(int W) { return ((size_t)W * JP + (size_t)CHUNK * R6) * 4 + 48; }

// the first two rows of the rotation matrix of a unit quaternion
EG_D void qd_rows01(QuatD q, float* o) {
    o[0] = (float)(1.0 - 2.0 * (q.y * q.y + q.z * q.z));
    o[1] = (float)(2.0 * (q.x * q.y - q.z * q.w));
    o[2] = (float)(2.0 * (q.x * q.z + q.y * q.w));
    o[3] = (float)(2.0 * (q.x * q.y + q.z * q.w));
    o[4] = (float)(1.0 - 2.0 * (q.x * q.x + q.z * q.z));
    o[5] = (float)(2.0 * (q.y * q.z - q.x * q.w));
}

// rotate_at_frame_smplh's yrot for the head rotation q (lafan1/utils.py:127-132): forward = (1, 1, 0) * (q . x), normalised with
// x / (|x| + 1e-8); quat_between(x, forward) = (|forward| + forward.x, 0, 0, forward.y), normalised the same way
EG_D QuatD heading_of(QuatD q) {
    const double ex[3] = {1.0, 0.0, 0.0};
    double f[3];
    qd_rotate(q, ex, f);
    const double n = sqrt(f[0] * f[0] + f[1] * f[1]) + 1e-8;
    const double fx = f[0] / n, fy = f[1] / n;
    const double w = sqrt(fx * fx + fy * fy) + fx;
    const double m = sqrt(w * w + fy * fy) + 1e-8;
    return QuatD{w / m, 0.0, 0.0, fy / m};
}

__global__ __launch_bounds__(CHUNK) void win_build_kernel(BuildArgs a) {
    extern __shared__ __align__(16) unsigned char win_smem[];
    double* sh_head = reinterpret_cast<double*>(win_smem);         // [4] the first frame's head rotation, [2] its head xy
    float* sh_pos = reinterpret_cast<float*>(win_smem + 48);        // [W][66] the positions as written
    float* sh_stage = sh_pos + (size_t)a.W * JP;                    // [64][132] inputs, then local 6D, then global 6D
    const int n = blockIdx.x, tid = threadIdx.x, W = a.W;
    int len = a.length[n];
    const int first = a.first[n];
    len = len < 0 ? 0 : len > W ? W : len;
    if (first < 0 || first > a.F - len) len = 0;  // a row that leaves the input: an empty window, never a read outside
    float* o_l6 = a.lrot6d + (size_t)n * W * R6;
    float* o_g6 = a.grot6d + (size_t)n * W * R6;

    for (int t0 = 0; t0 < W; t0 += CHUNK) {
        const int rows = W - t0 < CHUNK ? W - t0 : CHUNK;                          // rows of this chunk in the output
        const int real = len - t0 < 0 ? 0 : len - t0 < CHUNK ? len - t0 : CHUNK;   // of which hold a frame
        const int t = t0 + tid;
        const bool active = tid < real;
        // ---- the chunk's inputs, lane-linear, into the stage: [real][63], then [real][3], then [real][3]
        {
            const size_t f0 = (size_t)first + t0;
            for (int i = tid; i < real * 63; i += CHUNK) sh_stage[i] = a.body_pose[f0 * 63 + i];
            for (int i = tid; i < real * 3; i += CHUNK) {
                sh_stage[CHUNK * 63 + i] = a.root_orient[f0 * 3 + i];
                sh_stage[CHUNK * 66 + i] = a.trans[f0 * 3 + i];
            }
        }
        __syncthreads();
        QuatD lq[NJ], gq[NJ];
        double gp[NJ][3];
        double tr[3] = {0.0, 0.0, 0.0};
        lq[0] = QuatD{1.0, 0.0, 0.0, 0.0};
        if (active) {  // Rodrigues for the 22 joints
            const float* bp = sh_stage + tid * 63;
            const float* ro = sh_stage + CHUNK * 63 + tid * 3;
            const float* tp = sh_stage + CHUNK * 66 + tid * 3;
            tr[0] = tp[0]; tr[1] = tp[1]; tr[2] = tp[2];
            lq[0] = qd_from_aa(ro[0], ro[1], ro[2]);
            for (int j = 1; j < NJ; ++j) lq[j] = qd_from_aa(bp[3 * j - 3], bp[3 * j - 2], bp[3 * j - 1]);
        }
        __syncthreads();  // the inputs are in registers: the stage now takes the local 6D rows
        if (active) {
            // the chain down the tree (local2global_pose, quat_fk_torch), before the heading is known: it turns the result as a whole
            gq[0] = lq[0];
            gp[0][0] = a.rest[0]; gp[0][1] = a.rest[1]; gp[0][2] = a.rest[2];
            float* row = sh_stage + tid * R6;
            for (int j = 1; j < NJ; ++j) {
                const int p = a.parents[j];
                const double off[3] = {a.rest[3 * j], a.rest[3 * j + 1], a.rest[3 * j + 2]};
                double r[3];
                qd_rotate(gq[p], off, r);
                gp[j][0] = r[0] + gp[p][0]; gp[j][1] = r[1] + gp[p][1]; gp[j][2] = r[2] + gp[p][2];
                gq[j] = qd_std(qd_mul(gq[p], lq[j]));
                qd_rows01(lq[j], row + 6 * j);
            }
            if (t == 0) {
                sh_head[0] = gq[HEAD].w; sh_head[1] = gq[HEAD].x; sh_head[2] = gq[HEAD].y; sh_head[3] = gq[HEAD].z;
            }
        }
        __syncthreads();
        // ---- the heading (identical in every lane) and its inverse: `inv` as the reference applies it to the translation
        // (not quite unit: the 1e-8 of the normalisation), `invn` of unit length for the rotations (quaternion_to_matrix, dataset:439,
        // divides by the squared norm)
        QuatD yrot = QuatD{1.0, 0.0, 0.0, 0.0};
        if (a.canonicalize && len > 0) yrot = heading_of(QuatD{sh_head[0], sh_head[1], sh_head[2], sh_head[3]});
        const QuatD inv = QuatD{yrot.w, -yrot.x, -yrot.y, -yrot.z};
        const double im = sqrt(inv.w * inv.w + inv.z * inv.z);
        const QuatD invn = QuatD{inv.w / im, 0.0, 0.0, inv.z / im};
        if (t0 == 0 && tid == 0) {
            float* r = a.recover + (size_t)n * 4;
            r[0] = (float)yrot.w; r[1] = (float)yrot.x; r[2] = (float)yrot.y; r[3] = (float)yrot.z;
        }
        double ct[3] = {0.0, 0.0, 0.0};
        if (active) {
            qd_rows01(qd_mul(invn, lq[0]), sh_stage + tid * R6);
            qd_rotate(inv, tr, ct);
            if (t == 0) {  // the first frame's head, as the loop below computes it
                double r[3];
                qd_rotate(invn, gp[HEAD], r);
                sh_head[4] = r[0] + ct[0]; sh_head[5] = r[1] + ct[1];
            }
        }
        __syncthreads();
        for (int i = tid; i < rows * R6; i += CHUNK) o_l6[(size_t)t0 * R6 + i] = i < real * R6 ? sh_stage[i] : 0.f;
        __syncthreads();
        if (active) {
            float* row = sh_stage + tid * R6;
            for (int j = 0; j < NJ; ++j) qd_rows01(qd_mul(invn, gq[j]), row + 6 * j);
            const double hx = sh_head[4], hy = sh_head[5];
            float* p = sh_pos + (size_t)t * JP;
            for (int j = 0; j < NJ; ++j) {
                double r[3];
                qd_rotate(invn, gp[j], r);
                p[3 * j] = (float)(r[0] + ct[0] - hx); p[3 * j + 1] = (float)(r[1] + ct[1] - hy); p[3 * j + 2] = (float)(r[2] + ct[2]);
            }
        }
        __syncthreads();
        for (int i = tid; i < rows * R6; i += CHUNK) o_g6[(size_t)t0 * R6 + i] = i < real * R6 ? sh_stage[i] : 0.f;
        __syncthreads();  // the stage is free for the next chunk's inputs
    }
    // ---- positions and velocities, lane-linear: jvel[t] = jpos[t + 1] - jpos[t] on the fp32 values, zero in the last real frame
    float* o_p = a.jpos + (size_t)n * W * JP;
    float* o_v = a.jvel + (size_t)n * W * JP;
    for (int i = tid; i < W * JP; i += CHUNK) {
        const int t = i / JP;
        o_p[i] = t < len ? sh_pos[i] : 0.f;
        o_v[i] = t < len - 1 ? sh_pos[i + JP] - sh_pos[i] : 0.f;
    }
}

// out [gridDim.x][4][66]: min jpos, max jpos, min jvel, max jvel over the rows r = blockIdx.x, + gridDim.x, ... of the [n_rows]
// rows whose frame (r % W) lies below length[r / W] (length == nullptr: every row).  A workgroup without a row writes
// +inf / -inf, the neutral elements.
__global__ __launch_bounds__(MM_THREADS) void win_minmax_kernel(const float* jpos, const float* jvel, const int* length, int n_rows, int W,
                                                                 float* out) {
    const int tid = threadIdx.x;
    if (tid >= 2 * JP) return;
    const float* src = (tid < JP ? jpos : jvel) + tid % JP;
    float lo = INFINITY, hi = -INFINITY;
    for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
        if (length && r % W >= length[r / W]) continue;
        const float v = src[(size_t)r * JP];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    float* o = out + (size_t)blockIdx.x * 4 * JP + (tid < JP ? 0 : 2 * JP) + tid % JP;
    o[0] = lo;
    o[JP] = hi;
}
// part [n_part][4][66] -> out [4][66]
__global__ void win_minmax_fold_kernel(const float* part, int n_part, float* out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= 4 * JP) return;
    const bool is_max = (c / JP) & 1;
    float v = is_max ? -INFINITY : INFINITY;
    for (int r = 0; r < n_part; ++r) {
        const float x = part[(size_t)r * 4 * JP + c];
        v = is_max ? fmaxf(v, x) : fminf(v, x);
    }
    out[c] = v;
}

// motion [N][W][198]: the normalised positions, then the global 6D rotations; zero past each length (dataset:515-538)
__global__ void win_motion_kernel(const float* jpos, const float* grot6d, const int* length, const float* jmin, const float* jmax, size_t n_rows,
                                  int W, float* motion) {
    const size_t total = n_rows * FEATS;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / FEATS;
        const int c = (int)(i - r * FEATS);
        float v = 0.f;
        if ((int)(r % W) < length[r / W]) {
            if (c < JP) {
                const float lo = jmin[c];
                v = (jpos[r * JP + c] - lo) / (jmax[c] - lo) * 2.f - 1.f;
            } else {
                v = grot6d[r * R6 + (c - JP)];
            }
        }
        motion[i] = v;
    }
}

}  // namespace mwin
