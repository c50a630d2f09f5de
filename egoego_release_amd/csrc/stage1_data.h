// stage1_data.h — the stage-1 training batches, built on the device (HeadNet's: the second half of this file).  GravityNet's: AMASSHeadPoseDataset.__getitem__ with augment_traj
// (egoego/data/amass_headpose_dataset.py:38-76, 115-165) for every sample of a batch in one launch.  A sample is a window of one
// sequence's [len][7] head poses (xyz, quaternion w,x,y,z) under one random rotation Rr and one random scale s:
//   head_rot_mat_t = Rr R(q_t),   head_trans_t = s Rr (p_t - p_0),   floor_normal = Rr[:, 2].
// The reference builds the translation by adding the scaled differences one by one from x_0 = Rr (p_0 - p_0) = 0; that sum
// telescopes to s y_t, which every frame computes for itself here.  All arithmetic is fp64 on the fp32 inputs and each output is
// rounded once; Rr is rounded to fp32 first (the reference holds it as an fp32 tensor), so floor_normal and aligned_rot_mat are
// the very numbers the frames were rotated with.
#pragma once
#include "common.h"

namespace s1d {

// Counter word 3 of every draw of this file.  The dropout draws of train_step.h / stage1_train.h put layer * 4 + site there (below
// 64) and the sampler's noise its timestep (below 1000): under one seed no counter of theirs can equal one of these.
static constexpr uint32_t DRAW_TAG = 0x47424154u;  // "GBAT"
static constexpr int THREADS = 128;

// pytorch3d's quaternion_to_matrix: two_s = 2 / sum(q * q), no unit-norm assumption
EG_D void quat_to_matrix(const double q[4], double R[9]) {
    const double r = q[0], i = q[1], j = q[2], k = q[3];
    const double two_s = 2.0 / (((r * r + i * i) + j * j) + k * k);
    R[0] = 1.0 - two_s * (j * j + k * k);
    R[1] = two_s * (i * j - k * r);
    R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r);
    R[4] = 1.0 - two_s * (i * i + k * k);
    R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r);
    R[7] = two_s * (j * k + i * r);
    R[8] = 1.0 - two_s * (i * i + j * j);
}

struct GravityBatch {
    const float* pose;       // [N][7]
    const int32_t* offsets;  // [S + 1]
    const int32_t* seq_ids;  // [B]
    const int64_t* draw_ids; // [B]
    const int32_t* start;    // [B] or nullptr
    const float* rot;        // [B][9] or nullptr
    const float* scale;      // [B] or nullptr
    int N, S, W, for_eval;
    uint64_t seed;
    float *ori, *rotm, *trans;  // [B][W + 1][7 | 9 | 3]
    int32_t* seq_len;           // [B]
    float *aligned_rot, *aligned_scale, *normal;  // [B][9], [B], [B][3]
    int32_t* start_out;         // [B]
    float* scale_out;           // [B]
};

// One workgroup per sample.  Every thread derives the sample's draws for itself (two Philox calls: no LDS, no barrier) and then
// owns the frames t = thread, thread + THREADS, ...  A sample whose sequence id, offsets or planted start do not describe rows
// inside pose [N][7] is written as an empty sample (seq_len 0, every row zero); nothing outside the arrays is read.
__global__ __launch_bounds__(THREADS) void gravity_batch_kernel(GravityBatch a) {
    const int b = blockIdx.x;
    const int W = a.W;
    const int sid = a.seq_ids[b];
    long first = 0;
    int len = 0;
    if (sid >= 0 && sid < a.S) {
        const long o0 = a.offsets[sid], o1 = a.offsets[sid + 1];
        if (o0 >= 0 && o1 > o0 && o1 <= (long)a.N) {
            first = o0;
            len = (int)(o1 - o0);
        }
    }
    const uint64_t id = (uint64_t)a.draw_ids[b];
    const uint32_t id_lo = (uint32_t)id, id_hi = (uint32_t)(id >> 32);
    const Philox4 words = philox4x32_10(id_lo, id_hi, 1u, DRAW_TAG, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));

    // ---- the window (dataset:121-135)
    const int room = len - W - 1;
    int n = room <= 0 ? len : W + 1;
    int start = 0;
    if (room > 0) {
        if (a.start)
            start = a.start[b];
        else if (!a.for_eval)
            start = (int)(((uint64_t)words.c[0] * (uint64_t)(uint32_t)room) >> 32);
        if (start < 0 || start >= room) {  // a planted start outside range(len - W - 1)
            n = 0;
            start = 0;
        }
    } else if (a.start && a.start[b] != 0) {
        n = 0;
    }

    // ---- the rotation (pytorch3d's random_rotation) and the scale (np.random.uniform(0.1, 10))
    float Rr[9];
    if (a.rot) {
        for (int i = 0; i < 9; ++i) Rr[i] = a.rot[(size_t)b * 9 + i];
    } else {
        float o[4];
        philox_normal4(a.seed, id_lo, id_hi, 0u, DRAW_TAG, o);
        const double od[4] = {o[0], o[1], o[2], o[3]};
        const double nrm = copysign(sqrt(((od[0] * od[0] + od[1] * od[1]) + od[2] * od[2]) + od[3] * od[3]), od[0]);
        const double q[4] = {od[0] / nrm, od[1] / nrm, od[2] / nrm, od[3] / nrm};
        double R[9];
        quat_to_matrix(q, R);
        for (int i = 0; i < 9; ++i) Rr[i] = (float)R[i];
    }
    const float s = a.scale ? a.scale[b] : (float)(0.1 + 9.9 * (((double)words.c[1] + 0.5) * 2.3283064365386963e-10));

    if (threadIdx.x == 0) {
        a.seq_len[b] = n;
        a.start_out[b] = start;
        a.scale_out[b] = s;
        a.aligned_scale[b] = (float)(1.0 / (double)s);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) a.aligned_rot[(size_t)b * 9 + 3 * i + j] = Rr[3 * j + i];
            a.normal[(size_t)b * 3 + i] = Rr[3 * i + 2];
        }
    }

    const float* src = a.pose + (size_t)(first + start) * 7;
    double p0[3] = {0.0, 0.0, 0.0};
    if (n > 0)
        for (int i = 0; i < 3; ++i) p0[i] = src[i];
    for (int t = threadIdx.x; t <= W; t += THREADS) {
        const size_t row = (size_t)b * (W + 1) + t;
        float* po = a.ori + row * 7;
        float* ro = a.rotm + row * 9;
        float* to = a.trans + row * 3;
        if (t >= n) {
            for (int i = 0; i < 7; ++i) po[i] = 0.f;
            for (int i = 0; i < 9; ++i) ro[i] = 0.f;
            for (int i = 0; i < 3; ++i) to[i] = 0.f;
            continue;
        }
        float p[7];
        for (int i = 0; i < 7; ++i) p[i] = src[(size_t)t * 7 + i];
        for (int i = 0; i < 7; ++i) po[i] = p[i];
        const double q[4] = {p[3], p[4], p[5], p[6]};
        double R[9];
        quat_to_matrix(q, R);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                ro[3 * i + j] = (float)(((double)Rr[3 * i] * R[j] + (double)Rr[3 * i + 1] * R[3 + j]) + (double)Rr[3 * i + 2] * R[6 + j]);
        const double d[3] = {(double)p[0] - p0[0], (double)p[1] - p0[1], (double)p[2] - p0[2]};
        for (int i = 0; i < 3; ++i) {
            const double y = ((double)Rr[3 * i] * d[0] + (double)Rr[3 * i + 1] * d[1]) + (double)Rr[3 * i + 2] * d[2];
            to[i] = (float)((double)s * y);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// HeadNet's training batches: ARESHeadPoseDataset.__getitem__ (egoego/data/ares_headpose_dataset.py:270-333; the GIMO and
// real-world datasets share it) for every sample of a batch in one launch.  A sequence k of T_k = offsets[k + 1] - offsets[k]
// frames has T_k rows of pose and vels, F_k = T_k - 1 rows of features (at row offsets[k] - k of feats: every sequence before
// it is one row shorter there) and, optionally, L_k rows of a SLAM track.  A sample is rows start .. start + n of the pose and
// of the track (n + 1 rows, fewer where the track ends sooner) and rows start .. start + n - 1 of vels and feats.  Nothing is
// computed: every output word is a copy of an input word or a zero.
static constexpr uint32_t HEAD_DRAW_TAG = 0x48424154u;  // "HBAT": counter word 3 of the start's draw; GBAT above is another word
static constexpr int HEAD_THREADS = 256;
static constexpr int HEAD_FRAME_TILE = 4;  // frames per workgroup: at D = 512 each lane moves two 16-byte pieces of features
static constexpr int SLAM_COLS = 29;       // aligned trans 3 | aligned quat 4 | aligned rot 9 | original quat 4 | original rot 9

struct HeadBatch {
    const float* pose;             // [N][7]
    const float* vels;             // [N][6]
    const float4* feats;           // [N - S][D]
    const int32_t* offsets;        // [S + 1]
    const float* slam32;           // [M][29] or nullptr
    const double* slam_trans64;    // [M][3] or nullptr
    const int32_t* slam_offsets;   // [S + 1] or nullptr
    const int32_t* seq_ids;        // [B]
    const int64_t* draw_ids;       // [B]
    const int32_t* start;          // [B] or nullptr
    int N, S, M, D4, W, for_eval, tiles;
    uint64_t seed;
    float *head_pose, *head_vels;  // [B][W + 1][7], [B][W][6]
    float4* of;                    // [B][W][D]
    int32_t *seq_len, *start_out;  // [B]
    float *al_trans, *al_quat, *al_rot, *ori_quat, *ori_rot;  // [B][W + 1][3 | 4 | 9 | 4 | 9] or nullptr
    double* ori_trans;             // [B][W + 1][3] or nullptr
    int32_t* pose_len;             // [B] or nullptr
};

// how many of a tile's frames t0 .. t0 + HEAD_FRAME_TILE - 1 lie below `count`
EG_D int head_live(int count, int t0) {
    const int d = count - t0;
    return d < 0 ? 0 : (d > HEAD_FRAME_TILE ? HEAD_FRAME_TILE : d);
}

// Workgroup (sample b, tile x) owns frames x * HEAD_FRAME_TILE .. + HEAD_FRAME_TILE - 1 of sample b.  Every workgroup derives
// the sample's window for itself (one Philox call: no LDS, no barrier); all of that is uniform over the workgroup.  The feature
// rows of a tile are contiguous in the table and in the output, so consecutive lanes move consecutive 16-byte pieces.  A sample
// whose sequence id, offsets or planted start do not describe rows inside the tables, or whose sequence is shorter than the
// window in training, is written as an empty sample (seq_len 0, pose_len 0, every row zero); nothing outside the tables is read.
__global__ __launch_bounds__(HEAD_THREADS) void head_batch_kernel(HeadBatch a) {
    const int b = (int)(blockIdx.x / (unsigned)a.tiles);
    const int t0 = (int)(blockIdx.x % (unsigned)a.tiles) * HEAD_FRAME_TILE;
    const int W = a.W;
    const int sid = a.seq_ids[b];
    long first = 0, ffirst = 0, sfirst = 0;
    int F = 0, L = 0;
    if (sid >= 0 && sid < a.S) {
        const long o0 = a.offsets[sid], o1 = a.offsets[sid + 1];
        if (o0 >= 0 && o1 > o0 && o1 <= (long)a.N && o0 - sid >= 0 && o1 - 1 - sid <= (long)a.N - a.S) {
            first = o0;
            ffirst = o0 - sid;
            F = (int)(o1 - o0) - 1;
            if (a.slam_offsets) {
                const long s0 = a.slam_offsets[sid], s1 = a.slam_offsets[sid + 1];
                if (s0 >= 0 && s1 >= s0 && s1 <= (long)a.M) {
                    sfirst = s0;
                    L = (int)(s1 - s0);
                } else {
                    F = 0;
                }
            }
        }
    }

    // ---- the window (dataset:276-283)
    int n = 0, start = 0;
    if (a.for_eval) {
        n = F < W ? F : W;
    } else {
        const int room = F - W + 1;
        if (F >= 1 && room >= 1) {
            n = W;
            if (a.start) {
                start = a.start[b];
            } else {
                const uint64_t id = (uint64_t)a.draw_ids[b];
                const Philox4 words = philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), 1u, HEAD_DRAW_TAG, (uint32_t)a.seed,
                                                    (uint32_t)(a.seed >> 32));
                start = (int)(((uint64_t)words.c[0] * (uint64_t)(uint32_t)room) >> 32);
            }
            if (start < 0 || start >= room) {  // a planted start outside range(F - W + 1)
                n = 0;
                start = 0;
            }
        }
    }
    const int n_pose = n > 0 ? n + 1 : 0;
    int n_slam = L - start;
    n_slam = n_slam < 0 ? 0 : (n_slam > n_pose ? n_pose : n_slam);

    if (t0 == 0 && threadIdx.x == 0) {
        a.seq_len[b] = n;
        a.start_out[b] = start;
        if (a.pose_len) a.pose_len[b] = n_slam;
    }

    // ---- the features: rows t0 .. of [W][D], 16 bytes per lane
    {
        const int rows = W - t0 < HEAD_FRAME_TILE ? W - t0 : HEAD_FRAME_TILE;  // (<= 0 in the tile that holds row W alone)
        const int live = head_live(n, t0) * a.D4;                             // pieces below this index are copies
        const float4* src = a.feats + (size_t)(ffirst + start + t0) * a.D4;
        float4* dst = a.of + ((size_t)b * W + t0) * a.D4;
        for (int i = threadIdx.x; i < rows * a.D4; i += HEAD_THREADS) dst[i] = i < live ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- the small rows: word i of a tile is column i % cols of frame t0 + i / cols
    const int prow = W + 1 - t0 < HEAD_FRAME_TILE ? W + 1 - t0 : HEAD_FRAME_TILE;
    const size_t orow = (size_t)b * (W + 1) + t0;
    {
        const float* src = a.pose + (size_t)(first + start + t0) * 7;
        float* dst = a.head_pose + orow * 7;
        const int live = head_live(n_pose, t0) * 7;
        for (int i = threadIdx.x; i < prow * 7; i += HEAD_THREADS) dst[i] = i < live ? src[i] : 0.f;
    }
    {
        const int rows = W - t0 < HEAD_FRAME_TILE ? W - t0 : HEAD_FRAME_TILE;
        const float* src = a.vels + (size_t)(first + start + t0) * 6;
        float* dst = a.head_vels + ((size_t)b * W + t0) * 6;
        const int live = head_live(n, t0) * 6;
        for (int i = threadIdx.x; i < rows * 6; i += HEAD_THREADS) dst[i] = i < live ? src[i] : 0.f;
    }
    if (a.slam32) {
        const float* src = a.slam32 + (size_t)(sfirst + start + t0) * SLAM_COLS;
        const int live = head_live(n_slam, t0) * SLAM_COLS;
        for (int i = threadIdx.x; i < prow * SLAM_COLS; i += HEAD_THREADS) {
            const int r = i / SLAM_COLS, c = i - r * SLAM_COLS;
            const float v = i < live ? src[i] : 0.f;
            const size_t o = orow + r;
            if (c < 3) a.al_trans[o * 3 + c] = v;
            else if (c < 7) a.al_quat[o * 4 + (c - 3)] = v;
            else if (c < 16) a.al_rot[o * 9 + (c - 7)] = v;
            else if (c < 20) a.ori_quat[o * 4 + (c - 16)] = v;
            else a.ori_rot[o * 9 + (c - 20)] = v;
        }
        const double* src64 = a.slam_trans64 + (size_t)(sfirst + start + t0) * 3;
        double* dst64 = a.ori_trans + orow * 3;
        const int live64 = head_live(n_slam, t0) * 3;
        for (int i = threadIdx.x; i < prow * 3; i += HEAD_THREADS) dst64[i] = i < live64 ? src64[i] : 0.0;
    }
}

}  // namespace s1d
