// stage1_data.hip — host side of egoego_s1_gravity_batch and egoego_s1_head_batch: one launch each of a kernel of stage1_data.h
// on the caller's stream.  No allocation, no copy through the host and no synchronisation.  egoego_s1_data_last_error() reads this unit's error slot.
#include "host_util.h"
#include "stage1_data.h"

extern "C" {

const char* egoego_s1_data_last_error(void) { return last_err.c_str(); }

int egoego_s1_gravity_batch(const float* d_pose, int n_rows, const int32_t* d_offsets, int n_seqs, const int32_t* d_seq_ids,
                            const int64_t* d_draw_ids, int B, int window, uint64_t seed, int for_eval, const int32_t* d_start,
                            const float* d_rot, const float* d_scale, float* d_ori_head_pose, float* d_head_rot_mat, float* d_head_trans,
                            int32_t* d_seq_len, float* d_aligned_rot_mat, float* d_aligned_scale, float* d_floor_normal,
                            int32_t* d_start_t_idx, float* d_aug_scale, void* stream) {
    if (window < 1 || window > (1 << 20)) return fail(EGOEGO_E_INVALID, "window = %d: 1 .. 2^20 expected", window);
    if (B < 1) return fail(EGOEGO_E_INVALID, "B = %d: must be positive", B);
    if (n_rows < 1 || n_seqs < 1) return fail(EGOEGO_E_INVALID, "n_rows = %d, n_seqs = %d: must be positive", n_rows, n_seqs);
    if (!d_pose || !d_offsets || !d_seq_ids || !d_draw_ids) return fail(EGOEGO_E_INVALID, "an input pointer is NULL");
    if (!d_ori_head_pose || !d_head_rot_mat || !d_head_trans || !d_seq_len || !d_aligned_rot_mat || !d_aligned_scale || !d_floor_normal ||
        !d_start_t_idx || !d_aug_scale)
        return fail(EGOEGO_E_INVALID, "an output pointer is NULL");
    s1d::GravityBatch a;
    a.pose = d_pose; a.offsets = d_offsets; a.seq_ids = d_seq_ids; a.draw_ids = d_draw_ids;
    a.start = d_start; a.rot = d_rot; a.scale = d_scale;
    a.N = n_rows; a.S = n_seqs; a.W = window; a.for_eval = for_eval ? 1 : 0;
    a.seed = seed;
    a.ori = d_ori_head_pose; a.rotm = d_head_rot_mat; a.trans = d_head_trans;
    a.seq_len = d_seq_len;
    a.aligned_rot = d_aligned_rot_mat; a.aligned_scale = d_aligned_scale; a.normal = d_floor_normal;
    a.start_out = d_start_t_idx; a.scale_out = d_aug_scale;
    hipLaunchKernelGGL(s1d::gravity_batch_kernel, dim3(B), dim3(s1d::THREADS), 0, as_stream(stream), a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_s1_head_batch(const float* d_pose, const float* d_vels, const float* d_feats, int n_rows, int d_feats_dim,
                         const int32_t* d_offsets, int n_seqs, const float* d_slam32, const double* d_slam_trans64,
                         const int32_t* d_slam_offsets, int n_slam_rows, const int32_t* d_seq_ids, const int64_t* d_draw_ids, int B,
                         int window, uint64_t seed, int for_eval, const int32_t* d_start, float* d_head_pose, float* d_head_vels,
                         float* d_of, int32_t* d_seq_len, int32_t* d_start_t_idx, float* d_aligned_slam_trans,
                         float* d_aligned_slam_rot_quat, float* d_aligned_slam_rot_mat, double* d_ori_slam_trans,
                         float* d_ori_slam_rot_quat, float* d_ori_slam_rot_mat, int32_t* d_pose_len, void* stream) {
    if (window < 1 || window > (1 << 20)) return fail(EGOEGO_E_INVALID, "window = %d: 1 .. 2^20 expected", window);
    if (B < 1) return fail(EGOEGO_E_INVALID, "B = %d: must be positive", B);
    if (d_feats_dim < 4 || d_feats_dim % 4 != 0 || d_feats_dim > (1 << 16))
        return fail(EGOEGO_E_INVALID, "D = %d: a multiple of 4 in 4 .. 2^16 expected (rows move 16 bytes per lane)", d_feats_dim);
    if (n_rows < 1 || n_seqs < 1 || n_seqs > n_rows)
        return fail(EGOEGO_E_INVALID, "n_rows = %d, n_seqs = %d: 1 <= n_seqs <= n_rows expected", n_rows, n_seqs);
    if (!d_pose || !d_vels || !d_feats || !d_offsets || !d_seq_ids || !d_draw_ids) return fail(EGOEGO_E_INVALID, "an input pointer is NULL");
    if (!d_head_pose || !d_head_vels || !d_of || !d_seq_len || !d_start_t_idx) return fail(EGOEGO_E_INVALID, "an output pointer is NULL");
    const int n_tables = (d_slam32 != nullptr) + (d_slam_trans64 != nullptr) + (d_slam_offsets != nullptr);
    const int n_outs = (d_aligned_slam_trans != nullptr) + (d_aligned_slam_rot_quat != nullptr) + (d_aligned_slam_rot_mat != nullptr) +
                       (d_ori_slam_trans != nullptr) + (d_ori_slam_rot_quat != nullptr) + (d_ori_slam_rot_mat != nullptr) +
                       (d_pose_len != nullptr);
    if (n_tables != 0 && n_tables != 3) return fail(EGOEGO_E_INVALID, "%d of the 3 SLAM tables given: all or none expected", n_tables);
    if (n_outs != 0 && n_outs != 7) return fail(EGOEGO_E_INVALID, "%d of the 7 SLAM outputs given: all or none expected", n_outs);
    if ((n_tables == 3) != (n_outs == 7)) return fail(EGOEGO_E_INVALID, "the SLAM tables and the SLAM outputs go together");
    if (n_tables == 3 && n_slam_rows < 0) return fail(EGOEGO_E_INVALID, "n_slam_rows = %d: must not be negative", n_slam_rows);
    const int tiles = (window + 1 + s1d::HEAD_FRAME_TILE - 1) / s1d::HEAD_FRAME_TILE;
    if ((long long)tiles * B > 0x7fffffffLL) return fail(EGOEGO_E_INVALID, "B = %d at window = %d: more workgroups than one launch has", B, window);
    s1d::HeadBatch a;
    a.pose = d_pose; a.vels = d_vels; a.feats = reinterpret_cast<const float4*>(d_feats); a.offsets = d_offsets;
    a.slam32 = d_slam32; a.slam_trans64 = d_slam_trans64; a.slam_offsets = d_slam_offsets;
    a.seq_ids = d_seq_ids; a.draw_ids = d_draw_ids; a.start = d_start;
    a.N = n_rows; a.S = n_seqs; a.M = n_tables == 3 ? n_slam_rows : 0; a.D4 = d_feats_dim / 4; a.W = window;
    a.for_eval = for_eval ? 1 : 0; a.tiles = tiles;
    a.seed = seed;
    a.head_pose = d_head_pose; a.head_vels = d_head_vels; a.of = reinterpret_cast<float4*>(d_of);
    a.seq_len = d_seq_len; a.start_out = d_start_t_idx;
    a.al_trans = d_aligned_slam_trans; a.al_quat = d_aligned_slam_rot_quat; a.al_rot = d_aligned_slam_rot_mat;
    a.ori_trans = d_ori_slam_trans; a.ori_quat = d_ori_slam_rot_quat; a.ori_rot = d_ori_slam_rot_mat;
    a.pose_len = d_pose_len;
    hipLaunchKernelGGL(s1d::head_batch_kernel, dim3((unsigned)(tiles * B)), dim3(s1d::HEAD_THREADS), 0, as_stream(stream), a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
