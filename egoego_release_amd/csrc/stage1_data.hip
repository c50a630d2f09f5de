// stage1_data.hip — host side of egoego_s1_gravity_batch: one launch of stage1_data.h's kernel on the caller's stream.  No
// allocation, no copy through the host and no synchronisation.  egoego_s1_data_last_error() reads this unit's error slot.
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

}  // extern "C"
