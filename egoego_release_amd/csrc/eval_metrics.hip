// eval_metrics.hip — the C ABI (include/egoego_hip.h, egoego_eval_*) of the batched evaluation.  Kernels: eval_metrics.h.  The
// entries keep no state: no context, no workspace.  Nothing here touches another code path.
#include "host_util.h"
#include "eval_metrics.h"

using namespace evalm;

static int check_bt(int B, int T) {
    if (B < 1 || T < 1) return fail(EGOEGO_E_INVALID, "bad shape (B=%d, T=%d)", B, T);
    if ((int64_t)B * T > (int64_t)1 << 24) return fail(EGOEGO_E_INVALID, "B * T = %lld: at most 2^24 frames per call", (long long)B * T);
    return 0;
}
static unsigned grid_for(size_t n, int block) {
    const size_t g = (n + block - 1) / block;
    return (unsigned)(g < 65535 ? g : 65535);
}

extern "C" {

const char* egoego_eval_last_error(void) { return last_err.c_str(); }

int egoego_eval_max_frames(void) { return MAX_T; }

int egoego_eval_fk(const float* d_root, const float* d_aa, const float* d_rest_offsets, const int32_t* parents_host, int N, float* d_quat,
                   float* d_jpos, void* stream) {
    if (!d_root || !d_aa || !d_rest_offsets || !parents_host || !d_quat || !d_jpos) return fail(EGOEGO_E_INVALID, "NULL argument");
    if (N < 1 || N > 1 << 24) return fail(EGOEGO_E_INVALID, "n_frames %d: 1..2^24 accepted", N);
    FkArgs a{d_root, d_aa, d_rest_offsets, d_quat, d_jpos, {}, N};
    for (int j = 0; j < NJ; ++j) {
        a.parents[j] = j ? parents_host[j] : 0;
        if (j > 0 && (a.parents[j] < 0 || a.parents[j] >= j))
            return fail(EGOEGO_E_INVALID, "parents[%d] = %d is not an earlier joint", j, a.parents[j]);
    }
    (void)hipGetLastError();
    eval_fk_kernel<<<(N + 63) / 64, 64, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_eval_shift_xy(float* d_jpos, int B, int T, int joint, void* stream) {
    if (!d_jpos) return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_bt(B, T)) return rc;
    if (joint < 0 || joint >= NJ) return fail(EGOEGO_E_INVALID, "joint %d: 0..21 accepted", joint);
    (void)hipGetLastError();
    eval_shift_xy_kernel<<<grid_for((size_t)B * T * NJ, 256), 256, 0, (hipStream_t)stream>>>(d_jpos, B, T, joint);
    HIP_TRY(hipGetLastError());
    eval_shift_xy_origin_kernel<<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(d_jpos, B, T, joint);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_eval_floor_contacts(const float* d_jpos, const int32_t* d_lengths, int B, int T, float fps, float* d_floor_height,
                               float* d_offset_floor_height, float* d_contacts, int32_t* d_discard, int32_t* d_labels,
                               int32_t* d_n_static, int32_t* d_n_groups, void* stream) {
    if (!d_jpos || !d_floor_height || !d_offset_floor_height || !d_contacts || !d_discard || !d_n_static || !d_n_groups)
        return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_bt(B, T)) return rc;
    if (T > MAX_T) return fail(EGOEGO_E_INVALID, "T = %d frames: at most %d per sequence (2 T samples must fit the LDS)", T, MAX_T);
    if (!(fps >= 0.f) || fps > 1e6f) return fail(EGOEGO_E_INVALID, "fps %g: 0..1e6 accepted", (double)fps);
    const int cap = floor_cap(T);
    const size_t lds = floor_lds(cap).total;
    FloorArgs a{d_jpos, d_lengths, d_floor_height, d_offset_floor_height, d_contacts, d_discard, d_labels, d_n_static, d_n_groups,
                B, T, (int)(0.25 * (double)fps), cap};
    (void)hipGetLastError();
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void*)eval_floor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    eval_floor_kernel<<<B, FC_THREADS, lds, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_eval_metrics(const float* d_gt_quat, const float* d_gt_jpos, int gt_shared, const float* d_gt_floor_height,
                        const float* d_pred_quat, const float* d_pred_jpos, const float* d_pred_floor_height,
                        const int32_t* d_lengths, int B, int T, double* d_out, void* stream) {
    if (!d_gt_quat || !d_gt_jpos || !d_gt_floor_height || !d_pred_quat || !d_pred_jpos || !d_pred_floor_height || !d_out)
        return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_bt(B, T)) return rc;
    MetricArgs a{d_gt_quat, d_gt_jpos, d_pred_quat, d_pred_jpos, d_gt_floor_height, d_pred_floor_height, d_lengths, d_out, B, T,
                 gt_shared ? 1 : 0};
    (void)hipGetLastError();
    eval_metrics_kernel<<<B, MT_THREADS, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_eval_root_to_floor(const float* d_jpos, const float* d_floor_height, int B, int T, float* d_root, void* stream) {
    if (!d_jpos || !d_floor_height || !d_root) return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_bt(B, T)) return rc;
    (void)hipGetLastError();
    eval_root_to_floor_kernel<<<grid_for((size_t)B * T, 256), 256, 0, (hipStream_t)stream>>>(d_jpos, d_floor_height, B, T, d_root);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_eval_best(const double* d_metrics, int column, const int32_t* d_group, int B, int n_groups, int32_t* d_best, void* stream) {
    if (!d_metrics || !d_best) return fail(EGOEGO_E_INVALID, "NULL argument");
    if (B < 1 || n_groups < 1 || column < 0 || column >= N_METRICS)
        return fail(EGOEGO_E_INVALID, "bad shape (B=%d, n_groups=%d, column=%d)", B, n_groups, column);
    (void)hipGetLastError();
    eval_best_kernel<<<grid_for((size_t)n_groups, 64), 64, 0, (hipStream_t)stream>>>(d_metrics, N_METRICS, column, d_group, B, n_groups, d_best);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
