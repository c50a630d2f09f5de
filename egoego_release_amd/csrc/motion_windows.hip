// motion_windows.hip — the C ABI (include/egoego_hip.h, egoego_win_*) of the stage-2 motion windows.  Kernels: motion_windows.h.
// The entries keep no state: no context; the statistics take a caller's workspace.  Nothing here touches another code path.
#include "host_util.h"
#include "motion_windows.h"

using namespace mwin;

static int check_nw(int N, int W) {
    if (N < 1 || W < 1 || W > MAX_W) return fail(EGOEGO_E_INVALID, "bad shape (N=%d, window=%d): N >= 1, window 1..%d", N, W, MAX_W);
    if ((int64_t)N * W > (int64_t)1 << 26) return fail(EGOEGO_E_INVALID, "N * window = %lld: at most 2^26 rows per call", (long long)N * W);
    return 0;
}
static int minmax_blocks(int64_t rows) { return (int)(rows < MM_MAX_BLOCKS ? rows : MM_MAX_BLOCKS); }

extern "C" {

const char* egoego_win_last_error(void) { return last_err.c_str(); }

int egoego_win_max_window(void) { return MAX_W; }

int egoego_win_build(const float* d_trans, const float* d_root_orient, const float* d_body_pose, int n_frames, const float* d_rest_offsets,
                     const int32_t* parents_host, const int32_t* d_first, const int32_t* d_length, int N, int W, int canonicalize,
                     float* d_jpos, float* d_jvel, float* d_grot6d, float* d_lrot6d, float* d_recover, void* stream) {
    if (!d_trans || !d_root_orient || !d_body_pose || !d_rest_offsets || !parents_host || !d_first || !d_length || !d_jpos || !d_jvel ||
        !d_grot6d || !d_lrot6d || !d_recover)
        return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_nw(N, W)) return rc;
    if (n_frames < 1 || n_frames > 1 << 28) return fail(EGOEGO_E_INVALID, "n_frames %d: 1..2^28 accepted", n_frames);
    BuildArgs a{d_trans, d_root_orient, d_body_pose, d_rest_offsets, d_first, d_length, d_jpos, d_jvel, d_grot6d, d_lrot6d, d_recover,
                {}, n_frames, N, W, canonicalize ? 1 : 0};
    for (int j = 0; j < NJ; ++j) {
        a.parents[j] = j ? parents_host[j] : 0;
        if (j > 0 && (a.parents[j] < 0 || a.parents[j] >= j))
            return fail(EGOEGO_E_INVALID, "parents[%d] = %d is not an earlier joint", j, a.parents[j]);
    }
    const size_t lds = build_lds_bytes(W);
    (void)hipGetLastError();
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void*)win_build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    win_build_kernel<<<N, CHUNK, lds, as_stream(stream)>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t egoego_win_stats_workspace_bytes(int N, int W) {
    if (N < 1 || W < 1) return 0;
    return (size_t)minmax_blocks((int64_t)N * W) * 4 * JP * sizeof(float);
}

int egoego_win_stats(const float* d_jpos, const float* d_jvel, const int32_t* d_length, int N, int W, float* d_stats, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!d_jpos || !d_jvel || !d_length || !d_stats) return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_nw(N, W)) return rc;
    if (int rc = check_workspace(workspace, workspace_bytes, egoego_win_stats_workspace_bytes(N, W))) return rc;
    const int G = minmax_blocks((int64_t)N * W);
    (void)hipGetLastError();
    win_minmax_kernel<<<G, MM_THREADS, 0, as_stream(stream)>>>(d_jpos, d_jvel, d_length, N * W, W, (float*)workspace);
    HIP_TRY(hipGetLastError());
    win_minmax_fold_kernel<<<(4 * JP + 63) / 64, 64, 0, as_stream(stream)>>>((const float*)workspace, G, d_stats);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_win_motion(const float* d_jpos, const float* d_grot6d, const int32_t* d_length, const float* d_jpos_min, const float* d_jpos_max,
                      int N, int W, float* d_motion, void* stream) {
    if (!d_jpos || !d_grot6d || !d_length || !d_jpos_min || !d_jpos_max || !d_motion) return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_nw(N, W)) return rc;
    const size_t total = (size_t)N * W * FEATS;
    const size_t g = (total + 255) / 256;
    (void)hipGetLastError();
    win_motion_kernel<<<(unsigned)(g < 65535 ? g : 65535), 256, 0, as_stream(stream)>>>(d_jpos, d_grot6d, d_length, d_jpos_min, d_jpos_max,
                                                                                        (size_t)N * W, W, d_motion);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
