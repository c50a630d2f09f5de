// amass_prep.hip — the C ABI (include/egoego_hip.h, egoego_amass_*) of the AMASS preprocessing.  Kernels: amass_prep.h.  The
// entries keep no state: no context; the floor kernel takes a caller's workspace.  Nothing here touches another code path.
#include "host_util.h"
#include "amass_prep.h"

using namespace amass;

static int check_frames(int N) {
    if (N < 1 || N > 1 << 24) return fail(EGOEGO_E_INVALID, "n_frames %d: 1..2^24 accepted", N);
    return 0;
}

extern "C" {

const char* egoego_amass_last_error(void) { return last_err.c_str(); }

int egoego_amass_max_frames(void) { return MAX_LEN; }

int egoego_amass_joints(const float* d_root_orient, const float* d_pose_body, const float* d_trans, const float* d_j_template,
                        const int32_t* parents_host, int n_frames, float* d_joints, float* d_head_rot, void* stream) {
    if (!d_root_orient || !d_pose_body || !d_trans || !d_j_template || !parents_host || !d_joints || !d_head_rot)
        return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_frames(n_frames)) return rc;
    JointArgs a{d_root_orient, d_pose_body, d_trans, d_j_template, d_joints, d_head_rot, {}, n_frames};
    for (int j = 0; j < NJ; ++j) {
        a.parents[j] = j ? parents_host[j] : 0;
        if (j > 0 && (a.parents[j] < 0 || a.parents[j] >= j))
            return fail(EGOEGO_E_INVALID, "parents[%d] = %d is not an earlier joint", j, a.parents[j]);
    }
    (void)hipGetLastError();
    amass_joints_kernel<<<(n_frames + 63) / 64, 64, 0, as_stream(stream)>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t egoego_amass_floor_workspace_bytes(int n_frames, int B) {
    if (n_frames < 1 || n_frames > 1 << 24 || B < 1 || B > n_frames) return 0;
    return (WS_BYTES_PER_ELEM * ws_elems(n_frames, B) + 255) / 256 * 256;
}

int egoego_amass_floor_contacts(const float* d_joints, const int32_t* offsets_host, const int32_t* d_offsets, const int32_t* d_size_thresh,
                                int B, int force_long, float* d_floor_height, float* d_offset_floor_height, float* d_contacts,
                                int32_t* d_discard, int32_t* d_labels, int32_t* d_n_static, int32_t* d_n_groups, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (!d_joints || !offsets_host || !d_offsets || !d_size_thresh || !d_floor_height || !d_offset_floor_height || !d_contacts ||
        !d_discard || !d_n_static || !d_n_groups)
        return fail(EGOEGO_E_INVALID, "NULL argument");
    if (B < 1 || B > 1 << 24) return fail(EGOEGO_E_INVALID, "B = %d: 1..2^24 sequences accepted", B);
    if (offsets_host[0] != 0) return fail(EGOEGO_E_INVALID, "offsets[0] = %d: 0 expected", offsets_host[0]);
    int longest_short = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t L = (int64_t)offsets_host[b + 1] - offsets_host[b];
        if (L < 1) return fail(EGOEGO_E_INVALID, "sequence %d has %lld frames: at least 1 expected", b, (long long)L);
        if (L > MAX_LEN) return fail(EGOEGO_E_INVALID, "sequence %d has %lld frames: at most %d per sequence", b, (long long)L, MAX_LEN);
        if (offsets_host[b + 1] > 1 << 24) return fail(EGOEGO_E_INVALID, "offsets[%d] = %d: at most 2^24 frames per call", b + 1, offsets_host[b + 1]);
        if (!force_long && L <= evalm::MAX_T && L > longest_short) longest_short = (int)L;
    }
    const int N = offsets_host[B];
    if (int rc = check_workspace(workspace, workspace_bytes, egoego_amass_floor_workspace_bytes(N, B))) return rc;
    const int cap = evalm::floor_cap(longest_short);
    const size_t lds = evalm::floor_lds(cap).total;
    FloorArgs a{d_joints, d_offsets, d_size_thresh, d_floor_height, d_offset_floor_height, d_contacts, d_discard, d_labels, d_n_static,
                d_n_groups, (unsigned char*)workspace, B, N, cap, force_long ? 1 : 0};
    (void)hipGetLastError();
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void*)amass_floor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    amass_floor_kernel<<<B, THREADS, lds, as_stream(stream)>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int egoego_amass_head(const float* d_joints, const float* d_head_rot, const float* d_contacts, const float* d_offset_floor_height,
                      const int32_t* d_src, const int32_t* d_seq, const int32_t* d_out_offsets, int n_out, int n_frames, int B,
                      float* d_joints_out, double* d_contacts_out, float* d_head_trans, float* d_rot6d, float* d_qpos, float* d_rot6d_diff,
                      float* d_trans_diff, float* d_vels, uint8_t* d_same, void* stream) {
    if (!d_joints || !d_head_rot || !d_contacts || !d_offset_floor_height || !d_src || !d_seq || !d_out_offsets || !d_joints_out ||
        !d_contacts_out || !d_head_trans || !d_rot6d || !d_qpos || !d_rot6d_diff || !d_trans_diff || !d_vels || !d_same)
        return fail(EGOEGO_E_INVALID, "NULL argument");
    if (int rc = check_frames(n_frames)) return rc;
    if (n_out < 1 || n_out > n_frames || B < 1 || B > n_out)
        return fail(EGOEGO_E_INVALID, "bad shape (n_out=%d, n_frames=%d, B=%d): 1 <= B <= n_out <= n_frames", n_out, n_frames, B);
    HeadArgs a{d_joints, d_head_rot, d_contacts, d_offset_floor_height, d_src, d_seq, d_out_offsets, d_joints_out, d_contacts_out,
               d_head_trans, d_rot6d, d_qpos, d_rot6d_diff, d_trans_diff, d_vels, d_same, n_out, n_frames, B};
    (void)hipGetLastError();
    amass_head_kernel<<<(n_out + 63) / 64, 64, 0, as_stream(stream)>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
