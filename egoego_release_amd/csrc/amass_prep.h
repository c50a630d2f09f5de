// amass_prep.h — raw AMASS sequences -> the records of the reference's process_seq (utils/data_utils/process_amass_dataset.py
// 340-493) on the device, for a batch of sequences of different lengths and frame rates.  Frames are packed end to end: sequence b
// owns the raw frames offsets[b] .. offsets[b + 1]; nothing is padded to the longest sequence.
//
//   amass_joints_kernel  one fp64 thread per raw frame: Rodrigues, then the chain over the first 22 joints of the kintree with the
//                        model's J_template at zero betas; joints (+ trans) and the global rotation of the head (joint 15), each
//                        rounded once to fp32.  No joint below 22 has an ancestor at or beyond 22, so the hands' pose and the
//                        6890 vertices the reference computes on the way never reach Jtr[:, :22].
//   amass_floor_kernel   determine_floor_height_and_contacts (:160-338) at the raw frame rate, one 1024-thread workgroup per
//                        sequence: floor_common.h's floor_body<LONG> (steps 1-7 there), which eval_floor_kernel (eval_metrics.h)
//                        runs too.  A sequence of at most evalm::MAX_T frames keeps its arrays in LDS with a 12-bit frame field;
//                        a longer one (up to MAX_LEN frames) keeps them in its slice of the caller's workspace with a 32-bit
//                        frame and a 32-bit compacted index, and gives the same bits.  Still one workgroup per sequence: every
//                        hand-off is a __syncthreads(); no workgroup reads what another wrote.
//   amass_head_kernel    one fp64 thread per output frame: the gather through the downsample table, the floor shift, and the head
//                        tracks (:454-472 with get_head_vel :111-137).
#pragma once
#include "floor_common.h"
#include "quat_f64.h"

namespace amass {

using evalm::NJ;
using evalm::HEAD;
using evalm::MAX_LEN;

static constexpr int THREADS = evalm::FC_THREADS;
static constexpr int WS_BYTES_PER_ELEM = 8 + 4 * 6 + 1;        // sp (8), sh, lab, gmed, gsz, rootv, mask (4 each), vf (1)

// workspace elements: sequence b's slice of every array starts at element 4 * offsets[b] + 2 * b and holds 4 L + 2 of them
// (the sort pads 2 L samples to the next power of two, below 4 L; an empty sequence still writes two)
EG_HD size_t ws_elems(int n_frames, int B) { return 4 * (size_t)n_frames + 2 * (size_t)B; }

// ---------------------------------------------------------------- joints
struct JointArgs {
    const float* root_orient;  // [N][3]
    const float* pose_body;    // [N][63]
    const float* trans;        // [N][3]
    const float* j_template;   // [22][3] rest joints at zero betas
    float* joints;             // [N][22][3]
    float* head_rot;           // [N][9] row-major
    int parents[NJ];
    int N;
};

__global__ void amass_joints_kernel(JointArgs a) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.N) return;
    const float* ro = a.root_orient + 3 * (size_t)f;
    const float* pb = a.pose_body + 63 * (size_t)f;
    double G[NJ][9], t[NJ][3];
    rodrigues(ro[0], ro[1], ro[2], G[0]);
    t[0][0] = a.j_template[0]; t[0][1] = a.j_template[1]; t[0][2] = a.j_template[2];
    for (int j = 1; j < NJ; ++j) {
        const int p = a.parents[j];
        double R[9];
        rodrigues(pb[3 * (j - 1)], pb[3 * (j - 1) + 1], pb[3 * (j - 1) + 2], R);
        const double d[3] = {(double)a.j_template[3 * j] - (double)a.j_template[3 * p],
                             (double)a.j_template[3 * j + 1] - (double)a.j_template[3 * p + 1],
                             (double)a.j_template[3 * j + 2] - (double)a.j_template[3 * p + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            t[j][r] = G[p][3 * r] * d[0] + G[p][3 * r + 1] * d[1] + G[p][3 * r + 2] * d[2] + t[p][r];
#pragma unroll
            for (int c = 0; c < 3; ++c) G[j][3 * r + c] = G[p][3 * r] * R[c] + G[p][3 * r + 1] * R[3 + c] + G[p][3 * r + 2] * R[6 + c];
        }
    }
    const double tx = a.trans[3 * (size_t)f], ty = a.trans[3 * (size_t)f + 1], tz = a.trans[3 * (size_t)f + 2];
    float* jo = a.joints + (size_t)f * NJ * 3;
    for (int j = 0; j < NJ; ++j) {
        jo[3 * j] = (float)(t[j][0] + tx); jo[3 * j + 1] = (float)(t[j][1] + ty); jo[3 * j + 2] = (float)(t[j][2] + tz);
    }
    float* ho = a.head_rot + (size_t)f * 9;
    for (int k = 0; k < 9; ++k) ho[k] = (float)G[HEAD][k];
}

// ---------------------------------------------------------------- floor height and contacts
struct FloorArgs {
    const float* jpos;       // [N][22][3]
    const int* offsets;      // [B + 1]
    const int* size_thresh;  // [B]: int(0.25 * fps) of each sequence
    float* floor_h;          // [B]
    float* offset_h;         // [B]
    float* contacts;         // [N][22]
    int* discard;            // [B]
    int* labels;             // [2 N]: sequence b's 2 L labels from 2 * offsets[b], in compacted order, -2 past n_static; or nullptr
    int* n_static;           // [B]
    int* n_groups;           // [B]
    unsigned char* ws;       // WS_BYTES_PER_ELEM * ws_elems(N, B) bytes
    int B, N, cap, force_long;  // cap: power of two >= 64, the LDS layout evalm::floor_lds(cap) of the short path
};

// floor_common.h's floor_body on packed sequences: sequence b owns the frames offsets[b] .. offsets[b + 1] and writes its L rows
__global__ void __launch_bounds__(THREADS) amass_floor_kernel(FloorArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
    __shared__ float s_pair[2];
    __shared__ unsigned long long s_best;
    const int b = blockIdx.x;
    // whatever the offsets hold, a sequence stays inside the N frames and inside its slice of the workspace
    const int o0 = min(max(a.offsets[b], 0), a.N);
    const int L = min(min(max(a.offsets[b + 1], o0), a.N) - o0, MAX_LEN);
    const evalm::FloorSeq q{a.jpos + (size_t)o0 * NJ * 3, L, a.size_thresh[b], a.contacts + (size_t)o0 * NJ, L,
                            a.labels ? a.labels + 2 * (size_t)o0 : nullptr, 2 * L,
                            a.floor_h + b, a.offset_h + b, a.discard + b, a.n_static + b, a.n_groups + b};
    if (!a.force_long && 2 * L <= a.cap && L <= evalm::MAX_T) {
        evalm::floor_body<false>(q, evalm::floor_mem_lds(fc_lds, a.cap), s_pair, &s_best);
    } else {
        const size_t E = ws_elems(a.N, a.B), e0 = 4 * (size_t)o0 + 2 * (size_t)b;
        evalm::FloorMem<true> m;
        m.sp = (unsigned long long*)a.ws + e0;
        unsigned char* p = a.ws + 8 * E;
        m.sh = (float*)p + e0;             p += 4 * E;
        m.lab = (int*)p + e0;              p += 4 * E;
        m.gmed = (float*)p + e0;           p += 4 * E;
        m.gsz = (int*)p + e0;              p += 4 * E;
        m.rootv = (float*)p + e0;          p += 4 * E;
        m.mask = (uint32_t*)p + e0;        p += 4 * E;
        m.vf = p + e0;
        m.part = (int*)(fc_lds + evalm::floor_lds(a.cap).part);
        evalm::floor_body<true>(q, m, s_pair, &s_best);
    }
}

// ---------------------------------------------------------------- head tracks
struct HeadArgs {
    const float* joints;       // [N][22][3] raw frames, before the floor shift
    const float* head_rot;     // [N][9]
    const float* contacts;     // [N][22]
    const float* floor_h;      // [B]: the offset floor height each sequence's z is shifted by
    const int* src;            // [M]: the raw frame of each output frame (the downsample table plus the sequence's first frame)
    const int* seq;            // [M]: the sequence of each output frame
    const int* out_offsets;    // [B + 1]: sequence b's output frames
    float* joints_out;         // [M][22][3]
    double* contacts_out;      // [M][22]
    float* head_trans;         // [M][3]
    float* rot6d;              // [M][6]
    float* qpos;               // [M][7]
    float* rot6d_diff;         // [M][6]; a sequence's last row is zero
    float* trans_diff;         // [M][3]; a sequence's last row is zero
    float* vels;               // [M][6]
    uint8_t* same;             // [M]: 1 where the pair (t, t + 1) took the |1 -+ q0| < 1e-6 branch
    int M, N, B;
};

// pytorch3d's matrix_to_quaternion: the candidate of the largest |component|, then w >= 0
EG_D void mat_to_quat(const double (&R)[9], double (&q)[4]) {
    const double m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5], m20 = R[6], m21 = R[7], m22 = R[8];
    const double qa[4] = {sqrt(fmax(1.0 + m00 + m11 + m22, 0.0)), sqrt(fmax(1.0 + m00 - m11 - m22, 0.0)),
                          sqrt(fmax(1.0 - m00 + m11 - m22, 0.0)), sqrt(fmax(1.0 - m00 - m11 + m22, 0.0))};
    int k = 0;
    for (int i = 1; i < 4; ++i)
        if (qa[i] > qa[k]) k = i;
    double c[4];
    if (k == 0) { c[0] = qa[0] * qa[0]; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01; }
    else if (k == 1) { c[0] = m21 - m12; c[1] = qa[1] * qa[1]; c[2] = m10 + m01; c[3] = m02 + m20; }
    else if (k == 2) { c[0] = m02 - m20; c[1] = m10 + m01; c[2] = qa[2] * qa[2]; c[3] = m12 + m21; }
    else { c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = qa[3] * qa[3]; }
    const double d = 2.0 * fmax(qa[k], 0.1), sgn = c[0] < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 4; ++i) q[i] = sgn * c[i] / d;
}
// pytorch3d's quaternion_to_matrix (two_s = 2 / |q|^2), applied transposed: o = R(q)^T v
EG_D void quat_rot_t(double w, double x, double y, double z, const double (&v)[3], double (&o)[3]) {
    const double s = 2.0 / (w * w + x * x + y * y + z * z);
    const double R[9] = {1.0 - s * (y * y + z * z), s * (x * y - z * w),       s * (x * z + y * w),
                         s * (x * y + z * w),       1.0 - s * (x * x + z * z), s * (y * z - x * w),
                         s * (x * z - y * w),       s * (y * z + x * w),       1.0 - s * (x * x + y * y)};
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = R[c] * v[0] + R[3 + c] * v[1] + R[6 + c] * v[2];
}

struct HeadFrame {
    float pos[3];  // the head joint after the floor shift, fp32
    float q[4];    // head_qpos' quaternion, fp32
    double R[9];
};
EG_D HeadFrame head_frame(const HeadArgs& a, int s, float floor) {
    HeadFrame h;
    const float* p = a.joints + ((size_t)s * NJ + HEAD) * 3;
    h.pos[0] = p[0]; h.pos[1] = p[1]; h.pos[2] = p[2] - floor;
    for (int k = 0; k < 9; ++k) h.R[k] = (double)a.head_rot[(size_t)s * 9 + k];
    double q[4];
    mat_to_quat(h.R, q);
    for (int k = 0; k < 4; ++k) h.q[k] = (float)q[k];
    return h;
}

__global__ void amass_head_kernel(HeadArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int b = min(max(a.seq[i], 0), a.B - 1);
    const int lo = min(max(a.out_offsets[b], 0), a.M), hi = min(max(a.out_offsets[b + 1], lo), a.M);
    const int s = min(max(a.src[i], 0), a.N - 1);
    const float floor = a.floor_h[b];
    const float* ji = a.joints + (size_t)s * NJ * 3;
    float* jo = a.joints_out + (size_t)i * NJ * 3;
    for (int j = 0; j < NJ; ++j) {
        jo[3 * j] = ji[3 * j]; jo[3 * j + 1] = ji[3 * j + 1]; jo[3 * j + 2] = ji[3 * j + 2] - floor;
        a.contacts_out[(size_t)i * NJ + j] = (double)a.contacts[(size_t)s * NJ + j];
    }
    const HeadFrame h = head_frame(a, s, floor);
    for (int c = 0; c < 3; ++c) a.head_trans[3 * (size_t)i + c] = a.qpos[7 * (size_t)i + c] = h.pos[c];
    for (int c = 0; c < 4; ++c) a.qpos[7 * (size_t)i + 3 + c] = h.q[c];
    for (int c = 0; c < 6; ++c) a.rot6d[6 * (size_t)i + c] = a.head_rot[(size_t)s * 9 + c];

    const bool last = i + 1 >= hi;
    // the pair the velocity comes from: (i, i + 1), or for a sequence's last frame the pair before it (:135)
    const int i0 = last ? i - 1 : i;
    if (last) {
        for (int c = 0; c < 6; ++c) a.rot6d_diff[6 * (size_t)i + c] = 0.f;
        for (int c = 0; c < 3; ++c) a.trans_diff[3 * (size_t)i + c] = 0.f;
    }
    if (i0 < lo || i0 + 1 >= hi || i < lo) {  // a one-frame sequence has no pair
        for (int c = 0; c < 6; ++c) a.vels[6 * (size_t)i + c] = 0.f;
        a.same[i] = 0;
        return;
    }
    const int s1 = min(max(a.src[i0 + 1], 0), a.N - 1);
    const HeadFrame cur = last ? head_frame(a, min(max(a.src[i0], 0), a.N - 1), floor) : h;
    const HeadFrame nxt = last ? h : head_frame(a, s1, floor);
    if (!last) {
        // R[t]^-1 R[t + 1], the first two rows; the fp32 difference of the fp32 head positions
        for (int r = 0; r < 2; ++r)
            for (int c = 0; c < 3; ++c)
                a.rot6d_diff[6 * (size_t)i + 3 * r + c] = (float)(cur.R[r] * nxt.R[c] + cur.R[3 + r] * nxt.R[3 + c] + cur.R[6 + r] * nxt.R[6 + c]);
        for (int c = 0; c < 3; ++c) a.trans_diff[3 * (size_t)i + c] = nxt.pos[c] - cur.pos[c];
    }
    // get_head_vel (:111-137), dt = 1 / 30
    const double dt = 1.0 / 30.0;
    const double cw = cur.q[0], cx = cur.q[1], cy = cur.q[2], cz = cur.q[3];
    const double v[3] = {((double)nxt.pos[0] - (double)cur.pos[0]) / dt, ((double)nxt.pos[1] - (double)cur.pos[1]) / dt,
                         ((double)nxt.pos[2] - (double)cur.pos[2]) / dt};
    const double hn = sqrt(cw * cw + cz * cz);  // |(w, 0, 0, z)|
    double lin[3];
    quat_rot_t(cw / hn, 0.0, 0.0, cz / hn, v, lin);
    // qrel = next * conj(cur), standardised
    const double nw = nxt.q[0], nx = nxt.q[1], ny = nxt.q[2], nz = nxt.q[3];
    double r0 = nw * cw + nx * cx + ny * cy + nz * cz, r1 = -nw * cx + nx * cw - ny * cz + nz * cy,
           r2 = -nw * cy + nx * cz + ny * cw - nz * cx, r3 = -nw * cz - nx * cy + ny * cx + nz * cw;
    if (r0 < 0.0) { r0 = -r0; r1 = -r1; r2 = -r2; r3 = -r3; }
    double axis[3] = {1.0, 0.0, 0.0}, angle = 0.0;
    const bool same = fabs(1.0 - r0) < 1e-6 || fabs(1.0 + r0) < 1e-6;
    if (!same) {
        angle = 2.0 * acos(r0);
        const double sn = sin(angle / 2.0);
        axis[0] = r1 / sn; axis[1] = r2 / sn; axis[2] = r3 / sn;
        const double an = sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
        axis[0] /= an; axis[1] /= an; axis[2] /= an;
    }
    if (angle > 3.141592653589793) angle -= 2.0 * 3.141592653589793;
    const double rv[3] = {axis[0] * angle / dt, axis[1] * angle / dt, axis[2] * angle / dt};
    double ang[3];
    quat_rot_t(cw, cx, cy, cz, rv, ang);
    for (int c = 0; c < 3; ++c) {
        a.vels[6 * (size_t)i + c] = (float)lin[c];
        a.vels[6 * (size_t)i + 3 + c] = (float)ang[c];
    }
    a.same[i] = same ? 1 : 0;
}

}  // namespace amass
