// body_model.hip — context, model packing, workspace and the C ABI (include/egoego_hip.h, egoego_body_*) of the SMPL-H body
// model.  Kernels: body_model.h.  Nothing here touches another code path.
#include "host_util.h"
#include "body_model.h"

using namespace bodym;

static constexpr int DEFAULT_CHUNK = 8192;
static constexpr int MAX_BETAS = 512;

struct egoego_body_ctx {
    int device, chunk;
    bool loaded;
    int V, VG, nb, nw;
    DevMem mem;
    const float *v_template, *shapedirs, *j_template, *j_shapedirs, *skin_weight;
    const int *parents, *skin_joint;
    const uint16_t *phi, *plo;
};

static size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// workspace: v_shaped [S][V][3] | J [S][52][3] | A [Fc][52][12] | feature hi | feature lo ([ceil(Fc / 32)][30][512] bf16 each)
struct WsLayout {
    size_t v_shaped, J, A, fhi, flo, total;
};
static WsLayout ws_layout(const egoego_body_ctx* c, int n_frames, int n_seqs) {
    const size_t Fc = (size_t)(n_frames < c->chunk ? n_frames : c->chunk), MT = (Fc + 31) / 32;
    WsLayout w;
    size_t o = 0;
    w.v_shaped = o; o += align256((size_t)n_seqs * c->V * 3 * sizeof(float));
    w.J = o;        o += align256((size_t)n_seqs * NJ * 3 * sizeof(float));
    w.A = o;        o += align256(Fc * NJ * 12 * sizeof(float));
    w.fhi = o;      o += align256(MT * PK16 * 512 * sizeof(uint16_t));
    w.flo = o;      o += align256(MT * PK16 * 512 * sizeof(uint16_t));
    w.total = o;
    return w;
}

#define BD_LAUNCH(what)                                                                                                \
    do {                                                                                                               \
        hipError_t e_ = hipGetLastError();                                                                             \
        if (e_ != hipSuccess) return fail(EGOEGO_E_HIP, "body-model launch (%s) failed: %s", what, hipGetErrorString(e_)); \
    } while (0)

// Packs `m` into `c` on the current device; on failure the caller frees what was allocated so far.
static int pack_model(egoego_body_ctx* c, const egoego_body_model* m, void* stream) {
    HIP_TRY(hipStreamSynchronize(as_stream(stream)));  // the caller's tensors are written on its stream; the old model may still be read
    c->mem.free_all();
    c->loaded = false;
    const int V = m->n_verts, nb = m->n_betas, nw = m->n_weights, VG = (V + 31) / 32;
    std::vector<float> vt, sd, pd, jt, jsd, sw;
    std::vector<int32_t> par, sj;
    if (int rc = fetch(m->v_template, (size_t)V * 3, vt, "v_template")) return rc;
    if (nb)
        if (int rc = fetch(m->shapedirs, (size_t)V * 3 * nb, sd, "shapedirs")) return rc;
    if (int rc = fetch(m->posedirs, (size_t)V * 3 * K_FULL, pd, "posedirs")) return rc;
    if (int rc = fetch(m->j_template, (size_t)NJ * 3, jt, "j_template")) return rc;
    if (nb)
        if (int rc = fetch(m->j_shapedirs, (size_t)NJ * 3 * nb, jsd, "j_shapedirs")) return rc;
    if (int rc = fetch(m->parents, (size_t)NJ, par, "parents")) return rc;
    if (int rc = fetch(m->skin_joint, (size_t)nw * V, sj, "skin_joint")) return rc;
    if (int rc = fetch(m->skin_weight, (size_t)nw * V, sw, "skin_weight")) return rc;
    for (int j = 1; j < NJ; ++j)
        if (par[j] < 0 || par[j] >= j)
            return fail(EGOEGO_E_INVALID, "parents[%d] = %d: every joint's parent must precede it", j, par[j]);
    for (size_t i = 0; i < sj.size(); ++i)
        if (sj[i] < 0 || sj[i] >= NJ) return fail(EGOEGO_E_INVALID, "skin_joint[%zu] = %d is not a joint", i, sj[i]);
    if (!nb) {  // one zero direction keeps the kernels' pointers valid
        sd.assign(1, 0.f);
        jsd.assign(1, 0.f);
    }
    // posedirs (V, 3, 459) -> rows n' = 96 (v / 32) + 32 c + v % 32 of hi / lo fragment-tiled planes, K padded to 480
    const size_t plane = (size_t)VG * 3 * PK16 * 512;
    std::vector<uint16_t> hi(plane, 0), lo(plane, 0);
    for (int v = 0; v < V; ++v)
        for (int cc = 0; cc < 3; ++cc) {
            const int row = (v >> 5) * 96 + cc * 32 + (v & 31);
            const float* src = pd.data() + ((size_t)v * 3 + cc) * K_FULL;
            for (int k = 0; k < K_FULL; ++k) split_store(hi, lo, tiled_index(row, k, PK16), src[k]);
        }
    c->V = V; c->VG = VG; c->nb = nb; c->nw = nw;
    if (int rc = c->mem.upload(vt, &c->v_template)) return rc;
    if (int rc = c->mem.upload(sd, &c->shapedirs)) return rc;
    if (int rc = c->mem.upload(jt, &c->j_template)) return rc;
    if (int rc = c->mem.upload(jsd, &c->j_shapedirs)) return rc;
    if (int rc = c->mem.upload(par, &c->parents)) return rc;
    if (int rc = c->mem.upload(sj, &c->skin_joint)) return rc;
    if (int rc = c->mem.upload(sw, &c->skin_weight)) return rc;
    if (int rc = c->mem.upload(hi, &c->phi)) return rc;
    if (int rc = c->mem.upload(lo, &c->plo)) return rc;
    return 0;
}

extern "C" {

const char* egoego_body_last_error(void) { return last_err.c_str(); }

int egoego_body_ctx_create(int device, int chunk_frames, egoego_body_ctx** out) {
    if (!out) return fail(EGOEGO_E_INVALID, "NULL argument");
    *out = nullptr;
    if (chunk_frames < 0 || chunk_frames > 65536) return fail(EGOEGO_E_INVALID, "chunk_frames %d: 0..65536 accepted", chunk_frames);
    if (int rc = check_device(device)) return rc;
    egoego_body_ctx* c = new egoego_body_ctx();
    c->device = device;
    c->chunk = chunk_frames ? chunk_frames : DEFAULT_CHUNK;
    c->loaded = false;
    *out = c;
    return 0;
}

void egoego_body_ctx_destroy(egoego_body_ctx* c) { destroy_ctx(c); }

int egoego_body_load_model(egoego_body_ctx* c, const egoego_body_model* m, void* stream) {
    if (!c || !m) return fail(EGOEGO_E_INVALID, "NULL argument");
    // (the skin kernel puts four 32-vertex groups on each grid.y index: 2^22 vertices are 32768 of its 65535)
    if (m->n_verts < 1 || m->n_verts > (1 << 22)) return fail(EGOEGO_E_INVALID, "n_verts %d: 1..2^22 accepted", m->n_verts);
    if (m->n_betas < 0 || m->n_betas > MAX_BETAS) return fail(EGOEGO_E_INVALID, "n_betas %d: 0..%d accepted", m->n_betas, MAX_BETAS);
    if (m->n_weights < 1 || m->n_weights > NJ) return fail(EGOEGO_E_INVALID, "n_weights %d: 1..%d accepted", m->n_weights, NJ);
    DeviceGuard dev;
    if (int rc = dev.enter(c->device)) return rc;
    const int rc = pack_model(c, m, stream);
    if (rc == 0) c->loaded = true;
    else {
        c->mem.free_all();
        c->loaded = false;
    }
    return rc;
}

size_t egoego_body_workspace_bytes(const egoego_body_ctx* c, int n_frames, int n_seqs) {
    if (!c || !c->loaded) {
        fail(EGOEGO_E_STATE, "model not loaded");
        return 0;
    }
    if (n_frames < 1 || n_seqs < 1) {
        fail(EGOEGO_E_INVALID, "n_frames and n_seqs must be >= 1");
        return 0;
    }
    return ws_layout(c, n_frames, n_seqs).total;
}

int egoego_body_forward(egoego_body_ctx* c, const float* d_root_orient, const float* d_pose_body, const float* d_pose_hand,
                        const float* d_trans, const float* d_betas, const int32_t* d_seq, int N, int n_seqs, float* d_verts,
                        float* d_joints, float* d_pose_offsets, void* d_ws, size_t ws_n, void* stream) {
    if (!c || !d_root_orient || !d_pose_body || !d_trans || !d_betas || !d_seq || !d_verts || !d_joints)
        return fail(EGOEGO_E_INVALID, "NULL argument");
    if (!c->loaded) return fail(EGOEGO_E_STATE, "model not loaded");
    if (N < 1 || n_seqs < 1) return fail(EGOEGO_E_INVALID, "n_frames and n_seqs must be >= 1");
    const WsLayout L = ws_layout(c, N, n_seqs);
    if (int rc = check_workspace(d_ws, ws_n, L.total)) return rc;
    DeviceGuard dev;
    if (int rc = dev.enter(c->device)) return rc;
    (void)hipGetLastError();  // an error some earlier, unrelated call left pending is not ours to report
    hipStream_t s = as_stream(stream);
    char* ws = (char*)d_ws;
    float* v_shaped = (float*)(ws + L.v_shaped);
    float* J = (float*)(ws + L.J);
    float* A = (float*)(ws + L.A);
    __bf16* fhi = (__bf16*)(ws + L.fhi);
    __bf16* flo = (__bf16*)(ws + L.flo);
    const int chunk = N < c->chunk ? N : c->chunk;
    const int K16 = d_pose_hand ? PK16 : (K_BODY + 31) / 32 * 2;
    {
        const size_t n = (size_t)n_seqs * c->V * 3;
        body_shape_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(c->v_template, c->shapedirs, d_betas, c->V * 3, c->nb, n_seqs,
                                                                    v_shaped);
        BD_LAUNCH("v_shaped");
        const size_t nj = (size_t)n_seqs * NJ * 3;
        body_shape_kernel<<<(unsigned)((nj + 255) / 256), 256, 0, s>>>(c->j_template, c->j_shapedirs, d_betas, NJ * 3, c->nb, n_seqs,
                                                                     J);
        BD_LAUNCH("joints");
    }
    for (int f0 = 0; f0 < N; f0 += chunk) {
        const int F = N - f0 < chunk ? N - f0 : chunk;
        FrameArgs fa;
        fa.root = d_root_orient + (size_t)f0 * 3;
        fa.body = d_pose_body + (size_t)f0 * 63;
        fa.hand = d_pose_hand ? d_pose_hand + (size_t)f0 * 90 : nullptr;
        fa.trans = d_trans + (size_t)f0 * 3;
        fa.seq = d_seq + f0;
        fa.J = J; fa.parents = c->parents; fa.fhi = fhi; fa.flo = flo; fa.A = A;
        fa.joints = d_joints + (size_t)f0 * NJ * 3;
        fa.F = F; fa.S = n_seqs; fa.K16 = K16;
        body_frame_kernel<<<(F + 63) / 64, 64, 0, s>>>(fa);
        BD_LAUNCH("frames");
        SkinArgs sa;
        sa.fhi = (const u32x4*)fhi; sa.flo = (const u32x4*)flo;
        sa.phi = (const u32x4*)c->phi; sa.plo = (const u32x4*)c->plo;
        sa.v_shaped = v_shaped; sa.seq = fa.seq; sa.A = A; sa.trans = fa.trans;
        sa.skin_joint = c->skin_joint; sa.skin_weight = c->skin_weight;
        sa.verts = d_verts + (size_t)f0 * c->V * 3;
        sa.offsets = d_pose_offsets ? d_pose_offsets + (size_t)f0 * c->V * 3 : nullptr;
        sa.F = F; sa.S = n_seqs; sa.V = c->V; sa.VG = c->VG; sa.MT = (F + 31) / 32; sa.K16 = K16; sa.nw = c->nw;
        constexpr int TM = 2;
        body_skin_kernel<TM><<<dim3((sa.MT + TM - 1) / TM, (c->VG + 3) / 4), dim3(256), 0, s>>>(sa);
        BD_LAUNCH("skinning");
    }
    return 0;
}

}  // extern "C"
