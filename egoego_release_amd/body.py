"""The SMPL-H body model on libegoego_hip: the last step of the reference's pipeline, gen_full_body_vis -> run_smpl_model
(egoego/data/amass_diffusion_dataset.py:15-81) -> human_body_prior's BodyModel, which turns the sampled pose into 6890 mesh
vertices and 52 joints per frame, and save_verts_faces_to_mesh_file (egoego/vis/blender_vis_mesh_motion.py:103-117), which writes
them as one OBJ file per frame.

  BodyEngine   one body-model context of the library on one GPU: packs a model, owns the workspace, runs the forward
  BodyModel    nn.Module with the call surface run_smpl_model uses: bm(pose_body=, pose_hand=, betas=, root_orient=, trans=)
               -> an object with .v [N, V, 3], .Jtr [N, 52, 3] and .f
  run_smpl_model / save_verts_faces_to_mesh_file   the reference's functions, same signatures and returns

The algorithm is standard SMPL linear-blend skinning written from its definition (csrc/body_model.h); neither human_body_prior,
smplx nor trimesh is needed.  The licensed SMPL-H files are not shipped: synthetic.make_body_model draws a seeded model of the
same shape.  There is no CPU path: a forward on a CPU device raises.
"""
import ctypes as C
import os

import numpy as np
import torch
from torch import nn

from . import _lib
from ._engine import ContextEngine, EngineCacheMixin

N_JOINTS = _lib.BODY_N_JOINTS
POSE_FEATS = _lib.BODY_POSE_FEATS
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "kintree_table", "f")


def load_model_arrays(src, num_betas=16):
    """An SMPL-H model.npz (path) or a mapping with its arrays -> a dict of validated numpy arrays: v_template (V, 3), shapedirs
    (V, 3, <= num_betas), posedirs (V, 3, 459), J_regressor (52, V), weights (V, 52) float32; parents (52,) int32 with parents[0]
    = -1; f (n_faces, 3) int32.  Raises ValueError on anything that is not a 52-joint model whose parents precede their
    children."""
    if isinstance(src, (str, os.PathLike)):
        with np.load(src, allow_pickle=False) as z:
            missing = [k for k in MODEL_KEYS if k not in z.files]
            if missing:
                raise ValueError(f"{src}: not an SMPL-H model file: missing {missing}")
            src = {k: z[k] for k in MODEL_KEYS}
    else:
        missing = [k for k in MODEL_KEYS if k not in src]
        if missing:
            raise ValueError(f"body model: missing arrays {missing}")

    def arr(k):
        v = src[k]
        return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    vt = arr("v_template").astype(np.float32)
    if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
        raise ValueError(f"v_template {vt.shape}: (V, 3) expected")
    V = vt.shape[0]
    kt = arr("kintree_table").astype(np.int64)
    if kt.ndim != 2 or kt.shape[0] < 1 or kt.shape[1] != N_JOINTS:
        raise ValueError(f"kintree_table {kt.shape}: (2, {N_JOINTS}) expected — only the {N_JOINTS}-joint SMPL-H model is supported")
    parents = kt[0].copy()
    parents[0] = -1  # the file stores 2^32 - 1
    bad = [j for j in range(1, N_JOINTS) if not 0 <= parents[j] < j]
    if bad:
        raise ValueError(f"kintree_table: the parent of joint {bad[0]} is {int(parents[bad[0]])}; every joint's parent must precede it")
    sd = arr("shapedirs").astype(np.float32)
    if sd.ndim != 3 or sd.shape[:2] != (V, 3):
        raise ValueError(f"shapedirs {sd.shape}: ({V}, 3, n) expected")
    sd = np.ascontiguousarray(sd[:, :, :max(int(num_betas), 0)])
    pd = arr("posedirs").astype(np.float32)
    if pd.shape != (V, 3, POSE_FEATS):
        raise ValueError(f"posedirs {pd.shape}: ({V}, 3, {POSE_FEATS}) expected ({N_JOINTS} joints)")
    jr = arr("J_regressor").astype(np.float32)
    if jr.shape != (N_JOINTS, V):
        raise ValueError(f"J_regressor {jr.shape}: ({N_JOINTS}, {V}) expected")
    w = arr("weights").astype(np.float32)
    if w.shape != (V, N_JOINTS):
        raise ValueError(f"weights {w.shape}: ({V}, {N_JOINTS}) expected")
    f = arr("f").astype(np.int32)
    if f.ndim != 2 or f.shape[1] != 3 or (f.size and (f.min() < 0 or f.max() >= V)):
        raise ValueError(f"f {f.shape}: (n_faces, 3) vertex indices below {V} expected")
    return {"v_template": vt, "shapedirs": sd, "posedirs": pd, "J_regressor": jr, "weights": w,
            "parents": parents.astype(np.int32), "f": f}


def compress_weights(weights):
    """Dense skinning weights (V, 52) -> (joint [n, V] int32, weight [n, V] float32): each vertex's non-zero weights in joint
    order, n the model's largest non-zero count (at least 1), padded with (0, 0.0)."""
    w = np.asarray(weights, dtype=np.float32)
    nz = w != 0
    n = max(int(nz.sum(1).max()), 1)
    order = np.argsort(~nz, axis=1, kind="stable")[:, :n]  # the non-zero joints first, ascending
    ww = np.take_along_axis(w, order, 1)
    keep = np.take_along_axis(nz, order, 1)
    return (np.ascontiguousarray(np.where(keep, order, 0).T.astype(np.int32)),
            np.ascontiguousarray(np.where(keep, ww, 0).T.astype(np.float32)))


def regress_joints(J_regressor, v_template, shapedirs):
    """J_template = J_regressor . v_template (52, 3) and J_shapedirs = J_regressor . shapedirs (52, 3, n_betas), in fp64, rounded
    once to fp32."""
    jr = np.asarray(J_regressor, np.float64)
    jt = jr @ np.asarray(v_template, np.float64)
    jsd = np.einsum("jv,vcb->jcb", jr, np.asarray(shapedirs, np.float64))
    return jt.astype(np.float32), np.ascontiguousarray(jsd.astype(np.float32))


class BodyEngine(ContextEngine):
    """One body-model context of libegoego_hip on one GPU; frames run in chunks of `chunk_frames` (0 = the library's default)."""

    NOUN = "the body model"
    CREATE, DESTROY, WORKSPACE_BYTES = "egoego_body_ctx_create", "egoego_body_ctx_destroy", "egoego_body_workspace_bytes"
    CHECK = _lib.check_body

    def __init__(self, device, chunk_frames=0):
        super().__init__(device)
        self.chunk_frames = int(chunk_frames)
        self._create(self.dev_index, self.chunk_frames)
        self.n_verts = self.n_betas = self.n_weights = 0

    def load(self, arrays):
        """`arrays`: load_model_arrays' dict (numpy arrays or tensors)."""
        def np_(k):
            v = arrays[k]
            return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

        jt, jsd = regress_joints(np_("J_regressor"), np_("v_template"), np_("shapedirs"))
        sj, sw = compress_weights(np_("weights"))
        keep = []

        def p(a, dtype):
            t = torch.as_tensor(a).detach().to(device=self.device, dtype=dtype).contiguous()
            keep.append(t)
            return t.data_ptr() if t.numel() else None

        m = _lib.BodyModelDesc()
        m.n_verts, m.n_betas, m.n_weights = int(np_("v_template").shape[0]), int(jsd.shape[2]), int(sj.shape[0])
        m.v_template, m.shapedirs = p(arrays["v_template"], torch.float32), p(arrays["shapedirs"], torch.float32)
        m.posedirs = p(arrays["posedirs"], torch.float32)
        m.j_template, m.j_shapedirs = p(jt, torch.float32), p(jsd, torch.float32)
        m.skin_weight, m.skin_joint = p(sw, torch.float32), p(sj, torch.int32)
        m.parents = p(np.maximum(np_("parents"), 0), torch.int32)
        with torch.cuda.device(self.dev_index):
            _lib.check_body(self.lib.egoego_body_load_model(self._ctx, C.byref(m), self._stream()))
        del keep
        self.n_verts, self.n_betas, self.n_weights = m.n_verts, m.n_betas, m.n_weights

    def forward(self, root_orient, pose_body, pose_hand, trans, betas, seq_index, pose_offsets=False):
        """root_orient [N, 3], pose_body [N, 63], pose_hand [N, 90] or None, trans [N, 3], betas [S, n_betas], seq_index [N]
        (each frame's row of betas) -> vertices [N, V, 3], joints [N, 52, 3] (+ the pose offsets [N, V, 3] when asked)."""
        def f32(t, width):
            t = torch.as_tensor(t).to(self.device, torch.float32).contiguous()
            if t.dim() != 2 or t.shape[1] != width:
                raise ValueError(f"body model input {tuple(t.shape)}: [N, {width}] expected")
            return t

        root_orient, pose_body, trans = f32(root_orient, 3), f32(pose_body, 63), f32(trans, 3)
        N = root_orient.shape[0]
        pose_hand = f32(pose_hand, 90) if pose_hand is not None else None
        betas = f32(betas, self.n_betas)
        S = betas.shape[0]
        seq = torch.as_tensor(seq_index).to(self.device, torch.int32).contiguous()
        given = [pose_body, trans, seq] + ([pose_hand] if pose_hand is not None else [])
        if N < 1 or S < 1 or any(t.shape[0] != N for t in given):
            raise ValueError("body model inputs disagree on the number of frames, or there are none")
        lo, hi = int(seq.min()), int(seq.max())
        if lo < 0 or hi >= S:
            raise ValueError(f"seq_index spans {lo}..{hi} but betas has {S} rows")
        if not betas.numel():  # n_betas == 0: the library still wants a pointer
            betas = torch.zeros(S, 1, device=self.device)
        verts = torch.empty(N, self.n_verts, 3, device=self.device)
        joints = torch.empty(N, N_JOINTS, 3, device=self.device)
        off = torch.empty(N, self.n_verts, 3, device=self.device) if pose_offsets else None
        ws, n = self._workspace(N, S)
        with torch.cuda.device(self.dev_index):
            _lib.check_body(self.lib.egoego_body_forward(
                self._ctx, root_orient.data_ptr(), pose_body.data_ptr(), pose_hand.data_ptr() if pose_hand is not None else None,
                trans.data_ptr(), betas.data_ptr(), seq.data_ptr(), N, S, verts.data_ptr(), joints.data_ptr(),
                off.data_ptr() if off is not None else None, ws, n, self._stream()))
        return (verts, joints, off) if pose_offsets else (verts, joints)


class BodyOutput:
    """What human_body_prior's BodyModel returns, as far as run_smpl_model reads it."""

    def __init__(self, v, Jtr, f, pose_offsets=None):
        self.v, self.Jtr, self.f = v, Jtr, f
        if pose_offsets is not None:
            self.pose_offsets = pose_offsets


class BodyModel(EngineCacheMixin, nn.Module):
    """Drop-in for human_body_prior's BodyModel(bm_fname, num_betas) as run_smpl_model uses it, on libegoego_hip.

    `bm_fname` is an SMPL-H model.npz (v_template, shapedirs, posedirs, J_regressor, weights, kintree_table, f); `model` a
    mapping with the same arrays instead.  Shapedirs are truncated to `num_betas`.  Any vertex and face count is accepted;
    the model must have 52 joints and a kintree_table whose parents precede their children.  `chunk_frames` bounds the frames
    per pass through the workspace (0 = the library's default)."""

    ENGINE = BodyEngine

    def __init__(self, bm_fname=None, num_betas=16, device=None, model=None, chunk_frames=0):
        super().__init__()
        if (bm_fname is None) == (model is None):
            raise ValueError("BodyModel takes either bm_fname or model")
        a = load_model_arrays(bm_fname if bm_fname is not None else model, num_betas)
        self.num_betas = a["shapedirs"].shape[2]
        for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "f"):
            self.register_buffer(k, torch.from_numpy(a[k]))
        self.register_buffer("parents", torch.from_numpy(a["parents"]))
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.chunk_frames = int(chunk_frames)
        self._engine = None
        self._packed = None

    def _params_version(self):
        return tuple((b.data_ptr(), b._version) for b in self.buffers())

    def _engine_state(self):
        return dict(self.named_buffers())

    def forward(self, root_orient=None, pose_body=None, pose_hand=None, betas=None, trans=None, seq_index=None,
                return_pose_offsets=False, **unused):
        """Every input is optional (zeros).  `betas` is [N, num_betas] (one row per frame, as the reference passes it), a single
        row, or — with `seq_index` [N] — one row per sequence and each frame's row index.  Without `pose_hand` the hands keep
        their rest pose, bit-identical to a zero `pose_hand` and cheaper."""
        given = [t for t in (root_orient, pose_body, pose_hand, trans, seq_index) if t is not None]
        if given:
            N = int(torch.as_tensor(given[0]).shape[0])
        else:
            N = int(torch.as_tensor(betas).shape[0]) if betas is not None else 1
        e = self.engine()
        dev = e.device
        zeros = lambda w: torch.zeros(N, w, device=dev)  # noqa: E731
        if betas is None:
            betas = torch.zeros(1, self.num_betas, device=dev)
        betas = torch.as_tensor(betas)
        if seq_index is None:
            if betas.shape[0] == N:
                seq_index = torch.arange(N, dtype=torch.int32, device=dev)
            elif betas.shape[0] == 1:
                seq_index = torch.zeros(N, dtype=torch.int32, device=dev)
            else:
                raise ValueError(f"betas {tuple(betas.shape)}: {N} rows or one expected (or pass seq_index)")
        if N == 0:
            empty = torch.empty(0, self.v_template.shape[0], 3, device=dev)
            return BodyOutput(empty, torch.empty(0, N_JOINTS, 3, device=dev), self.f, empty if return_pose_offsets else None)
        out = e.forward(root_orient if root_orient is not None else zeros(3), pose_body if pose_body is not None else zeros(63),
                        pose_hand, trans if trans is not None else zeros(3), betas, seq_index, return_pose_offsets)
        return BodyOutput(out[0], out[1], self.f, out[2] if return_pose_offsets else None)


def run_smpl_model(root_trans, aa_rot_rep, betas, gender, bm_dict):
    """amass_diffusion_dataset.py:15-81.  root_trans [BS, T, 3], aa_rot_rep [BS, T, 22 or 52, 3], betas [BS, num_betas], gender
    BS names, bm_dict {'male': BodyModel, 'female': BodyModel} -> joints [BS, T, 22 or 52, 3], vertices [BS, T, V, 3], faces.

    Differences in mechanism only: betas go to the library once per sequence instead of repeated per frame, and a 22-joint
    pose runs without the 30 zero hand joints the reference pads (bit-identical, a shorter contraction)."""
    bs, T, nj, _ = aa_rot_rep.shape
    if nj not in (22, N_JOINTS):
        raise ValueError(f"aa_rot_rep {tuple(aa_rot_rep.shape)}: 22 or {N_JOINTS} joints expected")
    gender = [str(g) for g in np.asarray(gender).reshape(-1)]
    if len(gender) != bs:
        raise ValueError(f"gender has {len(gender)} entries for a batch of {bs}")
    unknown = sorted(set(gender) - {"male", "female"})
    if unknown:
        raise ValueError(f"gender {unknown}: 'male' or 'female' expected")
    joints = verts = faces = None
    for name in ("male", "female"):
        idx = [i for i, g in enumerate(gender) if g == name]
        if not idx:
            continue
        bm = bm_dict[name]
        dev = bm.engine().device
        ii = torch.as_tensor(idx, device=dev)
        aa = torch.as_tensor(aa_rot_rep).to(dev, torch.float32)[ii].reshape(len(idx) * T, nj, 3)
        tr = torch.as_tensor(root_trans).to(dev, torch.float32)[ii].reshape(len(idx) * T, 3)
        seq = torch.arange(len(idx), dtype=torch.int32, device=dev).repeat_interleave(T)
        body = bm(root_orient=aa[:, 0], pose_body=aa[:, 1:22].reshape(-1, 63),
                  pose_hand=aa[:, 22:].reshape(-1, 90) if nj == N_JOINTS else None,
                  betas=torch.as_tensor(betas).to(dev, torch.float32)[ii], trans=tr, seq_index=seq)
        if verts is None:
            verts = torch.empty(bs, T, body.v.shape[1], 3, device=dev)
            joints = torch.empty(bs, T, nj, 3, device=dev)
        if body.v.shape[1] != verts.shape[2]:
            raise ValueError("the male and female body models differ in their vertex count")
        verts[ii] = body.v.reshape(len(idx), T, -1, 3).to(verts.device)
        joints[ii] = body.Jtr[:, :nj].reshape(len(idx), T, nj, 3).to(verts.device)
        faces = body.f  # the reference returns the last model's faces
    if verts is None:
        raise ValueError("run_smpl_model needs at least one sequence")
    return joints, verts, faces


def save_verts_faces_to_mesh_file(mesh_verts, mesh_faces, save_mesh_folder, save_gt=False):
    """blender_vis_mesh_motion.py:103-117 without trimesh: mesh_verts [T, Nv, 3], mesh_faces [Nf, 3] (0-based) -> one Wavefront
    OBJ per frame, %05d.obj (%05d_gt.obj with save_gt): `v x y z` lines, then `f a b c` lines with 1-based indices."""
    os.makedirs(save_mesh_folder, exist_ok=True)
    verts = mesh_verts.detach().cpu().numpy() if isinstance(mesh_verts, torch.Tensor) else np.asarray(mesh_verts)
    faces = mesh_faces.detach().cpu().numpy() if isinstance(mesh_faces, torch.Tensor) else np.asarray(mesh_faces)
    face_text = "".join("f %d %d %d\n" % tuple(f) for f in (faces.astype(np.int64) + 1).tolist())
    for idx in range(verts.shape[0]):
        path = os.path.join(save_mesh_folder, "%05d" % idx + ("_gt.obj" if save_gt else ".obj"))
        with open(path, "w") as fh:
            fh.write("".join("v %.8f %.8f %.8f\n" % tuple(v) for v in verts[idx].astype(np.float64).tolist()))
            fh.write(face_text)
