"""Raw AMASS sequences -> the stage-2 motion file, on libegoego_hip: what the reference's
utils/data_utils/process_amass_dataset.py does per sequence on the host (process_seq :340-493: a full SMPL-H forward for 22
joints, sklearn's DBSCAN, a Python loop over frames for the head velocities), for a batch of sequences of different lengths and
frame rates in three launches.  Frames are packed end to end (`offsets [B + 1]`); memory grows with the total frame count.

  host arithmetic     corrected_fps (:360-363), trim_range (:376), is_short (:381), downsample_table (:427-448): index arithmetic
                      and exact copies of the caller's float64 arrays, nothing else
  body_joints         Jtr[:, :22] at zero betas and the global rotation of the head, one fp64 thread per raw frame
  floor_and_contacts  determine_floor_height_and_contacts (:160-338) at each sequence's raw frame rate; sequences of up to
                      MAX_FRAMES (65536) frames
  head_tracks         the gather through the downsample table, the floor shift and the head tracks (:454-472, :111-137)
  process_sequences   the three in a row, chunked by total frames -> one record (the arguments of np.savez at :477-491) or a
                      reason ("short", "terrain") per sequence
  collect, split      prep_smpl_to_single_data's dict (:523-536) and reorganize_data's train / test rule (:564-582)

There is no CPU path: the three stages need a ROCm device and raise EgoEgoHipError without one.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._engine import ContextEngine
from .body import regress_joints

N_JOINTS = 22
OUT_FPS = 30
MAX_FRAMES = 1 << 16  # egoego_amass_max_frames(): raw frames per sequence after the trim
LDS_FRAMES = 4096     # egoego_eval_max_frames(): up to here a sequence's samples stay in LDS
DISCARD_SHORTER_THAN = 1.0  # seconds
CHUNK_FRAMES = 1 << 20  # raw frames per pass of process_sequences (132 bytes of workspace each)
RECORD_KEYS = ("fps", "gender", "floor_height", "contacts", "trans", "root_orient", "pose_body", "betas", "joints", "head_qpos",
               "head_vels", "global_head_rot_6d", "global_head_trans", "global_head_rot_6d_diff", "global_head_trans_diff")
COLLECT_KEYS = {"root_orient": "root_orient", "body_pose": "pose_body", "trans": "trans", "beta": "betas", "gender": "gender",
                "head_qpos": "head_qpos", "head_vels": "head_vels", "global_head_trans": "global_head_trans",
                "global_head_rot_6d": "global_head_rot_6d", "global_head_rot_6d_diff": "global_head_rot_6d_diff",
                "global_head_trans_diff": "global_head_trans_diff"}
TRAIN_DATASETS = ("CMU", "MPI_Limits", "TotalCapture", "Eyes_Japan_Dataset", "KIT", "BioMotionLab_NTroje", "BMLmovi", "EKUT", "ACCAD")
TEST_DATASETS = ("Transitions_mocap", "HumanEva")
VAL_DATASETS = ("MPI_HDM05", "SFU", "MPI_mosh")


# ---------------------------------------------------------------- host arithmetic
def corrected_fps(path, fps):
    """:360-363: two mislabeled subsets, recognised by their path."""
    path = str(path)
    if path.find("BMLhandball") >= 0:
        fps = 240
    if path.find("20160930_50032") >= 0 or path.find("20161014_50033") >= 0:
        fps = 59
    return fps


def trim_range(num_frames):
    """:376: the middle 80 % of a sequence as [start, end)."""
    return int(0.1 * num_frames), int(0.9 * num_frames)


def is_short(num_frames, fps):
    """:381, on the trimmed length."""
    return bool(num_frames < DISCARD_SHORTER_THAN * fps)


def downsample_table(num_frames, fps, out_fps=OUT_FPS):
    """:427-448 -> (int64 indices into the trimmed frames, the fps the record keeps).  At out_fps, and below it ("cannot
    supersample"), every frame is kept and the fps stays what it was."""
    if out_fps != fps and not out_fps > fps:
        fps_ratio = float(out_fps) / fps
        new_num_frames = int(fps_ratio * num_frames)
        return np.linspace(0, num_frames - 1, num=new_num_frames, dtype=int).astype(np.int64), out_fps
    return np.arange(num_frames, dtype=np.int64), fps


# ---------------------------------------------------------------- plumbing
class _Prep(ContextEngine):
    """The grow-only workspace of one GPU (the floor kernel's long path); the library keeps no context for this module."""

    NOUN = "the AMASS preprocessing"
    CHECK = _lib.check_amass

    def workspace(self, n_frames, B):
        n = self.lib.egoego_amass_floor_workspace_bytes(int(n_frames), int(B))
        if n == 0:
            raise ValueError(f"{n_frames} frames in {B} sequences: 1 <= B <= frames <= 2^24 expected")
        return self._workspace_of(n)


_PREP = {}


def _prep(dev):
    if dev.index not in _PREP:
        _PREP[dev.index] = _Prep(dev)
    return _PREP[dev.index]


def _device_of(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _lib.EgoEgoHipError(f"{what} must be a tensor on a cuda (ROCm) device; the AMASS preprocessing has no CPU path")
    return t.device


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.EgoEgoHipError("the AMASS preprocessing needs a cuda (ROCm) device; there is no CPU path")
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise _lib.EgoEgoHipError("the AMASS preprocessing needs a cuda (ROCm) device; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _shaped(t, shape, what):
    """The shape check alone: it runs, like every check of host values, before the device is looked at."""
    t = torch.as_tensor(t)
    if t.dim() != len(shape) or any(w is not None and t.shape[i] != w for i, w in enumerate(shape)):
        raise ValueError(f"{what} {tuple(t.shape)}: {['N' if w is None else w for w in shape]} expected")
    return t


def _f32(t, dev):
    return t.to(dev, torch.float32).contiguous()


def _offsets(offsets, n_frames, what="offsets"):
    """Host values only (a list, an array or a CPU tensor): they are checked here, before anything is launched."""
    if isinstance(offsets, torch.Tensor):
        if offsets.device.type != "cpu":
            raise ValueError(f"{what} must be host values: they are validated before anything is launched")
        offsets = offsets.numpy()
    o = np.asarray(offsets).astype(np.int64).reshape(-1)
    if o.size < 2 or o[0] != 0 or o[-1] != n_frames or np.any(np.diff(o) < 0):
        raise ValueError(f"{what}: B + 1 ascending values from 0 to the {n_frames} frames expected")
    return o


def skeleton(body_model):
    """A body.BodyModel, or a mapping with J_regressor, v_template, shapedirs and kintree_table / parents -> (J_template[:22]
    float32 [22, 3] from body.regress_joints, the first 22 parents with parents[0] = 0).  Betas are zero and one skeleton serves
    every sequence, as the reference forces (gender = "male", betas = 0, :349-357)."""
    def get(k):
        if isinstance(body_model, torch.nn.Module):
            v = getattr(body_model, k, None)
        else:
            v = body_model[k] if k in body_model else None
        return None if v is None else (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))

    vt = get("v_template").astype(np.float32)  # the precision body.BodyModel keeps its buffers in
    jt, _ = regress_joints(get("J_regressor").astype(np.float32), vt, np.zeros((vt.shape[0], 3, 0)))
    par = get("parents")
    if par is None:
        par = get("kintree_table").astype(np.int64)[0]
    par = [int(p) for p in par[:N_JOINTS]]
    par[0] = 0
    if any(not 0 <= par[j] < j for j in range(1, N_JOINTS)):
        raise ValueError("the model's first 22 joints must each have an earlier parent")
    return np.ascontiguousarray(jt[:N_JOINTS]), par


# ---------------------------------------------------------------- the three stages
def body_joints(root_orient, pose_body, trans, body_model):
    """root_orient [N, 3], pose_body [N, 63], trans [N, 3] on the device (rounded to float32 here, as torch.Tensor(...) does at
    :151-156) -> (joints [N, 22, 3], head_rot [N, 3, 3]) float32: the reference's body.Jtr[:, :22] at zero betas and the global
    rotation of joint 15.  The first 22 joints have no ancestor at or beyond 22, so neither pose_hand nor a vertex is needed."""
    ro, pb, tr = _shaped(root_orient, (None, 3), "root_orient"), _shaped(pose_body, (None, 63), "pose_body"), _shaped(trans, (None, 3), "trans")
    N = ro.shape[0]
    if pb.shape[0] != N or tr.shape[0] != N:
        raise ValueError("root_orient, pose_body and trans disagree on the number of frames")
    jt, par = body_model if isinstance(body_model, tuple) else skeleton(body_model)
    dev = _device_of(ro, "root_orient")
    ro, pb, tr = _f32(ro, dev), _f32(pb, dev), _f32(tr, dev)
    joints = torch.empty(N, N_JOINTS, 3, device=dev)
    head_rot = torch.empty(N, 3, 3, device=dev)
    if N == 0:
        return joints, head_rot
    d_jt = torch.from_numpy(np.ascontiguousarray(jt, np.float32)).to(dev)
    with torch.cuda.device(dev):
        _lib.check_amass(_lib.load().egoego_amass_joints(ro.data_ptr(), pb.data_ptr(), tr.data_ptr(), d_jt.data_ptr(), (C.c_int32 * N_JOINTS)(*par), N,
                                                         joints.data_ptr(), head_rot.data_ptr(), _stream(dev)))
    return joints, head_rot


def floor_and_contacts(joints, offsets, fps, force_long=False, return_details=False):
    """joints [N, 22, 3] on the device (z up), the packed raw frames of B sequences; offsets: B + 1 host ints; fps: a number or one
    per sequence -> (offset_floor_height [B] fp32, contacts [N, 22] fp32 0 / 1, discard [B] bool).  `return_details=True` appends
    a dict: floor_height [B], labels [2 N] int32 (sequence b's 2 L entries from 2 * offsets[b], in the reference's order; -1
    noise, -2 past n_static), n_static [B], n_groups [B].

    A sequence needs 2..MAX_FRAMES frames; a longer one raises ValueError before anything is launched.  Up to LDS_FRAMES frames
    a sequence runs in LDS, beyond that in the workspace, with the same results bit for bit; `force_long` sends every sequence
    down the second path (for tests)."""
    x = _shaped(joints, (None, N_JOINTS, 3), "joints")
    N = x.shape[0]
    o = _offsets(offsets, N)
    B = o.size - 1
    L = np.diff(o)
    if L.min() < 2:
        raise ValueError(f"sequence {int(L.argmin())} has {int(L.min())} frames: at least 2 are needed")
    if L.max() > MAX_FRAMES:
        raise ValueError(f"sequence {int(L.argmax())} has {int(L.max())} frames: the floor-height kernel takes at most {MAX_FRAMES} per sequence")
    fps = np.asarray(fps, np.float64).reshape(-1)
    if fps.size == 1:
        fps = np.full(B, fps[0])
    if fps.shape != (B,) or not np.all((fps >= 0) & (fps <= 1e6)):
        raise ValueError(f"fps: a number or {B} numbers in 0..1e6 expected")
    thresh = np.asarray([int(0.25 * f) for f in fps], np.int32)  # :273
    dev = _device_of(x, "joints")
    x = _f32(x, dev)
    o32 = np.ascontiguousarray(o, np.int32)
    d_off, d_thr = torch.from_numpy(o32).to(dev), torch.from_numpy(thresh).to(dev)
    floor, offset = torch.empty(B, device=dev), torch.empty(B, device=dev)
    contacts = torch.empty(N, N_JOINTS, device=dev)
    discard, n_static, n_groups = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    labels = torch.empty(2 * N, dtype=torch.int32, device=dev) if return_details else None
    with torch.cuda.device(dev):
        ws, ws_bytes = _prep(dev).workspace(N, B)
        _lib.check_amass(_lib.load().egoego_amass_floor_contacts(
            x.data_ptr(), o32.ctypes.data_as(C.POINTER(C.c_int32)), d_off.data_ptr(), d_thr.data_ptr(), B, int(bool(force_long)),
            floor.data_ptr(), offset.data_ptr(), contacts.data_ptr(), discard.data_ptr(), labels.data_ptr() if labels is not None else None,
            n_static.data_ptr(), n_groups.data_ptr(), ws, ws_bytes, _stream(dev)))
    out = (offset, contacts, discard.bool())
    if return_details:
        out += ({"floor_height": floor, "labels": labels, "n_static": n_static, "n_groups": n_groups},)
    return out


HEAD_KEYS = ("joints", "contacts", "global_head_trans", "global_head_rot_6d", "head_qpos", "global_head_rot_6d_diff",
             "global_head_trans_diff", "head_vels", "same")


def head_tracks(joints, head_rot, contacts, offset_floor_height, offsets, tables=None):
    """joints [N, 22, 3], head_rot [N, 3, 3], contacts [N, 22] (the packed raw frames, before the floor shift), offset_floor_height
    [B] on the device; offsets: B + 1 host ints; tables: per sequence the raw frames to keep, relative to its first (None: all)
    -> (a dict of packed device tensors over the M output frames, out_offsets: B + 1 host ints).  joints [M, 22, 3] with the floor
    taken off z, contacts [M, 22] fp64, global_head_trans [M, 3], global_head_rot_6d [M, 6], head_qpos [M, 7], head_vels [M, 6]
    and `same` [M] uint8 (the pair took the |1 -+ q0| < 1e-6 branch) have a row per output frame; global_head_rot_6d_diff
    [M, 6] and global_head_trans_diff [M, 3] are zero in each sequence's last row, which the records drop."""
    x = _shaped(joints, (None, N_JOINTS, 3), "joints")
    N = x.shape[0]
    R, c = _shaped(head_rot, (N, 3, 3), "head_rot"), _shaped(contacts, (N, N_JOINTS), "contacts")
    o = _offsets(offsets, N)
    B = o.size - 1
    fl = _shaped(offset_floor_height, (B,), "offset_floor_height")
    if tables is None:
        tables = [np.arange(o[b + 1] - o[b], dtype=np.int64) for b in range(B)]
    if len(tables) != B:
        raise ValueError(f"tables: {B} index arrays expected")
    src, seq, out_off = [], [], [0]
    for b, t in enumerate(tables):
        t = np.asarray(t).astype(np.int64).reshape(-1)
        if t.size < 1 or t.min() < 0 or t.max() >= o[b + 1] - o[b]:
            raise ValueError(f"tables[{b}]: at least one index below the sequence's {int(o[b + 1] - o[b])} frames expected")
        src.append(t + o[b])
        seq.append(np.full(t.size, b, np.int32))
        out_off.append(out_off[-1] + t.size)
    src, seq = np.concatenate(src).astype(np.int32), np.concatenate(seq)
    M = src.size
    dev = _device_of(x, "joints")
    x, R, c, fl = _f32(x, dev), _f32(R, dev), _f32(c, dev), _f32(fl, dev)
    d_src, d_seq, d_oo = (torch.from_numpy(a).to(dev) for a in (src, seq, np.asarray(out_off, np.int32)))
    f32 = dict(device=dev, dtype=torch.float32)
    out = {"joints": torch.empty(M, N_JOINTS, 3, **f32), "contacts": torch.empty(M, N_JOINTS, device=dev, dtype=torch.float64),
           "global_head_trans": torch.empty(M, 3, **f32), "global_head_rot_6d": torch.empty(M, 6, **f32), "head_qpos": torch.empty(M, 7, **f32),
           "global_head_rot_6d_diff": torch.empty(M, 6, **f32), "global_head_trans_diff": torch.empty(M, 3, **f32),
           "head_vels": torch.empty(M, 6, **f32), "same": torch.empty(M, device=dev, dtype=torch.uint8)}
    with torch.cuda.device(dev):
        _lib.check_amass(_lib.load().egoego_amass_head(x.data_ptr(), R.data_ptr(), c.data_ptr(), fl.data_ptr(), d_src.data_ptr(), d_seq.data_ptr(),
                                                       d_oo.data_ptr(), M, N, B, *[out[k].data_ptr() for k in HEAD_KEYS], _stream(dev)))
    return out, np.asarray(out_off, np.int64)


# ---------------------------------------------------------------- the driver
def _sequence_arrays(s):
    """-> (name, root_orient, pose_body, trans, mocap_framerate): views of the caller's arrays, no conversion."""
    name = s.get("path", s.get("name"))
    if name is None:
        raise ValueError("a sequence needs a 'name' or a 'path' (the frame-rate corrections go by it)")
    if "poses" in s:
        poses = np.asarray(s["poses"])
        if poses.ndim != 2 or poses.shape[1] < 66:
            raise ValueError(f"{name}: poses {poses.shape}: [T, >= 66] expected")
        ro, pb = poses[:, :3], poses[:, 3:66]
    else:
        ro, pb = np.asarray(s["root_orient"]), np.asarray(s["pose_body"])
        if ro.ndim != 2 or ro.shape[1] != 3 or pb.shape != (ro.shape[0], 63):
            raise ValueError(f"{name}: root_orient {ro.shape} / pose_body {pb.shape}: [T, 3] / [T, 63] expected")
    tr = np.asarray(s["trans"])
    if tr.shape != (ro.shape[0], 3):
        raise ValueError(f"{name}: trans {tr.shape}: {(ro.shape[0], 3)} expected")
    return str(name), ro, pb, tr, s["mocap_framerate"]


def process_sequences(seqs, body_model, out_fps=OUT_FPS, device=None, chunk_frames=CHUNK_FRAMES):
    """`seqs`: a list of {name or path, poses [T, >= 66] or root_orient [T, 3] / pose_body [T, 63], trans [T, 3], mocap_framerate};
    `body_model`: a body.BodyModel or its arrays -> one entry per sequence: a dict with exactly the arguments np.savez gets at
    :477-491 (RECORD_KEYS, the reference's shapes and dtypes), or why there is none: "short" (:381) or "terrain" (:450).  The
    calls are chunked so that a pass holds at most `chunk_frames` raw frames (a single longer sequence runs alone).  A trimmed
    sequence of more than MAX_FRAMES frames raises ValueError before anything runs."""
    skel = skeleton(body_model)
    plan, results = [], [None] * len(seqs)
    for i, s in enumerate(seqs):
        name, ro, pb, tr, fps = _sequence_arrays(s)
        fps = corrected_fps(name, fps)
        lo, hi = trim_range(ro.shape[0])
        n = hi - lo
        if is_short(n, fps):
            results[i] = "short"
            continue
        if n > MAX_FRAMES:
            raise ValueError(f"{name}: {n} frames after the trim: at most {MAX_FRAMES} per sequence")
        if n < 2:
            raise ValueError(f"{name}: {n} frames after the trim: at least 2 are needed")
        plan.append((i, ro[lo:hi], pb[lo:hi], tr[lo:hi], fps, n))
    if not plan:
        return results
    dev = _device(device)
    chunk = []
    for item in plan:
        if chunk and sum(p[5] for p in chunk) + item[5] > chunk_frames:
            _run_chunk(chunk, skel, out_fps, dev, results)
            chunk = []
        chunk.append(item)
    if chunk:
        _run_chunk(chunk, skel, out_fps, dev, results)
    return results


def _run_chunk(chunk, skel, out_fps, dev, results):
    offsets = np.concatenate([[0], np.cumsum([p[5] for p in chunk])]).astype(np.int64)
    ro, pb, tr = (torch.from_numpy(np.concatenate([np.asarray(p[k], np.float32) for p in chunk])).to(dev) for k in (1, 2, 3))
    tables, fps_out = zip(*(downsample_table(p[5], p[4], out_fps) for p in chunk))
    joints, head_rot = body_joints(ro, pb, tr, skel)
    floor, contacts, discard = floor_and_contacts(joints, offsets, [float(p[4]) for p in chunk])
    out, oo = head_tracks(joints, head_rot, contacts, floor, offsets, tables)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    floor, discard = floor.cpu().numpy(), discard.cpu().numpy()
    for b, (i, ro_b, pb_b, tr_b, _, _) in enumerate(chunk):
        if discard[b]:
            results[i] = "terrain"
            continue
        a, e, t = int(oo[b]), int(oo[b + 1]), tables[b]
        trans = np.array(tr_b)      # :422 works on the caller's dtype: float64 minus the float32 floor
        trans[:, 2] -= floor[b]
        vels = host["head_vels"][a:e]
        if host["same"][a:e - 1].any():  # a row of the |1 -+ q0| branch is float64 in the reference, and np.vstack promotes
            vels = vels.astype(np.float64)
        results[i] = {"fps": fps_out[b], "gender": "male", "floor_height": floor[b], "contacts": host["contacts"][a:e].copy(),
                      "trans": trans[t], "root_orient": ro_b[t], "pose_body": pb_b[t], "betas": np.zeros(16),
                      "joints": host["joints"][a:e].copy(), "head_qpos": host["head_qpos"][a:e].copy(), "head_vels": vels.copy(),
                      "global_head_rot_6d": host["global_head_rot_6d"][a:e].copy(), "global_head_trans": host["global_head_trans"][a:e].copy(),
                      "global_head_rot_6d_diff": host["global_head_rot_6d_diff"][a:e - 1].copy(),
                      "global_head_trans_diff": host["global_head_trans_diff"][a:e - 1].copy()}


def record_file_name(stem, record):
    """:476: `stem` + '_%d_frames_%d_fps.npz'."""
    return stem + "_%d_frames_%d_fps.npz" % (record["trans"].shape[0], int(record["fps"]))


def collect(records):
    """prep_smpl_to_single_data (:523-536): `records` maps the reference's sequence names (subset-subject-file.npz) to records (or
    to what np.load gives for a saved one) -> {name: {root_orient, body_pose, trans, beta, seq_name, gender, head_qpos, ...}}."""
    out = {}
    for name, r in records.items():
        d = {k: np.asarray(r[src]) for k, src in COLLECT_KEYS.items()}
        d["seq_name"] = name
        out[name] = {k: d[k] for k in ("root_orient", "body_pose", "trans", "beta", "seq_name", "gender", "head_qpos", "head_vels",
                                        "global_head_trans", "global_head_rot_6d", "global_head_rot_6d_diff", "global_head_trans_diff")}
    return out


def split(data):
    """reorganize_data (:564-582) -> (train, test), each {0: entry, 1: entry, ...} in the order of `data`.  A name counts for
    train by the first training set it contains, and for test once per list (validation, test) it matches, as the reference's
    three loops do; a name that matches none is in neither."""
    train, test = {}, {}
    for name in data:
        if any(k in name for k in TRAIN_DATASETS):
            train[len(train)] = data[name]
        if any(k in name for k in VAL_DATASETS):
            test[len(test)] = data[name]
        if any(k in name for k in TEST_DATASETS):
            test[len(test)] = data[name]
    return train, test
