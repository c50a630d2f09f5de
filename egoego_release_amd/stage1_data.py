"""GravityNet's training batches on libegoego_hip (csrc/stage1_data.*): the reference's AMASSHeadPoseDataset
(egoego/data/amass_headpose_dataset.py) and the DataLoader in front of it, between a split's [T, 7] head poses per sequence
(the `head_qpos` amass_prep.process_sequences / tools/process_amass.py write) and the batch dicts trainer.Stage1Trainer takes.

    gravity_batch     egoego_s1_gravity_batch: __getitem__ with augment_traj (38-76, 115-165) for a whole batch in one launch
    GravityBatches    the epochs: packed poses uploaded once, a seeded host permutation per epoch, one batch dict per launch
    EpochPlan         its host side alone: orders, draw ids, the state dict
    split_by_dataset  divide_train_val (78-103)

A sample's random start, rotation and scale are Philox draws keyed by (seed, draw id); GravityBatches gives sample k of epoch e
the draw id e * S + k, so its data depends neither on the batch size nor on the shuffle order.  There is no CPU path: a device off
the GPU raises EgoEgoHipError.

HeadNet's training batches, the reference's ARESHeadPoseDataset (egoego/data/ares_headpose_dataset.py) and its DataLoader, between a
split's per-sequence arrays (head poses, head velocities, optical-flow features, DROID-SLAM tracks) and the same trainer:

    load_ares_split      ARESHeadPoseDataset.__init__ up to the arrays: the motion file, the filter, the feature and SLAM files
    pack_head_sequences  the host side: checks, the dropping rules, the SLAM alignment, the packed tables (no GPU)
    head_batch           egoego_s1_head_batch: __getitem__ (270-333) for a whole batch in one launch, a select-and-copy
    HeadBatches          the epochs, on EpochPlan: tables uploaded once, one batch dict per launch
"""
import json
import os

import numpy as np
import torch

from . import _lib
from .motion_data import _stream

TRAIN_DATASETS = ("CMU", "MPI_Limits", "TotalCapture", "Eyes_Japan_Dataset", "KIT", "BioMotionLab_NTroje", "BMLmovi", "EKUT", "ACCAD")
MIN_FRAMES = 30  # sequences of at most this many frames are dropped (dataset:97)


def _device(device):
    what = "the stage-1 training batches need a cuda (ROCm) device; they have no CPU path"
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.EgoEgoHipError(f"device {dev}: {what}")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def split_by_dataset(names):
    """divide_train_val's rule on sequence names -> (train names, validation names), each in the given order: the first
    '-'-separated field of a name in TRAIN_DATASETS goes to train, everything else to validation."""
    train, val = [], []
    for n in names:
        (train if str(n).split("-")[0] in TRAIN_DATASETS else val).append(n)
    return train, val


def _i32(a, dev, what, B=None):
    t = torch.as_tensor(a)
    if t.dim() != 1 or (B is not None and t.numel() != B):
        raise ValueError(f"{what} {tuple(t.shape)}: [{'B' if B is None else B}] expected")
    return t.to(dev, torch.int32).contiguous()


def gravity_batch(pose, offsets, seq_ids, draw_ids, window, seed, for_eval=False, start=None, rot=None, scale=None):
    """One batch of GravityNet's training data.  pose [N, 7] fp32 and offsets int32 [S + 1] on the GPU (a split's packed head poses:
    sequence k is rows offsets[k] .. offsets[k + 1] - 1); seq_ids [B], draw_ids [B]; start [B], rot [B, 3, 3], scale [B]: planted
    draws, None for "draw it".  -> the reference's keys as device tensors, fp32 unless said: ori_head_pose [B, window + 1, 7],
    head_rot_mat [B, window + 1, 3, 3], head_trans [B, window + 1, 3], seq_len int64 [B], aligned_rot_mat [B, 3, 3], aligned_scale
    [B], floor_normal [B, 3, 1]; and lengths (seq_len as int32: what HeadNormalFormer.forward masks by), start_t_idx int32 [B],
    aug_scale [B].  Sequence ids and offsets that are host data are checked here; device tensors are not read back (the kernel
    writes an empty sample, seq_len 0, for an id or a planted start that does not fit)."""
    if not (isinstance(pose, torch.Tensor) and pose.device.type == "cuda"):
        raise _lib.EgoEgoHipError("gravity_batch needs the head poses on a cuda (ROCm) device; there is no CPU path")
    dev = pose.device
    if pose.dim() != 2 or pose.shape[1] != 7 or pose.dtype != torch.float32 or not pose.is_contiguous():
        raise ValueError(f"pose {tuple(pose.shape)} {pose.dtype}: a contiguous fp32 [N, 7] expected")
    W = int(window)
    if W < 1:
        raise ValueError(f"window {W}: at least 1 expected")
    host_off = None if isinstance(offsets, torch.Tensor) and offsets.device.type == "cuda" else np.asarray(offsets, np.int64).reshape(-1)
    if host_off is not None:
        if host_off.size < 2 or host_off[0] != 0 or host_off[-1] != pose.shape[0] or (np.diff(host_off) < 1).any():
            raise ValueError("offsets: 0 = offsets[0] < ... < offsets[S] = N expected (no sequence of fewer than 1 frame)")
    off = _i32(offsets if host_off is None else host_off, dev, "offsets")
    S = off.numel() - 1
    if S < 1:
        raise ValueError("offsets: at least one sequence expected")
    if not (isinstance(seq_ids, torch.Tensor) and seq_ids.device.type == "cuda"):
        ids = np.asarray(seq_ids, np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= S):
            raise ValueError(f"seq_ids: values in 0 .. {S - 1} expected")
        seq_ids = ids
    sid = _i32(seq_ids, dev, "seq_ids")
    B = sid.numel()
    if B < 1:
        raise ValueError("an empty batch")
    did = torch.as_tensor(draw_ids)
    if tuple(did.shape) != (B,):
        raise ValueError(f"draw_ids {tuple(did.shape)}: [{B}] expected")
    did = did.to(dev, torch.int64).contiguous()
    p_start = None if start is None else _i32(start, dev, "start", B)
    p_rot = None if rot is None else torch.as_tensor(rot).to(dev, torch.float32).reshape(-1, 9).contiguous()
    p_scale = None if scale is None else torch.as_tensor(scale).to(dev, torch.float32).reshape(-1).contiguous()
    if p_rot is not None and p_rot.shape[0] != B or p_scale is not None and p_scale.numel() != B:
        raise ValueError(f"rot / scale: [{B}, 3, 3] / [{B}] expected")
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {"ori_head_pose": torch.empty(B, W + 1, 7, **f32), "head_rot_mat": torch.empty(B, W + 1, 3, 3, **f32),
           "head_trans": torch.empty(B, W + 1, 3, **f32), "lengths": torch.empty(B, **i32),
           "aligned_rot_mat": torch.empty(B, 3, 3, **f32), "aligned_scale": torch.empty(B, **f32),
           "floor_normal": torch.empty(B, 3, 1, **f32), "start_t_idx": torch.empty(B, **i32), "aug_scale": torch.empty(B, **f32)}
    opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        _lib.check_s1_data(_lib.load().egoego_s1_gravity_batch(
            pose.data_ptr(), pose.shape[0], off.data_ptr(), S, sid.data_ptr(), did.data_ptr(), B, W, int(seed) & (2 ** 64 - 1),
            int(bool(for_eval)), opt(p_start), opt(p_rot), opt(p_scale), out["ori_head_pose"].data_ptr(), out["head_rot_mat"].data_ptr(),
            out["head_trans"].data_ptr(), out["lengths"].data_ptr(), out["aligned_rot_mat"].data_ptr(), out["aligned_scale"].data_ptr(),
            out["floor_normal"].data_ptr(), out["start_t_idx"].data_ptr(), out["aug_scale"].data_ptr(), _stream(dev)))
    out["seq_len"] = out["lengths"].long()
    return out


def _head_poses(head_poses, names):
    """-> [(name, [T, 7] float32)] in the mapping's order (or `names`' order)."""
    if not hasattr(head_poses, "items"):
        raise ValueError("head_poses: a {name: [T, 7] array} mapping or the entries of a motion file expected")
    got = {}
    for key, v in head_poses.items():
        name = key
        if hasattr(v, "keys"):  # an entry of a motion file
            name = v.get("seq_name", key)
            v = v["head_qpos"]
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if a.ndim != 2 or a.shape[1] != 7:
            raise ValueError(f"{name}: head pose {a.shape}, [T, 7] expected")
        got[name] = np.ascontiguousarray(a, dtype=np.float32)  # the reference's .float() (dataset:117)
    if names is not None:
        got = {n: got[n] for n in names}
    return [(n, a) for n, a in got.items() if a.shape[0] > MIN_FRAMES]


class EpochPlan:
    """The host side of GravityBatches, free of the GPU: which sequences and draw ids each batch of each epoch holds.  Sample k
    (a sequence index) of epoch e has draw id e * S + k whatever the batch size and the order; the order comes from a CPU
    generator seeded with `seed` (shuffle=False: dataset order).  state_dict() / load_state_dict() carry `epoch` and the
    generator's state."""

    def __init__(self, n_sequences, batch_size, shuffle=True, seed=0):
        self.n_sequences, self.batch_size = int(n_sequences), int(batch_size)
        if self.n_sequences < 1 or self.batch_size < 1:
            raise ValueError("n_sequences and batch_size: at least 1 expected")
        self.shuffle, self.seed = bool(shuffle), int(seed)
        self.epoch = 0
        self.generator = torch.Generator().manual_seed(self.seed)

    def __len__(self):
        return -(-self.n_sequences // self.batch_size)

    def next_epoch(self):
        """Starts the next epoch -> (order int64 [S], draw ids int64 [S], [(first, end)] of its batches in `order`)."""
        S = self.n_sequences
        order = (torch.randperm(S, generator=self.generator) if self.shuffle else torch.arange(S)).numpy().astype(np.int64)
        draws = order + np.int64(self.epoch) * S
        self.epoch += 1
        return order, draws, [(a, min(a + self.batch_size, S)) for a in range(0, S, self.batch_size)]

    def state_dict(self):
        return {"epoch": self.epoch, "generator": self.generator.get_state()}

    def load_state_dict(self, state):
        self.epoch = int(state["epoch"])
        self.generator.set_state(torch.as_tensor(state["generator"], dtype=torch.uint8).cpu())


class GravityBatches(EpochPlan):
    """The reference's DataLoader(AMASSHeadPoseDataset(...), batch_size, shuffle, drop_last=False) as an iterable of batch dicts
    built on the GPU.  head_poses: {name: [T, 7]} or the entries of a motion file ({key: {'head_qpos', 'seq_name', ...}});
    `names` picks and orders a subset (e.g. one half of split_by_dataset); sequences of at most 30 frames are dropped.  The
    poses are packed and uploaded once.  Each __iter__ is one epoch (EpochPlan.next_epoch): one host-to-device copy of the order
    and the draw ids, then ceil(S / batch_size) dicts of gravity_batch's keys plus 'seq_name' (host strings); nothing is read
    back.  `train` is kept for the reference's signature only (the split is the caller's, through `names`)."""

    def __init__(self, head_poses, batch_size, window=120, train=True, for_eval=False, shuffle=True, seed=0, device=None, names=None):
        self.device = _device(device)
        self.window = int(window)
        if self.window < 1:
            raise ValueError("window: at least 1 expected")
        self.train, self.for_eval = bool(train), bool(for_eval)
        seqs = _head_poses(head_poses, names)
        if not seqs:
            raise ValueError("no sequence of more than 30 frames")
        super().__init__(len(seqs), batch_size, shuffle, seed)
        self.names = [n for n, _ in seqs]
        offsets = np.concatenate([[0], np.cumsum([a.shape[0] for _, a in seqs])])
        if offsets[-1] >= 2 ** 31:
            raise ValueError("more than 2^31 - 1 frames in one split")
        self.pose = torch.from_numpy(np.concatenate([a for _, a in seqs], 0)).to(self.device)
        self.offsets = torch.from_numpy(offsets.astype(np.int32)).to(self.device)

    def __iter__(self):
        order, draws, batches = self.next_epoch()
        both = torch.from_numpy(np.stack([order, draws])).to(self.device)  # the epoch's one host-to-device copy
        ids, draws = both[0].to(torch.int32), both[1]
        for a, e in batches:
            batch = gravity_batch(self.pose, self.offsets, ids[a:e], draws[a:e], self.window, self.seed, self.for_eval)
            batch["seq_name"] = [self.names[k] for k in order[a:e]]
            yield batch


# ====================================================================================================== HeadNet's batches
SLAM_KEYS = ("aligned_slam_trans", "aligned_slam_rot_quat", "aligned_slam_rot_mat", "ori_slam_trans", "ori_slam_rot_quat",
             "ori_slam_rot_mat")
SLAM_COLS = 29  # a row of slam32: aligned trans 3 | aligned quat 4 | aligned rot 9 | original quat 4 | original rot 9
_TABLES = (("pose", 7, torch.float32), ("vels", 6, torch.float32), ("feats", None, torch.float32))
_SLAM_TABLES = (("slam32", SLAM_COLS, torch.float32), ("slam_trans64", 3, torch.float64))


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def pack_head_sequences(sequences, window, for_eval=False, names=None):
    """The host side of HeadBatches, free of the GPU.  sequences: a list or a {key: entry} mapping of entries {seq_name,
    head_qpos | head_pose [T, 7], head_vels [T, 6], of_feats [T - 1, D], optionally slam: the raw [L, 7] DROID-SLAM array (xyz,
    quaternion w,x,y,z), or in its place the six arrays of SLAM_KEYS of a track aligned already, which are taken as they are};
    `names` picks and orders a subset by seq_name.  Shapes are checked (ValueError; D a multiple of 4), then
    the dropping rules: training drops F = T - 1 < window, for_eval drops F < 1, and if any sequence has a SLAM track those
    without one are dropped (the reference's rule).  Each kept track is aligned with its sequence's first pose by
    stage1.load_slam_res_and_align_first, as the reference does once per sequence, and cut at T rows (no slice reaches further).
    -> a dict of numpy arrays pose [N, 7], vels [N, 6] (rounded to fp32), feats [N - S, D], offsets int32 [S + 1] and, with SLAM,
    slam32 [M, 29], slam_trans64 [M, 3], slam_offsets int32 [S + 1]; names; n_dropped {'short', 'no_slam'}."""
    from .stage1 import load_slam, load_slam_res_and_align_first
    W = int(window)
    if W < 1:
        raise ValueError(f"window {W}: at least 1 expected")
    entries = list(sequences.items()) if hasattr(sequences, "items") else list(enumerate(sequences))
    got, D = [], None
    for key, e in entries:
        if not hasattr(e, "keys"):
            raise ValueError(f"sequence {key}: a mapping with head_qpos, head_vels and of_feats expected")
        name = e.get("seq_name", key)
        pose = _np(e["head_qpos"] if "head_qpos" in e else e["head_pose"])
        vels, feats = _np(e["head_vels"]), _np(e["of_feats"])
        slam = _np(e["slam"]) if e.get("slam") is not None else None
        if slam is None and e.get(SLAM_KEYS[0]) is not None:  # a track aligned already: the six arrays, taken as they are
            slam = {k: _np(e[k]) for k in SLAM_KEYS}
            L = slam[SLAM_KEYS[0]].shape[0]
            for k, tail in zip(SLAM_KEYS, ((3,), (4,), (3, 3), (3,), (4,), (3, 3))):
                if slam[k].shape != (L,) + tail or L < 1:
                    raise ValueError(f"{name}: {k} {slam[k].shape}, {(L,) + tail} expected")
        T = pose.shape[0]
        if pose.ndim != 2 or pose.shape[1] != 7 or T < 1:
            raise ValueError(f"{name}: head pose {pose.shape}, [T, 7] expected")
        if vels.shape != (T, 6):
            raise ValueError(f"{name}: head_vels {vels.shape}, [{T}, 6] expected")
        if feats.ndim != 2 or feats.shape[0] != T - 1:
            raise ValueError(f"{name}: of_feats {feats.shape}, [{T - 1}, D] expected")
        if feats.shape[1] < 4 or feats.shape[1] % 4 != 0 or (D is not None and feats.shape[1] != D):
            raise ValueError(f"{name}: of_feats {feats.shape}: one D for all sequences, a multiple of 4, expected")
        D = feats.shape[1]
        if slam is not None and not isinstance(slam, dict) and (slam.ndim != 2 or slam.shape[1] != 7 or slam.shape[0] < 1):
            raise ValueError(f"{name}: slam {slam.shape}, [L, 7] expected")
        got.append((name, pose, vels, feats, slam))
    if names is not None:
        by = {g[0]: g for g in got}
        got = [by[n] for n in names]
    dropped = {"short": 0, "no_slam": 0}
    any_slam = any(g[4] is not None for g in got)
    kept = []
    for g in got:
        F = g[1].shape[0] - 1
        if F < (1 if for_eval else W):
            dropped["short"] += 1
        elif any_slam and g[4] is None:
            dropped["no_slam"] += 1
        else:
            kept.append(g)
    if not kept:
        raise ValueError(f"no sequence left ({dropped}): training needs at least `window` = {W} feature frames, for_eval one")
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    lens = [g[1].shape[0] for g in kept]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 frames in one split")
    out = {"names": [g[0] for g in kept], "n_dropped": dropped, "offsets": offsets.astype(np.int32),
           "pose": f32(np.concatenate([g[1] for g in kept], 0)),       # the reference's collate keeps head_qpos' fp32
           "vels": f32(np.concatenate([g[2] for g in kept], 0)),       # fp64 in the reference: compute_loss's .float(), done once
           "feats": f32(np.concatenate([g[3] for g in kept], 0))}
    if any_slam:
        rows32, rows64, ls = [], [], []
        for _, pose, _, _, slam in kept:
            T = pose.shape[0]
            if isinstance(slam, dict):
                at, aq, ar, ot, oq, orot = (slam[k] for k in SLAM_KEYS)
            else:
                at, ar, aq = load_slam_res_and_align_first(slam, pose)
                ot, orot, oq = load_slam(slam)
            L = min(T, at.shape[0])
            rows32.append(np.concatenate([f32(at)[:L], f32(aq)[:L], f32(ar)[:L].reshape(L, 9), f32(oq)[:L], f32(orot)[:L].reshape(L, 9)], 1))
            rows64.append(np.ascontiguousarray(ot[:L], dtype=np.float64))   # not rounded: estimate_head_pose subtracts its first row
            ls.append(L)
        out.update(slam32=np.concatenate(rows32, 0), slam_trans64=np.concatenate(rows64, 0),
                   slam_offsets=np.concatenate([[0], np.cumsum(ls)]).astype(np.int32))
    return out


def _check_tables(tables):
    """The shapes and dtypes of head_batch's tables -> (N, S or None, D, with_slam); the device is not looked at."""
    if not hasattr(tables, "keys"):
        raise ValueError("tables: a dict of pose, vels, feats, offsets (and slam32, slam_trans64, slam_offsets) expected")
    have = [k for k in ("slam32", "slam_trans64", "slam_offsets") if tables.get(k) is not None]
    if len(have) not in (0, 3):
        raise ValueError(f"tables: {have} without the rest: the three SLAM tables go together")
    for name, cols, dtype in _TABLES + (_SLAM_TABLES if have else ()):
        t = tables[name]
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or (cols is not None and t.shape[1] != cols) or t.dtype != dtype or \
                not t.is_contiguous():
            raise ValueError(f"{name} {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}: a contiguous {dtype} "
                             f"[rows, {'D' if cols is None else cols}] tensor expected")
    N, D = tables["pose"].shape[0], tables["feats"].shape[1]
    if D < 4 or D % 4 != 0:
        raise ValueError(f"feats {tuple(tables['feats'].shape)}: D a multiple of 4 expected (rows move 16 bytes per lane)")
    if tables["vels"].shape[0] != N or N < 1:
        raise ValueError(f"pose {tuple(tables['pose'].shape)} and vels {tuple(tables['vels'].shape)}: the same N >= 1 rows expected")
    if have and tables["slam32"].shape[0] != tables["slam_trans64"].shape[0]:
        raise ValueError("slam32 and slam_trans64: the same rows expected")
    return N, D, bool(have)


def _offsets(offsets, rows, dev, what, least):
    """A table of row offsets: host data is checked (steps of at least `least`, the last one `rows`) -> int32 on the device."""
    if isinstance(offsets, torch.Tensor) and offsets.device.type == "cuda":
        return _i32(offsets, dev, what)
    off = np.asarray(_np(offsets), np.int64).reshape(-1)
    if off.size < 2 or off[0] != 0 or off[-1] != rows or (np.diff(off) < least).any():
        raise ValueError(f"{what}: 0 = {what}[0] <= ... <= {what}[S] = {rows} in steps of at least {least} expected")
    return _i32(off, dev, what)


def head_batch(tables, seq_ids, draw_ids, window, seed, for_eval=False, start=None):
    """One batch of HeadNet's training data.  tables: a dict of device tensors pose [N, 7], vels [N, 6], feats [N - S, D] fp32,
    offsets int32 [S + 1] (sequence k: rows offsets[k] .. offsets[k + 1] - 1 of pose and vels, its T_k - 1 feature rows from row
    offsets[k] - k) and optionally slam32 [M, 29] fp32, slam_trans64 [M, 3] fp64, slam_offsets [S + 1] (pack_head_sequences builds
    them); seq_ids [B], draw_ids [B]; start [B]: planted starts, None for "draw them" (for_eval always starts at 0 and takes
    n = min(F, window) frames: pass the batch's largest F as `window`).  -> the reference's keys as device tensors: of [B, window, D],
    head_pose [B, window + 1, 7], head_vels [B, window, 6] (fp32), seq_len int64 [B]; lengths (seq_len as int32), start_t_idx int32;
    with SLAM tables aligned_slam_trans / _rot_quat / _rot_mat and ori_slam_trans (fp64) / _rot_quat / _rot_mat [B, window + 1, ...]
    and pose_lengths int32 [B], the rows the reference's slice of the track has; rows past a sample's end are zero.  Ids and
    offsets that are host data are checked here; device tensors are not read back (the kernel writes an empty sample, seq_len 0,
    for an id, a sequence shorter than the window or a planted start that does not fit)."""
    N, D, with_slam = _check_tables(tables)
    pose = tables["pose"]
    if any(tables[k].device.type != "cuda" or tables[k].device != pose.device for k, _, _ in _TABLES + (_SLAM_TABLES if with_slam else ())):
        raise _lib.EgoEgoHipError("head_batch needs its tables on one cuda (ROCm) device; there is no CPU path")
    dev = pose.device
    W = int(window)
    if W < 1:
        raise ValueError(f"window {W}: at least 1 expected")
    off = _offsets(tables["offsets"], N, dev, "offsets", 1)
    S = off.numel() - 1
    if S < 1 or tables["feats"].shape[0] != N - S:
        raise ValueError(f"feats {tuple(tables['feats'].shape)}: N - S = {N - S} rows expected (one less than pose per sequence)")
    M = tables["slam32"].shape[0] if with_slam else 0
    soff = _offsets(tables["slam_offsets"], M, dev, "slam_offsets", 0) if with_slam else None
    if soff is not None and soff.numel() != S + 1:
        raise ValueError(f"slam_offsets [{soff.numel()}]: [{S + 1}] expected")
    if not (isinstance(seq_ids, torch.Tensor) and seq_ids.device.type == "cuda"):
        ids = np.asarray(_np(seq_ids), np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= S):
            raise ValueError(f"seq_ids: values in 0 .. {S - 1} expected")
        seq_ids = ids
    sid = _i32(seq_ids, dev, "seq_ids")
    B = sid.numel()
    if B < 1:
        raise ValueError("an empty batch")
    did = torch.as_tensor(draw_ids)
    if tuple(did.shape) != (B,):
        raise ValueError(f"draw_ids {tuple(did.shape)}: [{B}] expected")
    did = did.to(dev, torch.int64).contiguous()
    p_start = None if start is None else _i32(start, dev, "start", B)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {"head_pose": torch.empty(B, W + 1, 7, **f32), "head_vels": torch.empty(B, W, 6, **f32), "of": torch.empty(B, W, D, **f32),
           "lengths": torch.empty(B, **i32), "start_t_idx": torch.empty(B, **i32)}
    slam_out = [None] * 7
    if with_slam:
        out.update({"aligned_slam_trans": torch.empty(B, W + 1, 3, **f32), "aligned_slam_rot_quat": torch.empty(B, W + 1, 4, **f32),
                    "aligned_slam_rot_mat": torch.empty(B, W + 1, 3, 3, **f32),
                    "ori_slam_trans": torch.empty(B, W + 1, 3, device=dev, dtype=torch.float64),
                    "ori_slam_rot_quat": torch.empty(B, W + 1, 4, **f32), "ori_slam_rot_mat": torch.empty(B, W + 1, 3, 3, **f32),
                    "pose_lengths": torch.empty(B, **i32)})
        slam_out = [out[k].data_ptr() for k in SLAM_KEYS + ("pose_lengths",)]
    opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        _lib.check_s1_data(_lib.load().egoego_s1_head_batch(
            pose.data_ptr(), tables["vels"].data_ptr(), tables["feats"].data_ptr(), N, D, off.data_ptr(), S,
            opt(tables["slam32"] if with_slam else None), opt(tables["slam_trans64"] if with_slam else None), opt(soff), M,
            sid.data_ptr(), did.data_ptr(), B, W, int(seed) & (2 ** 64 - 1), int(bool(for_eval)), opt(p_start),
            out["head_pose"].data_ptr(), out["head_vels"].data_ptr(), out["of"].data_ptr(), out["lengths"].data_ptr(),
            out["start_t_idx"].data_ptr(), *slam_out, _stream(dev)))
    out["seq_len"] = out["lengths"].long()
    return out


class HeadBatches(EpochPlan):
    """The reference's DataLoader(ARESHeadPoseDataset(...), batch_size, shuffle, drop_last=False) as an iterable of batch dicts
    built on the GPU.  sequences: what load_ares_split returns (pack_head_sequences documents the entries, the checks and the
    dropping rules; n_dropped counts them by reason); `names` picks and orders a subset.  Construction aligns each SLAM track on
    the host, packs the tables and uploads them once.  Each __iter__ is one epoch (EpochPlan.next_epoch): one host-to-device copy
    of the order and the draw ids, then ceil(S / batch_size) dicts of head_batch's keys plus 'seq_name' (host strings); nothing is
    read back.  Sample k of epoch e has draw id e * S + k.  Training batches are windows of `window` frames at drawn starts;
    for_eval batches hold whole sequences from frame 0, padded to the batch's longest, and carry lengths_host and
    pose_lengths_host, the plain lists forward_for_eval(lengths=, pose_lengths=) and estimate_head_pose take.

    head_vels is fp32 here and fp64 in the reference's collate: its one consumer, compute_loss, converts it with .float() on
    arrival, and the upload rounds the same fp64 numbers the same way, so the loss sees the same bits.  `train` is kept for the
    reference's signature only (the split is the caller's)."""

    def __init__(self, sequences, batch_size, window=90, train=True, for_eval=False, shuffle=True, seed=0, device=None, names=None):
        self.window = int(window)
        self.train, self.for_eval = bool(train), bool(for_eval)
        packed = pack_head_sequences(sequences, self.window, self.for_eval, names)
        self.device = _device(device)
        self.names, self.n_dropped = packed["names"], packed["n_dropped"]
        super().__init__(len(self.names), batch_size, shuffle, seed)
        self.feat_lengths = (np.diff(packed["offsets"]) - 1).tolist()
        keys = ["pose", "vels", "feats", "offsets"] + (["slam32", "slam_trans64", "slam_offsets"] if "slam32" in packed else [])
        self.tables = {k: torch.from_numpy(packed[k]).to(self.device) for k in keys}
        self.slam_lengths = np.diff(packed["slam_offsets"]).tolist() if "slam32" in packed else None

    def __iter__(self):
        order, draws, batches = self.next_epoch()
        both = torch.from_numpy(np.stack([order, draws])).to(self.device)  # the epoch's one host-to-device copy
        ids, draws = both[0].to(torch.int32), both[1]
        for a, e in batches:
            F = [self.feat_lengths[k] for k in order[a:e]]
            batch = head_batch(self.tables, ids[a:e], draws[a:e], max(F) if self.for_eval else self.window, self.seed, self.for_eval)
            batch["seq_name"] = [self.names[k] for k in order[a:e]]
            if self.for_eval:
                batch["lengths_host"] = F
                if self.slam_lengths is not None:
                    batch["pose_lengths_host"] = [min(self.slam_lengths[k], f + 1) for k, f in zip(order[a:e], F)]
            yield batch


class AresSplit(list):
    """load_ares_split's result: the list of sequence entries, with n_dropped = {'filter', 'no_slam'}."""
    n_dropped = None


def load_ares_split(data_root_folder, train, window, cache=None):
    """ARESHeadPoseDataset.__init__ (ares_headpose_dataset.py:24-109) up to the arrays, without a GPU: the motion file
    <root>/ares_egoego_processed/{train,test}_ares_smplh_motion.p; the filter (a sequence stays iff T > window and T - 1 ==
    len(of_files)); each feature file, its recorded path moved from the folder above stage1.ARES_SRC_ROOT to <root>/ares and from
    raft_flows to raft_of_feats; the SLAM file <root>/ares/droid_slam_res/<scene>/<rest>.npy, sequences without one dropped and
    counted.  -> an AresSplit: a list of {seq_name, head_qpos, head_vels, of_feats [T - 1, D], slam [L, 7]}, what HeadBatches takes.

    cache=PATH: the arrays and names are written to that one file (numpy's zip of arrays); a later call with the same arguments
    reads it alone and opens neither the motion file nor any feature file."""
    from .stage1 import ARES_SRC_ROOT
    tag = json.dumps({"train": bool(train), "window": int(window)}, sort_keys=True)
    if cache is not None and os.path.exists(cache):
        with np.load(cache, allow_pickle=False) as z:
            if str(z["tag"]) != tag:
                raise ValueError(f"{cache} holds {z['tag']}, not {tag}")
            out = AresSplit()
            out.n_dropped = json.loads(str(z["n_dropped"]))
            rows, srows = np.cumsum(np.concatenate([[0], z["lengths"]])), np.cumsum(np.concatenate([[0], z["slam_lengths"]]))
            pose, vels, feats, slam = z["pose"], z["vels"], z["feats"], z["slam"]
            for k, name in enumerate(z["names"].tolist()):
                a, e = rows[k], rows[k + 1]
                out.append({"seq_name": name, "head_qpos": pose[a:e], "head_vels": vels[a:e], "of_feats": feats[a - k:e - k - 1],
                            "slam": slam[srows[k]:srows[k + 1]]})
        return out
    import joblib
    data = joblib.load(os.path.join(data_root_folder, "ares_egoego_processed", f"{'train' if train else 'test'}_ares_smplh_motion.p"))
    src, dst = os.path.dirname(ARES_SRC_ROOT), os.path.join(data_root_folder, "ares")
    out = AresSplit()
    out.n_dropped = {"filter": 0, "no_slam": 0}
    for k in data:
        item = data[k]
        T, files = item["head_qpos"].shape[0], item["of_files"]
        if not (T > window and T - 1 == len(files)):
            out.n_dropped["filter"] += 1
            continue
        name = item["seq_name"]
        npy = os.path.join(dst, "droid_slam_res", name.split("-")[0], "-".join(name.split("-")[1:]) + ".npy")
        if not os.path.exists(npy):
            out.n_dropped["no_slam"] += 1
            continue
        feats = np.stack([np.load(f.replace(src, dst).replace("raft_flows", "raft_of_feats")) for f in files])
        out.append({"seq_name": name, "head_qpos": np.asarray(item["head_qpos"]), "head_vels": np.asarray(item["head_vels"]),
                    "of_feats": feats, "slam": np.load(npy)})
    if cache is not None:
        if not out:
            raise ValueError("no sequence left to cache")
        os.makedirs(os.path.dirname(os.path.abspath(cache)), exist_ok=True)
        with open(cache, "wb") as f:
            np.savez(f, tag=np.array(tag), n_dropped=np.array(json.dumps(out.n_dropped)), names=np.array([s["seq_name"] for s in out]),
                     lengths=np.array([s["head_qpos"].shape[0] for s in out], np.int64),
                     slam_lengths=np.array([s["slam"].shape[0] for s in out], np.int64),
                     pose=np.concatenate([s["head_qpos"] for s in out], 0), vels=np.concatenate([s["head_vels"] for s in out], 0),
                     feats=np.concatenate([s["of_feats"] for s in out], 0), slam=np.concatenate([s["slam"] for s in out], 0))
    return out
