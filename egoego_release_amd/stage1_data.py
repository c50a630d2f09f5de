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
"""
import numpy as np
import torch

from . import _lib
from .motion_data import _stream

TRAIN_DATASETS = ("CMU", "MPI_Limits", "TotalCapture", "Eyes_Japan_Dataset", "KIT", "BioMotionLab_NTroje", "BMLmovi", "EKUT", "ACCAD")
MIN_FRAMES = 30  # sequences of at most this many frames are dropped (dataset:97)


def _device(device):
    what = "GravityNet's training batches need a cuda (ROCm) device; they have no CPU path"
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
