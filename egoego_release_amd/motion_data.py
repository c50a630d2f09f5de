"""Raw SMPL-H motion -> what stage 2 consumes, on libegoego_hip: the arithmetic of the reference's AMASSDataset
(egoego/data/amass_diffusion_dataset.py) between the raw arrays (`trans`, `root_orient`, `body_pose` per sequence, as in AMASS,
ARES and demo_ares_data.p) and the tensors, for all windows of all sequences in one launch.

  window_table             cal_normalize_data_input's enumeration of the windows (316-335), on the host
  build_motion_windows     process_window_data (409-510) for every window: canonicalised joints, velocities, 6D rotations
  MotionWindows.stats      extract_min_max_mean_std_from_data (355-377)
  MotionWindows.motion     __getitem__ (515-538): the normalised [N, window, 198] model input (`x_start`, `conditions`)
  MotionWindowDataset      the Dataset whose items are {'motion', 'seq_len'}
  rest_pose_offsets        get_rest_pose_joints (248-263) through body.BodyModel

File formats and loaders stay outside: the caller brings the arrays.  There is no CPU path: building, `stats()` and `motion()`
need a ROCm device and raise EgoEgoHipError without one.  The window dictionaries (`to_window_data_dict`,
`from_window_data_dict`) are host data in the reference's layout; a file written from them loads in the reference and back.
"""
import ctypes as C

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _lib
from .harness import SMPLH_PARENTS_22, SkeletonStats, prep_padding_mask

N_JOINTS = 22
STAT_KEYS = ("global_jpos_min", "global_jpos_max", "global_jvel_min", "global_jvel_max")


def window_table(lengths, window=120, min_frames=30):
    """The windows cal_normalize_data_input cuts from sequences of `lengths` frames, in its order, as int64 arrays
    (seq_index, start_t_idx, end_t_idx, length).  Its rule, oddities included: starts every window // 2 frames;
    end = start + window - 1, and end = num_steps (one past the last frame) once that leaves the sequence; a window with
    end - start < min_frames is skipped; the frames are [start : end + 1] clipped by the sequence, so `length` is
    min(end + 1, num_steps) - start while `end_t_idx` keeps the unclipped value."""
    window = int(window)
    if window < 2:
        raise ValueError(f"window {window}: at least 2 expected (the stride is window // 2)")
    rows = []
    for k, num_steps in enumerate(int(n) for n in np.asarray(lengths).reshape(-1)):
        for start in range(0, num_steps, window // 2):
            end = start + window - 1
            if end >= num_steps:
                end = num_steps
            if end - start < min_frames:
                continue
            rows.append((k, start, end, min(end + 1, num_steps) - start))
    t = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), t[:, 3].copy()


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.EgoEgoHipError("the motion windows need a cuda (ROCm) device; they have no CPU path")
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise _lib.EgoEgoHipError(f"device {dev}: the motion windows need a cuda (ROCm) device; they have no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _host_f32(a, width):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a.astype(np.float32).reshape(-1, width))  # the reference's .float() (dataset:410-412)


def _sequences(sequences):
    """-> (trans [F, 3], root_orient [F, 3], body_pose [F, 63] float32 on the host, lengths, one name per sequence)"""
    if isinstance(sequences, dict):
        seqs = [sequences[k] for k in sequences]
        if not seqs:
            raise ValueError("no sequences")
        parts = [[_host_f32(s[key], w) for s in seqs] for key, w in (("trans", 3), ("root_orient", 3), ("body_pose", 63))]
        lengths = [p.shape[0] for p in parts[0]]
        names = [s.get("seq_name", str(k)) for k, s in zip(sequences, seqs)]
        trans, root, body = (np.concatenate(p, 0) for p in parts)
    else:
        trans, root, body, lengths = sequences
        trans, root, body = _host_f32(trans, 3), _host_f32(root, 3), _host_f32(body, 63)
        lengths = [int(n) for n in np.asarray(lengths).reshape(-1)]
        names = [str(k) for k in range(len(lengths))]
    F = trans.shape[0]
    if root.shape[0] != F or body.shape[0] != F or sum(lengths) != F or any(n < 0 for n in lengths):
        raise ValueError(f"trans {trans.shape}, root_orient {root.shape}, body_pose {body.shape} and lengths (sum {sum(lengths)}) disagree")
    return trans, root, body, lengths, names


class MotionWindows:
    """N windows padded to `window` frames.  Tensors: global_jpos, global_jvel [N, W, 66], global_rot_6d, local_rot_6d
    [N, W, 132], recover_rot_quat [N, 4], seq_len [N] int32; rows past a window's length are zero.  Host data: the table
    (seq_index, start_t_idx, end_t_idx, length: int64 [N]) and seq_names (one per window)."""

    def __init__(self, window, global_jpos, global_jvel, global_rot_6d, local_rot_6d, recover_rot_quat, seq_len, seq_index, start_t_idx,
                 end_t_idx, length, seq_names, rest_offsets=None, parents=SMPLH_PARENTS_22):
        self.window = int(window)
        self.global_jpos, self.global_jvel, self.global_rot_6d, self.local_rot_6d = global_jpos, global_jvel, global_rot_6d, local_rot_6d
        self.recover_rot_quat, self.seq_len = recover_rot_quat, seq_len
        self.seq_index, self.start_t_idx, self.end_t_idx, self.length = seq_index, start_t_idx, end_t_idx, length
        self.seq_names = list(seq_names)
        self.rest_offsets, self.parents = rest_offsets, tuple(int(p) for p in parents)
        self._stats = None

    def __len__(self):
        return int(self.global_jpos.shape[0])

    @property
    def device(self):
        return self.global_jpos.device

    def _on_device(self, what):
        if self.device.type != "cuda":
            raise _lib.EgoEgoHipError(f"{what} needs the windows on a cuda (ROCm) device; it has no CPU path")
        return self.device

    def stats(self):
        """{'global_jpos_min', 'global_jpos_max', 'global_jvel_min', 'global_jvel_max'}: float32 [66] arrays over the real frames
        of all windows (overlapping windows count twice and every window's zero last velocity is included, as the reference
        stacks the stored windows).  Waits for the device once; the result is kept."""
        if self._stats is None:
            self._stats = dict(zip(STAT_KEYS, self._stats_tensor().cpu().numpy()))
        return {k: v.copy() for k, v in self._stats.items()}

    def _stats_tensor(self):
        dev = self._on_device("stats()")
        N, W = len(self), self.window
        if N == 0:
            raise ValueError("no windows: the statistics are undefined")
        lib = _lib.load()
        out = torch.empty(4, 3 * N_JOINTS, device=dev)
        nbytes = lib.egoego_win_stats_workspace_bytes(N, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check_win(lib.egoego_win_stats(self.global_jpos.data_ptr(), self.global_jvel.data_ptr(), self.seq_len.data_ptr(), N, W,
                                                out.data_ptr(), ws.data_ptr(), nbytes, _stream(dev)))
        return out

    def motion(self, stats=None):
        """[N, W, 198]: the positions min/max-normalised with `stats` (a dict with global_jpos_min / global_jpos_max, e.g. another
        split's; None: this object's own) followed by the global 6D rotations; zero rows past each length."""
        dev = self._on_device("motion()")
        N, W = len(self), self.window
        out = torch.empty(N, W, 9 * N_JOINTS, device=dev)
        if N == 0:
            return out
        if stats is None:
            st = self._stats_tensor()
            lo, hi = st[0].contiguous(), st[1].contiguous()
        else:
            lo, hi = (torch.as_tensor(np.asarray(stats[k], np.float32).reshape(-1)).to(dev) for k in STAT_KEYS[:2])
            if lo.numel() != 66 or hi.numel() != 66:
                raise ValueError("stats: 66 values per key expected")
        with torch.cuda.device(dev):
            _lib.check_win(_lib.load().egoego_win_motion(self.global_jpos.data_ptr(), self.global_rot_6d.data_ptr(), self.seq_len.data_ptr(),
                                                         lo.data_ptr(), hi.data_ptr(), N, W, out.data_ptr(), _stream(dev)))
        return out

    def padding_mask(self):
        """[N, 1, W + 1] bool: harness.prep_padding_mask on these windows."""
        return prep_padding_mask(self.global_jpos, self.seq_len, self.window)

    def skeleton_stats(self, stats=None):
        """A harness.SkeletonStats from `stats` (None: this object's own) and the rest offsets the windows were built with."""
        if self.rest_offsets is None:
            raise ValueError("these windows carry no rest offsets (from_window_data_dict): build a SkeletonStats directly")
        stats = self.stats() if stats is None else stats
        return SkeletonStats(stats["global_jpos_min"], stats["global_jpos_max"], self.rest_offsets, self.parents)

    def to_window_data_dict(self):
        """The reference's window_data_dict: {i: {'seq_name', 'start_t_idx', 'end_t_idx', 'global_jpos' [len, 66], 'global_jvel'
        [len, 66], 'global_rot_6d' [len, 132]}} with float32 numpy arrays."""
        arrays = [t.detach().cpu().numpy() for t in (self.global_jpos, self.global_jvel, self.global_rot_6d)]
        d = {}
        for i in range(len(self)):
            n = int(self.length[i])
            d[i] = {"seq_name": self.seq_names[i], "start_t_idx": int(self.start_t_idx[i]), "end_t_idx": int(self.end_t_idx[i]),
                    "global_jpos": arrays[0][i, :n].copy(), "global_jvel": arrays[1][i, :n].copy(), "global_rot_6d": arrays[2][i, :n].copy()}
        return d

    @classmethod
    def from_window_data_dict(cls, d, window=None, device=None):
        """The inverse of to_window_data_dict (a dictionary the reference wrote included).  `window` defaults to the longest
        window; the tensors stay on the host unless `device` is given.  What the dictionary does not hold is None: local_rot_6d,
        recover_rot_quat, seq_index, the rest offsets."""
        keys = list(d)
        length = np.asarray([np.asarray(d[k]["global_jpos"]).shape[0] for k in keys], dtype=np.int64)
        W = int(window) if window is not None else int(length.max()) if len(keys) else 0
        if len(keys) and length.max() > W:
            raise ValueError(f"a window of {int(length.max())} frames does not fit window={W}")
        out = [np.zeros((len(keys), W, w), np.float32) for w in (66, 66, 132)]
        for i, k in enumerate(keys):
            for o, name in zip(out, ("global_jpos", "global_jvel", "global_rot_6d")):
                o[i, :length[i]] = np.asarray(d[k][name], np.float32).reshape(length[i], -1)
        dev = torch.device("cpu") if device is None else _device(device)
        jpos, jvel, rot = (torch.from_numpy(o).to(dev) for o in out)
        return cls(W, jpos, jvel, rot, None, None, torch.from_numpy(length.astype(np.int32)).to(dev), None,
                   np.asarray([int(d[k]["start_t_idx"]) for k in keys], dtype=np.int64),
                   np.asarray([int(d[k]["end_t_idx"]) for k in keys], dtype=np.int64), length, [d[k]["seq_name"] for k in keys])


def build_motion_windows(sequences, rest_offsets, window=120, canonicalize_init_head=True, device=None, parents=None, min_frames=30):
    """`sequences`: a dict like the reference's data_dict ({k: {'trans' [T, 3], 'root_orient' [T, 3], 'body_pose' [T, 63],
    'seq_name', ...}}) or a tuple (trans [F, 3], root_orient [F, 3], body_pose [F, 63], lengths) of concatenated arrays;
    `rest_offsets` [22, 3] (rest_pose_offsets, or an .npy of them).  -> MotionWindows on `device`, in the reference's window order.
    canonicalize_init_head=False is the reference's other branch: the heading is the identity."""
    dev = _device(device)
    trans, root, body, lengths, names = _sequences(sequences)
    W = int(window)
    lib = _lib.load()
    if W > lib.egoego_win_max_window():
        raise ValueError(f"window {W}: at most {lib.egoego_win_max_window()} frames")
    seq_index, start, end, length = window_table(lengths, W, min_frames)
    N = len(seq_index)
    rest = torch.as_tensor(rest_offsets).detach().to(dev, torch.float32).reshape(-1).contiguous()
    if rest.numel() != 3 * N_JOINTS:
        raise ValueError(f"rest_offsets has {rest.numel()} values: {N_JOINTS} x 3 expected")
    parents = SMPLH_PARENTS_22 if parents is None else tuple(int(p) for p in parents)
    if len(parents) != N_JOINTS:
        raise ValueError(f"parents has {len(parents)} entries: {N_JOINTS} expected")
    f32 = dict(device=dev, dtype=torch.float32)
    jpos, jvel = torch.empty(N, W, 66, **f32), torch.empty(N, W, 66, **f32)
    grot, lrot, rec = torch.empty(N, W, 132, **f32), torch.empty(N, W, 132, **f32), torch.empty(N, 4, **f32)
    seq_len = torch.from_numpy(length.astype(np.int32)).to(dev)
    if N:
        first = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)[seq_index] + start
        d_first = torch.from_numpy(first.astype(np.int32)).to(dev)
        d_trans, d_root, d_body = (torch.from_numpy(a).to(dev) for a in (trans, root, body))
        par = (C.c_int32 * N_JOINTS)(*parents)
        with torch.cuda.device(dev):
            _lib.check_win(lib.egoego_win_build(d_trans.data_ptr(), d_root.data_ptr(), d_body.data_ptr(), trans.shape[0], rest.data_ptr(), par,
                                                d_first.data_ptr(), seq_len.data_ptr(), N, W, int(bool(canonicalize_init_head)),
                                                jpos.data_ptr(), jvel.data_ptr(), grot.data_ptr(), lrot.data_ptr(), rec.data_ptr(),
                                                _stream(dev)))
    return MotionWindows(W, jpos, jvel, grot, lrot, rec, seq_len, seq_index, start, end, length, [names[k] for k in seq_index],
                         rest.reshape(N_JOINTS, 3), parents)


class MotionWindowDataset(Dataset):
    """AMASSDataset.__getitem__ over prebuilt windows: item i is {'motion': [W, 198] (a row of windows.motion(stats), on the
    windows' device), 'seq_len': int}.  `stats`: the training split's statistics; None: the windows' own."""

    def __init__(self, windows, stats=None):
        self.windows = windows
        self.motion = windows.motion(stats)

    def __len__(self):
        return len(self.windows)

    def __getitem__(self, index):
        return {"motion": self.motion[index], "seq_len": int(self.windows.length[index])}


def rest_pose_offsets(body_model):
    """get_rest_pose_joints (dataset:248-263): the joints of `body_model` (a body.BodyModel) at zero pose, zero betas and zero
    translation, each minus its parent; the root's parent is the root itself, so its row is 0.  -> [22, 3] on the model's device."""
    joints = body_model().Jtr[0, :N_JOINTS]
    parents = body_model.parents[:N_JOINTS].to(joints.device, torch.long).clone()
    parents[0] = 0
    return joints - joints[parents]
