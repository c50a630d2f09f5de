"""Batched evaluation of sampled motions on libegoego_hip: what the reference's evaluation loop does per sample on the host
(eval_egoego.py:358-446, run_egoego.py:160-175), for hundreds of samples of different lengths in a handful of launches.

  fk_smpl                               fk_smpl (amass_diffusion_dataset.py:265-293) in fp64, rounded once
  determine_floor_height_and_contacts   utils/data_utils/process_amass_dataset.py:160-338, with sklearn's 1-D DBSCAN restated on the
                                        sorted line inside the kernel (csrc/eval_metrics.h)
  compute_metrics_for_smpl              kinpoly/scripts/eval_metrics_imu_rec.py:264-342
  evaluate_samples                      eval_egoego.py:369-446 in one call: FK, the xy shift by the first frame's head, floor
                                        heights, metrics, the root moved to the floor, and the best sample per group

All inputs and outputs are device tensors; neither sklearn nor numpy runs.  There is no CPU path: a call on a CPU tensor raises.
Sequences in a batch may differ in length: `lengths` [B] gives the real frames of each, the rest of the padded T is ignored.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .harness import HEAD_IDX, _parents_of

N_JOINTS = 22
MAX_FRAMES = 4096  # egoego_eval_max_frames(): 2 T static-height samples are sorted and clustered inside one workgroup's LDS
METRIC_KEYS = _lib.EVAL_METRIC_KEYS
MPJPE_COLUMN = METRIC_KEYS.index("mpjpe")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device_of(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _lib.EgoEgoHipError(f"{what} must be a tensor on a cuda (ROCm) device; the evaluation has no CPU path")
    return t.device


def _f32(t, dev):
    return torch.as_tensor(t).to(dev, torch.float32).contiguous()


def _lengths(lengths, B, T, dev, minimum):
    """None -> (None, no pointer); else an int32 device tensor.  Host values are validated here; a device tensor is taken as
    given (the kernels clamp it to 0..T) so that no call waits for the device."""
    if lengths is None:
        if T < minimum:
            raise ValueError(f"T = {T}: at least {minimum} frames are needed")
        return None, None
    if isinstance(lengths, torch.Tensor) and lengths.device.type == "cuda":
        t = lengths.to(dev, torch.int32).contiguous()
    else:
        a = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths).astype(np.int64).reshape(-1)
        if a.size and (a.min() < minimum or a.max() > T):
            raise ValueError(f"lengths span {int(a.min())}..{int(a.max())}: {minimum}..{T} (the padded T) expected")
        t = torch.as_tensor(a, dtype=torch.int32).to(dev)
    if t.shape != (B,):
        raise ValueError(f"lengths {tuple(t.shape)}: [{B}] expected")
    return t, t.data_ptr()


def fk_smpl(root_trans, local_aa, rest_offsets, parents=None):
    """root_trans [..., 3], local axis-angle [..., 22, 3], rest_offsets [22, 3] -> (global quaternions [..., 22, 4] (w, x, y, z;
    w >= 0), global joints [..., 22, 3])."""
    local_aa, root_trans, rest_offsets = torch.as_tensor(local_aa), torch.as_tensor(root_trans), torch.as_tensor(rest_offsets)
    if local_aa.dim() < 2 or local_aa.shape[-2:] != (N_JOINTS, 3):
        raise ValueError(f"local_aa {tuple(local_aa.shape)}: [..., {N_JOINTS}, 3] expected")
    if root_trans.shape != local_aa.shape[:-2] + (3,):
        raise ValueError(f"root_trans {tuple(root_trans.shape)}: {tuple(local_aa.shape[:-2]) + (3,)} expected")
    if rest_offsets.numel() != N_JOINTS * 3:
        raise ValueError(f"rest_offsets has {rest_offsets.numel()} values: {N_JOINTS} x 3 expected")
    dev = _device_of(local_aa, "local_aa")
    aa, root, rest = _f32(local_aa, dev), _f32(root_trans, dev), _f32(rest_offsets, dev).reshape(-1)
    parents = _parents_of(None, parents)
    if len(parents) != N_JOINTS:
        raise ValueError(f"parents has {len(parents)} entries: {N_JOINTS} expected")
    lead = aa.shape[:-2]
    N = int(np.prod(lead)) if lead else 1
    quat = torch.empty(lead + (N_JOINTS, 4), device=dev)
    jpos = torch.empty(lead + (N_JOINTS, 3), device=dev)
    if N == 0:
        return quat, jpos
    par = (C.c_int32 * N_JOINTS)(*[int(p) for p in parents])
    with torch.cuda.device(dev):
        _lib.check_eval(_lib.load().egoego_eval_fk(root.data_ptr(), aa.data_ptr(), rest.data_ptr(), par, N, quat.data_ptr(),
                                                   jpos.data_ptr(), _stream(dev)))
    return quat, jpos


def _check_jpos(t, what):
    if t.dim() != 4 or t.shape[-2:] != (N_JOINTS, 3) or t.shape[0] < 1:
        raise ValueError(f"{what} {tuple(t.shape)}: [B, T, {N_JOINTS}, 3] expected")


def shift_xy_(jpos, joint=HEAD_IDX):
    """In place: every joint of each sequence of jpos [B, T, 22, 3] moves by minus the xy of `joint` in its first frame
    (eval_egoego.py:376-383)."""
    _check_jpos(jpos, "jpos")
    dev = _device_of(jpos, "jpos")
    if jpos.dtype != torch.float32 or not jpos.is_contiguous():
        raise ValueError("jpos must be a contiguous float32 tensor")
    with torch.cuda.device(dev):
        _lib.check_eval(_lib.load().egoego_eval_shift_xy(jpos.data_ptr(), jpos.shape[0], jpos.shape[1], int(joint), _stream(dev)))
    return jpos


def root_to_floor(jpos, floor_height):
    """jpos [B, T, 22, 3], floor_height [B] -> [B, T, 3]: the root joint with the floor height taken off z (run_egoego.py:166-173)."""
    _check_jpos(jpos, "jpos")
    dev = _device_of(jpos, "jpos")
    jpos = _f32(jpos, dev)
    B, T = jpos.shape[:2]
    floor = _floor_tensor(floor_height, B, dev, "floor_height")
    root = torch.empty(B, T, 3, device=dev)
    with torch.cuda.device(dev):
        _lib.check_eval(_lib.load().egoego_eval_root_to_floor(jpos.data_ptr(), floor.data_ptr(), B, T, root.data_ptr(), _stream(dev)))
    return root


def determine_floor_height_and_contacts(body_joint_seq, fps, lengths=None, return_details=False):
    """body_joint_seq [B, T, 22, 3] on the device (z up) -> (offset_floor_height [B] fp32, contacts [B, T, 22] fp32 0 / 1,
    discard_seq [B] bool).  `return_details=True` appends a dict: floor_height [B] (the smallest group median; the first return
    is that minus 0.01), labels [B, 2 T] int32 (the DBSCAN label of each static toe sample in the reference's order: left-toe
    frames, then right-toe frames; -1 noise, -2 past n_static), n_static [B], n_groups [B] (clusters, plus the noise group if
    there is one).

    A single [T, 22, 3] tensor returns what the reference returns: (float, float64 ndarray [T, 22], bool) — that form waits for
    the device and copies the results to the host.  A sequence needs at least 2 frames and at most MAX_FRAMES."""
    body_joint_seq = torch.as_tensor(body_joint_seq)
    single = body_joint_seq.dim() == 3
    x = body_joint_seq[None] if single else body_joint_seq
    _check_jpos(x, "body_joint_seq")
    B, T = x.shape[:2]
    if T > MAX_FRAMES:
        raise ValueError(f"T = {T} frames: the floor-height kernel takes at most {MAX_FRAMES} frames per sequence")
    dev = _device_of(x, "body_joint_seq")
    x = _f32(x, dev)
    len_t, len_p = _lengths(lengths, B, T, dev, 2)
    floor = torch.empty(B, device=dev)
    offset = torch.empty(B, device=dev)
    contacts = torch.empty(B, T, N_JOINTS, device=dev)
    discard = torch.empty(B, dtype=torch.int32, device=dev)
    n_static = torch.empty(B, dtype=torch.int32, device=dev)
    n_groups = torch.empty(B, dtype=torch.int32, device=dev)
    labels = torch.empty(B, 2 * T, dtype=torch.int32, device=dev) if return_details else None
    with torch.cuda.device(dev):
        _lib.check_eval(_lib.load().egoego_eval_floor_contacts(
            x.data_ptr(), len_p, B, T, float(fps), floor.data_ptr(), offset.data_ptr(), contacts.data_ptr(), discard.data_ptr(),
            labels.data_ptr() if labels is not None else None, n_static.data_ptr(), n_groups.data_ptr(), _stream(dev)))
    del len_t
    details = {"floor_height": floor, "labels": labels, "n_static": n_static, "n_groups": n_groups}
    if single:
        out = (float(offset[0]), contacts[0].double().cpu().numpy(), bool(discard[0]))
        if return_details:
            details = {k: v[0] for k, v in details.items()}
    else:
        out = (offset, contacts, discard.bool())
    return out + (details,) if return_details else out


def _floor_tensor(v, B, dev, what):
    if isinstance(v, torch.Tensor):
        t = v.to(dev, torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(B)
        if t.shape != (B,):
            raise ValueError(f"{what} {tuple(v.shape)}: a scalar or [{B}] expected")
        return t.contiguous()
    return torch.full((B,), float(v), device=dev)


def _metrics_table(gt_global_quat, gt_global_jpos, gt_floor_height, pred_global_quat, pred_global_jpos, pred_floor_height, lengths):
    pq, pp, gq, gp = (torch.as_tensor(t) for t in (pred_global_quat, pred_global_jpos, gt_global_quat, gt_global_jpos))
    _check_jpos(pp, "pred_global_jpos")
    B, T = pp.shape[:2]
    if pq.shape != (B, T, N_JOINTS, 4):
        raise ValueError(f"pred_global_quat {tuple(pq.shape)}: {(B, T, N_JOINTS, 4)} expected")
    shared = gp.dim() == 3
    want = (T, N_JOINTS) if shared else (B, T, N_JOINTS)
    if gp.shape != want + (3,) or gq.shape != want + (4,):
        raise ValueError(f"ground truth {tuple(gq.shape)} / {tuple(gp.shape)}: {want + (4,)} / {want + (3,)} expected "
                         f"(shared by all samples) or with a leading [{B}]")
    dev = _device_of(pp, "pred_global_jpos")
    pq, pp, gq, gp = (_f32(t, dev) for t in (pq, pp, gq, gp))
    len_t, len_p = _lengths(lengths, B, T, dev, 1)
    gf, pf = _floor_tensor(gt_floor_height, B, dev, "gt_floor_height"), _floor_tensor(pred_floor_height, B, dev, "pred_floor_height")
    out = torch.empty(B, _lib.EVAL_N_METRICS, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check_eval(_lib.load().egoego_eval_metrics(gq.data_ptr(), gp.data_ptr(), int(shared), gf.data_ptr(), pq.data_ptr(),
                                                        pp.data_ptr(), pf.data_ptr(), len_p, B, T, out.data_ptr(), _stream(dev)))
    del len_t
    return out


def _metrics_dict(table):
    res = {k: table[:, i] for i, k in enumerate(METRIC_KEYS)}
    res["single_jpe"] = table[:, len(METRIC_KEYS):]
    for j in range(N_JOINTS):
        res["jpe_%d" % j] = table[:, len(METRIC_KEYS) + j]
    return res


def compute_metrics_for_smpl(gt_global_quat, gt_global_jpos, gt_floor_height, pred_global_quat, pred_global_jpos, pred_floor_height,
                             lengths=None):
    """pred_global_quat [B, T, 22, 4], pred_global_jpos [B, T, 22, 3]; the ground truth [T, 22, ...] (shared by every sample) or
    [B, T, 22, ...]; floor heights a number or [B] -> the reference's dictionary with one float64 [B] tensor per key
    (`single_jpe` [B, 22]), in the reference's units (mm where it multiplies by 1000).  The acceleration keys need 3 frames and
    are NaN below.  A sample's numbers are bit-identical alone, at any position of a batch and under any padded T."""
    return _metrics_dict(_metrics_table(gt_global_quat, gt_global_jpos, gt_floor_height, pred_global_quat, pred_global_jpos,
                                        pred_floor_height, lengths))


def evaluate_samples(ds, local_aa, root_trans, gt_global_quat, gt_global_jpos, gt_floor_height=0., lengths=None, group=None, fps=30,
                     parents=None):
    """eval_egoego.py:369-446 for B samples at once.  `ds` carries rest_human_offsets (and optionally parents), as SkeletonStats
    and the reference's AMASSDataset do; local_aa [B, T, 22, 3], root_trans [B, T, 3]; the ground truth as in
    compute_metrics_for_smpl (it is not modified: the xy shift works on a copy); `group` an int tensor [B] of ids 0..G-1 (None:
    one group).  Returns a dict:

      metrics              the dictionary of compute_metrics_for_smpl
      floor_height         [B]: determine_floor_height_and_contacts' first return, what the reference calls pred_floor_height
      contacts, discard    [B, T, 22], [B]
      global_quat, global_jpos   FK of the samples, the joints after the xy shift
      root_trans           [B, T, 3]: the shifted root with the floor height taken off z
      best                 int32 [G]: per group the index of the sample with the smallest mpjpe (-1 for an id no sample has)
    """
    local_aa = torch.as_tensor(local_aa)
    if local_aa.dim() != 4 or local_aa.shape[-2:] != (N_JOINTS, 3):
        raise ValueError(f"local_aa {tuple(local_aa.shape)}: [B, T, {N_JOINTS}, 3] expected")
    B, T = local_aa.shape[:2]
    if T > MAX_FRAMES:
        raise ValueError(f"T = {T} frames: the floor-height kernel takes at most {MAX_FRAMES} frames per sequence")
    dev = _device_of(local_aa, "local_aa")
    len_t, _ = _lengths(lengths, B, T, dev, 2)
    quat, jpos = fk_smpl(root_trans, local_aa, ds.rest_human_offsets, _parents_of(ds, parents))
    shift_xy_(jpos)
    gp = _f32(gt_global_jpos, dev).clone()
    shift_xy_(gp[None] if gp.dim() == 3 else gp)
    floor, contacts, discard = determine_floor_height_and_contacts(jpos, fps, len_t)
    table = _metrics_table(gt_global_quat, gp, gt_floor_height, quat, jpos, floor, len_t)
    if group is None:
        grp, n_groups = None, 1
    else:
        grp = torch.as_tensor(group).to(dev, torch.int32).contiguous()
        if grp.shape != (B,):
            raise ValueError(f"group {tuple(grp.shape)}: [{B}] expected")
        n_groups = int(grp.max()) + 1
        if int(grp.min()) < 0:
            raise ValueError("group ids must be >= 0")
    root = root_to_floor(jpos, floor)
    best = torch.empty(n_groups, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check_eval(_lib.load().egoego_eval_best(table.data_ptr(), MPJPE_COLUMN, grp.data_ptr() if grp is not None else None, B, n_groups,
                                             best.data_ptr(), _stream(dev)))
    return {"metrics": _metrics_dict(table), "floor_height": floor, "contacts": contacts, "discard": discard, "global_quat": quat,
            "global_jpos": jpos, "root_trans": root, "best": best}


def evaluate_pipeline(headnet, gravitynet, model, ds, batch, gt_root_trans, gt_local_aa, lengths, samples_per_sequence=1, fps=30,
                      sequence_offset=0, **sampler_kw):
    """eval_egoego.py:241-483 for a whole evaluation set of S sequences of different lengths in one call: ragged stage 1, its
    score, the move onto the floor, ragged stage 2 and the full-body metrics.

    batch: the stage-1 inputs, padded (of [S, Tmax, 512]; head_pose, aligned_slam_trans, ori_slam_trans, ori_slam_rot_mat
    [S, Tmax + 1, ...]); lengths [S] (host integers or a CPU tensor): the feature frames T_s of each sequence — every pose-like
    entry and the ground truth gt_root_trans [S, Tmax + 1, 3] / gt_local_aa [S, Tmax + 1, 22, 3] (SMPL root translation and local
    axis-angle; the reference's qpos conversion is the caller's) hold T_s + 1 frames.  sampler_kw goes to
    full_body_gen_cond_head_pose_sliding_window_ragged (sampler, n_steps, eta, noise, parents).

      lines 275-294   GravityNet's translation with HeadNet's rotation, the xy of the first frame taken off
      lines 296-312   the stage-1 metrics against batch['head_pose'] with the same xy shift
      lines 327-335   FK of the ground truth, its floor height off z, the head trajectory moved onto its first head joint
      lines 358-446   stage 2 and evaluate_samples(..., lengths=, group=): sample j of sequence s is row s * n + j, group s

    -> evaluate_samples' dictionary plus stage1_metrics [S, 3] float64 (head_dist, head_dist_rot_only, head_trans_err in mm),
    head_pose [S, Tmax + 1, 7] float64 (what stage 2 was conditioned on, zero past each end) and lengths [S] (CPU, T_s + 1).
    A sequence's numbers are the same bits alone (with sequence_offset moved on by its index) and in any batch."""
    from . import harness, stage1
    hp, _, _, n = stage1.stage1_ragged(headnet, gravitynet, batch, lengths)
    dev = _device_of(hp, "the stage-1 head pose")
    S, N = hp.shape[:2]
    n_dev = torch.as_tensor(n, dtype=torch.int64).to(dev)
    hp[:, :, :2] -= hp[:, 0:1, :2].clone()
    gt_pose = torch.as_tensor(batch["head_pose"]).to(dev).double()[:, :N].clone()
    gt_pose[:, :, :2] -= gt_pose[:, 0:1, :2].clone()
    s1 = stage1.head_pose_metrics(hp, gt_pose, n_dev)
    root_gt, aa_gt = torch.as_tensor(gt_root_trans).to(dev)[:, :N], torch.as_tensor(gt_local_aa).to(dev)[:, :N]
    parents = sampler_kw.get("parents")
    gq, gp = fk_smpl(root_gt, aa_gt, ds.rest_human_offsets, _parents_of(ds, parents))
    floor, _, _ = determine_floor_height_and_contacts(gp, fps, n)
    gp[:, :, :, 2] -= floor[:, None, None]
    hp[:, :, :3] += gp[:, 0:1, HEAD_IDX, :].double() - hp[:, 0:1, :3]
    hp = stage1._keep_rows(hp, n_dev)
    n_smp = int(samples_per_sequence)
    aa, root, out_len = harness.full_body_gen_cond_head_pose_sliding_window_ragged(
        model, ds, hp, samples_per_sequence=n_smp, sequence_offset=sequence_offset, lengths=n, **sampler_kw)
    Tp = aa.shape[1]
    rep = lambda t: t[:, :Tp].repeat_interleave(n_smp, 0) if n_smp > 1 else t[:, :Tp]  # noqa: E731
    group = torch.arange(S, device=dev).repeat_interleave(n_smp)
    res = evaluate_samples(ds, aa, root, rep(gq), rep(gp), 0., lengths=out_len, group=group, fps=fps, parents=parents)
    res.update(stage1_metrics=s1, head_pose=hp, lengths=torch.as_tensor(n, dtype=torch.int64))
    return res
