"""Ragged stage 1 off the GPU: the planar closed form against the oracle's SVD Umeyama, the restated stage-1 score against the
reference's golden, the two new entry points' declarations, and the `lengths=` keyword as far as the missing device."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import stage1_ragged_cases as K
from egoego_release_amd import _lib, evaluate, stage1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egoego_s1_gravity_align", "egoego_s1_head_pose_metrics")


def test_case_table_has_both_determinant_signs_and_edges():
    cases = K.trajectory_cases()
    dets = [np.linalg.det(K.planar_covariance(e, r)) for _, e, r, _ in cases["compared"]]
    assert sum(d > 0 for d in dets) >= 3 and sum(d < 0 for d in dets) >= 3
    for (_, e, r, reflected), d in zip(cases["compared"], dets):
        assert (d < 0) == reflected
    assert any(len(e) > 1024 for _, e, _, _ in cases["compared"])  # more than two LDS chunks of the kernel
    assert cases["lines"] and cases["single"]


@pytest.mark.parametrize("i", range(len(K.trajectory_cases()["compared"])))
def test_planar_closed_form_is_the_oracles_umeyama(i):
    name, est, ref, reflected = K.trajectory_cases()["compared"][i]
    assert K.sigma_ratio(est, ref) >= 1e-2, name  # the precondition: A is well away from rank 1
    got, want = K.planar_umeyama(est, ref), K.oracle_umeyama(est, ref)
    assert np.abs(got - want).max() < 1e-12, (name, np.abs(got - want).max())
    assert got[2, 2] == (-1.0 if reflected else 1.0)
    assert abs(np.linalg.det(got) - 1) < 1e-12


def test_planar_closed_form_on_degenerate_input():
    cases = K.trajectory_cases()
    for name, est, ref, _ in cases["lines"]:
        r = K.planar_umeyama(est, ref)
        assert np.isfinite(r).all() and np.abs(r.dot(r.T) - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(r) - 1) < 1e-12, name
    for name, est, ref, _ in cases["single"]:
        assert np.array_equal(K.planar_umeyama(est, ref), np.eye(3)), name


def test_restated_head_pose_metrics_match_the_reference_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "head_metrics_golden.npz"))
    pred, gt = K.metric_poses(int(g["seed"]), len(g["lengths"]), int(g["lengths"].max()))
    for b, n in enumerate(g["lengths"]):
        assert np.array_equal(pred[b, :n], g["pred"][b, :n]) and np.array_equal(gt[b, :n], g["gt"][b, :n])  # the seeded inputs
        got = K.head_pose_metrics_np(pred[b, :n, :3], K.quat_to_matrix(pred[b, :n, 3:]), gt[b, :n, :3], K.quat_to_matrix(gt[b, :n, 3:]))
        for j in range(3):
            assert abs(got[j] - g["metrics"][b, j]) <= 1e-10 * abs(g["metrics"][b, j]), (n, j, got[j], g["metrics"][b, j])
    assert 1 in g["lengths"].tolist()


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    source = open(os.path.join(ROOT, "egoego_release_amd", "csrc", "stage1.hip")).read()
    lib_py = open(os.path.join(ROOT, "egoego_release_amd", "_lib.py")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"\bint %s\(" % name, source), name
        assert name in _lib.EXPORTS
        assert "lib.%s.argtypes" % name in lib_py
    assert "#define EGOEGO_ABI_VERSION 8 " in header  # additive: the version stays
    assert not any(n.startswith("egoego_eval_") for n in NEW)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.egoego_abi_version() == 8
        assert len(lib.egoego_s1_gravity_align.argtypes) == 13 and len(lib.egoego_s1_head_pose_metrics.argtypes) == 7


def _opt():
    return Namespace(window=31, n_dec_layers=1, n_head=4, d_k=256, d_v=256, d_model=256, dist_scale=10.0, input_of_feats=True,
                     normal_window=31, normal_n_dec_layers=1, normal_n_head=4, normal_d_k=256, normal_d_v=256, normal_d_model=256)


def test_lengths_keyword_reaches_the_missing_device():
    """On a CPU device the ragged calls check their lengths first (ValueError) and then meet the usual error: no CPU path."""
    hn = stage1.HeadFormer(_opt(), "cpu")
    gn = stage1.HeadNormalFormer(_opt(), "cpu", eval_whole_pipeline=True)
    T, L = [5, 40], [6, 41]
    batch = K.padded_batch(K.stage1_sequences(1, T, L))
    with pytest.raises(ValueError, match="lengths"):
        hn.forward_for_eval(batch, lengths=[5, 41])
    with pytest.raises(ValueError, match="lengths"):
        hn.forward_for_eval(batch, lengths=[5])
    with pytest.raises(ValueError, match="pose_lengths"):
        hn.forward_for_eval(batch, lengths=T, pose_lengths=[6, 42])
    with pytest.raises(_lib.EgoEgoHipError):
        hn.forward_for_eval(batch, lengths=T)
    with pytest.raises(_lib.EgoEgoHipError):
        hn.forward_for_eval(batch, lengths=torch.tensor(T), pose_lengths=L)
    nin = {"head_trans": batch["ori_slam_trans"], "head_rot_mat": batch["ori_slam_rot_mat"], "ori_head_pose": batch["head_pose"]}
    with pytest.raises(ValueError, match="ref_lengths"):
        gn.forward_for_eval(nin, torch.ones(2), lengths=L, ref_lengths=[6, 99])
    with pytest.raises(NotImplementedError, match="use_gt_aligned_rot"):
        gn.forward_for_eval(nin, torch.ones(2), use_gt_aligned_rot=True, lengths=L)
    with pytest.raises(_lib.EgoEgoHipError):
        gn.forward_for_eval(nin, torch.ones(2), lengths=L, ref_lengths=L)
    with pytest.raises(_lib.EgoEgoHipError):
        stage1.estimate_head_pose(hn, gn, batch, lengths=T)
    with pytest.raises(ValueError, match="needs lengths"):
        hn.forward_for_eval(batch, pose_lengths=L)


def test_head_pose_metrics_have_no_cpu_path():
    pred, gt = K.metric_poses(3, 2, 5)
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        stage1.compute_head_pose_metrics(t(pred[..., :3]), t(K.quat_to_matrix(pred[..., 3:])), t(gt[..., :3]), t(K.quat_to_matrix(gt[..., 3:])))
    with pytest.raises(ValueError):
        stage1.compute_head_pose_metrics(t(pred[..., :3]), t(pred[..., 3:]), t(gt[..., :3]), t(gt[..., 3:]))
    assert callable(evaluate.evaluate_pipeline)
