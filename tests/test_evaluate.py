"""The batched evaluation, the parts that need no GPU: the fp64 oracle against the recorded results of the reference's own
functions (tests/golden/make_eval_golden.py), its sorted 1-D DBSCAN against sklearn, the library's symbols, and the argument
checks of egoego_release_amd.evaluate."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eval_cases
import eval_oracle as O
from egoego_release_amd import _lib, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_DISTANCE = O.REFERENCE_DISTANCE


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "eval_golden.npz"))


def test_oracle_matches_the_reference_floor_and_contacts(gold):
    fps = int(gold["fps"])
    seen = set()
    for name in gold["names"]:
        o = O.floor_and_contacts(gold[name + "/jpos"], fps)
        assert np.array_equal(o["labels"], gold[name + "/labels"]), name
        assert np.array_equal(o["contacts"], gold[name + "/contacts"]), name
        assert o["discard_seq"] == bool(gold[name + "/discard"]), name
        assert abs(float(o["offset_floor_height"]) - float(gold[name + "/offset_floor_height"])) <= 1e-7, name
        assert o["n_groups"] == np.unique(gold[name + "/labels"]).size
        seen.add((o["labels"].size == 0, bool(o["discard_seq"]), bool((o["labels"] == -1).any())))
    assert len(seen) >= 4  # no static sample, discard on and off, with and without noise


def test_oracle_matches_the_reference_metrics(gold):
    worst = {}
    for name in ("walk_31", "walk_139", "walk_300"):
        L = gold[name + "/jpos"].shape[0]
        m = O.metrics(gold["gt_quat"][:L], gold["gt_jpos"][:L], 0., gold[name + "/quat"], gold[name + "/jpos"],
                      float(gold[name + "/offset_floor_height"]))
        for k in O.METRIC_KEYS:
            ref = float(gold[name + "/metric/" + k])
            worst[k] = max(worst.get(k, 0.), abs(ref - m[k]) / abs(m[k]))
        ref = gold[name + "/metric/single_jpe"]
        assert ref[0] == 0 and m["single_jpe"][0] == 0
        worst["single_jpe"] = max(worst.get("single_jpe", 0.), np.max(np.abs(ref[1:] - m["single_jpe"][1:]) / m["single_jpe"][1:]))
    for k, v in worst.items():
        # the recorded distances, re-measured here (libm and BLAS builds may move the last digits)
        assert v <= 2 * REFERENCE_DISTANCE[k] + 1e-15, (k, v)


def test_oracle_dbscan_equals_sklearn():
    cluster = pytest.importorskip("sklearn.cluster")
    g = np.random.default_rng(17)
    kinds = set()
    for _ in range(400):
        n = int(g.integers(1, 60))
        h = (g.choice([0.0, 0.02, 0.1], n) + g.standard_normal(n) * g.uniform(0.001, 0.01)).astype(np.float32)
        want = cluster.DBSCAN(eps=0.005, min_samples=3).fit(h.reshape(-1, 1)).labels_
        got = O.dbscan_1d(h)
        assert np.array_equal(got, want), (h, got, want)
        assert np.array_equal(synthetic._eval_dbscan(h.astype(np.float64)), want)
        kinds.add((bool((want == -1).any()), int(want.max()) >= 1))
    assert len(kinds) >= 3  # with and without noise, one cluster and several


def test_hand_built_cases_show_what_they_claim():
    names, jpos, expect = eval_cases.batch()
    for name, j, e in zip(names, jpos, expect):
        o = O.floor_and_contacts(j, eval_cases.FPS)
        if "n_static" in e:
            assert o["labels"].size == e["n_static"], name
        if "n_groups" in e:
            assert o["n_groups"] == e["n_groups"], name
        if "labels" in e:
            assert o["labels"].tolist() == e["labels"], name
        if "discard" in e:
            assert o["discard_seq"] == e["discard"], name
        if "floor" in e:
            assert float(o["floor_height"]) == np.float32(e["floor"]), name
    o = O.floor_and_contacts(jpos[names.index("noise_lowest")], eval_cases.FPS)
    on = {j: int(o["contacts"][:, j].sum()) for j in synthetic.EVAL_CONTACT_JOINTS}
    assert on[20] == 2 and on[21] == 0 and on[4] == 1 and on[8] == 1 and on[11] == 1 and on[10] == 0
    both = jpos[names.index("both_toes")]
    o = O.floor_and_contacts(both, eval_cases.FPS)
    assert np.unique(o["static_inds"]).size < o["static_inds"].size  # a frame static for both toes


def test_make_eval_motion_is_seeded_and_margin_checked():
    a = synthetic.make_eval_motion(3, 40, 2)
    b = synthetic.make_eval_motion(3, 40, 2)
    assert all(np.array_equal(a[k], b[k]) for k in ("local_aa", "root_trans", "gt_local_aa", "gt_root_trans"))
    assert a["local_aa"].shape == (3, 40, 22, 3) and a["root_trans"].shape == (3, 40, 3) and a["local_aa"].dtype == np.float32
    j = eval_cases.build([(eval_cases.L_TOE, 5, [0.0, 0.005 * (1 + 1e-6)])])  # a velocity one part in a million off the threshold
    with pytest.raises(AssertionError):
        synthetic.assert_eval_margins(j)


def test_oracle_fk_agrees_with_the_harness_fk():
    from egoego_release_amd import harness
    m = synthetic.make_eval_motion(1, 12, 2)
    ds = harness.SkeletonStats(np.zeros(66), np.ones(66), m["rest_offsets"], m["parents"])
    q, p = ds.fk_smpl(torch.from_numpy(m["root_trans"][0]), torch.from_numpy(m["local_aa"][0]))
    oq, op = O.fk(m["root_trans"][0], m["local_aa"][0], m["rest_offsets"], m["parents"])
    assert np.abs(p.numpy() - op).max() < 5e-6
    assert np.abs(O.quat_to_matrix(q.numpy()) - O.quat_to_matrix(oq)).max() < 5e-6
    assert np.abs(op - synthetic.eval_fk(m["root_trans"][0], m["local_aa"][0], m["rest_offsets"])).max() < 1e-12


def test_library_exports_the_eval_entries():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = [n for n in _lib.EXPORTS if n.startswith("egoego_eval_")]
    assert len(names) == 8
    for n in names:
        assert hasattr(lib, n), n
    header = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    for n in names:
        assert n + "(" in header, n
    assert "#define EGOEGO_ABI_VERSION 8" in header and _lib.ABI_VERSION == 8
    lib.egoego_eval_max_frames.restype = ctypes.c_int
    from egoego_release_amd import evaluate
    assert lib.egoego_eval_max_frames() == evaluate.MAX_FRAMES == 4096


def test_evaluate_rejects_wrong_shapes_and_long_sequences():
    from egoego_release_amd import evaluate
    with pytest.raises(ValueError, match="22, 3"):
        evaluate.determine_floor_height_and_contacts(torch.zeros(2, 10, 21, 3), 30)
    with pytest.raises(ValueError, match="4096"):
        evaluate.determine_floor_height_and_contacts(torch.zeros(1, 4097, 22, 3), 30)
    with pytest.raises(ValueError, match="4096"):
        evaluate.evaluate_samples(None, torch.zeros(1, 5000, 22, 3), torch.zeros(1, 5000, 3), None, None)
    with pytest.raises(ValueError, match="pred_global_quat"):
        evaluate.compute_metrics_for_smpl(torch.zeros(10, 22, 4), torch.zeros(10, 22, 3), 0., torch.zeros(2, 10, 22, 3),
                                          torch.zeros(2, 10, 22, 3), 0.)
    with pytest.raises(ValueError, match="ground truth"):
        evaluate.compute_metrics_for_smpl(torch.zeros(9, 22, 4), torch.zeros(9, 22, 3), 0., torch.zeros(2, 10, 22, 4),
                                          torch.zeros(2, 10, 22, 3), 0.)
    with pytest.raises(ValueError, match="root_trans"):
        evaluate.fk_smpl(torch.zeros(4, 2), torch.zeros(4, 22, 3), torch.zeros(22, 3))
    # no CPU path: well-formed inputs on the CPU raise instead of falling back
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        evaluate.determine_floor_height_and_contacts(torch.zeros(1, 10, 22, 3), 30)
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        evaluate.fk_smpl(torch.zeros(4, 3), torch.zeros(4, 22, 3), torch.zeros(22, 3))
