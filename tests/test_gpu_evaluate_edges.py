"""The evaluation kernels on the GPU (csrc/eval_metrics.h) at rotation and length edges, against the fp64 oracle
(tests/eval_oracle.py); the cases are tests/rotation_edge_cases.py's fk_chains() and metric_inputs().

  fk_smpl     local rotations at zero, on both sides of qd_from_aa's series switch, at pi, 2 pi and beyond, and chains whose
              composed rotation passes pi and 2 pi, so that qd_std flips (600 of the products have w < 0 before it): w >= 0,
              every quaternion component within 2^-24 of the oracle's (rounded once from fp64; the builder keeps every |w| >= 1e-9,
              so the sign is no coin toss), joints and rotation matrices under test_fk_against_the_oracle's bounds.
  metrics     lengths 1, 2, 3, 4, 63 .. 65, 255 .. 257 and 513 (a wave's 64 lanes, the 256-thread stride); quaternions scaled by
              0.25 and 4, negated, exactly zero, and with norm^2 = 1e-16 and 1e-15 on either side of quaternion_matrix's identity
              branch; feet 1 m under the floor and within 0.01 m of their contact heights; one sample equal to its ground truth.
              Bound per key: test_gpu_evaluate.BOUND, unchanged.  Where the oracle's value is rounding residue (below 1e-12: the
              identical sample's distances) |HIP| <= 1e-12 is asked; where it is NaN (accel_* below 3 frames) NaN is asked.
  best        egoego_eval_best on a planted table: ties, NaN first and later in a group, an id nobody has, no groups.

Below 3 frames the kernel divided the acceleration sums by L - 2: 0 / 0 = NaN at L = 2, as the reference's mean of nothing, but
0 / -1 = -0.0 at L = 1.  This file showed it; the kernel now divides by 0 for every L < 3.

Measured on an MI355X (profiles/rotation_edges_error.json; EGOEGO_EDGES_RECORD=<file> writes it): FK quaternion components
2.980e-08 (bar 5.960e-08), joints 4.237e-08 of max |fp64|, rotation matrices 8.065e-08; metrics: no key above 3.8e-16
(root_trans_dist; BOUND 9.1e-16) but single_jpe 1.297e-15 (BOUND 1.3e-14), the identical sample's residue 5.4e-16 (bar 1e-12).
No key needed another bound: the scaled and tiny quaternions cost nothing, both sides normalise in fp64.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_oracle as O
import rotation_edge_cases as RC
from test_gpu_evaluate import BOUND

pytestmark = pytest.mark.gpu
F32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ev():
    from egoego_release_amd import evaluate
    return evaluate


def test_fk_at_the_chains(ev):
    fc = RC.fk_chains()
    q, p = ev.fk_smpl(torch.from_numpy(fc["root_trans"]).cuda(), torch.from_numpy(fc["local_aa"]).cuda(),
                      torch.from_numpy(fc["rest_offsets"]).cuda(), fc["parents"])
    q, p = q.cpu().numpy(), p.cpu().numpy()
    oq, op = fc["oracle_quat"], fc["oracle_jpos"]
    assert (q[..., 0] >= 0).all()
    e_q = np.abs(q - oq).max()
    e_pos = np.abs(p - op).max() / np.abs(op).max()
    e_rot = np.abs(O.quat_to_matrix(q) - O.quat_to_matrix(oq)).max()
    print("GPU FK at the chains vs fp64: quaternion components %.3e, joints %.3e of max |fp64|, rotation matrices %.3e" % (e_q, e_pos, e_rot))
    RC.record("fk_chains", quat_component=e_q, quat_bar=F32, joints=e_pos, joints_bar=F32 * (1 + 1e-6), rot=e_rot, rot_bar=8 * F32,
              flips=fc["flips"], min_w=fc["min_w"])
    assert e_q <= F32
    assert e_pos <= F32 * (1 + 1e-6) and e_rot <= 8 * F32  # test_fk_against_the_oracle's


def _table(ev, m, rows=slice(None), T=None):
    T = RC.METRIC_T if T is None else T
    d = lambda k: torch.from_numpy(np.ascontiguousarray(m[k][rows][:, :T] if m[k].ndim > 1 else m[k][rows])).cuda()  # noqa: E731
    res = ev.compute_metrics_for_smpl(d("gt_quat"), d("gt_jpos"), d("gt_floor"), d("pred_quat"), d("pred_jpos"), d("pred_floor"),
                                      torch.from_numpy(np.ascontiguousarray(m["lengths"][rows])))
    return torch.cat([torch.stack([res[k] for k in O.METRIC_KEYS], 1), res["single_jpe"]], 1)


def test_metrics_at_the_length_and_quaternion_edges(ev):
    m = RC.metric_inputs()
    want = RC.metric_oracle()
    got = _table(ev, m).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    worst, failures = {}, []
    for b, L in enumerate(m["lengths"]):
        figs = RC.metric_figures(got[b], want[b], BOUND)
        print("L = %3d%s:" % (L, " (identical)" if b == m["identical"] else ""), {k: "%.2e" % f for k, (f, _) in figs.items()})
        for k, (f, bar) in figs.items():
            if bar != RC.RESIDUE:
                worst[k] = max(worst.get(k, 0.0), f)
            if not f <= bar:
                failures.append((int(L), k, f, bar))
        assert got[b, len(O.METRIC_KEYS)] == 0.0  # jpe_0: root-relative
    print("GPU vs fp64 oracle at the edges, worst relative error per key:", {k: "%.3e" % v for k, v in worst.items()})
    RC.record("metrics", worst_relative=worst, bound={k: BOUND[k] for k in worst},
              residue_worst=float(np.abs(got[m["identical"]][np.abs(want[m["identical"]]) < RC.RESIDUE]).max()), residue_bar=RC.RESIDUE)
    acc = [O.METRIC_KEYS.index(k) for k in ("accel_pred", "accel_gt", "accel_err")]
    assert np.isnan(got[:2][:, acc]).all(), got[:2][:, acc]  # 1 and 2 frames: the mean over no frame
    assert np.isnan(got).sum() == 6
    assert got[0, O.METRIC_KEYS.index("pred_fs")] == 0.0 and got[0, O.METRIC_KEYS.index("gt_fs")] == 0.0
    assert not failures, failures


def test_a_sample_of_each_length_is_bit_identical_alone_permuted_and_unpadded(ev):
    m = RC.metric_inputs()
    base = _table(ev, m)
    perm = np.random.default_rng(5).permutation(len(m["lengths"]))
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))  # noqa: E731  (NaN included)
    assert same(_table(ev, m, perm), base[torch.from_numpy(perm).cuda()])
    for b, L in enumerate(m["lengths"]):
        assert same(_table(ev, m, slice(b, b + 1))[0], base[b]), L
        assert same(_table(ev, m, slice(b, b + 1), T=int(L))[0], base[b]), L  # T padded to its own length: no padding at all


def _best(values, group, n_groups):
    from egoego_release_amd import _lib, evaluate
    B = len(values)
    table = torch.full((B, _lib.EVAL_N_METRICS), 1e9, dtype=torch.float64)
    table[:, evaluate.MPJPE_COLUMN] = torch.tensor(values, dtype=torch.float64)
    table = table.cuda()
    grp = torch.tensor(group, dtype=torch.int32).cuda() if group is not None else None
    best = torch.full((n_groups,), -7, dtype=torch.int32, device="cuda")
    _lib.check_eval(_lib.load().egoego_eval_best(table.data_ptr(), evaluate.MPJPE_COLUMN, grp.data_ptr() if grp is not None else None, B,
                                                 n_groups, best.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    want = O.best_per_group(values, group if group is not None else [0] * B)  # the loop of eval_oracle.evaluate_samples
    return best.cpu().tolist(), [want.get(g, -1) for g in range(n_groups)]


def test_best_of_group_ties_nan_and_missing_ids():
    nan = float("nan")
    #         group 0: a tie      1: NaN first   2: NaN later   4: a tie of two; nobody has id 3
    values = [5.0, 3.0, 3.0,      nan, 1.0,      2.0, nan,      7.0, 7.0]
    group = [0, 0, 0,             1, 1,          2, 2,          4, 4]
    got, want = _best(values, group, 5)
    assert want == [1, 3, 5, -1, 7] and got == want
    order = [8, 3, 0, 6, 1, 4, 7, 2, 5]  # the same samples interleaved; group 2's NaN now comes first and stays
    got, want = _best([values[i] for i in order], [group[i] for i in order], 5)
    assert want == [4, 1, 3, -1, 0] and got == want
    for vals, first in (([5.0, 3.0, nan, 3.0, 9.0], 1), ([nan, 1.0, 0.5], 0), ([4.0], 0)):  # group=None: one group
        got, want = _best(vals, None, 1)
        assert want == [first] and got == want
