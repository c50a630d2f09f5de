"""The batched evaluation on the GPU (egoego_release_amd.evaluate over csrc/eval_metrics.h) against the fp64 oracle
(tests/eval_oracle.py) and the recorded results of the reference's own functions (tests/golden/eval_golden.npz).

Discrete outputs (DBSCAN labels, contacts, discard flag, group count) and floor_height (as float32 bits) are compared exactly;
offset_floor_height within 1e-7 m.  That is fair because every input passed assert_eval_margins: nothing thresholded lies within
a relative 1e-4 of its threshold (synthetic.make_eval_motion, tests/eval_cases.py).

One case the issue lists cannot be built: a border point within eps of two clusters.  With min_samples = 3 a point within eps of
a core on either side has three points in its own neighbourhood, is core itself and joins the two clusters.  `border` in
eval_cases.py is the nearest thing: a lone sample 0.0045 from one cluster and 0.0055 from the other.

Continuous outputs are compared as relative errors per key.  Measured, worst over the sequences of this file (the walks of
3-300 frames against a shared ground truth, and one 4096-frame pair):

  key               reference's own results vs the fp64 oracle (CPU, golden inputs)   GPU vs the fp64 oracle (MI355X)
  root_dist         1.205e-15                                                         2.582e-15
  root_rot_dist     1.276e-15                                                         2.799e-15
  root_trans_dist   8.451e-08                                                         2.287e-16
  head_dist         2.026e-15                                                         1.335e-15
  head_rot_dist     2.411e-15                                                         1.560e-15
  head_trans_dist   7.644e-08                                                         2.142e-16
  mpjpe             7.099e-08                                                         2.608e-16
  mpjpe_wo_hand     2.549e-07                                                         2.334e-16
  accel_pred        6.481e-08                                                         2.317e-16
  accel_gt          1.586e-08                                                         2.005e-16
  accel_err         8.769e-07                                                         2.766e-16
  pred_fs           1.433e-07                                                         3.713e-16
  gt_fs             3.309e-08                                                         1.356e-16
  single_jpe        1.679e-06                                                         3.251e-15

(The reference computes the four pose distances in fp64, through numpy's 4 x 4 inverse, and the rest in float32.)  The bound per
key is 4 x the GPU figure, and never more than 4 x the reference's own distance; for root_dist and root_rot_dist the second is the
smaller.  FK is rounded once from fp64, so its bound comes from the format: half a float32 ulp of the largest joint coordinate, and
eight ulps of one for a rotation-matrix entry of the rounded quaternion; measured 4.753e-08 and 4.049e-08.
"""
import os

import numpy as np
import pytest
import torch

import eval_cases
import eval_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (3, 31, 64, 139, 300)
T_PAD = 300
SEED = 3
# worst relative error of the GPU results against the fp64 oracle, measured on an MI355X over the sequences of this file
GPU_MEASURED = {
    "root_dist": 2.582e-15, "root_rot_dist": 2.799e-15, "root_trans_dist": 2.287e-16, "head_dist": 1.335e-15, "head_rot_dist": 1.560e-15,
    "head_trans_dist": 2.142e-16, "mpjpe": 2.608e-16, "mpjpe_wo_hand": 2.334e-16, "accel_pred": 2.317e-16, "accel_gt": 2.005e-16,
    "accel_err": 2.766e-16, "pred_fs": 3.713e-16, "gt_fs": 1.356e-16, "single_jpe": 3.251e-15}
BOUND = {k: min(4 * GPU_MEASURED[k], 4 * O.REFERENCE_DISTANCE[k]) for k in GPU_MEASURED}


@pytest.fixture(scope="module")
def ev():
    from egoego_release_amd import evaluate
    return evaluate


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "eval_golden.npz"))


def _pad(seqs, T, width):
    out = np.full((len(seqs), T) + width, 7.5, np.float32)  # padding no result may depend on
    for b, s in enumerate(seqs):
        out[b, :s.shape[0]] = s
    return out


@pytest.fixture(scope="module")
def walks(gold):
    """The golden walks padded to T_PAD, their oracle results, on the device."""
    names = ["walk_%d" % L for L in LENGTHS]
    jpos = [gold[n + "/jpos"] for n in names]
    quat = []
    g = np.random.default_rng(5)
    for n, j in zip(names, jpos):  # the golden file keeps the rotations of three walks; the others get seeded unit quaternions
        q = gold[n + "/quat"] if n + "/quat" in gold.files else g.standard_normal((j.shape[0], 22, 4)).astype(np.float32)
        quat.append(q / np.linalg.norm(q, axis=-1, keepdims=True).astype(np.float32))
    fc = [O.floor_and_contacts(j, int(gold["fps"])) for j in jpos]
    met = [O.metrics(gold["gt_quat"][:L], gold["gt_jpos"][:L], 0., q, j, float(f["offset_floor_height"]))
           for L, q, j, f in zip(LENGTHS, quat, jpos, fc)]
    dev = torch.device("cuda")
    return {"names": names, "jpos_np": jpos, "quat_np": quat, "fc": fc, "met": met,
            "jpos": torch.from_numpy(_pad(jpos, T_PAD, (22, 3))).to(dev), "quat": torch.from_numpy(_pad(quat, T_PAD, (22, 4))).to(dev),
            "gt_jpos": torch.from_numpy(gold["gt_jpos"]).to(dev), "gt_quat": torch.from_numpy(gold["gt_quat"]).to(dev),
            "lengths": torch.tensor(LENGTHS, dtype=torch.int32, device=dev)}


def _check_floor(ev, jpos_dev, lengths, seqs, oracles, fps, gold=None, names=None):
    off, contacts, discard, d = ev.determine_floor_height_and_contacts(jpos_dev, fps, lengths, return_details=True)
    torch.cuda.synchronize()
    off, contacts, discard = off.cpu().numpy(), contacts.cpu().numpy(), discard.cpu().numpy()
    floor, labels, n_static, n_groups = (d[k].cpu().numpy() for k in ("floor_height", "labels", "n_static", "n_groups"))
    for b, (j, o) in enumerate(zip(seqs, oracles)):
        L, n = j.shape[0], o["labels"].size
        tag = names[b] if names else b
        assert n_static[b] == n, tag
        assert np.array_equal(labels[b, :n], o["labels"]), tag
        assert (labels[b, n:] == -2).all(), tag
        assert n_groups[b] == o["n_groups"], tag
        assert floor[b].view(np.uint32) == np.float32(o["floor_height"]).view(np.uint32), (tag, floor[b], o["floor_height"])
        assert abs(float(off[b]) - float(o["offset_floor_height"])) <= 1e-7, tag
        assert np.array_equal(contacts[b, :L], o["contacts"]), tag
        assert not contacts[b, L:].any(), tag
        assert bool(discard[b]) == o["discard_seq"], tag
        if gold is not None:
            assert np.array_equal(labels[b, :n], gold[tag + "/labels"]), tag
            assert np.array_equal(contacts[b, :L], gold[tag + "/contacts"]), tag
            assert bool(discard[b]) == bool(gold[tag + "/discard"]), tag
            assert abs(float(off[b]) - float(gold[tag + "/offset_floor_height"])) <= 1e-7, tag
    return floor, off


def test_floor_and_contacts_of_the_walks_are_exact(ev, walks, gold):
    _check_floor(ev, walks["jpos"], walks["lengths"], walks["jpos_np"], walks["fc"], int(gold["fps"]), gold, walks["names"])
    assert sum(o["discard_seq"] for o in walks["fc"]) >= 1 and max(o["n_groups"] for o in walks["fc"]) >= 10


def test_floor_and_contacts_of_the_hand_built_cases_are_exact(ev, gold):
    names, jpos, expect = eval_cases.batch()
    oracles = [O.floor_and_contacts(j, eval_cases.FPS) for j in jpos]
    floor, _ = _check_floor(ev, torch.from_numpy(jpos).cuda(), None, list(jpos), oracles, eval_cases.FPS, gold, names)
    assert floor[names.index("no_static")] == 0 and floor[names.index("noise_lowest")] == 0
    assert [e.get("discard") for e in expect].count(True) == 2


def test_floor_and_contacts_at_the_length_limit(ev):
    j = eval_cases.long_case(ev.MAX_FRAMES)
    o = O.floor_and_contacts(j, eval_cases.FPS)
    assert o["labels"].size > 4096 and (o["labels"] == -1).any() and o["discard_seq"]  # more samples than frames
    _check_floor(ev, torch.from_numpy(j)[None].cuda(), None, [j], [o], eval_cases.FPS)
    with pytest.raises(ValueError, match="4096"):
        ev.determine_floor_height_and_contacts(torch.zeros(1, ev.MAX_FRAMES + 1, 22, 3, device="cuda"), 30)


def _relative(table_row, m):
    out = {}
    for i, k in enumerate(O.METRIC_KEYS):
        if m[k] == 0:  # (a foot that never comes below its height: no sliding to measure)
            assert float(table_row[i]) == 0, k
            out[k] = 0.0
        else:
            out[k] = abs(float(table_row[i]) - m[k]) / abs(m[k])
            assert np.isfinite(out[k]), k
    sj = table_row[len(O.METRIC_KEYS):]
    assert sj[0] == 0.0
    out["single_jpe"] = float(np.max(np.abs(sj[1:] - m["single_jpe"][1:]) / m["single_jpe"][1:]))
    return out


def test_metrics_against_the_oracle(ev, walks):
    pf = torch.tensor([float(f["offset_floor_height"]) for f in walks["fc"]], device="cuda")
    res = ev.compute_metrics_for_smpl(walks["gt_quat"], walks["gt_jpos"], 0., walks["quat"], walks["jpos"], pf, walks["lengths"])
    table = torch.cat([torch.stack([res[k] for k in O.METRIC_KEYS], 1), res["single_jpe"]], 1).cpu().numpy()
    assert table.dtype == np.float64 and all(torch.equal(res["jpe_%d" % j], res["single_jpe"][:, j]) for j in range(22))
    worst = {}
    for b, m in enumerate(walks["met"]):
        for k, v in _relative(table[b], m).items():
            worst[k] = max(worst.get(k, 0.), v)
    # the limit length, with a ground truth per sample
    jp, jg = eval_cases.long_case(4096, 1), eval_cases.long_case(4096, 2)
    g = np.random.default_rng(9)
    q = g.standard_normal((2, 4096, 22, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    t = ev.compute_metrics_for_smpl(torch.from_numpy(q[1:]).cuda(), torch.from_numpy(jg)[None].cuda(), 0.02,
                                    torch.from_numpy(q[:1]).cuda(), torch.from_numpy(jp)[None].cuda(), -0.01)
    m = O.metrics(q[1], jg, np.float32(0.02), q[0], jp, np.float32(-0.01))
    row = np.concatenate([[float(t[k][0]) for k in O.METRIC_KEYS], t["single_jpe"][0].cpu().numpy()])
    for k, v in _relative(row, m).items():
        worst[k] = max(worst.get(k, 0.), v)
    print("GPU vs fp64 oracle, worst relative error per key:", {k: "%.3e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


def test_fk_against_the_oracle(ev):
    from egoego_release_amd import synthetic
    m = synthetic.make_eval_motion(5, T_PAD, SEED, lengths=LENGTHS)
    aa, root = m["local_aa"].reshape(-1, 22, 3), m["root_trans"].reshape(-1, 3)
    q, p = ev.fk_smpl(torch.from_numpy(root).cuda(), torch.from_numpy(aa).cuda(), torch.from_numpy(m["rest_offsets"]).cuda(),
                      m["parents"])
    oq, op = O.fk(root, aa, m["rest_offsets"], m["parents"])
    q, p = q.cpu().numpy(), p.cpu().numpy()
    assert (q[..., 0] >= 0).all()
    e_pos = np.abs(p - op).max() / np.abs(op).max()
    e_rot = np.abs(O.quat_to_matrix(q) - O.quat_to_matrix(oq)).max()
    print("GPU FK vs fp64 oracle: joints %.3e of max |fp64|, rotation matrices %.3e" % (e_pos, e_rot))
    # rounded once from fp64: half an ulp of float32 on the joints; a unit quaternion rounded per component moves its matrix by
    # at most ~4 components x 2 x 2^-24
    assert e_pos <= 2.0 ** -24 * (1 + 1e-6) and e_rot <= 8 * 2.0 ** -24


def test_a_sample_is_bit_identical_alone_in_a_batch_and_under_another_padding(ev, walks):
    pf = torch.tensor([float(f["offset_floor_height"]) for f in walks["fc"]], device="cuda")

    def run(jpos, quat, lengths, floors):
        off, con, dis, d = ev.determine_floor_height_and_contacts(jpos, 30, lengths, return_details=True)
        t = ev._metrics_table(walks["gt_quat"][:jpos.shape[1]], walks["gt_jpos"][:jpos.shape[1]], 0., quat, jpos, floors, lengths)
        return off, d["floor_height"], t

    off, floor, table = run(walks["jpos"], walks["quat"], walks["lengths"], pf)
    perm = [3, 0, 4, 2, 1]
    off_p, floor_p, table_p = run(walks["jpos"][perm], walks["quat"][perm], walks["lengths"][perm], pf[perm])
    assert torch.equal(off_p, off[perm]) and torch.equal(floor_p, floor[perm]) and torch.equal(table_p, table[perm])
    b, L = 3, LENGTHS[3]  # alone, padded to its own length and to 150
    for T in (L, 150):
        j = torch.zeros(1, T, 22, 3, device="cuda")
        q = torch.ones(1, T, 22, 4, device="cuda")
        j[0, :L], q[0, :L] = walks["jpos"][b, :L], walks["quat"][b, :L]
        o1, f1, t1 = run(j, q, torch.tensor([L]), pf[b:b + 1])
        assert torch.equal(o1[0], off[b]) and torch.equal(f1[0], floor[b]) and torch.equal(t1[0], table[b]), T
    # a shared ground truth and the same one repeated per sample give the same bits
    rep = ev._metrics_table(walks["gt_quat"][None].expand(5, -1, -1, -1), walks["gt_jpos"][None].expand(5, -1, -1, -1), 0.,
                            walks["quat"], walks["jpos"], pf, walks["lengths"])
    assert torch.equal(rep, table)


def test_evaluate_samples_picks_the_oracles_best_per_group(ev):
    from egoego_release_amd import harness, synthetic
    B, T = 6, 139
    lengths = [139, 120, 139, 64, 139, 100]
    group = [0, 1, 0, 1, 2, 1]
    m = synthetic.make_eval_motion(B, T, 2, lengths=lengths)
    gq, gp = O.fk(m["gt_root_trans"], m["gt_local_aa"], m["rest_offsets"], m["parents"])
    gq, gp = gq.astype(np.float32), gp.astype(np.float32)
    want, floors, best = O.evaluate_samples(m["rest_offsets"], m["parents"], m["local_aa"], m["root_trans"], gq, gp, 0., lengths, group)
    for g in set(group):  # the two best of a group are further apart than anything rounding can do
        v = sorted(want[b]["mpjpe"] for b in range(B) if group[b] == g)
        assert len(v) < 2 or v[1] - v[0] > 1e-4 * v[1]
    ds = harness.SkeletonStats(np.zeros(66), np.ones(66), m["rest_offsets"], m["parents"])
    dev = torch.device("cuda")
    gp_dev = torch.from_numpy(gp).to(dev)
    keep = gp_dev.clone()
    out = ev.evaluate_samples(ds, torch.from_numpy(m["local_aa"]).to(dev), torch.from_numpy(m["root_trans"]).to(dev),
                              torch.from_numpy(gq).to(dev), gp_dev, 0., lengths, torch.tensor(group))
    assert torch.equal(gp_dev, keep)  # the caller's ground truth is not shifted in place
    assert out["best"].cpu().tolist() == [best[g] for g in range(3)]
    assert np.abs(out["floor_height"].cpu().numpy() - floors).max() <= 1e-6
    for b in range(B):
        for k in ("mpjpe", "root_dist", "head_trans_dist", "accel_err", "pred_fs"):
            assert abs(float(out["metrics"][k][b]) - want[b][k]) <= 1e-4 * abs(want[b][k]), (b, k)
        L = lengths[b]
        root = out["root_trans"][b, :L].cpu().numpy()
        jp = out["global_jpos"][b, :L].cpu().numpy()
        assert np.array_equal(root[:, :2], jp[:, 0, :2]) and np.array_equal(root[:, 2], jp[:, 0, 2] - out["floor_height"][b].item())
        assert abs(jp[0, 15, 0]) == 0 and abs(jp[0, 15, 1]) == 0
    one = ev.evaluate_samples(ds, torch.from_numpy(m["local_aa"]).to(dev), torch.from_numpy(m["root_trans"]).to(dev),
                              torch.from_numpy(gq).to(dev), gp_dev, 0., lengths)
    assert one["best"].cpu().tolist() == [min(range(B), key=lambda b: want[b]["mpjpe"])]


def test_a_single_sequence_returns_the_references_types(ev, walks):
    L = LENGTHS[2]
    off, contacts, discard = ev.determine_floor_height_and_contacts(walks["jpos"][2, :L], 30)
    assert type(off) is float and type(discard) is bool
    assert isinstance(contacts, np.ndarray) and contacts.dtype == np.float64 and contacts.shape == (L, 22)
    o = walks["fc"][2]
    assert abs(off - float(o["offset_floor_height"])) <= 1e-7 and np.array_equal(contacts, o["contacts"]) and discard == o["discard_seq"]
