"""Ragged stage 1 on the MI355X: egoego_s1_gravity_align and egoego_s1_head_pose_metrics on planted inputs, forward_for_eval(...,
lengths=) of both estimators and estimate_head_pose against the per-sequence oracle, batch / padding / NaN / stream invariance,
and evaluate_pipeline against itself one sequence at a time."""
import ctypes as C
import functools
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import stage1_oracle as O
import stage1_ragged_cases as K
import stream_cases as SC
from egoego_release_amd import _lib, evaluate, stage1, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
HEADNETS = [(31, 1), (60, 2)]
GRAVITYNETS = [(31, 1), (120, 2)]
NAN = float("nan")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _opt(hw, hl, gw, gl):
    return Namespace(window=hw, n_dec_layers=hl, n_head=4, d_k=256, d_v=256, d_model=256, dist_scale=10.0, input_of_feats=True,
                     normal_window=gw, normal_n_dec_layers=gl, normal_n_head=4, normal_d_k=256, normal_d_v=256, normal_d_model=256)


@functools.lru_cache(maxsize=None)
def headnet(window, n_layers):
    hn = stage1.HeadFormer(_opt(window, n_layers, 31, 1), DEV)
    sd = synthetic.make_stage1_weights("headnet", hn.cfg, 200 + window)
    hn.load_state_dict(sd)
    return hn, sd


@functools.lru_cache(maxsize=None)
def gravitynet(window, n_layers):
    gn = stage1.HeadNormalFormer(_opt(31, 1, window, n_layers), DEV, eval_whole_pipeline=True)
    sd = synthetic.make_stage1_weights("gravitynet", gn.cfg, 300 + window)
    gn.load_state_dict(sd)
    return gn, sd


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


# ------------------------------------------------------------------------------------------------ 1. gravity_align, planted
def align(trans, lens, normal, scale, ref, ref_lens):
    """egoego_s1_gravity_align on device tensors; Rn and Ralign hold NaN on entry."""
    S, Lmax = trans.shape[:2]
    Rn = torch.full((S, 3, 3), NAN, dtype=torch.float64, device=DEV)
    Ral = torch.full((S, 3, 3), NAN, dtype=torch.float64, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rl = torch.tensor(ref_lens, dtype=torch.int32, device=DEV)
    _lib.check_s1(_lib.load().egoego_s1_gravity_align(None, trans.data_ptr(), ln.data_ptr(), S, Lmax, normal.data_ptr(),
                                                      scale.data_ptr(), ref.data_ptr(), rl.data_ptr(), ref.shape[1], Rn.data_ptr(),
                                                      Ral.data_ptr(), _stream()))
    return Rn, Ral


@functools.lru_cache(maxsize=None)
def planted():
    """Every case of the table as one sequence: a normal at least 1e-3 off z, a scale, and the SLAM positions that put the case's
    est through scale * Rn; the lengths alternate between ref_len > len and len > ref_len (n is the shorter).  -> per-sequence
    host arrays, the oracle's Rn and Ralign (fp64 formulas on the fp32 inputs, rounded through fp32), and the case's group."""
    cases = K.trajectory_cases()
    rng = np.random.default_rng(77)
    seqs = []
    for group in ("compared", "lines", "single"):
        for i, (name, est, ref, _) in enumerate(cases[group]):
            nrm = rng.standard_normal(3) if i % 3 else np.array([1.5e-3 * (1 + i), -2e-3, 1.0 if i % 2 else -1.0])
            nrm = (nrm * rng.uniform(0.5, 2)).astype(np.float32)
            assert np.linalg.norm(np.cross(nrm.astype(np.float64), [0, 0, 1.0])) / np.linalg.norm(nrm.astype(np.float64)) >= 1e-3
            Rn = O.rotation_from_floor_normal(nrm.astype(np.float64)).astype(np.float32).astype(np.float64)
            sc = float(rng.uniform(0.5, 2.0))
            n = len(est)
            p = (est[:1] + (est - est[:1]).dot(Rn) / sc).astype(np.float32)  # Rn^T (est_i - est_0) / scale, from est_0
            extra_p, extra_r = ((0, 3) if i % 2 else (2, 0)) if n > 1 else (0, 0)
            if n == 1 and group == "single":
                extra_r = 4
            p = np.concatenate([p, rng.standard_normal((extra_p, 3)).astype(np.float32)])
            r7 = np.concatenate([ref, rng.standard_normal((n, 4))], 1)
            r7 = np.concatenate([r7, rng.standard_normal((extra_r, 7))])
            p64 = p.astype(np.float64)
            a = np.concatenate([p64[:1], p64[:1] + np.cumsum(sc * (p64[1:] - p64[:-1]).dot(Rn.T), 0)])
            want = K.oracle_umeyama(a[:n], ref).astype(np.float32).astype(np.float64) if group == "compared" else None
            seqs.append(dict(name=name, group=group, trans=p, ref=r7, normal=nrm, scale=sc, n=n, Rn=Rn, Ralign=want, est=a[:n]))
    return seqs


def _align_batch(seqs, extra=0, fill=NAN):
    trans = torch.from_numpy(K.pad([s["trans"] for s in seqs], max(len(s["trans"]) for s in seqs) + extra, fill)).to(DEV)
    ref = torch.from_numpy(K.pad([s["ref"] for s in seqs], max(len(s["ref"]) for s in seqs) + extra, fill)).to(DEV)
    normal = torch.from_numpy(np.stack([s["normal"] for s in seqs])).to(DEV)
    scale = torch.tensor([s["scale"] for s in seqs], dtype=torch.float64, device=DEV)
    return align(trans, [len(s["trans"]) for s in seqs], normal, scale, ref, [len(s["ref"]) for s in seqs])


def test_gravity_align_on_planted_inputs():
    """Rn and Ralign of every well-conditioned case within one fp32 ulp at 1.0 of the oracle's (both sides round an fp64 value to
    fp32); straight lines and a single frame for their properties only.  Padded frames and the outputs on entry hold NaN."""
    seqs = planted()
    assert any(len(s["trans"]) > len(s["ref"]) for s in seqs) and any(len(s["trans"]) < len(s["ref"]) for s in seqs)
    Rn, Ral = (t.cpu().numpy() for t in _align_batch(seqs))
    signs = set()
    for i, s in enumerate(seqs):
        e_rn = np.abs(Rn[i] - s["Rn"]).max()
        print(s["name"], "n", s["n"], "|dRn|", e_rn, "|dRalign|", None if s["Ralign"] is None else np.abs(Ral[i] - s["Ralign"]).max())
        assert e_rn <= K.ULP32, (s["name"], e_rn)
        r = Ral[i]
        assert np.isfinite(r).all() and np.abs(r.dot(r.T) - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(r) - 1) < 1e-6, s["name"]
        assert np.array_equal(r.astype(np.float32).astype(np.float64), r), s["name"]  # rounded through fp32
        if s["group"] == "compared":
            assert K.sigma_ratio(s["est"], s["ref"][:s["n"]]) >= 1e-2
            assert np.abs(r - s["Ralign"]).max() <= K.ULP32, (s["name"], np.abs(r - s["Ralign"]).max())
            signs.add(r[2, 2])
        if s["group"] == "single":
            assert np.array_equal(r, np.eye(3)), s["name"]
    assert signs == {1.0, -1.0}


def test_gravity_align_same_bits_alone_anywhere_and_under_any_padding():
    seqs = planted()
    Rn, Ral = _align_batch(seqs)
    order = list(reversed(range(len(seqs))))
    Rn2, Ral2 = _align_batch([seqs[i] for i in order], extra=5, fill=0.0)
    assert torch.equal(Rn2, Rn[order]) and torch.equal(Ral2, Ral[order])
    for i in (0, len(seqs) // 2, len(seqs) - 1):
        a, b = _align_batch([seqs[i]], extra=i % 3)
        assert torch.equal(a[0], Rn[i]) and torch.equal(b[0], Ral[i]), seqs[i]["name"]


# ------------------------------------------------------------------------------------------------ 2. against the oracle
@functools.lru_cache(maxsize=None)
def headnet_case(window, n_layers):
    T, L = K.headnet_lengths(window)
    return T, L, K.stage1_sequences(1000 + window, T, L)


@functools.lru_cache(maxsize=None)
def headnet_run(window, n_layers):
    """The ragged batch once (zero padding), kept unchanged for the tests that compare against it."""
    T, L, seqs = headnet_case(window, n_layers)
    hn, _ = headnet(window, n_layers)
    return hn.forward_for_eval(K.padded_batch(seqs), lengths=T, pose_lengths=L)


@pytest.mark.parametrize("window,n_layers", HEADNETS)
def test_ragged_headnet_against_oracle(window, n_layers):
    T, L, seqs = headnet_case(window, n_layers)
    _, sd = headnet(window, n_layers)
    out = headnet_run(window, n_layers)
    assert out["lengths"].tolist() == [min(l, t + 1) for t, l in zip(T, L)] and any(l == t for t, l in zip(T, L))
    refs = [O.headnet_eval(sd, window, n_layers, seqs["of"][b], seqs["head_pose"][b][0, 3:], seqs["aligned_slam_trans"][b], 10.0)
            for b in range(len(T))]
    va_max = np.abs(np.concatenate([torch.cat(r["va"]).numpy() for r in refs])).max()
    dist_max = np.abs(np.concatenate([torch.cat(r["dist"]).numpy() for r in refs])).max()
    for b, ref in enumerate(refs):
        t, n = T[b], min(L[b], T[b] + 1)
        va, dist = torch.cat(ref["va"]).numpy(), torch.cat(ref["dist"]).numpy()
        assert np.abs(out["head_va"][b, :t].cpu().numpy() - va).max() < 1e-4 * va_max, b
        assert np.abs(out["head_dist_scalar"][b, :t].cpu().numpy() - dist).max() < 1e-4 * dist_max, b
        q = out["head_rot_quat"][b].cpu().numpy()
        assert np.abs(q[:t + 1] - ref["quat"]).max() < 2e-4, b
        e_scale = abs(float(out["pred_scale"][b]) - ref["pred_scale"]) / abs(ref["pred_scale"])
        # (tests/test_gpu_stage1.py's bar: 1e-5, or what the distance bar allows when this sequence's mean distance is small)
        assert e_scale < max(1e-5, 1e-4 * dist_max / abs(float(dist[:max(min(t, L[b] - 1), 1)].mean()))), (b, e_scale)
        assert ref["head_pose"].shape[0] == n
        assert np.abs(out["head_pose"][b, :n].cpu().numpy() - ref["head_pose"]).max() < 2e-4, b
        # zero past each end
        assert not out["head_pose"][b, n:].any() and not out["head_va"][b, t:].any() and not out["head_dist_scalar"][b, t:].any()
        assert not out["head_rot_quat"][b, t + 1:].any()


@functools.lru_cache(maxsize=None)
def gravity_case(window, n_layers):
    L, R = K.gravity_lengths(window)
    rng = np.random.default_rng(2000 + window)
    rot = [O.quat2mat(K.unit_quats(rng, l)).astype(np.float32) for l in L]
    tr = [np.cumsum(rng.standard_normal((l, 3)) * 0.05, 0).astype(np.float32) for l in L]
    tr = [t - t[:1] for t in tr]
    gt = []
    for r in R:
        g = np.zeros((r, 7), np.float32)
        g[:, :3] = np.cumsum(rng.standard_normal((r, 3)) * 0.05, 0)
        g[:, 3:] = K.unit_quats(rng, r)
        gt.append(g)
    scale = rng.uniform(0.5, 2.0, len(L)).astype(np.float32)
    return L, R, dict(head_rot_mat=rot, head_trans=tr, ori_head_pose=gt), scale


def _gravity_batch(seqs, rows=None, extra=0, fill=0.0, device=None):
    b = K.padded_batch(seqs, rows, extra, fill)
    return {k: v.to(device) for k, v in b.items()} if device else b


@functools.lru_cache(maxsize=None)
def gravity_run(window, n_layers):
    L, R, seqs, scale = gravity_case(window, n_layers)
    gn, _ = gravitynet(window, n_layers)
    return gn.forward_for_eval(_gravity_batch(seqs), torch.from_numpy(scale), lengths=L, ref_lengths=R)


@pytest.mark.parametrize("window,n_layers", GRAVITYNETS)
def test_ragged_gravitynet_against_oracle(window, n_layers):
    L, R, seqs, scale = gravity_case(window, n_layers)
    assert any(r < l for l, r in zip(L, R)) and any(r > l for l, r in zip(L, R))
    assert min(L) < window + 1 and window + 1 in L and max(L) > window + 1
    _, sd = gravitynet(window, n_layers)
    out = gravity_run(window, n_layers)
    assert out["normal_rot"].is_cuda and out["align_rot"].is_cuda and out["normal_rot"].dtype == torch.float64
    for b, l in enumerate(L):
        n = min(l, R[b])
        ref = O.gravity_eval(sd, window, n_layers, seqs["head_rot_mat"][b], seqs["head_trans"][b], seqs["ori_head_pose"][b][:n],
                             float(scale[b]))
        assert rel(out["pred_normal"][b].cpu(), ref["pred_normal"]) < 1e-4, b
        e = np.abs(out["head_pose"][b, :l].cpu().numpy() - ref["head_pose"]).max()
        assert e < 2e-4, (b, e)
        assert not out["head_pose"][b, l:].any() and not out["head_rot_mat"][b, l:].any()
        assert not out["gt_head_pose"][b, R[b]:].any() and not out["gt_head_rot_mat"][b, R[b]:].any()
        assert torch.equal(out["gt_head_trans"][b, :R[b]].cpu(), torch.from_numpy(seqs["ori_head_pose"][b][:, :3]).double())


@pytest.mark.parametrize("hw,hl,gw,gl", [(31, 1, 31, 1), (60, 2, 120, 2)])
def test_ragged_estimate_head_pose_against_oracle(hw, hl, gw, gl):
    T, L, seqs = headnet_case(hw, hl)
    (hn, sd_h), (gn, sd_g) = headnet(hw, hl), gravitynet(gw, gl)
    hp, out, nout, n = stage1.estimate_head_pose(hn, gn, K.padded_batch(seqs), lengths=T, pose_lengths=L)
    assert hp.dtype == torch.float64 and hp.is_cuda and n.tolist() == [min(l, t + 1) for t, l in zip(T, L)]
    assert hp.shape == (len(T), max(n.tolist()), 7)
    for b, t in enumerate(T):
        oh = O.headnet_eval(sd_h, hw, hl, seqs["of"][b], seqs["head_pose"][b][0, 3:], seqs["aligned_slam_trans"][b], 10.0)
        tr = seqs["ori_slam_trans"][b] - seqs["ori_slam_trans"][b][0:1]
        og = O.gravity_eval(sd_g, gw, gl, seqs["ori_slam_rot_mat"][b], tr, seqs["head_pose"][b], oh["pred_scale"])
        want = O.assemble(og["head_pose"], oh["head_pose"], seqs["head_pose"][b])
        got = hp[b, :int(n[b])].cpu().numpy()
        assert got.shape == want.shape
        if L[b] <= 2:  # two aligned points lie on a line: the reference's rotation is arbitrary between r and its z-flipping twin
            got, want = got.copy(), want.copy()
            got[:, 2], want[:, 2] = np.abs(got[:, 2] - got[0, 2]), np.abs(want[:, 2] - want[0, 2])
        assert np.abs(got - want).max() < 2e-4, (b, np.abs(got - want).max())
        assert not hp[b, int(n[b]):].any()


# ------------------------------------------------------------------------------------------------ 3. same bits
def _same_rows(one, many, b, names_rows):
    for k, rows in names_rows.items():
        assert torch.equal(one[k][0, :rows], many[k][b, :rows]), (k, b)


@pytest.mark.parametrize("window,n_layers", HEADNETS)
def test_headnet_rows_are_the_same_bits_alone_anywhere_and_under_any_padding(window, n_layers):
    T, L, seqs = headnet_case(window, n_layers)
    hn, _ = headnet(window, n_layers)
    allo = headnet_run(window, n_layers)
    order = [4, 0, 5, 2, 1, 3]
    perm = hn.forward_for_eval(K.padded_batch(seqs, order, extra=3), lengths=[T[i] for i in order], pose_lengths=[L[i] for i in order])
    for j, i in enumerate(order):
        n = min(L[i], T[i] + 1)
        for k, rows in dict(head_pose=n, head_va=T[i], head_dist_scalar=T[i], head_rot_quat=T[i] + 1).items():
            assert torch.equal(perm[k][j, :rows], allo[k][i, :rows]), (k, i)
        assert torch.equal(perm["pred_scale"][j], allo["pred_scale"][i])
    for b in (0, 3, 5):
        one = hn.forward_for_eval(K.padded_batch(seqs, [b], extra=b), lengths=[T[b]], pose_lengths=[L[b]])
        _same_rows(one, allo, b, dict(head_pose=min(L[b], T[b] + 1), head_va=T[b], head_dist_scalar=T[b], head_rot_quat=T[b] + 1))
        assert torch.equal(one["pred_scale"][0], allo["pred_scale"][b])
    # all lengths equal: the bits of the lengths=None path
    t = window + 1
    eq = K.padded_batch(K.stage1_sequences(5, [t, t], [t + 1, t + 1]))
    a, r = hn.forward_for_eval(eq), hn.forward_for_eval(eq, lengths=[t, t])
    for k in ("head_pose", "pred_scale", "head_va", "head_dist_scalar", "head_rot_quat"):
        assert torch.equal(a[k], r[k]), k


@pytest.mark.parametrize("window,n_layers", GRAVITYNETS)
def test_gravitynet_rows_are_the_same_bits_alone_anywhere_and_under_any_padding(window, n_layers):
    L, R, seqs, scale = gravity_case(window, n_layers)
    gn, _ = gravitynet(window, n_layers)
    allo = gravity_run(window, n_layers)
    order = [5, 1, 0, 4, 3, 2]
    perm = gn.forward_for_eval(_gravity_batch(seqs, order, extra=2), torch.from_numpy(scale[order]), lengths=[L[i] for i in order],
                               ref_lengths=[R[i] for i in order])
    for j, i in enumerate(order):
        assert torch.equal(perm["head_pose"][j, :L[i]], allo["head_pose"][i, :L[i]]), i
        for k in ("pred_normal", "normal_rot", "align_rot"):
            assert torch.equal(perm[k][j], allo[k][i]), (k, i)
    for b in (0, 2, 5):
        one = gn.forward_for_eval(_gravity_batch(seqs, [b], extra=b), torch.from_numpy(scale[b:b + 1]), lengths=[L[b]], ref_lengths=[R[b]])
        assert torch.equal(one["head_pose"][0, :L[b]], allo["head_pose"][b, :L[b]]), b
        assert torch.equal(one["align_rot"][0], allo["align_rot"][b]) and torch.equal(one["normal_rot"][0], allo["normal_rot"][b])
    # all lengths equal: the host path rounds the same fp64 rotations through fp32 and may straddle a rounding boundary: one
    # ulp (6e-8) in an entry, three entries per coordinate -> 1e-6 of the trajectory's extent
    l = window + 2
    rng = np.random.default_rng(9)
    eq = {"head_rot_mat": torch.from_numpy(O.quat2mat(K.unit_quats(rng, 2 * l)).astype(np.float32).reshape(2, l, 3, 3)),
          "head_trans": torch.from_numpy(np.cumsum(rng.standard_normal((2, l, 3)) * 0.05, 1).astype(np.float32)),
          "ori_head_pose": torch.from_numpy(np.concatenate([np.cumsum(rng.standard_normal((2, l, 3)) * 0.05, 1),
                                                            K.unit_quats(rng, 2 * l).reshape(2, l, 4)], -1).astype(np.float32))}
    sc = torch.tensor([0.8, 1.7])
    a, r = gn.forward_for_eval(eq, sc), gn.forward_for_eval(eq, sc, lengths=[l, l])
    assert torch.equal(a["pred_normal"], r["pred_normal"])
    for b in range(2):
        p = a["head_pose"][b, :, :3]
        bar = 1e-6 * max(1.0, float((p - p[0]).norm(dim=-1).max()))
        assert float((a["head_pose"][b] - r["head_pose"][b]).abs().max()) <= bar, b
        assert float((a["normal_rot"][b] - r["normal_rot"][b].cpu()).abs().max()) <= K.ULP32
        assert float((a["align_rot"][b] - r["align_rot"][b].cpu()).abs().max()) <= K.ULP32


# ------------------------------------------------------------------------------------------------ 4. NaN padding
def test_nan_filled_padding_changes_nothing():
    (hw, hl), (gw, gl) = HEADNETS[0], GRAVITYNETS[0]
    T, L, seqs = headnet_case(hw, hl)
    hn, _ = headnet(hw, hl)
    clean = headnet_run(hw, hl)
    dirty = hn.forward_for_eval(K.padded_batch(seqs, extra=2, fill=NAN), lengths=T, pose_lengths=L)
    for k in ("head_pose", "head_va", "head_dist_scalar", "head_rot_quat"):
        w = clean[k].shape[1]
        assert torch.equal(dirty[k][:, :w], clean[k]) and not dirty[k][:, w:].any(), k
    assert torch.equal(dirty["pred_scale"], clean["pred_scale"])
    Lg, R, gseqs, scale = gravity_case(gw, gl)
    gn, _ = gravitynet(gw, gl)
    gclean = gravity_run(gw, gl)
    gdirty = gn.forward_for_eval(_gravity_batch(gseqs, extra=2, fill=NAN), torch.from_numpy(scale), lengths=Lg, ref_lengths=R)
    for k in ("head_pose", "head_trans", "head_rot_mat", "gt_head_trans", "gt_head_rot_mat", "gt_head_pose"):
        w = gclean[k].shape[1]
        assert torch.equal(gdirty[k][:, :w], gclean[k]) and not gdirty[k][:, w:].any(), k
    for k in ("pred_normal", "normal_rot", "align_rot"):
        assert torch.equal(gdirty[k], gclean[k]), k
    hp_c = stage1.estimate_head_pose(hn, gn, K.padded_batch(seqs), lengths=T, pose_lengths=L)[0]
    hp_d = stage1.estimate_head_pose(hn, gn, K.padded_batch(seqs, extra=1, fill=NAN), lengths=T, pose_lengths=L)[0]
    assert torch.equal(hp_d, hp_c)


# ------------------------------------------------------------------------------------------------ 5. head-pose metrics
def metrics_raw(pred, gt, lengths):
    """egoego_s1_head_pose_metrics on device tensors; the output holds NaN on entry."""
    B, T = pred.shape[:2]
    out = torch.full((B, 3), NAN, dtype=torch.float64, device=DEV)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    _lib.check_s1(_lib.load().egoego_s1_head_pose_metrics(pred.data_ptr(), gt.data_ptr(), ln.data_ptr(), B, T, out.data_ptr(), _stream()))
    return out


def test_head_pose_metrics_against_golden_and_restatement():
    """1e-10 relative: the fp64 closed form sits 1e-14 from the reference's np.linalg.inv path, the same formula in fp32 2e-5."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "head_metrics_golden.npz"))
    lengths = g["lengths"].tolist()
    pred, gt = g["pred"].copy(), g["gt"].copy()
    for b, n in enumerate(lengths):
        pred[b, n:] = NAN
        gt[b, n:] = NAN
    pd, gd = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    raw = metrics_raw(pd, gd, lengths)
    got = raw.cpu().numpy()
    print("max relative difference from the golden:", np.abs(got / g["metrics"] - 1).max())
    assert (np.abs(got - g["metrics"]) <= 1e-10 * np.abs(g["metrics"])).all(), np.abs(got / g["metrics"] - 1).max()
    assert torch.equal(stage1.head_pose_metrics(pd, gd, lengths), raw)
    assert torch.equal(stage1.head_pose_metrics(pd, gd, torch.tensor(lengths, device=DEV)), raw)
    # the reference's signature: matrices in, three [B] tensors out; and against the numpy restatement on another ragged batch
    lens2 = [1, 17, 64, 200, 129]
    p2, g2 = K.metric_poses(99, len(lens2), max(lens2))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    Rp, Rg = K.quat_to_matrix(p2[..., 3:]), K.quat_to_matrix(g2[..., 3:])
    e, o, tt = stage1.compute_head_pose_metrics(t(p2[..., :3]), t(Rp), t(g2[..., :3]), t(Rg), lengths=lens2)
    assert e.shape == (len(lens2),) and e.dtype == torch.float64
    for b, n in enumerate(lens2):
        want = K.head_pose_metrics_np(p2[b, :n, :3], Rp[b, :n], g2[b, :n, :3], Rg[b, :n])
        for j, v in enumerate((e, o, tt)):
            assert abs(float(v[b]) - want[j]) <= 1e-10 * abs(want[j]), (n, j)
        one = stage1.compute_head_pose_metrics(t(p2[b, :n, :3]), t(Rp[b, :n]), t(g2[b, :n, :3]), t(Rg[b, :n]))  # [T, ...] alone
        assert all(torch.equal(x[0], v[b]) for x, v in zip(one, (e, o, tt))), n
    # alone, reordered and under another padding: the same bits
    order = [3, 6, 0, 5, 1, 4, 2]
    wide = torch.full((len(order), max(lengths) + 9, 7), NAN, dtype=torch.float64, device=DEV)
    wide_g = wide.clone()
    wide[:, :pd.shape[1]], wide_g[:, :pd.shape[1]] = pd[order], gd[order]
    assert torch.equal(metrics_raw(wide, wide_g, [lengths[i] for i in order]), raw[order])


# ------------------------------------------------------------------------------------------------ 6. streams
def test_new_calls_run_on_the_callers_stream():
    """tests/stream_cases.py's late-input run: both entry points and the ragged Python calls give the default stream's bits on a
    side stream held back by a delay, and leave the null stream idle."""
    (hw, hl), (gw, gl) = HEADNETS[0], GRAVITYNETS[0]
    (hn, _), (gn, _) = headnet(hw, hl), gravitynet(gw, gl)
    rng = np.random.default_rng(31)
    S, Lm = 5, 70
    lens, rlens = [70, 3, 40, 66, 12], [60, 9, 70, 66, 5]
    trans = torch.from_numpy(np.cumsum(rng.standard_normal((S, Lm, 3)) * 0.05, 1).astype(np.float32)).to(DEV)
    ref = torch.from_numpy(np.cumsum(rng.standard_normal((S, Lm, 7)) * 0.05, 1)).to(DEV)
    normal = torch.from_numpy(rng.standard_normal((S, 3)).astype(np.float32)).to(DEV)
    scale = torch.from_numpy(rng.uniform(0.5, 2, S)).to(DEV)
    rot = torch.from_numpy(O.quat2mat(K.unit_quats(rng, S * Lm)).astype(np.float32).reshape(S, Lm, 3, 3)).to(DEV)
    pred, gt = (torch.from_numpy(a).to(DEV) for a in K.metric_poses(5, S, Lm))
    T, L = [69, 2, 39, 65, 11], lens
    of = torch.from_numpy(rng.standard_normal((S, 69, 512)).astype(np.float32)).to(DEV)
    hp = torch.from_numpy(np.concatenate([np.cumsum(rng.standard_normal((S, Lm, 3)) * 0.02, 1),
                                          K.unit_quats(rng, S * Lm).reshape(S, Lm, 4)], -1).astype(np.float32)).to(DEV)

    def c_align(tr, nm, sc, rf):
        return align(tr, lens, nm, sc, rf, rlens)

    def c_metrics(p, g):
        return metrics_raw(p, g, lens)

    def c_gravity(r, tr, rf, sc):
        o = gn.forward_for_eval({"head_rot_mat": r, "head_trans": tr, "ori_head_pose": rf}, sc, lengths=lens, ref_lengths=rlens)
        return [o[k] for k in ("head_pose", "pred_normal", "normal_rot", "align_rot", "gt_head_pose")]

    def c_headnet(f, h, sl):
        o = hn.forward_for_eval({"of": f, "head_pose": h, "aligned_slam_trans": sl}, lengths=T, pose_lengths=L)
        return [o[k] for k in ("head_pose", "pred_scale", "head_va", "head_rot_quat")]

    def c_pose(f, h, sl, ot, orot):
        return stage1.estimate_head_pose(hn, gn, {"of": f, "head_pose": h, "aligned_slam_trans": sl, "ori_slam_trans": ot,
                                                  "ori_slam_rot_mat": orot}, lengths=T, pose_lengths=L)[0]

    calls = {"egoego_s1_gravity_align": (SC.ENQUEUES, c_align, [trans, normal, scale, ref]),
             "egoego_s1_head_pose_metrics": (SC.ENQUEUES, c_metrics, [pred, gt]),
             "HeadNormalFormer.forward_for_eval(lengths=)": (SC.ENQUEUES, c_gravity, [rot, trans, ref, scale]),
             "HeadFormer.forward_for_eval(lengths=)": ("uploads its lengths with blocking copies", c_headnet, [of, hp, trans]),
             "estimate_head_pose(lengths=)": ("HeadFormer uploads its lengths with blocking copies", c_pose, [of, hp, trans, trans, rot])}
    for _, call, true in calls.values():  # warm every shape
        call(*[t.clone() for t in true])
    torch.cuda.synchronize()
    delay = SC.Delay().calibrate({k: (lambda c=call, tr=true: c(*tr)) for k, (m, call, true) in calls.items() if m == SC.ENQUEUES})
    side = torch.cuda.Stream()
    for name, (mode, call, true) in calls.items():
        SC.check(name, mode, call, true, side, delay)


def test_ragged_gravitynet_never_waits_for_the_device():
    """Under torch's sync debug mode "error" a ragged HeadNormalFormer.forward_for_eval on device inputs raises nothing: no
    device-to-host copy, no blocking upload."""
    gw, gl = GRAVITYNETS[0]
    gn, _ = gravitynet(gw, gl)
    L, R, seqs, scale = gravity_case(gw, gl)
    batch = _gravity_batch(seqs, device=DEV)
    sc = torch.from_numpy(scale).to(DEV)
    gn.forward_for_eval(batch, sc, lengths=L, ref_lengths=R)  # (warm: weights packed, workspace and pinned blocks allocated)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            implemented = False
        except RuntimeError:
            implemented = True
        if implemented:
            out = gn.forward_for_eval(batch, sc, lengths=L, ref_lengths=R)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not implemented:
        pytest.skip("this torch build does not raise on a synchronising call under set_sync_debug_mode('error')")
    assert torch.equal(out["head_pose"], gravity_run(gw, gl)["head_pose"])


# ------------------------------------------------------------------------------------------------ 7. the whole pipeline
def test_evaluate_pipeline_is_the_same_bits_one_sequence_at_a_time():
    """Three sequences of different lengths through evaluate_pipeline (stage 1, its score, the floor, stage 2 with the strided
    sampler, the full-body metrics): every number of sequence s equals the call on that sequence alone with sequence_offset = s."""
    from test_gpu_ddim_harness import P3, _draws, _harness_setup
    m, ds = _harness_setup(P3)
    (hw, hl), (gw, gl) = HEADNETS[0], GRAVITYNETS[0]
    (hn, _), (gn, _) = headnet(hw, hl), gravitynet(gw, gl)
    T = [39, 139, 249]
    L = [t + 1 for t in T]
    seqs = K.stage1_sequences(77, T, L)
    rng = np.random.default_rng(78)
    gt_root = [(np.cumsum(rng.standard_normal((l, 3)) * 0.01, 0) + [0, 0, 0.9]).astype(np.float32) for l in L]
    gt_aa = [(rng.standard_normal((l, 22, 3)) * 0.2).astype(np.float32) for l in L]
    draws = [_draws(1, l, 50 + s) for s, l in enumerate(L)]
    kw = dict(sampler="ddim", n_steps=4)

    def run(rows, offset):
        return evaluate.evaluate_pipeline(hn, gn, m, ds, K.padded_batch(seqs, rows), torch.from_numpy(K.pad([gt_root[i] for i in rows])),
                                          torch.from_numpy(K.pad([gt_aa[i] for i in rows])), [T[i] for i in rows],
                                          sequence_offset=offset, noise=[draws[i] for i in rows], **kw)

    allr = run([0, 1, 2], 0)
    assert allr["stage1_metrics"].shape == (3, 3) and allr["stage1_metrics"].dtype == torch.float64
    assert allr["lengths"].tolist() == L and allr["head_pose"].shape == (3, max(L), 7)
    assert bool(torch.isfinite(allr["stage1_metrics"]).all()) and allr["best"].tolist() == [0, 1, 2]
    for s, l in enumerate(L):
        one = run([s], s)
        assert one["lengths"].tolist() == [l] and one["best"].tolist() == [0]
        assert torch.equal(one["stage1_metrics"][0], allr["stage1_metrics"][s]), s
        assert torch.equal(one["head_pose"][0, :l], allr["head_pose"][s, :l]) and not allr["head_pose"][s, l:].any(), s
        for k, v in one["metrics"].items():
            assert torch.equal(v[0], allr["metrics"][k][s]) or (bool(torch.isnan(v[0]).all()) and bool(torch.isnan(allr["metrics"][k][s]).all())), (k, s)
        for k in ("floor_height", "discard"):
            assert torch.equal(one[k][0], allr[k][s]), (k, s)
        for k in ("contacts", "global_quat", "global_jpos", "root_trans"):
            assert torch.equal(one[k][0, :l], allr[k][s, :l]), (k, s)
