"""Stage 1 on the MI355X: the HIP estimators against the reference's golden (both shape sets) and against the fp32 oracle on
randomised batches, batch invariance."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import stage1_oracle as O
from egoego_release_amd import stage1, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"demo": dict(window=60, n_dec_layers=2, normal_window=120, normal_n_dec_layers=2),
        "default": dict(window=90, n_dec_layers=2, normal_window=90, normal_n_dec_layers=4)}


def opt_for(s):
    return Namespace(window=s["window"], n_dec_layers=s["n_dec_layers"], n_head=4, d_k=256, d_v=256, d_model=256,
                     dist_scale=10.0, input_of_feats=True, normal_window=s["normal_window"],
                     normal_n_dec_layers=s["normal_n_dec_layers"], normal_n_head=4, normal_d_k=256, normal_d_v=256,
                     normal_d_model=256)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "stage1_golden.npz"))


def models(g, tag):
    s = SETS[tag]
    opt = opt_for(s)
    sh, sg = (int(v) for v in g["seeds"])
    hn = stage1.HeadFormer(opt, "cuda:0")
    hn.load_state_dict(synthetic.make_stage1_weights("headnet", hn.cfg, sh))
    gn = stage1.HeadNormalFormer(opt, "cuda:0", eval_whole_pipeline=True)
    gn.load_state_dict(synthetic.make_stage1_weights("gravitynet", gn.cfg, sg))
    return hn, gn


def batch_of(g):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None]  # noqa: E731
    return {"of": t(g["of"]), "head_pose": t(g["head_pose"]), "aligned_slam_trans": t(g["aligned_slam_trans"]),
            "ori_slam_trans": t(g["ori_slam_trans"]), "ori_slam_rot_mat": t(g["ori_slam_rot_mat"]),
            "seq_len": torch.tensor([int(g["seq_len"])])}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("tag", list(SETS))
def test_stage1_matches_reference_golden(g, tag):
    s = SETS[tag]
    P = tag + "_"
    hn, gn = models(g, tag)
    sd_h, sd_g = hn.state_dict(), gn.state_dict()
    T = int(g["seq_len"])
    # every layer of every HeadNet block against the oracle (itself bit-equal to the reference), the last against the golden
    spans = stage1.block_spans(T, s["window"])
    feats = torch.zeros(len(spans), s["window"], 512)
    for i, (st, n) in enumerate(spans):
        feats[i, :n] = torch.from_numpy(g["of"][st:st + n])
    valid = torch.tensor([n for _, n in spans], dtype=torch.int32)
    heads, layers = hn.engine().encode(feats.cuda(), valid.cuda(), layers=True)
    ref_layers = O.decoder({k: v.cpu() for k, v in sd_h.items()}, feats, valid, s["n_dec_layers"])
    for l in range(s["n_dec_layers"]):
        e = (layers[l].cpu() - ref_layers[l]).abs().max().item()
        assert e < 1e-4, (tag, "headnet layer", l, e)
    for b in range(len(spans)):
        L = s["n_dec_layers"] - 1
        assert np.abs(layers[L, b].cpu().numpy() - g[P + f"h_block{b}_layer{L}"]).max() < 1e-4
    out = hn.forward_for_eval(batch_of(g))
    assert rel(out["head_va"][0].cpu(), g[P + "va"]) < 1e-4
    assert rel(out["head_dist_scalar"][0].cpu(), g[P + "dist"]) < 1e-4
    assert np.abs(out["head_rot_quat"][0, -1].cpu().numpy() - g[P + "headnet_head_pose"][-1, 3:]).max() < 2e-4
    assert abs(float(out["pred_scale"]) - float(g[P + "pred_scale"])) / abs(float(g[P + "pred_scale"])) < 1e-5
    # GravityNet
    tr = g["ori_slam_trans"] - g["ori_slam_trans"][0:1]
    f, n = O.gravity_features(g["ori_slam_rot_mat"], tr, s["normal_window"])
    nd = {"head_trans": torch.from_numpy(tr)[None], "head_rot_mat": torch.from_numpy(g["ori_slam_rot_mat"])[None]}
    normal = gn.forward(nd)["pred_normal"]
    assert rel(normal[0].cpu(), g[P + "pred_normal"]) < 1e-4
    _, glayers = gn.engine().encode(f[None].cuda(), torch.tensor([n], dtype=torch.int32).cuda(), layers=True)
    gref = O.decoder({k: v.cpu() for k, v in sd_g.items()}, f[None], torch.tensor([n]), s["normal_n_dec_layers"])
    for l in range(s["normal_n_dec_layers"]):
        e = (glayers[l].cpu() - gref[l]).abs().max().item()
        assert e < 1e-4, (tag, "gravity layer", l, e)
    hp, _, nout = stage1.estimate_head_pose(hn, gn, batch_of(g))
    assert np.abs(nout["head_pose"][0].cpu().numpy() - g[P + "gravity_head_pose"]).max() < 2e-4
    e = np.abs(hp[0].cpu().numpy() - g[P + "head_pose"]).max()
    assert e < 2e-4, e


def _heads_oracle(sd, kind, last, valid):
    if kind == "headnet":
        va, dist = O.headnet_heads(sd, last)
        return torch.cat([va, dist], -1)
    return O.gravity_head(sd, last[:, 0])


@pytest.mark.parametrize("window,n_layers,kind", [(60, 1, "headnet"), (90, 2, "headnet"), (120, 3, "gravitynet"),
                                                  (128, 4, "headnet"), (60, 2, "gravitynet"), (128, 1, "gravitynet"),
                                                  (1, 2, "headnet"), (31, 3, "gravitynet"), (31, 1, "headnet")])
def test_random_batches_against_oracle(window, n_layers, kind):
    cfg = synthetic.Stage1Config(kind, window, n_layers)
    sd = synthetic.make_stage1_weights(kind, cfg, 100 + window + n_layers)
    eng = stage1.Stage1Engine(cfg, "cuda:0")
    eng.load(sd)
    rng = np.random.default_rng(window * 10 + n_layers)
    feats, valid = [], []
    for T in (1, 19, 59, 60, 61, 119, 120, 121, 139, 500):
        for st, n in stage1.block_spans(T, window):
            f = np.zeros((window, cfg.d_feats), np.float32)
            f[:n] = rng.standard_normal((n, cfg.d_feats))
            feats.append(f)
            valid.append(n)
    feats = torch.from_numpy(np.stack(feats))
    valid = torch.tensor(valid, dtype=torch.int32)
    out, layers = eng.encode(feats.cuda(), valid.cuda(), layers=True)
    ref = O.decoder(sd, feats, valid, n_layers)
    for l in range(n_layers):
        e = (layers[l].cpu() - ref[l]).abs().max().item()
        assert e < 1e-4, (l, e)
    rh = _heads_oracle(sd, kind, ref[-1], valid)
    got = out.cpu()
    if kind == "headnet":
        m = (torch.arange(window)[None, :] < valid[:, None].long())
        for c in range(4):
            assert rel(got[..., c][m], rh[..., c][m]) < 1e-4, c
    else:
        assert rel(got, rh) < 1e-4
    if window > 1:
        assert any(0 < n < window for n in valid.tolist())  # short last blocks (padded rows as keys) are in the batch


def test_padded_rows_are_keys():
    """A block of 19 valid tokens in a 60-token window: its valid rows differ from those of a 19-token window (the padded rows
    are attended to, TM:126-141), and the HIP output follows the 60-token computation."""
    cfg = synthetic.Stage1Config("headnet", 60, 2)
    sd = synthetic.make_stage1_weights("headnet", cfg, 5)
    rng = np.random.default_rng(1)
    f = torch.zeros(1, 60, 512)
    f[0, :19] = torch.from_numpy(rng.standard_normal((19, 512)).astype(np.float32))
    v = torch.tensor([19], dtype=torch.int32)
    full = O.decoder(sd, f, v, 2)[-1][0, :19]
    sd19 = dict(sd)
    short = O.decoder(sd19, f[:, :19].contiguous(), v, 2)[-1][0, :19]
    assert (full - short).abs().max().item() > 1e-2
    eng = stage1.Stage1Engine(cfg, "cuda:0")
    eng.load(sd)
    _, layers = eng.encode(f.cuda(), v.cuda(), layers=True)
    assert (layers[-1, 0, :19].cpu() - full).abs().max().item() < 1e-4


def test_batch_invariance():
    cfg = synthetic.Stage1Config("headnet", 60, 2)
    sd = synthetic.make_stage1_weights("headnet", cfg, 9)
    eng = stage1.Stage1Engine(cfg, "cuda:0")
    eng.load(sd)
    rng = np.random.default_rng(2)
    W = 64
    f = torch.from_numpy(rng.standard_normal((W, 60, 512)).astype(np.float32)).cuda()
    v = torch.from_numpy(rng.integers(1, 61, W).astype(np.int32)).cuda()
    allw = eng.encode(f, v)
    for i in (0, 17, 63):
        one = eng.encode(f[i:i + 1].contiguous(), v[i:i + 1].contiguous())
        assert torch.equal(one[0], allw[i]), i
    gcfg = synthetic.Stage1Config("gravitynet", 120, 2)
    geng = stage1.Stage1Engine(gcfg, "cuda:0")
    geng.load(synthetic.make_stage1_weights("gravitynet", gcfg, 9))
    gf = torch.from_numpy(rng.standard_normal((W, 120, 18)).astype(np.float32)).cuda()
    gv = torch.from_numpy(rng.integers(1, 121, W).astype(np.int32)).cuda()
    ga = geng.encode(gf, gv)
    for i in (0, 40):
        assert torch.equal(geng.encode(gf[i:i + 1].contiguous(), gv[i:i + 1].contiguous())[0], ga[i])


def test_gravity_features_kernel_against_oracle():
    rng = np.random.default_rng(3)
    m = stage1.HeadNormalFormer(Namespace(window=90, n_dec_layers=1, n_head=4, d_k=256, d_v=256, d_model=256), "cuda:0")
    for L in (140, 91, 90, 30, 2):
        q = rng.standard_normal((L, 4))
        rot = O.quat2mat(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        tr = rng.standard_normal((L, 3)).astype(np.float32)
        eng = m.engine()
        r = torch.from_numpy(rot).reshape(1, L, 9).cuda()
        t = torch.from_numpy(tr)[None].cuda()
        ln = torch.tensor([L], dtype=torch.int32).cuda()
        f = torch.empty(1, 90, 18, device="cuda")
        v = torch.empty(1, dtype=torch.int32, device="cuda")
        from egoego_release_amd import _lib
        _lib.check_s1(eng.lib.egoego_s1_gravity_features(r.data_ptr(), t.data_ptr(), ln.data_ptr(), 1, L, 90, f.data_ptr(),
                                                         v.data_ptr(), eng._stream()))
        rf, rn = O.gravity_features(rot, tr, 90)
        assert int(v[0]) == rn
        assert (f[0].cpu() - rf).abs().max().item() < 1e-6


# ------------------------------------------------------------------------------------------ whole sequences, many per call
LENGTHS = (1, 19, 59, 60, 61, 119, 120, 121, 139, 500)


def _opt(window, n_layers, normal_window=90, normal_layers=2):
    return Namespace(window=window, n_dec_layers=n_layers, n_head=4, d_k=256, d_v=256, d_model=256, dist_scale=10.0,
                     input_of_feats=True, normal_window=normal_window, normal_n_dec_layers=normal_layers, normal_n_head=4,
                     normal_d_k=256, normal_d_v=256, normal_d_model=256)


def _unit_quats(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.where(q[:, :1] < 0, -q, q)


def _sequences(rng, B, T):
    """B random sequences of T feature frames: features, a ground-truth head pose of T + 1 frames, an aligned SLAM walk."""
    of = rng.standard_normal((B, T, 512)).astype(np.float32)
    hp = np.zeros((B, T + 1, 7), np.float32)
    hp[:, :, :3] = np.cumsum(rng.standard_normal((B, T + 1, 3)) * 0.02, 1)
    hp[:, :, 3:] = _unit_quats(rng, B * (T + 1)).reshape(B, T + 1, 4)
    slam = (np.cumsum(rng.standard_normal((B, T + 1, 3)) * 0.03, 1)).astype(np.float32)
    return of, hp, slam


@pytest.mark.parametrize("window,n_layers", [(60, 2), (90, 1), (120, 3), (128, 4)])
def test_headnet_sequences_against_oracle(window, n_layers):
    """forward_for_eval on B = 3 sequences per call at every length: the integrated quaternions, pred_scale and the head pose of
    every sequence against the oracle's, with the issue's bars."""
    hn = stage1.HeadFormer(_opt(window, n_layers), "cuda:0")
    sd = synthetic.make_stage1_weights("headnet", hn.cfg, 200 + window)
    hn.load_state_dict(sd)
    rng = np.random.default_rng(window + n_layers)
    for T in LENGTHS:
        of, hp, slam = _sequences(rng, 3, T)
        out = hn.forward_for_eval({"of": torch.from_numpy(of), "head_pose": torch.from_numpy(hp),
                                   "aligned_slam_trans": torch.from_numpy(slam)})
        refs = [O.headnet_eval(sd, window, n_layers, of[b], hp[b, 0, 3:], slam[b], 10.0) for b in range(3)]
        # "relative to each output's max-abs": the output of this call (3 sequences x T frames).  The split-bf16 error is absolute
        # (set by the activations, ~1e-6), so a single near-zero value of one sequence says nothing on its own.
        va_all = np.concatenate([torch.cat(r["va"]).numpy() for r in refs])
        dist_all = np.concatenate([torch.cat(r["dist"]).numpy() for r in refs])
        va_max, dist_max = np.abs(va_all).max(), np.abs(dist_all).max()
        for b, ref in enumerate(refs):
            va, dist = torch.cat(ref["va"]).numpy(), torch.cat(ref["dist"]).numpy()
            assert np.abs(out["head_va"][b].cpu().numpy() - va).max() < 1e-4 * va_max, (T, b)
            assert np.abs(out["head_dist_scalar"][b].cpu().numpy() - dist).max() < 1e-4 * dist_max, (T, b)
            q = out["head_rot_quat"][b].cpu().numpy()
            assert q.shape == (T + 1, 4)
            assert np.abs(q[-1] - ref["quat"][-1]).max() < 2e-4, (T, b)
            # pred_scale = mean(dist / dist_scale) / mean |SLAM step|: the integration must compute exactly that from the HIP
            # distances; against the oracle its relative error is 1e-5, or what the distance bar allows when the mean of this
            # sequence's distances is small against their scale (a few frames, cancellation): 1e-4 * max|dist| / |mean dist|.
            d_hip = out["head_dist_scalar"][b, :, 0].double().cpu().numpy() / 10.0
            st = np.linalg.norm(np.diff(slam[b].astype(np.float64), axis=0), axis=1)
            assert abs(float(out["pred_scale"][b]) - d_hip.mean() / st.mean()) / abs(d_hip.mean() / st.mean()) < 1e-6, (T, b)
            e_scale = abs(float(out["pred_scale"][b]) - ref["pred_scale"]) / abs(ref["pred_scale"])
            assert e_scale < max(1e-5, 1e-4 * dist_max / abs(float(dist.mean()))), (T, b, e_scale)
            assert np.abs(out["head_pose"][b].cpu().numpy() - ref["head_pose"]).max() < 2e-4, (T, b)


@pytest.mark.parametrize("window,n_layers", [(60, 2), (90, 4), (120, 2), (31, 1)])
def test_gravitynet_sequences_against_oracle(window, n_layers):
    """forward_for_eval on B = 3 sequences per call: the normal, and the de-headed pose (GravityNet's features, its trajectory
    kernel on each sequence's own normal, scale and Umeyama rotation) against the oracle."""
    gn = stage1.HeadNormalFormer(_opt(60, 2, window, n_layers), "cuda:0", eval_whole_pipeline=True)
    sd = synthetic.make_stage1_weights("gravitynet", gn.cfg, 300 + window)
    gn.load_state_dict(sd)
    rng = np.random.default_rng(window * 7 + n_layers)
    for L in (5, 20, window, window + 1, window + 2, 140):
        B = 3
        rot = O.quat2mat(_unit_quats(rng, B * L)).astype(np.float32).reshape(B, L, 3, 3)
        tr = np.cumsum(rng.standard_normal((B, L, 3)) * 0.05, 1).astype(np.float32)
        tr -= tr[:, :1]
        gt = np.zeros((B, L, 7), np.float32)
        gt[:, :, :3] = np.cumsum(rng.standard_normal((B, L, 3)) * 0.05, 1)
        gt[:, :, 3:] = _unit_quats(rng, B * L).reshape(B, L, 4)
        scale = rng.uniform(0.5, 2.0, B).astype(np.float32)
        out = gn.forward_for_eval({"head_trans": torch.from_numpy(tr), "head_rot_mat": torch.from_numpy(rot),
                                   "ori_head_pose": torch.from_numpy(gt)}, torch.from_numpy(scale))
        for b in range(B):
            ref = O.gravity_eval(sd, window, n_layers, rot[b], tr[b], gt[b], float(scale[b]))
            assert rel(out["pred_normal"][b].cpu(), ref["pred_normal"]) < 1e-4, (L, b)
            e = np.abs(out["head_pose"][b].cpu().numpy() - ref["head_pose"]).max()
            assert e < 2e-4, (L, b, e)


def _demo_like_batch(rng, B, T):
    of, hp, slam = _sequences(rng, B, T)
    ori = (np.cumsum(rng.standard_normal((B, T + 1, 3)) * 0.03, 1)).astype(np.float32)
    rot = O.quat2mat(_unit_quats(rng, B * (T + 1))).astype(np.float32).reshape(B, T + 1, 3, 3)
    return {"of": torch.from_numpy(of), "head_pose": torch.from_numpy(hp), "aligned_slam_trans": torch.from_numpy(slam),
            "ori_slam_trans": torch.from_numpy(ori), "ori_slam_rot_mat": torch.from_numpy(rot)}


def test_stage1_pose_is_batch_invariant():
    """estimate_head_pose: a sequence's whole stage-1 pose is bit-identical alone and among 63 others."""
    s = SETS["demo"]
    hn = stage1.HeadFormer(opt_for(s), "cuda:0")
    hn.load_state_dict(synthetic.make_stage1_weights("headnet", hn.cfg, 21))
    gn = stage1.HeadNormalFormer(opt_for(s), "cuda:0", eval_whole_pipeline=True)
    gn.load_state_dict(synthetic.make_stage1_weights("gravitynet", gn.cfg, 22))
    batch = _demo_like_batch(np.random.default_rng(5), 64, 139)
    allp, _, _ = stage1.estimate_head_pose(hn, gn, batch)
    assert allp.shape == (64, 140, 7) and allp.dtype == torch.float64
    for i in (0, 17, 63):
        one, _, _ = stage1.estimate_head_pose(hn, gn, {k: v[i:i + 1] for k, v in batch.items()})
        assert torch.equal(one[0], allp[i]), i


# ------------------------------------------------------------------------------------------ stage 1 into stage 2
def test_stage1_into_stage2_matches_oracles(g):
    """Config 5 end to end on the demo sequence: the HIP stage-1 head pose (float64, on the GPU, as estimate_head_pose returns it)
    into the stage-2 harness at precision 3, against the stage-1 oracle's pose into oracle/harness_oracle.py, with the same
    injected draws and a 10-step chain (the window-loop golden's setup); final poses within 1e-3."""
    from scipy.spatial.transform import Rotation as Rot

    from egoego_release_amd import ModelConfig, harness, make_weights
    from egoego_release_amd.model import CondGaussianDiffusion
    from oracle import egoego_oracle as EO
    from oracle import harness_oracle as HO

    s = SETS["demo"]
    hn, gn = models(g, "demo")
    hp_hip, _, _ = stage1.estimate_head_pose(hn, gn, batch_of(g))
    assert hp_hip.is_cuda and hp_hip.dtype == torch.float64 and hp_hip.shape == (1, 140, 7)
    sd_h, sd_g = ({k: v.cpu() for k, v in m.state_dict().items()} for m in (hn, gn))
    oh = O.headnet_eval(sd_h, s["window"], s["n_dec_layers"], g["of"], g["head_pose"][0, 3:], g["aligned_slam_trans"], 10.0)
    tr = g["ori_slam_trans"] - g["ori_slam_trans"][0:1]
    og = O.gravity_eval(sd_g, s["normal_window"], s["normal_n_dec_layers"], g["ori_slam_rot_mat"], tr, g["head_pose"], oh["pred_scale"])
    hp_ref = O.assemble(og["head_pose"], oh["head_pose"], g["head_pose"])[None]
    assert np.abs(hp_hip.cpu().numpy() - hp_ref).max() < 2e-4

    wl = np.load(os.path.join(ROOT, "tests", "golden", "window_loop_golden.npz"))
    hg = np.load(os.path.join(ROOT, "tests", "golden", "harness_golden.npz"))
    seq_len, S = int(wl["seq_len"]), int(wl["num_timesteps"])
    cfg = ModelConfig(max_timesteps=seq_len + 1)
    sd = make_weights(cfg, int(wl["weight_seed"]))
    sd["denoise_fn.linear_out.bias"] = torch.from_numpy(wl["linear_out_bias"]).float()
    sd["denoise_fn.linear_out.weight"] = sd["denoise_fn.linear_out.weight"] * float(wl["linear_out_scale"])
    lo, hi = hg["stats_global_jpos_min"], hg["stats_global_jpos_max"]
    ds = harness.SkeletonStats(lo, hi, wl["rest_offsets"], parents=tuple(int(p) for p in wl["parents"]))
    dso = HO.SkeletonOracle(lo, hi, wl["rest_offsets"])
    T = hp_ref.shape[1]
    spans = harness.window_spans(T, seq_len)
    torch.manual_seed(int(wl["seed"]))
    noise = {"x_all": torch.randn(1, T, 198), "cond": [], "steps": []}
    for _, n in spans:
        noise["cond"].append(torch.randn(1, n, 198))
        noise["steps"].append(torch.stack([torch.randn(1, n, 198) for _ in range(S)]))
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    m.num_timesteps = S
    m.hip_precision = 3
    aa, root = harness.full_body_gen_cond_head_pose_sliding_window(m, ds, hp_hip, noise=noise)
    cm = EO.head_condition_mask((1, T, 198))
    aa_ref, root_ref = HO.sliding_window(sd, EO.make_schedule(1000), dso, seq_len, S, hp_ref[..., :3], hp_ref[..., 3:], cm, noise)
    assert aa.shape == aa_ref.shape and root.shape == root_ref.shape
    d_root = np.abs(root.cpu().numpy() - root_ref).max()
    dr = Rot.from_rotvec(aa.cpu().numpy().astype(np.float64).reshape(-1, 3)) * Rot.from_rotvec(aa_ref.reshape(-1, 3)).inv()
    assert d_root < 1e-3, d_root
    assert dr.magnitude().max() < 1e-3, dr.magnitude().max()


def test_driver_runs_the_pipeline(g, tmp_path):
    """tools/run_egoego_demo.py as a child process on a demo folder in the reference's layout (written from the golden's arrays)."""
    import json
    import pickle
    import subprocess
    import sys

    from test_stage1 import write_demo_folder

    data = tmp_path / "ares"
    data.mkdir()
    write_demo_folder(g, data)
    wl = np.load(os.path.join(ROOT, "tests", "golden", "window_loop_golden.npz"))
    hg = np.load(os.path.join(ROOT, "tests", "golden", "harness_golden.npz"))
    with open(tmp_path / "stats.p", "wb") as f:
        pickle.dump({"global_jpos_min": hg["stats_global_jpos_min"], "global_jpos_max": hg["stats_global_jpos_max"]}, f)
    np.save(tmp_path / "rest.npy", wl["rest_offsets"])
    out = tmp_path / "out.npz"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_egoego_demo.py"), "--data_root_folder", str(data),
           "--weight_root_folder", str(tmp_path / "no_weights"), "--stats", str(tmp_path / "stats.p"), "--rest_offsets",
           str(tmp_path / "rest.npy"), "--window", "60", "--normal_window", "120", "--normal_n_dec_layers", "2", "--input_of_feats",
           "--diffusion_window", "120", "--timesteps", "3", "--out", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    rep = json.loads(lines[-1])
    assert rep["stage1_seconds"] > 0 and rep["stage2_seconds"] > 0
    assert all("synthetic" in v for v in rep["weights"].values())
    r = np.load(out)
    assert r["head_pose"].shape == (1, 140, 7)
    assert r["local_aa"].shape == (1, 140, 22, 3) and r["root_trans"].shape == (1, 140, 3)
    assert r["global_jpos"].shape == (1, 140, 22, 3)
    assert all(np.isfinite(r[k]).all() for k in r.files)
