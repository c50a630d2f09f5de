"""The SMPL-H body model on the GPU against the fp64 torch oracle (tests/body_oracle.py), its bit-exactness properties, one
full-size run and the driver.

Accuracy figures are max |HIP - fp64| / max |fp64| per quantity.  CEILING is the bar the project holds its split-bf16 stages to;
where the measured worst value is more than 10x under it, the assertion is 4x that measured value (the margin covers poses the
test does not draw).  Measured worst values over the cases below on an MI355X: MEASURED (pose offsets 5.5e-6, final vertices
3.9e-7, joints 2.4e-7; the worst of each falls on an F = 1 case, where max |fp64| is taken over a single frame).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import body_oracle as BO
from egoego_release_amd import body
from egoego_release_amd.synthetic import make_body_model, make_body_poses

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 211            # no multiple of 32 nor of 96
F_ALL = 70
SEQ = np.repeat(np.arange(3), [10, 25, 35])  # sequence boundaries inside the first M tile
CEILING = 5e-5
# measured worst figures (this file's parity, run_smpl_model and full-size cases).  The pose offsets are 9x under the ceiling,
# not more than 10x, so they keep the ceiling; vertices and joints are asserted at 4x their measured worst.
MEASURED = {"offsets": 5.534e-06, "v": 3.922e-07, "Jtr": 2.386e-07}


def bound(q):
    m = MEASURED[q]
    return 4 * m if m is not None and m < CEILING / 10 else CEILING


def rel(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(scope="module")
def models():
    return {nw: make_body_model(10 + nw, n_verts=V, n_faces=40, max_weights=nw) for nw in (4, 52)}


@pytest.fixture(scope="module")
def inputs():
    aa, trans = make_body_poses(F_ALL, 52, seed=7)
    betas = np.random.default_rng(8).uniform(-2.5, 2.5, (3, 16)).astype(np.float32)
    return aa, trans, betas


@pytest.fixture(scope="module")
def oracle(models, inputs):
    """fp64 results of all 70 frames, per (max_weights, joints); frames are independent, so a shorter call compares to a slice."""
    aa, trans, betas = inputs
    return {(nw, nj): BO.forward(models[nw], aa[:, :nj], trans, betas[SEQ]) for nw in (4, 52) for nj in (22, 52)}


@pytest.fixture(scope="module")
def bms(models):
    return {nw: body.BodyModel(model=models[nw], device="cuda") for nw in (4, 52)}


def run(bm, aa, trans, betas, seq, nj, offsets=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return bm(root_orient=t(aa[:, 0]), pose_body=t(aa[:, 1:22].reshape(len(aa), 63)),
              pose_hand=t(aa[:, 22:].reshape(len(aa), 90)) if nj == 52 else None, betas=t(betas), trans=t(trans),
              seq_index=t(seq.astype(np.int32)), return_pose_offsets=offsets)


@pytest.mark.parametrize("F", [1, 33, 70])
@pytest.mark.parametrize("nj", [22, 52])
@pytest.mark.parametrize("nw", [4, 52])
def test_parity_with_the_fp64_oracle(bms, inputs, oracle, nw, nj, F):
    aa, trans, betas = inputs
    sel = np.arange(F_ALL)[-F:] if F < F_ALL else np.arange(F_ALL)  # the last F frames: F = 33 starts in sequence 2
    out = run(bms[nw], aa[sel], trans[sel], betas, SEQ[sel], nj)
    ref = oracle[(nw, nj)]
    assert out.v.shape == (F, V, 3) and out.Jtr.shape == (F, 52, 3) and out.f.shape == (40, 3)
    fig = {"offsets": rel(out.pose_offsets, ref["offsets"][sel]), "v": rel(out.v, ref["v"][sel]), "Jtr": rel(out.Jtr, ref["Jtr"][sel])}
    print(f"body parity nw={nw} nj={nj} F={F}: " + json.dumps({k: float(f"{x:.3e}") for k, x in fig.items()}))
    for k, x in fig.items():
        assert x < bound(k), (k, x, bound(k))


@pytest.mark.parametrize("nj", [22, 52])
def test_run_smpl_model_two_genders_interleaved(models, bms, nj):
    BS, T = 4, 9
    aa, trans = make_body_poses(BS * T, nj, seed=21)
    betas = np.random.default_rng(22).uniform(-2, 2, (BS, 16)).astype(np.float32)
    gender = ["female", "male", "male", "female"]
    bm_dict = {"male": bms[4], "female": bms[52]}
    jn, vt, faces = body.run_smpl_model(torch.from_numpy(trans).reshape(BS, T, 3), torch.from_numpy(aa).reshape(BS, T, nj, 3),
                                        torch.from_numpy(betas), gender, bm_dict)
    assert jn.shape == (BS, T, nj, 3) and vt.shape == (BS, T, V, 3) and torch.equal(faces.cpu(), bms[52].f.cpu())
    fig = {"v": 0.0, "Jtr": 0.0}
    for i, g in enumerate(gender):
        ref = BO.forward(models[4 if g == "male" else 52], aa[i * T:(i + 1) * T], trans[i * T:(i + 1) * T], np.repeat(betas[i:i + 1], T, 0))
        fig["v"] = max(fig["v"], rel(vt[i], ref["v"]))
        fig["Jtr"] = max(fig["Jtr"], rel(jn[i], ref["Jtr"][:, :nj]))
    print(f"body run_smpl_model nj={nj}: " + json.dumps({k: float(f"{x:.3e}") for k, x in fig.items()}))
    for k, x in fig.items():
        assert x < bound(k), (k, x, bound(k))


def test_a_frame_is_bit_identical_alone_anywhere_and_across_chunks(models, bms, inputs):
    aa, trans, betas = inputs
    base = run(bms[4], aa, trans, betas, SEQ, 52)
    perm = np.random.default_rng(3).permutation(F_ALL)
    moved = run(bms[4], aa[perm], trans[perm], betas, SEQ[perm], 52)
    for k in ("v", "Jtr", "pose_offsets"):
        assert torch.equal(getattr(moved, k), getattr(base, k)[torch.from_numpy(perm).cuda()]), k
    for f in (0, 37, 69):
        one = run(bms[4], aa[f:f + 1], trans[f:f + 1], betas, SEQ[f:f + 1], 52)
        assert torch.equal(one.v[0], base.v[f]) and torch.equal(one.Jtr[0], base.Jtr[f]), f
    chunked = body.BodyModel(model=models[4], device="cuda", chunk_frames=5)
    c = run(chunked, aa, trans, betas, SEQ, 52)
    for k in ("v", "Jtr", "pose_offsets"):
        assert torch.equal(getattr(c, k), getattr(base, k)), k


@pytest.mark.parametrize("nw", [4, 52])
def test_22_joint_call_is_bit_identical_to_a_zero_hand_pose(bms, inputs, nw):
    aa, trans, betas = inputs
    padded = aa.copy()
    padded[:, 22:] = 0
    a, b = run(bms[nw], aa, trans, betas, SEQ, 22), run(bms[nw], padded, trans, betas, SEQ, 52)
    for k in ("v", "Jtr", "pose_offsets"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not torch.equal(a.v, run(bms[nw], aa, trans, betas, SEQ, 52, offsets=False).v)  # the hands do matter


def test_betas_per_frame_as_the_reference_passes_them(bms, inputs):
    aa, trans, betas = inputs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    a = run(bms[4], aa, trans, betas, SEQ, 52, offsets=False)
    b = bms[4](root_orient=t(aa[:, 0]), pose_body=t(aa[:, 1:22].reshape(F_ALL, 63)), pose_hand=t(aa[:, 22:].reshape(F_ALL, 90)),
               betas=t(betas[SEQ]), trans=t(trans))
    assert torch.equal(a.v, b.v) and torch.equal(a.Jtr, b.Jtr)
    with pytest.raises(ValueError, match="seq_index spans"):
        run(bms[4], aa, trans, betas[:2], SEQ, 52)


def test_full_size_model_once():
    m = make_body_model(1)
    assert m["v_template"].shape == (6890, 3) and m["f"].shape == (13776, 3)
    aa, trans = make_body_poses(3, 52, seed=31)
    betas = np.random.default_rng(32).uniform(-2, 2, (3, 16)).astype(np.float32)
    bm = body.BodyModel(model=m, device="cuda")
    out = run(bm, aa, trans, betas, np.arange(3), 52)
    ref = BO.forward(m, aa, trans, betas)
    fig = {"offsets": rel(out.pose_offsets, ref["offsets"]), "v": rel(out.v, ref["v"]), "Jtr": rel(out.Jtr, ref["Jtr"])}
    print("body full size V=6890 F=3: " + json.dumps({k: float(f"{x:.3e}") for k, x in fig.items()}))
    assert out.v.shape == (3, 6890, 3) and torch.isfinite(out.v).all()
    for k, x in fig.items():
        assert x < bound(k), (k, x, bound(k))


def test_driver_writes_the_meshes(tmp_path):
    """tools/run_egoego_demo.py --body_model --gen_vis as a child process: mesh_verts, mesh_jnts and one OBJ per frame."""
    import pickle

    from test_stage1 import write_demo_folder

    g = np.load(os.path.join(ROOT, "tests", "golden", "stage1_golden.npz"))
    hg = np.load(os.path.join(ROOT, "tests", "golden", "harness_golden.npz"))
    data = tmp_path / "ares"
    data.mkdir()
    write_demo_folder(g, data)
    m = make_body_model(0)
    (tmp_path / "smplh" / "male").mkdir(parents=True)
    np.savez(tmp_path / "smplh" / "male" / "model.npz", **m)
    # the skeleton the FK runs on is the body model's own rest pose (zero betas), so both stages describe one body
    jt, _ = body.regress_joints(m["J_regressor"], m["v_template"], m["shapedirs"])
    par = BO.parents_of(m)
    rest = jt[:22].copy()
    rest[1:] = jt[1:22] - jt[par[1:22]]
    np.save(tmp_path / "rest.npy", rest)
    with open(tmp_path / "stats.p", "wb") as f:
        pickle.dump({"global_jpos_min": hg["stats_global_jpos_min"], "global_jpos_max": hg["stats_global_jpos_max"]}, f)
    out = tmp_path / "out.npz"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_egoego_demo.py"), "--data_root_folder", str(data),
           "--weight_root_folder", str(tmp_path / "no_weights"), "--stats", str(tmp_path / "stats.p"), "--rest_offsets",
           str(tmp_path / "rest.npy"), "--window", "60", "--normal_window", "120", "--normal_n_dec_layers", "2", "--input_of_feats",
           "--diffusion_window", "120", "--timesteps", "3", "--out", str(out), "--gen_vis", "--body_model", str(tmp_path / "smplh")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert not any("visualisation" in s for s in rep["not_done"]) and any("Blender" in s for s in rep["not_done"])
    r = np.load(out)
    T = r["global_jpos"].shape[1]
    assert r["mesh_verts"].shape == (T, 6890, 3) and r["mesh_jnts"].shape == (T, 22, 3)
    assert np.isfinite(r["mesh_verts"]).all()
    # the mesh joints are the FK joints moved by the tool's xy shift, plus the root's rest position the reference adds twice
    d = r["mesh_jnts"].astype(np.float64) - r["global_jpos"][0] - r["mesh_shift"]
    assert r["mesh_shift"][2] == 0
    # (fk_smpl is held to 1e-6 of the fp64 oracle in test_body.py, the HIP joints to bound("Jtr"))
    assert np.abs(d - jt[0]).max() < (1e-6 + bound("Jtr")) * max(1.0, np.abs(r["global_jpos"]).max())
    objs = sorted(os.listdir(rep["mesh_folders"][0]))
    assert objs == ["%05d.obj" % i for i in range(T)]
    first = open(os.path.join(rep["mesh_folders"][0], objs[0])).read().splitlines()
    assert sum(ln.startswith("v ") for ln in first) == 6890 and sum(ln.startswith("f ") for ln in first) == 13776
