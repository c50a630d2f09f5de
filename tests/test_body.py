"""The SMPL-H body model, the parts that need no GPU: the torch oracle against closed forms and the existing FK, the model
loader, the C struct, the OBJ writer and the skinning-weight compression."""
import math
import os
import re

import numpy as np
import pytest
import torch

import body_oracle as BO
from egoego_release_amd import _lib, body, harness
from egoego_release_amd.synthetic import body_model_parents, make_body_model, make_body_poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 211


@pytest.fixture(scope="module")
def model():
    return make_body_model(3, n_verts=V, n_faces=64, max_weights=4)


@pytest.fixture(scope="module")
def betas():
    return np.random.default_rng(5).uniform(-2, 2, (4, 16)).astype(np.float32)


def test_oracle_identity_pose_is_the_shaped_template(model, betas):
    trans = np.array([[1.5, -2.0, 0.25]] * 4, np.float32)
    o = BO.forward(model, np.zeros((4, 52, 3), np.float32), trans, betas)
    t = torch.from_numpy(trans).double()[:, None]
    assert torch.equal(o["offsets"], torch.zeros_like(o["offsets"]))
    # the fp32 skinning weights of a vertex sum to 1 only to a few ulp: v = (sum w) v_shaped + trans
    wsum = np.abs(model["weights"].astype(np.float64).sum(1) - 1).max()
    assert wsum < 3e-7
    assert (o["v"] - (o["v_shaped"] + t)).abs().max() <= wsum * o["v_shaped"].abs().max() + 1e-14
    assert (o["Jtr"] - (o["J"] + t)).abs().max() < 1e-14
    assert (o["v_shaped"][0] - o["v_shaped"][1]).abs().max() > 1e-3  # the betas matter


def test_oracle_root_rotation_is_rigid_about_joint_0(model, betas):
    aa = np.zeros((2, 52, 3), np.float32)
    aa[:, 0] = [[0.3, -1.1, 0.7], [0.0, 0.0, math.pi / 2]]
    o = BO.forward(model, aa, np.zeros((2, 3), np.float32), betas[:2])
    R = BO.rodrigues(torch.from_numpy(aa[:, 0]).double())
    j0 = o["J"][:, :1]
    wsum = np.abs(model["weights"].astype(np.float64).sum(1) - 1).max()  # see the identity test
    tol = wsum * o["v"].abs().max() + 1e-13  # (sum w - 1) scales the posed vertex
    assert ((R[:, None] @ (o["v_shaped"] - j0)[..., None])[..., 0] + j0 - o["v"]).abs().max() < tol
    assert ((R[:, None] @ (o["J"] - j0)[..., None])[..., 0] + j0 - o["Jtr"]).abs().max() < 1e-13
    # a quarter turn about z: x -> y
    d = o["v_shaped"][1] - j0[1]
    assert (o["v"][1] - j0[1] - torch.stack([-d[:, 1], d[:, 0], d[:, 2]], -1)).abs().max() < tol


def test_oracle_joints_agree_with_the_existing_fk(model, betas):
    aa, trans = make_body_poses(6, 22, seed=2)
    b = np.repeat(betas[:1], 6, 0)
    o = BO.forward(model, aa, trans, b)
    par = BO.parents_of(model)
    assert tuple(par[:22]) == harness.SMPLH_PARENTS_22
    J = o["J"][0]
    rest = J[:22].clone()
    rest[1:] = J[1:22] - J[par[1:22]]
    ds = harness.SkeletonStats(np.zeros((22, 3)), np.ones((22, 3)), rest.float().numpy())
    _, gj = ds.fk_smpl(torch.from_numpy(trans), torch.from_numpy(aa))
    err = (gj.double() - o["Jtr"][:, :22]).abs().max().item()
    print(f"oracle joints vs SkeletonStats.fk_smpl: {err:.3e}")
    assert err < 1e-6 * max(1.0, o["Jtr"].abs().max().item())


def test_fp32_oracle_is_close_to_fp64(model, betas):
    aa, trans = make_body_poses(8, 52, seed=4)
    b = np.repeat(betas, 2, 0)
    o64, o32 = BO.forward(model, aa, trans, b), BO.forward(model, aa, trans, b, dtype=torch.float32)
    for k in ("v", "Jtr"):
        rel = ((o32[k].double() - o64[k]).abs().max() / o64[k].abs().max()).item()
        print(f"fp32 oracle {k}: {rel:.3e} of max |fp64|")
        assert rel < 1e-5


def test_rodrigues_matches_the_package_and_is_exact_at_zero():
    from egoego_release_amd import rotations
    aa = torch.from_numpy(make_body_poses(5, 7, seed=1)[0]).double()
    assert (BO.rodrigues(aa) - rotations.axis_angle_to_matrix(aa)).abs().max() < 1e-12
    assert torch.equal(BO.rodrigues(torch.zeros(2, 3, dtype=torch.float64)), torch.eye(3, dtype=torch.float64).expand(2, 3, 3))


# ---------------------------------------------------------------------------------------------- loader
def test_npz_round_trips_through_the_loader(model, tmp_path):
    path = tmp_path / "male" / "model.npz"
    path.parent.mkdir()
    np.savez(path, **model)
    a = body.load_model_arrays(str(path))
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"):
        assert a[k].dtype == np.float32 and np.array_equal(a[k], model[k]), k
    assert np.array_equal(a["f"], model["f"].astype(np.int32)) and a["f"].dtype == np.int32
    assert a["parents"][0] == -1 and np.array_equal(a["parents"], body_model_parents())
    bm = body.BodyModel(bm_fname=str(path), device="cpu")
    assert isinstance(bm, torch.nn.Module) and bm.num_betas == 16
    assert torch.equal(bm.posedirs, torch.from_numpy(model["posedirs"])) and tuple(bm.f.shape) == (64, 3)
    bm2 = body.BodyModel(model=model, device="cpu")
    assert all(torch.equal(x, y) for x, y in zip(bm.buffers(), bm2.buffers()))


def test_num_betas_truncates(model):
    bm = body.BodyModel(model=model, num_betas=10, device="cpu")
    assert bm.num_betas == 10 and tuple(bm.shapedirs.shape) == (V, 3, 10)
    assert torch.equal(bm.shapedirs, torch.from_numpy(model["shapedirs"][:, :, :10]))
    jt, jsd = body.regress_joints(bm.J_regressor.numpy(), bm.v_template.numpy(), bm.shapedirs.numpy())
    assert jt.shape == (52, 3) and jsd.shape == (52, 3, 10) and jt.dtype == np.float32
    assert np.abs(jt - model["J_regressor"].astype(np.float64) @ model["v_template"].astype(np.float64)).max() < 1e-7


def test_bad_models_are_refused_with_a_clear_error(model):
    m = dict(model)
    kt = model["kintree_table"].copy()
    kt[0, 5] = 9  # a parent after its child
    m["kintree_table"] = kt
    with pytest.raises(ValueError, match="parent of joint 5 is 9.*precede"):
        body.BodyModel(model=m, device="cpu")
    m = dict(model)
    m["kintree_table"] = model["kintree_table"][:, :24]  # SMPL, not SMPL-H
    with pytest.raises(ValueError, match=r"kintree_table \(2, 24\).*52"):
        body.BodyModel(model=m, device="cpu")
    m = dict(model)
    m["posedirs"] = model["posedirs"][:, :, :207]
    with pytest.raises(ValueError, match="posedirs.*459"):
        body.BodyModel(model=m, device="cpu")
    m = dict(model)
    del m["weights"]
    with pytest.raises(ValueError, match="missing.*weights"):
        body.BodyModel(model=m, device="cpu")
    with pytest.raises(ValueError, match="either bm_fname or model"):
        body.BodyModel()


def test_there_is_no_cpu_path(model):
    bm = body.BodyModel(model=model, device="cpu")
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        bm(root_orient=torch.zeros(1, 3))


# ---------------------------------------------------------------------------------------------- header
def test_body_model_struct_matches_the_header():
    src = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    blk = src[src.index("typedef struct {", src.index("typedef struct egoego_body_ctx")):src.index("} egoego_body_model;")]
    blk = re.sub(r"/\*.*?\*/", "", blk, flags=re.S)
    fields = re.findall(r"^\s*(int32_t|const float\*|const int32_t\*)\s*(\w+);", blk, flags=re.M)
    ctype = {"int32_t": _lib.C.c_int32, "const float*": _lib.C.c_void_p, "const int32_t*": _lib.C.c_void_p}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.BodyModelDesc._fields_)
    assert len(fields) == 11
    assert int(re.search(r"#define EGOEGO_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 8
    for name in ("egoego_body_ctx_create", "egoego_body_ctx_destroy", "egoego_body_load_model", "egoego_body_workspace_bytes",
                 "egoego_body_forward", "egoego_body_last_error"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, src), name
    assert _lib.BODY_N_JOINTS == 52 and _lib.BODY_POSE_FEATS == 459


# ---------------------------------------------------------------------------------------------- OBJ files
@pytest.mark.parametrize("gt", [False, True])
def test_mesh_files_are_parseable_obj(tmp_path, gt):
    g = np.random.default_rng(0)
    verts = g.standard_normal((3, 17, 3)).astype(np.float32)
    faces = g.integers(0, 17, (9, 3))
    faces[0] = [0, 16, 5]
    folder = tmp_path / "seq" / "objs"
    body.save_verts_faces_to_mesh_file(torch.from_numpy(verts), torch.from_numpy(faces), str(folder), save_gt=gt)
    assert sorted(os.listdir(folder)) == ["%05d%s.obj" % (i, "_gt" if gt else "") for i in range(3)]
    for i in range(3):
        lines = open(folder / ("%05d%s.obj" % (i, "_gt" if gt else ""))).read().splitlines()
        v = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("v ")])
        f = np.array([[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("f ")])
        assert len(lines) == 17 + 9 and v.shape == (17, 3) and f.shape == (9, 3)
        assert np.abs(v - verts[i]).max() < 1e-7
        assert np.array_equal(f, faces + 1) and f.min() >= 1 and f.max() <= 17


# ---------------------------------------------------------------------------------------------- weight compression
@pytest.mark.parametrize("nw", [1, 4, 52])
def test_weight_compression_reproduces_the_dense_blend(nw):
    m = make_body_model(nw, n_verts=V, n_faces=8, max_weights=nw)
    w = m["weights"]
    assert (w != 0).sum(1).max() == nw and np.abs(w.sum(1) - 1).max() < 1e-6
    sj, sw = body.compress_weights(w)
    assert sj.shape == sw.shape == (nw, V) and sj.dtype == np.int32 and sw.dtype == np.float32
    assert sj.min() >= 0 and sj.max() < 52
    back = np.zeros_like(w)
    for k in range(nw):
        keep = sw[k] != 0
        assert (back[np.flatnonzero(keep), sj[k, keep]] == 0).all()  # no joint twice
        back[np.flatnonzero(keep), sj[k, keep]] = sw[k, keep]
    assert np.array_equal(back, w)
    assert all((np.diff(sj[:, v][sw[:, v] != 0]) > 0).all() for v in range(V))  # joint order
    assert (sj[sw == 0] == 0).all()  # padding
    # the blend of fp32 matrices, joints summed in order: bit-equal
    A = np.random.default_rng(1).standard_normal((52, 12)).astype(np.float32)
    dense = np.zeros((V, 12), np.float32)
    for j in range(52):
        dense += w[:, j:j + 1] * A[j]
    sparse = np.zeros((V, 12), np.float32)
    for k in range(nw):
        sparse += sw[k][:, None] * A[sj[k]]
    assert np.array_equal(dense, sparse)
