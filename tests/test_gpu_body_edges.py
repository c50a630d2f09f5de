"""The SMPL-H body model on the GPU at rotation edges, at the zero pose, at small angles and at tile and shape edges, against the
fp64 oracle (tests/body_oracle.py); the poses are tests/rotation_edge_cases.body_edge_poses().

The figure is test_gpu_body.py's: max |HIP - fp64| / max |fp64| per quantity over the call.  The bar per quantity is computed on
the CPU for the same inputs,
    min(CEILING, 2 (e_emul + e_32)),
e_emul: the oracle with posedirs and the pose features read as hi + lo bf16 and an exact accumulation (forward(split_offsets=
True)); e_32: the oracle in fp32 (forward(dtype=float32)).  The kernel carries both the operand rounding and an fp32 accumulation,
hence the sum; the factor 2 allows for another order of the same roundings.  For a frame whose every angle is <= 1e-4 the same
figure and bar are taken per frame (max |fp64 offsets of that frame| in the denominator): over a whole call such a frame's
offsets, 1e-6 and less, vanish under the ordinary frames', and its error could not be seen at all.

Measured on an MI355X (profiles/rotation_edges_error.json; EGOEGO_EDGES_RECORD=<file> writes it), worst figure / its bar: pose
offsets 5.603e-06 / 1.237e-05 (edge poses, 52 weights, 22 joints), vertices 2.023e-07 / 4.147e-07 (V = 129, F = 31), joints
1.269e-07 / 1.449e-07 (V = 52, F = 31), a single small-angle frame 1.241e-05 / 2.480e-05.  Every figure also stays inside
test_gpu_body.bound() (5e-5, 1.57e-06, 9.5e-07), which is not raised.
"""
import numpy as np
import pytest
import torch

import body_oracle as BO
import rotation_edge_cases as RC
from egoego_release_amd import body
from egoego_release_amd.synthetic import make_body_model
from test_gpu_body import CEILING, bound, run

pytestmark = pytest.mark.gpu
QUANTITIES = {"offsets": "pose_offsets", "v": "v", "Jtr": "Jtr"}
F_TILES = (31, 32, 63, 64, 65, 96, 97)
V_SHAPES = (52, 128, 129)


def rel(got, ref):
    return ((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max()).item()


def oracles(model, aa, trans, betas, num_betas=16):
    """-> (fp64, emulated split-bf16, fp32) forward dicts"""
    return (BO.forward(model, aa, trans, betas, num_betas=num_betas),
            BO.forward(model, aa, trans, betas, num_betas=num_betas, split_offsets=True),
            BO.forward(model, aa, trans, betas, dtype=torch.float32, num_betas=num_betas))


def bars(orc, sel=slice(None)):
    r64, emul, f32 = orc
    return {k: min(CEILING, 2 * (rel(emul[k][sel], r64[k][sel]) + rel(f32[k][sel], r64[k][sel]))) for k in QUANTITIES}


def check(case, out, orc, sel=slice(None)):
    bar = bars(orc, sel)
    fig = {k: rel(getattr(out, a), orc[0][k][sel]) for k, a in QUANTITIES.items()}
    print(case, {k: "%.3e / %.3e" % (fig[k], bar[k]) for k in fig})
    RC.record(case, figure=fig, bar=bar, inside_test_gpu_body_bound={k: bool(fig[k] < bound(k)) for k in fig})
    for k in fig:
        assert fig[k] <= bar[k], (case, k, fig[k], bar[k])
    return fig


@pytest.fixture(scope="module")
def betas():
    return np.random.default_rng(81).uniform(-2.5, 2.5, (3, 16)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ edge poses
@pytest.fixture(scope="module")
def edge_models():
    return {nw: make_body_model(10 + nw, n_verts=211, n_faces=40, max_weights=nw) for nw in (4, 52)}


@pytest.mark.parametrize("nj", [22, 52])
@pytest.mark.parametrize("nw", [4, 52])
def test_edge_poses_against_the_fp64_oracle(edge_models, betas, nw, nj):
    """Each vector of axis_angles() in turn on the root, on body joints 2, 9, 16, 21 and on hand joints 25 and 51 (at rest in the
    22-joint call), interleaved with ordinary frames; then the small-angle frames one by one."""
    p = RC.body_edge_poses()
    aa, trans = p["aa"][:, :nj], p["trans"]
    seq = np.arange(aa.shape[0]) % 3
    orc = oracles(edge_models[nw], aa, trans, betas[seq])
    out = run(body.BodyModel(model=edge_models[nw], device="cuda"), aa, trans, betas, seq, nj)
    check(f"edge_poses nw={nw} nj={nj}", out, orc)
    r64, emul, f32 = (o["offsets"] for o in orc)
    got = out.pose_offsets.double().cpu()
    worst, n_zero = (0.0, 0.0, -1), 0
    for f in np.flatnonzero(p["small"]):
        den = r64[f].abs().max().item()
        if den == 0:  # the root's rotation is no pose feature; a zero vector; a hand joint in the 22-joint call
            assert not got[f].any() and not emul[f].any() and not f32[f].any(), f
            n_zero += 1
            continue
        fig = (got[f] - r64[f]).abs().max().item() / den
        bar = min(CEILING, 2 * ((emul[f] - r64[f]).abs().max().item() + (f32[f].double() - r64[f]).abs().max().item()) / den)
        assert fig <= bar, (f, fig, bar, den)
        if fig / bar > worst[0] / max(worst[1], 1e-300):
            worst = (fig, bar, int(f))
    print(f"small-angle frames nw={nw} nj={nj}: worst per-frame figure {worst[0]:.3e} under {worst[1]:.3e} (frame {worst[2]}), {n_zero} exact zeros")
    RC.record(f"small_angle_frames nw={nw} nj={nj}", worst_figure=worst[0], its_bar=worst[1], frame=worst[2], exact_zero_frames=n_zero)
    assert n_zero == (6 * 6 + 6 * 6 + (2 * 5 * 6 if nj == 22 else 0))  # the root's and the zero vector's (+ the hands')


def test_zero_pose_has_exactly_zero_offsets(edge_models, betas):
    F = 33
    aa = np.zeros((F, 52, 3), np.float32)
    trans = RC.body_edge_poses()["trans"][:F]
    seq = np.arange(F) % 3
    bm = body.BodyModel(model=edge_models[4], device="cuda")
    a, b = run(bm, aa, trans, betas, seq, 22), run(bm, aa, trans, betas, seq, 52)
    assert not a.pose_offsets.any() and not b.pose_offsets.any()
    assert not torch.signbit(a.pose_offsets).any() and not torch.signbit(b.pose_offsets).any()  # 0.0, not -0.0
    for k in QUANTITIES.values():
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    ref = BO.forward(edge_models[4], aa, trans, betas[seq])
    assert not ref["offsets"].any() and rel(a.v, ref["v"]) < bound("v") and rel(a.Jtr, ref["Jtr"]) < bound("Jtr")


# ------------------------------------------------------------------------------------------------ tile and shape edges
@pytest.fixture(scope="module")
def shape_cases(betas):
    """Per V: the model, 97 frames (every third an edge frame) and their three oracles; a call of F frames compares to a slice."""
    p = RC.body_edge_poses()
    pick = np.arange(97) * 11 % 1092  # 11 is odd: edge and ordinary frames alternate, the edge frames walk through the set
    aa, trans = p["aa"][pick], p["trans"][pick]
    seq = np.arange(97) % 3
    out = {}
    for V in V_SHAPES:
        m = make_body_model(20 + V, n_verts=V, n_faces=8, max_weights=4)
        out[V] = {"model": m, "aa": aa, "trans": trans, "seq": seq, "orc": oracles(m, aa, trans, betas[seq])}
    return out


@pytest.mark.parametrize("V", V_SHAPES)
def test_tile_and_vertex_group_edges(shape_cases, betas, V):
    """F around the 32-frame tile: 31, 32, 63, 64, 65, 96, 97.  V = 52: two vertex groups, half of a workgroup's waves leave at
    once; V = 128: one workgroup and no padded vertex; V = 129: one vertex in the last group."""
    c = shape_cases[V]
    bm = body.BodyModel(model=c["model"], device="cuda")
    for F in F_TILES:
        out = run(bm, c["aa"][:F], c["trans"][:F], betas, c["seq"][:F], 52)
        assert out.v.shape == (F, V, 3)
        check(f"tiles V={V} F={F}", out, c["orc"], slice(0, F))


@pytest.mark.parametrize("chunk", [32, 33, 64])
def test_chunked_calls_carry_the_same_bits(shape_cases, betas, chunk):
    """97 frames in chunks of 32 (whole tiles), 33 (a second tile with one live row) and 64."""
    c = shape_cases[129]
    base = run(body.BodyModel(model=c["model"], device="cuda"), c["aa"], c["trans"], betas, c["seq"], 52)
    got = run(body.BodyModel(model=c["model"], device="cuda", chunk_frames=chunk), c["aa"], c["trans"], betas, c["seq"], 52)
    for k in QUANTITIES.values():
        assert torch.equal(getattr(got, k), getattr(base, k)), k


@pytest.mark.parametrize("nb", [0, 10])
def test_fewer_betas(shape_cases, betas, nb):
    c = shape_cases[129]
    F = 65
    bm = body.BodyModel(model=c["model"], num_betas=nb, device="cuda")
    assert bm.num_betas == nb
    out = run(bm, c["aa"][:F], c["trans"][:F], betas[:, :nb], c["seq"][:F], 52)
    check(f"num_betas={nb}", out, oracles(c["model"], c["aa"][:F], c["trans"][:F], betas[c["seq"][:F], :nb], num_betas=nb))
    if nb == 0:  # no shape direction at all: the bits of the full model at zero betas
        full = run(body.BodyModel(model=c["model"], device="cuda"), c["aa"][:F], c["trans"][:F], np.zeros((3, 16), np.float32), c["seq"][:F], 52)
        for k in QUANTITIES.values():
            assert torch.equal(getattr(out, k), getattr(full, k)), k
