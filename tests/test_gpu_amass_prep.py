"""The AMASS preprocessing on the GPU (egoego_amass_*; egoego_release_amd/amass_prep.py over csrc/amass_prep.h) against the
recorded results of the reference's own process_seq (tests/golden/amass_golden.npz), the fp64 oracle (tests/amass_oracle.py), the
existing evaluation entry and itself: the long path of the floor kernel, packing, the workspace, the stream, the limits and the
tool end to end.

Continuous outputs are measured as the worst |a - b| over the largest |b| per sequence against the fp64 oracle; the bound is 4 x
the kernels' measured figure (KERNEL_DISTANCE, MI355X) and never more than 4 x the reference's own distance from that oracle
(amass_oracle.REFERENCE_DISTANCE), the rule of DESIGN 5f.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amass_oracle as O  # noqa: E402
import eval_cases  # noqa: E402
import eval_oracle  # noqa: E402
import stream_cases as SC  # noqa: E402
from egoego_release_amd import _lib, amass_prep as A, body, evaluate, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "amass_golden.npz")

# worst relative difference of the kernels from the fp64 oracle over the golden sequences, measured on an MI355X
KERNEL_DISTANCE = {"joints": 7.833e-08, "head_qpos": 5.248e-08, "head_vels": 6.811e-05, "global_head_rot_6d": 2.980e-08,
                   "global_head_rot_6d_diff": 8.397e-08, "global_head_trans": 5.248e-08, "global_head_trans_diff": 2.856e-06,
                   "joints_vs_body_model": 0.0}  # the body model's Jtr[:, :22] and these joints carry the same bits


def bound(key, ref_key=None):
    return min(4 * KERNEL_DISTANCE[key], 4 * O.REFERENCE_DISTANCE[ref_key or key])


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    seed, n_verts, n_faces = (int(v) for v in z["model"])
    model = synthetic.make_body_model(seed, n_verts=n_verts, n_faces=n_faces)
    seqs, oracle = [], {}
    for name in z["names"]:
        s = {"path": str(z[name + "/path"]), "poses": z[name + "/poses"].astype(np.float64), "trans": z[name + "/trans"].astype(np.float64),
             "mocap_framerate": z[name + "/mocap_framerate"]}
        seqs.append(s)
        oracle[name] = O.process_seq(model, s["path"], s["poses"], s["trans"], s["mocap_framerate"])
    return {"z": z, "model": model, "names": [str(n) for n in z["names"]], "seqs": seqs, "oracle": oracle}


@pytest.fixture(scope="module")
def records(gold):
    return A.process_sequences(gold["seqs"], gold["model"])


def raw_inputs(gold, name):
    """The trimmed raw frames of a golden sequence -> (root_orient, pose_body, trans float32 arrays, the corrected fps)."""
    s = gold["seqs"][gold["names"].index(name)]
    lo, hi = A.trim_range(s["poses"].shape[0])
    p, t = s["poses"][lo:hi].astype(np.float32), s["trans"][lo:hi].astype(np.float32)
    return p[:, :3], p[:, 3:66], t, float(A.corrected_fps(s["path"], s["mocap_framerate"]))


# ------------------------------------------------------------------------------------------------ the golden records
def test_golden_reasons_keys_shapes_and_dtypes(gold, records):
    z = gold["z"]
    for name, rec in zip(gold["names"], records):
        want = str(z[name + "/result"])
        if want != "kept":
            assert rec == want, name
            continue
        assert tuple(rec) == A.RECORD_KEYS == O.RECORD_KEYS, name
        for k in A.RECORD_KEYS:
            ref = z[name + "/ref/" + k]
            assert np.asarray(rec[k]).shape == ref.shape, (name, k)
            assert str(np.asarray(rec[k]).dtype) == str(z[name + "/dtype/" + k]), (name, k, np.asarray(rec[k]).dtype)


def test_golden_exact_parts(gold, records):
    """contacts, floor_height and the float64 copies equal the reference's bit for bit."""
    z = gold["z"]
    for name, rec in zip(gold["names"], records):
        if str(z[name + "/result"]) != "kept":
            continue
        assert np.array_equal(rec["contacts"], z[name + "/ref/contacts"].astype(np.float64)), name
        assert np.asarray(rec["floor_height"]).tobytes() == z[name + "/ref/floor_height"].tobytes(), name
        for k in ("trans", "root_orient", "pose_body", "betas"):
            assert np.asarray(rec[k]).tobytes() == z[name + "/ref/" + k].tobytes(), (name, k)
        assert int(rec["fps"]) == int(z[name + "/ref/fps"]) and str(rec["gender"]) == str(z[name + "/ref/gender"])
        assert A.record_file_name("x", rec) == "x_%d_frames_%d_fps.npz" % (z[name + "/ref/trans"].shape[0], int(z[name + "/ref/fps"]))


def test_golden_labels_and_discard_flag(gold):
    """The DBSCAN labels sklearn gave inside the reference's run, the discard flag and the group count, through the two stages."""
    z = gold["z"]
    for name in gold["names"]:
        if str(z[name + "/result"]) == "short":
            continue
        ro, pb, tr, fps = raw_inputs(gold, name)
        joints, _ = A.body_joints(dev(ro), dev(pb), dev(tr), gold["model"])
        _, _, discard, det = A.floor_and_contacts(joints, [0, ro.shape[0]], fps, return_details=True)
        n = int(det["n_static"][0])
        want = z[name + "/labels"]
        assert n == want.size and np.array_equal(det["labels"][:n].cpu().numpy(), want), name
        assert bool(discard[0]) == (str(z[name + "/result"]) == "terrain"), name
        assert int(det["n_groups"][0]) == np.unique(want).size, name


def test_golden_continuous_keys(gold, records):
    worst = {k: 0.0 for k in O.CONTINUOUS_KEYS}
    ref = {k: 0.0 for k in O.CONTINUOUS_KEYS}
    for name, rec in zip(gold["names"], records):
        if not isinstance(rec, dict):
            continue
        orc = gold["oracle"][name][0]
        for k in O.CONTINUOUS_KEYS:
            worst[k] = max(worst[k], O.rel_diff(rec[k], orc[k]))
            ref[k] = max(ref[k], O.rel_diff(gold["z"][name + "/ref/" + k], orc[k]))
    for k in O.CONTINUOUS_KEYS:
        print(f"{k:26s} kernels {worst[k]:.3e}   reference {ref[k]:.3e}   bound {bound(k):.3e}")
    for k in O.CONTINUOUS_KEYS:
        assert worst[k] <= bound(k), (k, worst[k], bound(k))


def test_joints_against_the_body_model(gold):
    """body.BodyModel(...).Jtr[:, :22] at zero betas, with and without a hand pose: the 22 joints do not depend on it."""
    ro, pb, tr, _ = raw_inputs(gold, "kept_60")
    joints, head_rot = A.body_joints(dev(ro), dev(pb), dev(tr), gold["model"])
    bm = body.BodyModel(model=gold["model"], device="cuda")
    hand = torch.from_numpy(synthetic.make_body_poses(ro.shape[0], 30, 1)[0].reshape(ro.shape[0], 90)).cuda()
    via_model = A.body_joints(dev(ro), dev(pb), dev(tr), bm)[0]
    assert torch.equal(via_model, joints)  # the module and its arrays give one skeleton
    j64, R64 = O.joints_and_head_rot(gold["model"], ro, pb, tr)
    for pose_hand in (None, hand):
        Jtr = bm(root_orient=dev(ro), pose_body=dev(pb), pose_hand=pose_hand, trans=dev(tr)).Jtr[:, :22]
        d_model = O.rel_diff(Jtr.cpu().numpy(), j64)
        d = O.rel_diff(joints.cpu().numpy(), Jtr.cpu().numpy())
        print(f"joints: kernels vs the body model {d:.3e}   the body model vs the oracle {d_model:.3e}   bound {bound('joints_vs_body_model', 'joints'):.3e}")
        assert d <= bound("joints_vs_body_model", "joints")
    assert O.rel_diff(joints.cpu().numpy(), j64) <= bound("joints")
    assert O.rel_diff(head_rot.cpu().numpy(), R64) <= bound("global_head_rot_6d")


# ------------------------------------------------------------------------------------------------ the long path
@pytest.fixture(scope="module")
def long_cases():
    return {T: eval_cases.long_case(T, 0) for T in (4096, 4097, 5000, 9001)}


def details_of(joints, offsets, fps, **kw):
    off, contacts, discard, det = A.floor_and_contacts(joints, offsets, fps, return_details=True, **kw)
    return {"offset": off, "contacts": contacts, "discard": discard, **det}


@pytest.mark.parametrize("T", [4097, 5000, 9001])
def test_long_sequences_equal_the_oracle(long_cases, T):
    j = long_cases[T]
    o = eval_oracle.floor_and_contacts(j, 120)
    d = details_of(dev(j), [0, T], 120)
    n = int(d["n_static"][0])
    assert n == o["labels"].size > T
    assert np.array_equal(d["labels"][:n].cpu().numpy(), o["labels"])
    assert torch.all(d["labels"][n:] == -2)
    assert np.array_equal(d["contacts"].cpu().numpy(), o["contacts"].astype(np.float32))
    assert bool(d["discard"][0]) == o["discard_seq"] and int(d["n_groups"][0]) == o["n_groups"]
    assert d["floor_height"].cpu().numpy()[0].tobytes() == o["floor_height"].tobytes()
    assert d["offset"].cpu().numpy()[0].tobytes() == np.float32(o["offset_floor_height"]).tobytes()


def test_forced_long_path_equals_the_evaluation_entry(long_cases):
    """eval_cases.batch() and the 4096-frame case: every output of the workspace path, and of the LDS path, carries the bits of
    evaluate.determine_floor_height_and_contacts."""
    _, batch, _ = eval_cases.batch()
    for seqs, fps in ((list(batch), eval_cases.FPS), ([long_cases[4096]], eval_cases.FPS)):
        T = seqs[0].shape[0]
        x = dev(np.stack(seqs))
        off, contacts, discard, det = evaluate.determine_floor_height_and_contacts(x, fps, return_details=True)
        offsets = [T * b for b in range(len(seqs) + 1)]
        for force in (True, False):
            d = details_of(x.reshape(-1, 22, 3), offsets, fps, force_long=force)
            assert torch.equal(d["offset"], off) and torch.equal(d["floor_height"], det["floor_height"]), force
            assert torch.equal(d["contacts"].reshape(len(seqs), T, 22), contacts) and torch.equal(d["discard"], discard), force
            assert torch.equal(d["labels"].reshape(len(seqs), 2 * T), det["labels"]), force
            assert torch.equal(d["n_static"], det["n_static"]) and torch.equal(d["n_groups"], det["n_groups"]), force


def test_ragged_lengths_equal_the_evaluation_entry():
    """The sequences of eval_cases.batch() cut to different lengths (2, the shortest the evaluation entry takes; odd ones; the
    full T): padded to T with `lengths` through the evaluation entry, packed end to end through this one, on both paths.  Per
    sequence every output carries the same bits; the evaluation entry's rows past L are zero, its labels past n_static are -2,
    and the padded frames hold 1e30, so that nothing past L can have been read."""
    _, batch, _ = eval_cases.batch()
    B, T = batch.shape[:2]
    lengths = [T, 2, 17, T, 33, T - 1, 31]
    assert len(lengths) == B
    x_padded = np.full_like(batch, 1e30)
    for b, L in enumerate(lengths):
        x_padded[b, :L] = batch[b, :L]
    off, contacts, discard, det = evaluate.determine_floor_height_and_contacts(dev(x_padded), eval_cases.FPS, lengths=lengths,
                                                                               return_details=True)
    assert int(det["n_static"][0]) == 0 and sum(int(n) > 0 for n in det["n_static"]) >= 4  # with and without static samples
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    packed = dev(np.concatenate([batch[b, :L] for b, L in enumerate(lengths)]))
    for force in (True, False):
        d = details_of(packed, offsets, eval_cases.FPS, force_long=force)
        assert torch.equal(d["offset"], off) and torch.equal(d["floor_height"], det["floor_height"]), force
        assert torch.equal(d["discard"], discard), force
        assert torch.equal(d["n_static"], det["n_static"]) and torch.equal(d["n_groups"], det["n_groups"]), force
        for b, L in enumerate(lengths):
            o, n = int(offsets[b]), int(det["n_static"][b])
            assert torch.equal(d["contacts"][o:o + L], contacts[b, :L]) and not contacts[b, L:].any(), (force, b)
            assert torch.equal(d["labels"][2 * o:2 * (o + L)], det["labels"][b, :2 * L]), (force, b)
            assert n <= 2 * L and torch.all(det["labels"][b, n:] == -2), (force, b)


# ------------------------------------------------------------------------------------------------ packing
def pipeline(seqs, model, force_long=False):
    """seqs: [(root_orient, pose_body, trans, fps)] float32 arrays -> per sequence the tensors of the three stages."""
    lens = [s[0].shape[0] for s in seqs]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    ro, pb, tr = (dev(np.concatenate([s[k] for s in seqs])) for k in range(3))
    joints, head_rot = A.body_joints(ro, pb, tr, model)
    d = details_of(joints, offsets, [s[3] for s in seqs], force_long=force_long)
    tables = [A.downsample_table(n, s[3])[0] for n, s in zip(lens, seqs)]
    out, oo = A.head_tracks(joints, head_rot, d["contacts"], d["offset"], offsets, tables)
    res = []
    for b in range(len(seqs)):
        r = {"joints_raw": joints[offsets[b]:offsets[b + 1]], "head_rot": head_rot[offsets[b]:offsets[b + 1]],
             "contacts_raw": d["contacts"][offsets[b]:offsets[b + 1]], "labels": d["labels"][2 * offsets[b]:2 * offsets[b + 1]]}
        r.update({k: d[k][b] for k in ("offset", "floor_height", "discard", "n_static", "n_groups")})
        r.update({k: v[oo[b]:oo[b + 1]] for k, v in out.items()})
        res.append(r)
    return res


def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


def test_a_sequence_does_not_depend_on_its_batch(gold):
    model = A.skeleton(gold["model"])
    X = raw_inputs(gold, "kept_60")
    Y, Z = raw_inputs(gold, "kept_120"), raw_inputs(gold, "handball_240")
    nan = tuple(np.full_like(a, np.nan) for a in Y[:3]) + (120.0,)
    two = tuple(a[:2].copy() for a in Z[:3]) + (30.0,)
    m = synthetic.make_eval_motion(1, 4200, 9, check=False)
    long_ = (m["local_aa"][0].reshape(4200, 66)[:, :3].copy(), m["local_aa"][0].reshape(4200, 66)[:, 3:].copy(), m["root_trans"][0], 120.0)
    alone = pipeline([X], model)[0]
    assert not bool(alone["discard"]) and int(alone["n_static"]) > 0
    assert same_bits(pipeline([X, Y, Z], model)[0], alone)          # first
    assert same_bits(pipeline([Y, Z, X], model)[2], alone)          # last
    assert same_bits(pipeline([Y, X, Z], model)[1], alone)          # in the middle, between other frame rates
    assert same_bits(pipeline([nan, X, nan], model)[1], alone)      # between neighbours whose poses are NaN
    assert same_bits(pipeline([two, X, two], model)[1], alone)      # next to 2-frame neighbours
    mixed = pipeline([long_, X, two, long_], model)                 # short and long sequences in one call
    assert same_bits(mixed[1], alone)
    assert int(mixed[0]["n_static"]) > 0 and same_bits(mixed[0], mixed[3])
    assert same_bits(pipeline([X, Y], model, force_long=True)[0], alone)  # ... and on the workspace path


def test_the_workspace_may_hold_anything(gold, long_cases):
    """0xFF and zeros in the workspace on entry, LDS-sized and long sequences in one call, forced long or not: the same bits."""
    j = np.concatenate([long_cases[4097], eval_cases.batch()[1][2], long_cases[5000]])
    offsets = [0, 4097, 4097 + eval_cases.T_CASE, 4097 + eval_cases.T_CASE + 5000]
    x = dev(j)
    for force in (False, True):
        base = details_of(x, offsets, [120, 30, 60], force_long=force)
        ws = A._prep(x.device)._ws
        for fill in (0xFF, 0):
            ws.fill_(fill)
            again = details_of(x, offsets, [120, 30, 60], force_long=force)
            assert A._prep(x.device)._ws is ws
            assert same_bits(again, base), (force, fill)


# ------------------------------------------------------------------------------------------------ the stream
def test_the_work_lands_on_the_callers_stream(gold, long_cases):
    """The three stage functions upload small host tables (offsets, thresholds, the downsample table) and so wait for their
    stream: they are held to the bits and the idle null stream; the three library entries with every argument on the device are
    held to all three checks (late input, null stream, asynchrony)."""
    model = A.skeleton(gold["model"])
    X, Y = raw_inputs(gold, "kept_60"), raw_inputs(gold, "kept_120")
    lens = [X[0].shape[0], Y[0].shape[0]]
    offsets = np.asarray([0, lens[0], lens[0] + lens[1]], np.int32)
    N, B = int(offsets[-1]), 2
    true = [dev(np.concatenate([X[k], Y[k]])) for k in range(3)]
    tables = [A.downsample_table(n, f)[0] for n, f in zip(lens, (X[3], Y[3]))]

    def stages(ro, pb, tr):
        joints, head_rot = A.body_joints(ro, pb, tr, model)
        off, contacts, discard, det = A.floor_and_contacts(joints, offsets, [X[3], Y[3]], return_details=True, force_long=True)
        out, _ = A.head_tracks(joints, head_rot, contacts, off, offsets, tables)
        return [joints, head_rot, off, contacts, discard, det, out]

    lib = _lib.load()
    jt, par = dev(model[0]), (C.c_int32 * 22)(*model[1])
    d_off, d_thr = dev(offsets), dev(np.asarray([int(0.25 * X[3]), int(0.25 * Y[3])], np.int32))
    src = np.concatenate([t + o for t, o in zip(tables, offsets[:-1])]).astype(np.int32)
    seq = np.concatenate([np.full(t.size, b, np.int32) for b, t in enumerate(tables)])
    M = src.size
    d_src, d_seq, d_oo = dev(src), dev(seq), dev(np.asarray([0, tables[0].size, M], np.int32))
    nbytes = lib.egoego_amass_floor_workspace_bytes(N, B)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    host_off = offsets.ctypes.data_as(C.POINTER(C.c_int32))

    def library(ro, pb, tr):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        f32 = dict(device="cuda", dtype=torch.float32)
        joints, head_rot = torch.empty(N, 22, 3, **f32), torch.empty(N, 9, **f32)
        _lib.check_amass(lib.egoego_amass_joints(ro.data_ptr(), pb.data_ptr(), tr.data_ptr(), jt.data_ptr(), par, N, joints.data_ptr(),
                                                 head_rot.data_ptr(), st))
        floor, off, contacts = torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(N, 22, **f32)
        ints = [torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(3)]
        labels = torch.empty(2 * N, dtype=torch.int32, device="cuda")
        _lib.check_amass(lib.egoego_amass_floor_contacts(joints.data_ptr(), host_off, d_off.data_ptr(), d_thr.data_ptr(), B, 1, floor.data_ptr(),
                                                         off.data_ptr(), contacts.data_ptr(), ints[0].data_ptr(), labels.data_ptr(),
                                                         ints[1].data_ptr(), ints[2].data_ptr(), ws_ptr, nbytes, st))
        outs = [torch.empty(M, 22, 3, **f32), torch.empty(M, 22, device="cuda", dtype=torch.float64), torch.empty(M, 3, **f32),
                torch.empty(M, 6, **f32), torch.empty(M, 7, **f32), torch.empty(M, 6, **f32), torch.empty(M, 3, **f32), torch.empty(M, 6, **f32),
                torch.empty(M, dtype=torch.uint8, device="cuda")]
        _lib.check_amass(lib.egoego_amass_head(joints.data_ptr(), head_rot.data_ptr(), contacts.data_ptr(), off.data_ptr(), d_src.data_ptr(),
                                               d_seq.data_ptr(), d_oo.data_ptr(), M, N, B, *[t.data_ptr() for t in outs], st))
        return [joints, head_rot, floor, off, contacts, labels] + ints + outs

    stages(*true), library(*true)
    delay = SC.Delay().calibrate({"the three egoego_amass_* entries": lambda: library(*true)})
    S = torch.cuda.Stream()
    SC.check("amass_prep stage functions", "upload their host tables", stages, true, S, delay)
    got = SC.check("egoego_amass_joints / floor_contacts / head", SC.ENQUEUES, library, true, S, delay)
    assert torch.equal(got[0], SC.flat(stages(*true))[0])


# ------------------------------------------------------------------------------------------------ the limits
def test_one_frame_over_the_limit_raises_and_launches_nothing(gold):
    assert A.MAX_FRAMES == _lib.load().egoego_amass_max_frames() >= 65536 and A.LDS_FRAMES == evaluate.MAX_FRAMES == 4096
    N = A.MAX_FRAMES + 11
    x = torch.zeros(N, 22, 3, device="cuda")
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        torch.cuda._sleep(20_000_000)  # anything launched now would queue behind this on S
        with pytest.raises(ValueError, match="at most 65536"):
            A.floor_and_contacts(x[10:], [0, N - 10], 120)
        with pytest.raises(ValueError, match="sequence 1 has 65537 frames"):
            A.floor_and_contacts(x, [0, 10, N], 120, force_long=True)
        # the library refuses it by itself, too
        off = (C.c_int32 * 2)(0, A.MAX_FRAMES + 1)
        rc = _lib.load().egoego_amass_floor_contacts(x.data_ptr(), off, x.data_ptr(), x.data_ptr(), 1, 0, x.data_ptr(), x.data_ptr(), x.data_ptr(),
                                                     x.data_ptr(), None, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1 << 40,
                                                     C.c_void_p(S.cuda_stream))
        assert rc == -1 and "at most 65536 per sequence" in _lib.load().egoego_amass_last_error().decode()
    S.synchronize()
    assert not x.any()  # the outputs the refused call named are untouched
    seq = {"name": "too_long", "poses": np.zeros((82000, 66)), "trans": np.zeros((82000, 3)), "mocap_framerate": 120.0}
    with pytest.raises(ValueError, match="at most 65536"):
        A.process_sequences([seq], gold["model"])
    with pytest.raises(ValueError, match="at most 4096"):  # the evaluation's own limit stays
        evaluate.determine_floor_height_and_contacts(torch.zeros(1, 4097, 22, 3, device="cuda"), 30)
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        A.floor_and_contacts(torch.zeros(4, 22, 3), [0, 4], 30)


# ------------------------------------------------------------------------------------------------ the tool, end to end
def test_the_tool_writes_what_build_motion_windows_reads(gold, tmp_path):
    import joblib
    z = gold["z"]
    root = tmp_path / "amass"
    for name in ("kept_60", "kept_30", "short"):
        s = gold["seqs"][gold["names"].index(name)]
        path = root / s["path"]
        path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(path, poses=s["poses"], trans=s["trans"], mocap_framerate=s["mocap_framerate"], gender="female", betas=np.ones(16))
    model_dir = tmp_path / "smplh" / "male"
    model_dir.mkdir(parents=True)
    np.savez(model_dir / "model.npz", **gold["model"])
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "process_amass.py"), "--amass_root", str(root), "--body_model",
                        str(tmp_path / "smplh"), "--out", str(out)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("kept_60", "kept_30"):
        s = gold["seqs"][gold["names"].index(name)]
        n, fps = z[name + "/ref/trans"].shape[0], int(z[name + "/ref/fps"])
        saved = np.load(out / (s["path"][:-4] + "_%d_frames_%d_fps.npz" % (n, fps)))
        assert tuple(saved.files) == A.RECORD_KEYS
        assert saved["trans"].tobytes() == z[name + "/ref/trans"].tobytes()
    data = joblib.load(out / "amass_smplh_motion.p")
    train, test = joblib.load(out / "train_amass_smplh_motion.p"), joblib.load(out / "test_amass_smplh_motion.p")
    assert len(data) == 2 and len(train) == 1 and len(test) == 1  # CMU trains, SFU validates, the short one is dropped
    assert train[0]["seq_name"] == "CMU-s2-kept_60_poses_80_frames_30_fps.npz" and train[0]["body_pose"].shape == (80, 63)
    win = tmp_path / "windows"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_motion_windows.py"), "--data", str(out / "train_amass_smplh_motion.p"),
                        "--test_data", str(out / "test_amass_smplh_motion.p"), "--body_model", str(tmp_path / "smplh"), "--window", "60",
                        "--out", str(win)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    windows = joblib.load(win / "cano_train_diffusion_amass_window_60.p")
    assert len(windows) == 2 and windows[0]["seq_name"] == train[0]["seq_name"] and windows[0]["global_jpos"].shape == (60, 66)
    assert len(joblib.load(win / "cano_test_diffusion_amass_window_60.p")) == 2
