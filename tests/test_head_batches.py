"""HeadNet's training batches without a GPU (egoego_release_amd/stage1_data.py, csrc/stage1_data.*): the numpy oracle against the
reference's recorded items, the host packing and its dropping rules, load_ares_split on a temporary ARES tree with its cache, the
keyed draw on the numpy Philox replica, the ABI, the argument checks that return before any launch and the tools' flags.  The GPU
side is tests/test_gpu_head_batches.py.

The golden (tests/golden/make_head_batch_golden.py) holds the reference's own ARESHeadPoseDataset items.  Its SLAM arrays were
aligned by the reference under stand-ins for pytorch3d (scipy's rotations, evaluated in fp64), which differ from pytorch3d's fp32
formulas, the ones stage1.load_slam_res_and_align_first restates, in the last bit; so the recorded whole tracks are what the
select-and-copy is held to bit for bit, and the host alignment is held to its own function's bits and to 4 fp32 eps of them.
"""
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest
import torch

import head_batch_oracle as O
from egoego_release_amd import _lib, build, stage1, stage1_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "head_batch_golden.npz")
SEED = 2 ** 33 + 5
EPS = float(np.finfo(np.float32).eps)


def golden_sequences(aligned=True):
    """-> (window, the tree's six entries in file order: with the recorded whole SLAM arrays, or with the raw track)."""
    g = np.load(GOLDEN)
    seqs = []
    for n in (str(n) for n in g["names"]):
        e = {"seq_name": n, **{k: g[f"seq/{n}/{k}"] for k in ("head_qpos", "head_vels", "of_feats")}}
        if f"seq/{n}/slam" in g.files:
            if aligned and f"seq/{n}/aligned_slam_trans" in g.files:
                e.update({k: g[f"seq/{n}/{k}"] for k in O.SLAM_KEYS})
            else:
                e["slam"] = g[f"seq/{n}/slam"]
        seqs.append(e)
    return int(g["window"]), seqs


def golden_items(mode):
    g = np.load(GOLDEN)
    for j in range(int(g[f"{mode}/count"])):
        P = f"{mode}/{j}/"
        yield {k[len(P):]: g[k] for k in g.files if k.startswith(P)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- the oracle and the golden
def test_oracle_is_the_reference_bit_for_bit():
    W, seqs = golden_sequences()
    by = {s["seq_name"]: s for s in seqs}
    dtypes = {"head_pose": "float32", "head_vels": "float64", "of": "float32", "aligned_slam_trans": "float32",
              "aligned_slam_rot_quat": "float32", "aligned_slam_rot_mat": "float32", "ori_slam_trans": "float64",
              "ori_slam_rot_quat": "float32", "ori_slam_rot_mat": "float32"}
    seen = []
    for mode in ("train", "eval"):
        for rec in golden_items(mode):
            s = by[str(rec["seq"])]
            F = len(s["head_qpos"]) - 1
            start, n = int(rec["start"]), int(rec["seq_len"])
            assert O.window_of(F, F if mode == "eval" else W, mode == "eval", start) == (start, n)
            want = O.item(s, start, n)
            for k, dt in dtypes.items():
                assert str(rec[k].dtype) == dt and same_bits(rec[k], want[k]), (mode, str(rec["seq"]), k)
            seen.append((mode, str(rec["seq"]), len(rec["aligned_slam_trans"])))
    assert len(seen) == 12
    assert ("eval", "room_1-seq_d", 7) in seen                      # T = 9, a track of 7 rows: fewer than the 9 pose rows
    assert ("eval", "apartment_0-seq_b", 5) in seen                 # a track of 8 rows cut by the slice at T = 5


def test_dropping_rules_and_the_packed_tables():
    W, seqs = golden_sequences()
    assert [O.passes_filter(len(s["head_qpos"]), len(s["of_feats"]), W) for s in seqs] == [True, True, False, True, True, True]
    p = stage1_data.pack_head_sequences(seqs, W)
    keep, dropped = O.kept(seqs, W, False)
    assert p["names"] == [seqs[k]["seq_name"] for k in keep] == [str(n) for n in np.load(GOLDEN)["kept"]]
    assert p["n_dropped"] == dropped == {"short": 1, "no_slam": 1}
    assert p["offsets"].tolist() == [0, 6, 11, 20, 28] and p["slam_offsets"].tolist() == [0, 6, 11, 18, 26]  # tracks cut at T
    assert p["feats"].shape == (28 - 4, 12) and p["vels"].dtype == np.float32 and p["slam_trans64"].dtype == np.float64
    for k, i in enumerate(keep):
        o, s = p["offsets"][k], seqs[i]
        assert same_bits(p["feats"][o - k:o - k + len(s["of_feats"])], s["of_feats"])         # the offsets[k] - k feature base
        assert same_bits(p["vels"][o:o + len(s["head_vels"])], s["head_vels"].astype(np.float32))
        so, L = p["slam_offsets"][k], p["slam_offsets"][k + 1] - p["slam_offsets"][k]
        assert same_bits(p["slam_trans64"][so:so + L], s["ori_slam_trans"][:L])
        assert same_bits(p["slam32"][so:so + L, 7:16].reshape(L, 3, 3), s["aligned_slam_rot_mat"][:L])
    ev = stage1_data.pack_head_sequences(seqs, W, for_eval=True)
    assert ev["n_dropped"] == O.kept(seqs, W, True)[1] == {"short": 0, "no_slam": 1} and len(ev["names"]) == 5
    no_slam = [{k: v for k, v in s.items() if k not in O.SLAM_KEYS + ("slam",)} for s in seqs]
    q = stage1_data.pack_head_sequences(no_slam, W)
    assert "slam32" not in q and q["n_dropped"] == {"short": 1, "no_slam": 0} and len(q["names"]) == 5
    assert stage1_data.pack_head_sequences(seqs, W, names=["office_2-seq_e", "apartment_0-seq_a"])["names"] == \
        ["office_2-seq_e", "apartment_0-seq_a"]


def test_host_alignment_is_the_existing_arithmetic(tmp_path):
    """pack_head_sequences on raw tracks: the bits of load_slam_res_and_align_first / load_slam, which give for an array what they
    give for its file; the reference's arrays (aligned under the stand-ins) lie within 4 eps of the largest entry."""
    W, raw = golden_sequences(aligned=False)
    _, rec = golden_sequences()
    p = stage1_data.pack_head_sequences(raw, W)
    by = {s["seq_name"]: s for s in raw}
    for k, name in enumerate(p["names"]):
        s = by[name]
        path = tmp_path / f"{k}.npy"
        np.save(path, s["slam"])
        at, ar, aq = stage1.load_slam_res_and_align_first(str(path), s["head_qpos"])
        ot, orot, oq = stage1.load_slam(str(path))
        for a, b in zip((at, ar, aq), stage1.load_slam_res_and_align_first(s["slam"], s["head_qpos"])):
            assert same_bits(a, b)
        for a, b in zip((ot, orot, oq), stage1.load_slam(s["slam"])):
            assert same_bits(a, b)
        so, L = p["slam_offsets"][k], p["slam_offsets"][k + 1] - p["slam_offsets"][k]
        assert L == min(len(s["slam"]), len(s["head_qpos"]))
        row = p["slam32"][so:so + L]
        parts = {"aligned_slam_trans": (row[:, :3], at), "aligned_slam_rot_quat": (row[:, 3:7], aq),
                 "aligned_slam_rot_mat": (row[:, 7:16].reshape(L, 3, 3), ar), "ori_slam_rot_quat": (row[:, 16:20], oq),
                 "ori_slam_rot_mat": (row[:, 20:].reshape(L, 3, 3), orot)}
        ref = next(r for r in rec if r["seq_name"] == name)
        for key, (got, want) in parts.items():
            assert same_bits(got, np.asarray(want[:L], np.float32)), (name, key)
            assert np.abs(got.astype(np.float64) - ref[key][:L]).max() <= 4 * EPS * np.abs(ref[key]).max(), (name, key)
        assert same_bits(p["slam_trans64"][so:so + L], ot[:L])


# ---------------------------------------------------------------------------------------------- the host checks
def _entry(T=8, D=12, **kw):
    e = {"seq_name": "s", "head_qpos": np.zeros((T, 7), np.float32), "head_vels": np.zeros((T, 6)), "of_feats": np.zeros((T - 1, D), np.float32)}
    e.update(kw)
    return e


def test_host_checks_raise_without_a_gpu():
    for bad in (_entry(head_qpos=np.zeros((8, 6))), _entry(head_vels=np.zeros((7, 6))), _entry(of_feats=np.zeros((8, 12))),
                _entry(D=10), _entry(D=2), _entry(slam=np.zeros((5, 6))), _entry(aligned_slam_trans=np.zeros((5, 3)))):
        with pytest.raises((ValueError, KeyError)):
            stage1_data.HeadBatches([bad], 2, window=4, device="cpu")
    with pytest.raises(ValueError, match="one D"):
        stage1_data.HeadBatches([_entry(), _entry(D=16)], 2, window=4, device="cpu")
    with pytest.raises(ValueError, match="no sequence left"):
        stage1_data.HeadBatches([_entry(T=4)], 2, window=4, device="cpu")
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        stage1_data.HeadBatches([_entry()], 2, window=4, device="cpu")
    t = {"pose": torch.zeros(8, 7), "vels": torch.zeros(8, 6), "feats": torch.zeros(7, 12), "offsets": [0, 8]}
    with pytest.raises(_lib.EgoEgoHipError, match="no CPU path"):
        stage1_data.head_batch(t, [0], [0], 4, 0)
    with pytest.raises(ValueError, match="go together"):                    # mixed SLAM presence
        stage1_data.head_batch(dict(t, slam32=torch.zeros(8, 29)), [0], [0], 4, 0)
    with pytest.raises(ValueError, match="multiple of 4"):
        stage1_data.head_batch(dict(t, feats=torch.zeros(7, 10)), [0], [0], 4, 0)
    for k, v in (("pose", torch.zeros(8, 6)), ("vels", torch.zeros(7, 6)), ("feats", torch.zeros(7, 12, dtype=torch.float64))):
        with pytest.raises(ValueError):
            stage1_data.head_batch(dict(t, **{k: v}), [0], [0], 4, 0)


# ---------------------------------------------------------------------------------------------- the window rule and the draw
def test_window_rule_and_draws():
    assert O.window_of(4, 4, False, 0) == (0, 4) and O.window_of(4, 4, False, 1) is None        # a room of 1
    assert O.window_of(5, 4, False, 1) == (1, 4) and O.window_of(5, 4, False, 2) is None and O.window_of(5, 4, False, -1) is None
    assert O.window_of(3, 4, False, 0) is None and O.window_of(3, 4, True, 9) == (0, 3) and O.window_of(0, 4, True, 0) is None
    assert O.window_of(61, 7, True, 0) == (0, 7)
    ids = np.arange(4096)
    assert set(O.draw_start(SEED, ids, 1).tolist()) == {0}
    assert set(O.draw_start(SEED, ids, 7).tolist()) == set(range(7))
    a = O.draw_start(SEED, [3, 2 ** 40 + 3, 3], 2 ** 20)
    assert a[0] == a[2] != a[1] and O.draw_start(SEED + 1, [3], 2 ** 20)[0] != a[0]
    # a tag of its own in counter word 3: not GravityNet's, and above every dropout / sampler counter
    import gravity_batch_oracle as G
    assert O.DRAW_TAG != G.DRAW_TAG and O.DRAW_TAG > 1000
    src = open(os.path.join(ROOT, "egoego_release_amd", "csrc", "stage1_data.h")).read().lower()
    assert f"head_draw_tag = 0x{O.DRAW_TAG:08x}u" in src and f"draw_tag = 0x{G.DRAW_TAG:08x}u" in src
    assert not np.array_equal(O.draw_start(SEED, ids, 2 ** 20), G.draw_start(SEED, ids, 2 ** 20))


# ---------------------------------------------------------------------------------------------- load_ares_split
def test_load_ares_split_on_a_tree_and_its_cache(tmp_path, monkeypatch):
    W, seqs = golden_sequences(aligned=False)
    root = str(tmp_path / "data")
    O.write_ares_tree(root, seqs, stage1.ARES_SRC_ROOT, short_files=("office_2-seq_e",))
    got = stage1_data.load_ares_split(root, True, W)
    assert [s["seq_name"] for s in got] == ["apartment_0-seq_a", "apartment_0-seq_b", "room_1-seq_d"]
    assert got.n_dropped == {"filter": 2, "no_slam": 1}          # T = 4 and the sequence short of a file; no SLAM file
    by = {s["seq_name"]: s for s in seqs}
    for s in got:
        for k in ("head_qpos", "head_vels", "of_feats", "slam"):
            assert same_bits(s[k], by[s["seq_name"]][k]), k       # of_feats: the rewritten paths, frame by frame
    assert len(stage1_data.load_ares_split(root, False, 3)) == 4  # the test split's file, the filter at another window
    cache = str(tmp_path / "cache" / "feats.npz")
    first = stage1_data.load_ares_split(root, True, W, cache=cache)
    assert os.path.exists(cache) and len(first) == 3
    opened = []
    load = np.load
    monkeypatch.setattr(np, "load", lambda f, *a, **kw: (opened.append(str(f)), load(f, *a, **kw))[1])
    import joblib
    monkeypatch.setattr(joblib, "load", lambda *a, **kw: pytest.fail("the motion file was opened"))
    again = stage1_data.load_ares_split(root, True, W, cache=cache)
    assert opened == [cache]                                      # neither a feature nor a SLAM file
    assert again.n_dropped == first.n_dropped and len(again) == 3
    for a, b in zip(first, again):
        assert a["seq_name"] == b["seq_name"] and all(same_bits(a[k], b[k]) for k in ("head_qpos", "head_vels", "of_feats", "slam"))
    with pytest.raises(ValueError):
        stage1_data.load_ares_split(root, False, W, cache=cache)  # another split's cache
    # and the packed tables of the loaded split are those of the arrays themselves
    p, q = stage1_data.pack_head_sequences(again, W), stage1_data.pack_head_sequences([by[s["seq_name"]] for s in again], W)
    assert all(same_bits(p[k], q[k]) for k in ("pose", "vels", "feats", "offsets", "slam32", "slam_trans64", "slam_offsets"))


# ---------------------------------------------------------------------------------------------- the library and the tools
def test_abi():
    src = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    assert "egoego_s1_head_batch" in _lib.EXPORTS and re.search(r"\begoego_s1_head_batch\s*\(", src)
    assert "stage1_data.hip" in build.SOURCES
    assert "egoego_s1_head_batch" in open(os.path.join(ROOT, "egoego_release_amd", "csrc", "stage1_data.hip")).read()
    assert int(re.search(r"#define EGOEGO_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 8  # additive: the version stays
    build.build()
    assert hasattr(_lib.load(), "egoego_s1_head_batch")


def test_bad_arguments_return_before_any_launch():
    """window < 1, B < 1, D < 4, D % 4 != 0, NULL required pointers and SLAM tables or outputs given in part are refused on the
    host (EGOEGO_E_INVALID): nothing is launched, so no GPU is needed and the made-up addresses are never touched."""
    build.build()
    lib = _lib.load()
    p = 4096  # stands for a non-NULL pointer

    def call(window=16, B=2, D=512, n_rows=100, n_seqs=3, tables=(p, p, p, p), slam=(None,) * 3, ids=(p, p), outs=(p,) * 5,
             slam_outs=(None,) * 7):
        return lib.egoego_s1_head_batch(tables[0], tables[1], tables[2], n_rows, D, tables[3], n_seqs, *slam, 10, ids[0], ids[1], B,
                                        window, 1, 0, None, *outs, *slam_outs, None)

    bad = [dict(window=0), dict(window=-3), dict(B=0), dict(B=-1), dict(D=0), dict(D=2), dict(D=510), dict(D=-4), dict(n_rows=0),
           dict(n_seqs=0)]
    bad += [dict(tables=tuple(None if j == i else p for j in range(4))) for i in range(4)]
    bad += [dict(ids=tuple(None if j == i else p for j in range(2))) for i in range(2)]
    bad += [dict(outs=tuple(None if j == i else p for j in range(5))) for i in range(5)]
    bad += [dict(slam=tuple(None if j == i else p for j in range(3)), slam_outs=(p,) * 7) for i in range(3)]
    bad += [dict(slam=(p,) * 3, slam_outs=tuple(None if j == i else p for j in range(7))) for i in range(7)]
    bad += [dict(slam=(p,) * 3), dict(slam_outs=(p,) * 7), dict(slam=(p, None, None)), dict(slam_outs=(p,) + (None,) * 6)]
    for kw in bad:
        rc = call(**kw)
        assert rc != 0, kw
        with pytest.raises(_lib.EgoEgoHipError, match="stage-1 data"):
            _lib.check_s1_data(rc)
    assert "D = 510" in (call(D=510), _lib.check_s1_data.last_error())[1]
    assert int(re.search(r"EGOEGO_E_INVALID\s*=\s*(-?\d+)", open(os.path.join(ROOT, "include", "egoego_hip.h")).read()).group(1)) == \
        call(B=0) == call(slam=(p, None, p), slam_outs=(p,) * 7)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_take_the_new_flags_and_keep_the_old_defaults(capsys):
    tool = _tool("train_stage1")
    opt = tool.parse_opt(["--kind", "headnet", "--data_root", "data", "--feature_cache", "f"])
    assert (opt.data_root, opt.feature_cache, opt.window, opt.kind) == ("data", "f", 90, "headnet")
    old = tool.parse_opt([])
    assert (old.kind, old.window, old.batch_size, old.epochs, old.data_root, old.feature_cache, old.motion, old.data_seed,
            old.synthetic_batches, old.learning_rate, old.fused_update) == ("headnet", 90, 32, 1000, None, None, None, 0, 8, 1e-4, False)
    assert tool.parse_opt(["--kind", "gravitynet"]).window == 120
    for argv, text in ((["--kind", "headnet", "--motion", "m.p"], "--motion feeds GravityNet only"),
                       (["--kind", "gravitynet", "--data_root", "d"], "--data_root feeds HeadNet only"),
                       (["--feature_cache", "f"], "--feature_cache needs --data_root")):
        with pytest.raises(SystemExit):
            tool.parse_opt(argv)
        assert text in capsys.readouterr().err
    assert "are not part of this package" not in tool.__doc__
    ev = _tool("eval_stage1").parse_opt(["--data_root", "d"])
    assert (ev.split, ev.window, ev.normal_window, ev.normal_n_dec_layers, ev.z_offset, ev.headnet) == ("test", 90, 90, 4, 0.0, None)


def test_the_golden_is_data_only_and_small():
    assert os.path.getsize(GOLDEN) < 200 * 1024
    with np.load(GOLDEN, allow_pickle=False) as g:                 # (loads without pickle: arrays and strings only)
        assert len(g.files) > 100 and pickle is not None
