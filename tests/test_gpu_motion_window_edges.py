"""The motion-window kernels (egoego_win_build, egoego_win_stats, egoego_win_motion; csrc/motion_windows.h) on the GPU at the edges
that the golden recipe of test_gpu_motion_windows.py never reaches, on the inputs of tests/window_cases.py (whose CPU preconditions
tests/test_window_cases.py asserts):

  chunk sweep        W in 2 .. 480 (one to eight passes of the 64-frame loop, the > 64 KiB LDS attribute from W = 121, all of
                     MAX_W's 156.8 KiB), one window per length in {0, 1, 2, 63, 64, 65, 127, 128, 129, W - 1, W}: lengths on and
                     next to a chunk edge, chunks with real == 0 < rows, empty windows
  heading edges      first-frame headings up to pi - 1e-3, head x-axis up to 1.52 rad above the horizontal
  rotation edges     joint angles 0, either side of qd_from_aa's series threshold, near pi, 4.0, 2 pi - 1e-3 and 7.0, both signs
  many rows          87 960 rows: win_motion_kernel's grid-stride loop takes a second element, win_minmax_kernel 85 rows per workgroup

Bound against the fp64 oracle (tests/windows_oracle.py) for global_jpos, global_rot_6d, local_rot_6d and recover_rot_quat (up to
sign): 2 x one float32 ulp of the output's largest magnitude in the case.  The kernels compute in fp64 and round once; the CPU
preconditions show that two fp64 paths differ by 1e-14.  The reference's own float32 distance (up to 2.3e-6 on these inputs) is
not part of the bound.  global_jvel is the float32 difference of the kernel's own global_jpos, exactly.

Measured worst |kernel - oracle| on MI355X (bound in brackets):
  case group                      global_jpos           global_rot_6d         local_rot_6d          recover_rot_quat
  chunk sweep, W = 2 .. 480       1.192e-07 [4.77e-07]  2.980e-08 [2.38e-07]  2.980e-08 [2.38e-07]  2.545e-08 [2.38e-07]
  heading cases, pitch 0          2.382e-07 [9.54e-07]  2.980e-08 [2.38e-07]  2.976e-08 [2.38e-07]  2.979e-08 [2.38e-07]
  heading cases, pitch 1.4        2.343e-07 [9.54e-07]  2.980e-08 [2.38e-07]  2.978e-08 [2.38e-07]  2.671e-08 [2.38e-07]
  heading cases, pitch 1.52       2.382e-07 [9.54e-07]  2.980e-08 [2.38e-07]  2.980e-08 [2.38e-07]  2.852e-08 [2.38e-07]
  angle draws, W = 120            5.959e-08 [2.38e-07]  2.980e-08 [2.38e-07]  2.979e-08 [2.38e-07]  2.838e-08 [1.19e-07]
  many rows, five windows         5.952e-08 [2.38e-07]  2.979e-08 [1.19e-07]  2.980e-08 [1.19e-07]  2.748e-08 [1.19e-07]
Every figure is the final rounding alone: half a float32 ulp of the largest magnitude.  Canonicalised first-frame head: xy 0 exactly,
|R10| at most 6.1e-07 of its tolerance.  Turn invariance: the kernels' two results differ by 3.58e-07 (global_jpos) and 2.98e-07
(global_rot_6d) where the oracle's differ by 3.69e-07 and 2.97e-07; worst excess over the oracle's own difference 1.18e-07 [2.38e-07].
motion() equals the torch formula on all 87 960 rows exactly.

No case here found a defect in the kernels.  Scratch builds with one arithmetic slip each (the heading dropped from the third
chunk on; a length of exactly 64 or 128 treated as empty; |cos(a / 2)| above pi; w = 1 + f.x in heading_of; either grid-stride loop
cut to its first pass) each failed here, and all but the statistics' loop passed test_gpu_motion_windows.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from egoego_release_amd import _lib, motion_data as MD
from egoego_release_amd.harness import SMPLH_PARENTS_22

import window_cases as WC
from test_harness_golden import REST_OFFSETS
from test_motion_windows import ulp32

pytestmark = pytest.mark.gpu
ROWS = (("global_jpos", 66), ("global_jvel", 66), ("global_rot_6d", 132), ("local_rot_6d", 132))
IDENTITY = np.float32([1, 0, 0, 0])
SAME_FRAMES_W = (63, 64, 65, 193, 480)


def _np(t):
    return t.cpu().numpy()


def run_build(seq, first, length, W, cano):
    """One egoego_win_build call over the frames of `seq` with the caller's own `first` / `length` -> the five outputs as device
    tensors (filled with NaN before the call: what the kernel does not write shows)."""
    first, length = np.asarray(first, np.int32), np.asarray(length, np.int32)
    n_frames, N = len(seq[0]), len(first)
    assert N >= 1 and (first >= 0).all() and (length >= 0).all() and (length <= W).all() and (first.astype(np.int64) + length <= n_frames).all()
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_in = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in seq]
    rest = torch.from_numpy(REST_OFFSETS.astype(np.float32).reshape(-1)).to(dev)
    d_first, d_len = torch.from_numpy(first).to(dev), torch.from_numpy(length).to(dev)
    out = {k: torch.full((N, W, w), float("nan"), device=dev) for k, w in ROWS}
    out["recover_rot_quat"] = torch.full((N, 4), float("nan"), device=dev)
    par = (C.c_int32 * 22)(*SMPLH_PARENTS_22)
    _lib.check_win(lib.egoego_win_build(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), n_frames, rest.data_ptr(), par,
                                        d_first.data_ptr(), d_len.data_ptr(), N, W, int(cano), out["global_jpos"].data_ptr(),
                                        out["global_jvel"].data_ptr(), out["global_rot_6d"].data_ptr(), out["local_rot_6d"].data_ptr(),
                                        out["recover_rot_quat"].data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize()
    out["seq_len"] = d_len
    return out


def distances(got, orc, lengths):
    """{output: (worst |kernel - oracle| over the real rows, the bound)} for the four continuous outputs."""
    real = np.arange(got["global_jpos"].shape[1])[None, :] < np.asarray(lengths)[:, None]
    d = {k: (float(np.abs(got[k][real] - orc[k][real]).max()) if real.any() else 0.0, 2 * ulp32(orc[k])) for k in WC.CONTINUOUS[:3]}
    d["recover_rot_quat"] = (float(WC.up_to_sign(got["recover_rot_quat"], orc["recover_rot_quat"]).max()), 2 * ulp32(orc["recover_rot_quat"]))
    return d


def assert_within(d, what):
    print(what, " ".join(f"{k} {v:.3e} [{b:.3e}]" for k, (v, b) in d.items()))
    for k, (v, b) in d.items():
        assert v <= b, (what, k, v, b)


def assert_rows_exact(got, lengths):
    """Padded rows are zero in all four row outputs, nothing is left unwritten, the velocity is the float32 difference of the
    kernel's own positions with a zero last real row."""
    lengths = np.asarray(lengths)
    W = got["global_jpos"].shape[1]
    pad = np.arange(W)[None, :] >= lengths[:, None]
    for k, _ in ROWS:
        assert np.isfinite(got[k]).all() and not got[k][pad].any(), k
    assert np.isfinite(got["recover_rot_quat"]).all()
    p, v = got["global_jpos"], got["global_jvel"]
    want_v = np.zeros_like(v)
    want_v[:, :-1] = p[:, 1:] - p[:, :-1]  # float32
    want_v[np.arange(W)[None, :] >= lengths[:, None] - 1] = 0.0
    assert np.array_equal(v, want_v)


def built(case, W, cano, **kw):
    """build_motion_windows over the case's one sequence -> (the windows, their outputs on the host)."""
    seq = case["seq"]
    mw = MD.build_motion_windows(seq + ([len(seq[0])],), REST_OFFSETS, window=W, canonicalize_init_head=cano, **kw)
    assert np.array_equal(np.stack([mw.seq_index, mw.start_t_idx, mw.end_t_idx, mw.length], 1), case["table"])
    return mw, {k: _np(getattr(mw, k)) for k in ("global_jpos", "global_jvel", "global_rot_6d", "local_rot_6d", "recover_rot_quat")}


# ------------------------------------------------------------------------------------------ chunk sweep
@pytest.fixture(scope="module")
def sweep():
    """(W, canonicalize) -> the host copies of one call's outputs; each call is made once."""
    done = {}

    def get(W, cano):
        if (W, cano) not in done:
            c = WC.chunk_case(W, cano)
            out = run_build(c["seq"], c["table"][:, 1], c["table"][:, 3], W, cano)
            done[(W, cano)] = {k: _np(v) for k, v in out.items()}
        return done[(W, cano)]
    return get


@pytest.mark.parametrize("cano", [True, False])
@pytest.mark.parametrize("W", WC.CHUNK_WINDOWS)
def test_chunk_sweep(sweep, W, cano):
    c, got = WC.chunk_case(W, cano), sweep(W, cano)
    lengths = c["table"][:, 3]
    assert list(lengths) == WC.chunk_lengths(W)
    assert_within(distances(got, c["oracle"], lengths), f"chunks W={W} cano={cano}:")
    assert_rows_exact(got, lengths)
    i0, i1 = list(lengths).index(0), list(lengths).index(1)
    assert all(not got[k][i0].any() for k, _ in ROWS) and np.array_equal(got["recover_rot_quat"][i0], IDENTITY)
    assert not got["global_jvel"][i1].any() and got["global_jpos"][i1, 0].any() and not got["global_jpos"][i1, 1:].any()
    if not cano:
        assert np.array_equal(got["recover_rot_quat"], np.tile(IDENTITY, (len(lengths), 1)))


@pytest.mark.parametrize("cano", [True, False])
def test_the_same_frames_are_bit_identical_under_every_window(sweep, cano):
    """The 63 frames from frame 1 at W = 63 (one pass, full), 64, 65, 193 and 480 (a second to an eighth pass with real == 0); and
    every shorter length that the sweeps share."""
    base = sweep(SAME_FRAMES_W[0], cano)
    base_len = WC.chunk_lengths(SAME_FRAMES_W[0])
    for W in SAME_FRAMES_W[1:]:
        got, lens = sweep(W, cano), WC.chunk_lengths(W)
        for n in (0, 1, 2, 63):
            i, j = base_len.index(n), lens.index(n)
            for k, _ in ROWS:
                assert np.array_equal(got[k][j, :n], base[k][i, :n]), (W, n, k)
            assert np.array_equal(got["recover_rot_quat"][j], base["recover_rot_quat"][i]), (W, n)
    big, lens = sweep(480, cano), WC.chunk_lengths(480)
    for W in (129, 193):  # three-pass windows against the eight-pass one
        got, mine = sweep(W, cano), WC.chunk_lengths(W)
        for n in (64, 65, 127, 128, 129):
            for k, _ in ROWS:
                assert np.array_equal(got[k][mine.index(n), :n], big[k][lens.index(n), :n]), (W, n, k)


# ------------------------------------------------------------------------------------------ heading and pitch edges
@pytest.fixture(scope="module")
def heading_runs():
    return {cano: built(WC.rule_case("heading", 64, cano), 64, cano) for cano in (True, False)}


def test_heading_and_pitch_edges_against_the_oracle(heading_runs):
    for cano in (True, False):
        c, (mw, got) = WC.rule_case("heading", 64, cano), heading_runs[cano]
        lengths = c["table"][:, 3]
        assert_rows_exact(got, lengths)
        assert_within(distances(got, c["oracle"], lengths), f"heading cases cano={cano}:")
        for p, pitch in enumerate(WC.PITCHES):  # the same bound, per pitch group, for the record
            rows = [i for i in range(len(lengths)) if WC.HEADING_CASES[i % 21][1] == pitch]
            sub = lambda a: {k: v[rows] for k, v in a.items() if k != "seq_len"}
            assert_within(distances(sub(got), sub(c["oracle"]), lengths[rows]), f"  pitch {pitch}:")


def test_heading_edges_on_the_kernels_own_outputs(heading_runs):
    c, (mw, got) = WC.rule_case("heading", 64, True), heading_runs[True]
    raw = heading_runs[False][1]
    p, six = got["global_jpos"], got["global_rot_6d"]
    head_xy = np.abs(p[:, 0, 45:47]).max()
    assert head_xy <= ulp32(p), head_xy
    worst = 0.0
    for i, (_, start, _, _) in enumerate(c["table"]):
        horiz, one_plus_fx = WC.first_head_conditioning(c["seq"][1][start:start + 1], c["seq"][2][start:start + 1])
        r00, r10 = six[i, 0, 6 * 15], six[i, 0, 6 * 15 + 3]
        tol = 2 * ulp32(np.float32(1.0)) / horiz
        worst = max(worst, abs(r10) / tol)
        assert abs(r10) <= tol and r00 > 0, (i, r10, r00, horiz)
        assert abs(r00 - horiz) <= tol  # the canonical head x-axis keeps its horizontal length
    print(f"first-frame head xy {head_xy:.3e}; worst |R10| / tolerance {worst:.3e}")
    # canonicalize_init_head=False on the same inputs
    assert np.array_equal(raw["recover_rot_quat"], np.tile(IDENTITY, (len(c["table"]), 1)))
    dz = np.abs(raw["global_jpos"][..., 2::3] - p[..., 2::3]).max()
    assert dz <= ulp32(p), dz
    assert np.array_equal(raw["local_rot_6d"][..., 6:], got["local_rot_6d"][..., 6:])
    assert np.abs(raw["local_rot_6d"][..., :6] - got["local_rot_6d"][..., :6]).max() > 0.1  # the root's does turn
    assert np.abs(raw["global_jpos"][:, 0, 45:47]).max() <= ulp32(raw["global_jpos"])


# ------------------------------------------------------------------------------------------ turn invariance
def test_turn_invariance():
    """A sequence and its copy turned 2.0 rad about z and shifted canonicalise to the same window, up to what re-rounding the
    turned inputs to float32 costs: the oracle's own difference on the same two inputs, element by element, plus 2 ulp32."""
    a, b = WC.rule_case("angle", 64), WC.rule_case("turned", 64)
    (_, got_a), (_, got_b) = built(a, 64, True), built(b, 64, True)
    assert np.abs(got_a["recover_rot_quat"] - got_b["recover_rot_quat"]).max() > 0.5  # the inputs do differ by the turn
    for k in ("global_jpos", "global_rot_6d"):
        own = np.abs(a["oracle"][k] - b["oracle"][k])
        d = np.abs(got_a[k].astype(np.float64) - got_b[k].astype(np.float64))
        slack = 2 * ulp32(a["oracle"][k])
        print(f"turn invariance {k}: kernels {d.max():.3e}, oracle {own.max():.3e}, worst excess {(d - own).max():.3e} [{slack:.3e}]")
        assert own.max() > 0 and (d <= own + slack).all(), (k, (d - own).max())


# ------------------------------------------------------------------------------------------ rotation edges
def test_rotation_edges():
    c = WC.rule_case("angle", 120)
    assert WC.holds_every_angle(c["seq"][1], c["seq"][2]) == set()  # at the root, on the head chain and on a leaf, both signs
    for cano in (True, False):
        c = WC.rule_case("angle", 120, cano)
        mw, got = built(c, 120, cano)
        lengths = c["table"][:, 3]
        assert list(lengths) == [120, 120, 60]
        assert_rows_exact(got, lengths)
        assert_within(distances(got, c["oracle"], lengths), f"angle draws W=120 cano={cano}:")


# ------------------------------------------------------------------------------------------ many rows
def test_many_rows():
    """87 960 rows: past win_motion_kernel's grid cap.  The oracle on five windows (the first, the last, the one holding row 84 734 and its
    two neighbours); the exact relations of test_exact_relations_on_the_kernels_own_outputs on all rows."""
    c = WC.many_rows_case()
    W, table = WC.MANY_WINDOW, c["table"]
    mw, got = built(c, W, True, min_frames=WC.MANY_MIN_FRAMES)
    N = len(mw)
    lengths = table[:, 3]
    assert N * W * 198 > 65535 * 256
    pick = c["pick"]
    assert_within(distances({k: v[pick] for k, v in got.items()}, c["oracle"], lengths[pick]), "many rows, five windows:")
    assert_rows_exact(got, lengths)
    real = np.arange(W)[None, :] < lengths[:, None]
    p, v = got["global_jpos"], got["global_jvel"]
    st = mw.stats()
    assert np.array_equal(st["global_jpos_min"], p[real].min(0)) and np.array_equal(st["global_jpos_max"], p[real].max(0))
    assert np.array_equal(st["global_jvel_min"], v[real].min(0)) and np.array_equal(st["global_jvel_max"], v[real].max(0))
    assert (st["global_jpos_max"] > st["global_jpos_min"]).all()  # no division by zero in the normalisation
    lo, hi = (torch.from_numpy(st[k]).cuda() for k in MD.STAT_KEYS[:2])
    want = torch.cat(((mw.global_jpos - lo) / (hi - lo) * 2 - 1, mw.global_rot_6d), -1) * torch.from_numpy(real).cuda()[..., None]
    motion = torch.full((N, W, 198), float("nan"), device=mw.device)  # the kernel into a buffer that shows what it leaves out
    _lib.check_win(_lib.load().egoego_win_motion(mw.global_jpos.data_ptr(), mw.global_rot_6d.data_ptr(), mw.seq_len.data_ptr(), lo.data_ptr(),
                                                 hi.data_ptr(), N, W, motion.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(motion).all())
    d = float((motion - want).abs().max())
    print(f"many rows: motion vs the torch formula {d:.3e}")
    assert d <= 1e-6
    assert torch.equal(motion[..., 66:], mw.global_rot_6d) and torch.equal(mw.motion(), motion)
    assert not bool(motion[torch.from_numpy(~real).cuda()].any())


def test_stats_where_most_workgroups_see_no_row():
    """win_minmax_kernel's workgroups without a real row write +inf / -inf, which the fold must ignore.  (motion() is left out: with one
    real row max == min, and the division by zero gives NaN in the reference as well.)"""
    seq = tuple(a[:1] for a in WC.chunk_sequence())
    mw = MD.build_motion_windows(seq + ([1],), REST_OFFSETS, window=2, min_frames=0)  # N = 1, W = 2, one real row of two
    assert len(mw) == 1 and mw.seq_len.tolist() == [1]
    st, p = mw.stats(), _np(mw.global_jpos)
    assert np.array_equal(st["global_jpos_min"], p[0, 0]) and np.array_equal(st["global_jpos_max"], p[0, 0]) and np.abs(p[0, 0]).max() > 0.1
    assert not st["global_jvel_min"].any() and not st["global_jvel_max"].any() and not p[0, 1].any()
    # 40 windows of 64 rows (all 1024 workgroups, two or three rows each), 39 of them empty
    length = np.zeros(40, np.int32)
    length[17] = 5
    out = run_build(WC.chunk_sequence(), np.arange(40) % WC.CHUNK_EDGE_FRAMES, length, 64, True)
    mw = MD.MotionWindows(64, out["global_jpos"], out["global_jvel"], out["global_rot_6d"], out["local_rot_6d"], out["recover_rot_quat"],
                          out["seq_len"], None, None, None, length.astype(np.int64), ["w"] * 40)
    got = {k: _np(v) for k, v in out.items()}
    assert_rows_exact(got, length)
    assert np.array_equal(np.delete(got["recover_rot_quat"], 17, 0), np.tile(IDENTITY, (39, 1)))
    st, p, v = mw.stats(), got["global_jpos"][17, :5], got["global_jvel"][17, :5]
    assert np.isfinite(np.stack(list(st.values()))).all()
    assert np.array_equal(st["global_jpos_min"], p.min(0)) and np.array_equal(st["global_jpos_max"], p.max(0))
    assert np.array_equal(st["global_jvel_min"], v.min(0)) and np.array_equal(st["global_jvel_max"], v.max(0))
