"""The four per-window harness kernels of csrc/pointwise.h (k_convert_model_res, k_window_condition, k_window_prefix,
k_rot6d_to_matrix) on the inputs of tests/harness_cases.py: every matrix_to_quaternion branch, both sides of the small-angle
threshold, rotations near pi, headings towards -x, steep pitches, a second kinematic tree and head joint, the shapes at which the
launches change (one item, partial blocks, several blocks, n_last = Tw, n_last = 1, the grid-stride loops).

Against the fp64 numpy/scipy oracle (oracle/harness_oracle.py), NOT against the product's torch chains.  There is no fixed
tolerance: per output and per run a kernel may be off the oracle by
    4 x max(E_plain, 2^-23 x the output's largest magnitude)
where E_plain is what the plain float32 torch chain (pinned to the reference by tests/test_window_loop_golden.py) is off the oracle
on the same inputs, measured in the same test run; tests/test_harness_cases.py keeps E_plain itself below 2e-6 (5e-7 for `recover`),
so a kernel wrong by 1e-5 in one branch fails.  Everything else is bit for bit: row independence, the grid-stride loops against
the small call, the wrappers' dtype / stride handling, and degenerate 6D inputs against the oracle.

Measured on an MI355X (worst over the shapes of each group: kernel | E_plain on that machine's CPU | largest kernel / bound of any
one run; rad for angles, metres for convert's root / head, normalised units for pos; run with -s for every line):
  convert   smplh    angle 8.4e-07 | 7.3e-07 | 0.29;  root 5.1e-07 | 6.8e-07 | 0.19;  head 5.0e-07 | 6.8e-07 | 0.34
  convert   chain    angle 7.4e-07 | 8.7e-07 | 0.34;  root 5.1e-07 | 6.8e-07 | 0.19;  head 4.4e-07 | 6.3e-07 | 0.18
  condition head 15  pos 3.2e-07 | 3.2e-07 | 0.25;  6d 5.1e-07 | 5.3e-07 | 0.24;  recover 2.5e-07 | 2.5e-07 | 0.25
  condition head 12  pos 3.0e-07 | 3.0e-07 | 0.25;  6d 5.1e-07 | 5.3e-07 | 0.24;  recover 2.5e-07 | 2.5e-07 | 0.25
  prefix    smplh    pos 1.2e-06 | 8.1e-07 | 0.41;  6d 1.6e-06 | 6.4e-07 | 0.65
  prefix    chain    pos 1.0e-06 | 1.0e-06 | 0.26;  6d 6.9e-07 | 1.1e-06 | 0.26
  rot6d              2.2e-07 | 2.4e-07 | 0.23
"""
import ctypes as C

import numpy as np
import pytest
import torch

import harness_cases as HC
from egoego_release_amd import harness, rotations as R, _lib
from oracle import harness_oracle as HO

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 32  # floats behind every output that must come back untouched


# ------------------------------------------------------------------------------------------ the C ABI, any tree and head
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stats(v):
    """66 statistics on the device, with room behind them (the caller keeps the tensor until its launch is queued)."""
    buf = torch.zeros(66 + PAD, device="cuda")
    buf[:66] = torch.as_tensor(np.asarray(v, np.float32).reshape(66))
    return buf[:66]


def _out(*shape):
    """An output of NaNs (an element the kernel leaves out fails every comparison) with a guard of PAD NaNs behind it."""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), NAN, device="cuda")
    return buf, buf[:n].view(*shape)


def _guards_intact(*bufs):
    return all(bool(torch.isnan(b[-PAD:]).all()) for b in bufs)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _par(parents):
    return (C.c_int32 * 22)(*[int(p) for p in parents])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def hip_convert(c, x, rec, rc_only=False, B=None, T=None, head=None, parents=None):
    x, rec = x.contiguous(), rec.reshape(-1, 4).contiguous()
    b, t = x.shape[:2]
    (ba, aa), (br, root), (bh, hd) = _out(b, t, 22, 3), _out(b, t, 3), _out(b, t, 3)
    lo, hi = _stats(c["lo"]), _stats(c["hi"])
    rc = _lib.load().egoego_convert_model_res(x.data_ptr(), rec.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                              _par(c["parents"] if parents is None else parents), c["head"] if head is None else head,
                                              b if B is None else B, t if T is None else T, aa.data_ptr(), root.data_ptr(), hd.data_ptr(), _stream())
    if rc_only:
        return rc
    _lib.check(rc)
    torch.cuda.synchronize()
    assert _guards_intact(ba, br, bh)
    return aa, root, hd


def hip_condition(c, pos, quat, rc_only=False, B=None, Tw=None, head=None):
    pos, quat = pos.contiguous(), quat.contiguous()
    b, tw = pos.shape[:2]
    (bx, x), (br, rec) = _out(b, tw, 198), _out(b, 4)
    lo, hi = _stats(c["lo"]), _stats(c["hi"])
    rc = _lib.load().egoego_window_condition(pos.data_ptr(), quat.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                             c["head"] if head is None else head, b if B is None else B, tw if Tw is None else Tw,
                                             x.data_ptr(), rec.data_ptr(), _stream())
    if rc_only:
        return rc
    _lib.check(rc)
    torch.cuda.synchronize()
    assert _guards_intact(bx, br)
    return x, rec.reshape(b, 1, 1, 4)


def hip_prefix(c, aa, root, n_last, rc_only=False, B=None, Tw=None, head=None, parents=None, out_frames=None):
    aa, root = aa.contiguous(), root.contiguous()
    b, tw = aa.shape[:2]
    bo, out = _out(b, n_last if out_frames is None else out_frames, 198)
    rest, lo, hi = _stats(HC.REST_OFFSETS), _stats(c["lo"]), _stats(c["hi"])
    rc = _lib.load().egoego_window_prefix(aa.data_ptr(), root.data_ptr(), rest.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                          _par(c["parents"] if parents is None else parents), c["head"] if head is None else head,
                                          b if B is None else B, tw if Tw is None else Tw, n_last, out.data_ptr(), _stream())
    if rc_only:
        return rc
    _lib.check(rc)
    torch.cuda.synchronize()
    assert _guards_intact(bo)
    return out


def hip_rot6d(d6):
    d6 = d6.contiguous()
    n = d6.numel() // 6
    bo, out = _out(n, 3, 3)
    _lib.check(_lib.load().egoego_rot6d_to_matrix(d6.data_ptr(), out.data_ptr(), n, _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(bo)
    return out


class _Ledger:
    """Prints every figure, then fails on all that lie outside their bound."""

    def __init__(self):
        self.bad = []

    def hold(self, label, kernel, plain):
        for k, (d, big) in kernel.items():
            e = plain[k][0]
            lim = HC.bound(e, big)
            print(f"  {label:34s} {k:8s} kernel {d:.3e}   E_plain {e:.3e}   bound {lim:.3e}")
            if not d <= lim:
                self.bad.append((label, k, float(d), float(e), lim))

    def close(self):
        assert not self.bad, self.bad


# ------------------------------------------------------------------------------------------ parity with the fp64 oracle
@pytest.mark.parametrize("tree", list(HC.TREES))
def test_convert_kernel_vs_oracle(tree):
    """egoego_convert_model_res through the C ABI (the chain tree with head 12 included) at (B, T) = (1, 1), (4, 64), (3, 41), and
    the known answer: the poses that built the window come back."""
    c = HC.convert_case(tree)
    led = _Ledger()
    for shape, sl in HC.CONVERT_SLICES.items():
        got = tuple(v.cpu().numpy() for v in hip_convert(c, _dev(c["x"][sl]), _dev(c["rec"][sl[0]])))
        assert got[0].shape == shape + (22, 3) and got[1].shape == got[2].shape == shape + (3,)
        plain = HC.convert_distances(HC.plain_convert(c, sl), c, sl)
        kern = HC.convert_distances(got, c, sl)
        led.hold(f"convert/{tree}/{shape}", kern, plain)
        # known answer: within the kernel's bound plus what rounding the window to float32 moved the oracle's own answer
        for k, mine, known, theirs in (("angle", got[0], c["known_aa"][sl], c["aa"][sl]), ("root", got[1], c["known_root"][sl], c["root"][sl]),
                                       ("head", got[2], c["known_head"][sl], c["head_pos"][sl])):
            dist = (lambda a, b: HC.angle(a, b).max()) if k == "angle" else (lambda a, b: np.abs(HC.up(a) - b).max())
            d, slack = dist(mine, known), dist(theirs, known)
            print(f"  convert/{tree}/{shape} known {k}: kernel {d:.3e}   oracle {slack:.3e}")
            assert d <= HC.bound(plain[k][0], kern[k][1]) + slack, (shape, k, d)
    led.close()


@pytest.mark.parametrize("tree", list(HC.TREES))
def test_condition_kernel_vs_oracle(tree):
    """egoego_window_condition with head 15 and head 12 at (B, Tw) = (24, 1), (24, 31), (5, 120): positions and 6D element-wise
    (every other rotation dim must be 0, every other joint the normalised origin), recover up to sign."""
    c = HC.condition_case(tree)
    led = _Ledger()
    for shape, sl in HC.CONDITION_SLICES.items():
        pos, quat = np.ascontiguousarray(c["pos"][sl]), np.ascontiguousarray(c["quat"][sl])
        want = (c["x_start"][sl], c["recover"][sl[0]])
        x, rec = hip_condition(c, _dev(pos), _dev(quat))
        assert x.shape == shape + (198,) and rec.shape == (shape[0], 1, 1, 4)
        led.hold(f"condition/head {c['head']}/{shape}", HC.condition_distances((x.cpu().numpy(), rec.cpu().numpy()), want),
                 HC.condition_distances(HC.plain_condition(c, pos, quat), want))
        others = np.ones(198, bool)
        others[66 + 6 * c["head"]:66 + 6 * c["head"] + 6] = False
        others[:66] = False
        assert not x.cpu().numpy()[..., others].any()
    led.close()


@pytest.mark.parametrize("tree", list(HC.TREES))
def test_prefix_kernel_vs_oracle(tree):
    """egoego_window_prefix at (B, Tw, n_last) = (9, 64, 10) [two 64-thread blocks], (9, 10, 10) [n_last = Tw], (3, 64, 1) and
    (70, 12, 1) [n_last = 1, two blocks]."""
    led = _Ledger()
    for shape in HC.PREFIX_SHAPES:
        c = HC.prefix_case(tree, *shape)
        got = hip_prefix(c, _dev(c["aa"]), _dev(c["root"]), c["n_last"])
        assert got.shape == (shape[0], shape[2], 198)
        led.hold(f"prefix/{tree}/{shape}", HC.prefix_distances(got.cpu().numpy(), c["prefix"]), HC.prefix_distances(HC.plain_prefix(c), c["prefix"]))
    led.close()


def test_rot6d_kernel_vs_oracle():
    """Well-conditioned rows (|a1| = 1.7, a2's orthogonal part 0.6) within the bound; degenerate rows (all zeros; a1 = 0, a2 = e_y;
    a1 = e_x, a2 = 2 e_x), where the clamped norms decide, equal to the oracle bit for bit and finite."""
    d6 = HC.rot6d_case()
    want = HO.rot6d_to_mat(HC.up(d6))
    e = np.abs(R.rotation_6d_to_matrix(torch.from_numpy(d6)).numpy() - want).max()
    d = np.abs(HC.up(hip_rot6d(_dev(d6)).cpu().numpy()) - want).max()
    print(f"  rot6d kernel {d:.3e}   E_plain {e:.3e}   bound {HC.bound(e, 1.0):.3e}")
    assert d <= HC.bound(e, 1.0)
    got = hip_rot6d(_dev(HC.ROT6D_EXACT)).cpu()
    assert bool(torch.isfinite(got).all())
    assert _same_bits(got, torch.from_numpy(HO.rot6d_to_mat(HC.up(HC.ROT6D_EXACT)).astype(np.float32)))


# ------------------------------------------------------------------------------------------ row independence, bit for bit
def test_convert_rows_do_not_depend_on_the_batch():
    c = HC.convert_case("chain")
    x, rec = _dev(c["x"]), _dev(c["rec"])
    full = hip_convert(c, x, rec)
    perm = [2, 0, 3, 1]
    assert all(_same_bits(a, b[perm]) for a, b in zip(hip_convert(c, x[perm], rec[perm]), full))
    for b in range(4):
        assert all(_same_bits(a, f[b:b + 1]) for a, f in zip(hip_convert(c, x[b:b + 1], rec[b:b + 1]), full)), b
    for k in (1, 17):  # the first k frames of a window do not change when the window is longer
        assert all(_same_bits(a, f[:, :k]) for a, f in zip(hip_convert(c, x[:, :k], rec), full)), k


def test_condition_rows_do_not_depend_on_the_batch():
    c = HC.condition_case("smplh")
    pos, quat = _dev(c["pos"]), _dev(c["quat"])
    full = hip_condition(c, pos, quat)
    perm = np.random.default_rng(5).permutation(24).tolist()
    assert all(_same_bits(a, b[perm]) for a, b in zip(hip_condition(c, pos[perm], quat[perm]), full))
    for b in (0, 17, 23):
        assert all(_same_bits(a, f[b:b + 1]) for a, f in zip(hip_condition(c, pos[b:b + 1], quat[b:b + 1]), full)), b
    for k in (1, 31):  # the condition depends on frame 0 and the frame itself only
        x, rec = hip_condition(c, pos[:, :k], quat[:, :k])
        assert _same_bits(x, full[0][:, :k]) and _same_bits(rec, full[1]), k


def test_prefix_rows_do_not_depend_on_the_batch():
    c = HC.prefix_case("smplh", 9, 64, 10)
    aa, root = _dev(c["aa"]), _dev(c["root"])
    full = hip_prefix(c, aa, root, 10)
    perm = [4, 8, 0, 2, 7, 1, 6, 3, 5]
    assert _same_bits(hip_prefix(c, aa[perm], root[perm], 10), full[perm])
    for b in (0, 5, 8):
        assert _same_bits(hip_prefix(c, aa[b:b + 1], root[b:b + 1], 10), full[b:b + 1]), b
    # frames before the last n_last are not read: the slice alone is the same window prefix
    assert _same_bits(hip_prefix(c, aa[:, -10:], root[:, -10:], 10), full)


# ------------------------------------------------------------------------------------------ the grid-stride loops
def test_convert_and_rot6d_past_the_launch_cap():
    """Both kernels launch at most 8192 x 256 threads and stride past that: B = 1600, T = 60 is 2 112 000 (window, frame, joint)
    items, 2 097 152 + 4097 6D rows leave the second round partial.  The inputs repeat the case
    batch on the device; the results must repeat the small call's bits."""
    c = HC.convert_case("smplh")
    x, rec = _dev(c["x"][:, :60]), _dev(c["rec"])
    small = hip_convert(c, x, rec)
    big = hip_convert(c, x.repeat(400, 1, 1), rec.repeat(400, 1, 1, 1))
    assert big[0].shape == (1600, 60, 22, 3) and 1600 * 60 * 22 > 8192 * 256
    for s, b in zip(small, big):
        assert _same_bits(b, s.repeat(400, *([1] * (s.dim() - 1))))
    d6 = _dev(HC.rot6d_case())
    n = 8192 * 256 + 4097
    reps = -(-n // d6.shape[0])
    small6 = hip_rot6d(d6)
    assert _same_bits(hip_rot6d(d6.repeat(reps, 1)[:n]), small6.repeat(reps, 1, 1)[:n])


# ------------------------------------------------------------------------------------------ the Python wrappers' inputs
def _strided(t):
    """The same values behind a stride of 2 in the last axis."""
    wide = torch.zeros(t.shape + (2,), dtype=t.dtype, device=t.device)
    wide[..., 0] = t
    v = wide[..., 0]
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def test_wrappers_take_float64_and_strided_inputs():
    """harness.convert_model_res_to_data / _window_condition_hip / _window_prefix_hip and rotations.rotation_6d_to_matrix on float64
    tensors and on non-contiguous views give the bits of the float32 contiguous call through the C ABI."""
    c = HC.convert_case("smplh")
    x, rec = _dev(c["x"][1:4, 23:64]), _dev(c["rec"][1:4])
    want = hip_convert(c, x, rec)
    for xx, rr in ((x, rec), (x.double(), rec.double()), (_strided(x), _strided(rec)), (x, c["rec"][1:4].astype(np.float64))):
        got = harness.convert_model_res_to_data(c["ds"], xx, rr)
        assert all(_same_bits(a, b) for a, b in zip(got, want))
    c = HC.condition_case("smplh")
    pos, quat = _dev(c["pos"][:, :31]), _dev(c["quat"][:, :31])
    want = hip_condition(c, pos, quat)
    for pp, qq in ((pos, quat), (pos.double(), quat.double()), (_strided(pos), _strided(quat)), (_dev(c["pos"])[:, :31], _dev(c["quat"])[:, :31])):
        got = harness._window_condition_hip(c["ds"], pp, qq)
        assert all(_same_bits(a, b) for a, b in zip(got, want))
    c = HC.prefix_case("smplh", 9, 64, 10)
    aa, root = _dev(c["aa"]), _dev(c["root"])
    want = hip_prefix(c, aa, root, 10)
    for a2, r2 in ((aa, root), (aa.double(), root.double()), (_strided(aa), _strided(root))):
        assert _same_bits(harness._window_prefix_hip(c["ds"], a2, r2, 10), want)
    d6 = _dev(HC.rot6d_case()[:1000])
    want = hip_rot6d(d6)
    for dd in (d6, d6.double(), _strided(d6), d6.reshape(10, 100, 6)):
        assert _same_bits(R.rotation_6d_to_matrix(dd).reshape(-1, 3, 3), want)


# ------------------------------------------------------------------------------------------ argument errors of the C ABI
def test_argument_errors_are_reported_before_any_launch():
    """EGOEGO_E_INVALID with its message; the buffers handed over are large enough for what is asked all the same."""
    bad_tree = (-1,) + (5,) * 21
    cp = HC.prefix_case("smplh", 3, 64, 1)
    aa, root = torch.zeros(5, 64, 22, 3, device="cuda"), torch.zeros(5, 64, 3, device="cuda")
    aa[1:4], root[1:4] = _dev(cp["aa"]), _dev(cp["root"])
    calls = [("n_last=65", lambda: hip_prefix(cp, aa[1:4], root[1:4], 65, rc_only=True)),
             ("n_last=0", lambda: hip_prefix(cp, aa[1:4], root[1:4], 0, rc_only=True, out_frames=1)),
             ("n_last=-1", lambda: hip_prefix(cp, aa[1:4], root[1:4], -1, rc_only=True, out_frames=1)),
             ("B=0", lambda: hip_prefix(cp, aa[1:4], root[1:4], 1, rc_only=True, B=0)),
             ("head_idx=22", lambda: hip_prefix(cp, aa[1:4], root[1:4], 1, rc_only=True, head=22)),
             ("not an earlier joint", lambda: hip_prefix(cp, aa[1:4], root[1:4], 1, rc_only=True, parents=bad_tree)),
             ("not an earlier joint", lambda: hip_prefix(cp, aa[1:4], root[1:4], 1, rc_only=True, parents=(-1, 0, 2) + tuple(range(2, 21))))]
    cc = HC.convert_case("smplh")
    x, rec = _dev(cc["x"][:2, :3]), _dev(cc["rec"][:2])
    calls += [("B=0", lambda: hip_convert(cc, x, rec, rc_only=True, B=0)), ("B=-1", lambda: hip_convert(cc, x, rec, rc_only=True, B=-1)),
              ("head_idx=22", lambda: hip_convert(cc, x, rec, rc_only=True, head=22)),
              ("not an earlier joint", lambda: hip_convert(cc, x, rec, rc_only=True, parents=bad_tree))]
    cd = HC.condition_case("smplh")
    pos, quat = _dev(cd["pos"][:2, :3]), _dev(cd["quat"][:2, :3])
    calls += [("B=0", lambda: hip_condition(cd, pos, quat, rc_only=True, B=0)), ("head_idx=22", lambda: hip_condition(cd, pos, quat, rc_only=True, head=22))]
    for text, call in calls:
        assert call() == -1, text  # EGOEGO_E_INVALID
        assert text in _lib.check.last_error(), (text, _lib.check.last_error())
    with pytest.raises(_lib.EgoEgoHipError, match="n_last=65"):
        _lib.check(hip_prefix(cp, aa[1:4], root[1:4], 65, rc_only=True))
    torch.cuda.synchronize()
    # and the same buffers in a valid call afterwards
    assert _same_bits(hip_prefix(cp, aa[1:4], root[1:4], 1), hip_prefix(cp, _dev(cp["aa"]), _dev(cp["root"]), 1))
