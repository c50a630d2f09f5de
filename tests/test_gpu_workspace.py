"""No result depends on what a workspace held on entry (include/egoego_hip.h, Conventions; the audit: DESIGN.md 4a and
tests/test_workspace_audit.py).

Every GPU entry point works in a caller-supplied workspace that the Python engines allocate with torch.empty: in a long-lived
process the block may come back from a freed int32 tensor of -1 (fp32 and bf16 NaN) or from a diverged loss.  Here every entry
point runs on workspaces filled, in place, with

    ZERO  all bytes 0x00                      0
    FF    all bytes 0xFF                      fp32 and bf16 NaN, int8 -1, int32 -1
    BIG   all bytes 0x7F                      fp32 and bf16 3.39e38 (finite), int8 127
    INF   the buffer as fp32, filled with +inf  as bf16: +inf and 0 alternating

and every result must be finite and torch.equal to the ZERO run of the same call on the same engine.  Stage 2: the whole
eng._ws[(B, T)] tensor is filled before EVERY call (pointers and captured graphs stay), then the one persistent region — the outlier
monitor — is re-established the documented way, eng.outlier_stats(B, T, reset=True), and nothing else.  Satellites: one warm-up call of
the shape, then eng._ws is filled before every call.  Equal bits prove nothing if every run is wrong, so one small configuration of
each module also compares its FF-filled result with the oracle and the bar of that module's own GPU test file.

Prepared forms (precision.prepare_int8_state) change tensors, not kernels: they are left out of the sweep.

What ran, on an MI355X (patterns ZERO / FF / BIG / INF everywhere; no dependence on the workspace contents was found):
  stage 2, every kernel form  5 forms x T in {120, 196, 30, 150}, every B of test_gpu_dispatch.SWEEP_B: denoise (kernel names against
                              the dispatch table), p_sample_ with injected and with Philox noise, the monitor after both
  stage 2, other entries      B = 3, T in {20, 65, 120, 196}, precisions 3 / 8 / 9, step graph on and off: ragged denoise, masked
                              denoise, 4-step ragged sample_loop_, 3-step ragged ddim_loop_ (eta 0.5), Philox, prefix, ids;
                              debug_stage at every stop, B in {2, 25}, T in {120, 196}
  stage 1                     headnet 31 x 1, gravitynet 120 x 2, headnet 128 x 2; W = 3, valid [window, 1, window // 2]
  flow CNN                    3 frames, default chunk and chunk_frames = 2
  body model                  V = 211, max_weights {4, 52}, joints {22, 52}, F = 33, default chunk and chunk_frames = 5
  window statistics           N = 3, W = 40, lengths [40, 0, 7]
Wall time of the file: 20 s for its 75 cases (satellites and anchors 2 s, the B = 3 stage-2 cases 7 s, the sweep 11 s); the slowest
case, T120-bf16x3 of the sweep, takes 1.4 s.
That the file can fail: with the sv8 clear of pack_inputs taken out of a scratch build, test_stage2_every_kernel_form[T196-i8x3]
fails at its first B under FF (77444 of the 78408 denoiser outputs differ from the ZERO run, by up to 4.0e-5: fmaxf drops the NaN
of the stale scales, so the damage is finite and silent)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import body_oracle as BO
import flow_cnn_oracle as FO
import stage1_oracle as S1O
from egoego_release_amd import ModelConfig, _lib, body, make_weights, stage1, synthetic
from egoego_release_amd.model import CondGaussianDiffusion
from oracle import egoego_oracle as O
from test_gpu_body import bound as body_bound, rel as body_rel
from test_gpu_dispatch import EXPECT, FLAG_FORMS, POSE_TOL, SLOTS, STOPS, SWEEP_B, _engine, _form_engine, expected_names
from test_gpu_flow_cnn import FEAT_BAR, _frames as flow_cnn_frames
from test_gpu_stage1 import _heads_oracle, rel as s1_rel

pytestmark = pytest.mark.gpu
P3, P8, P9 = _lib.PREC_BF16X3, _lib.PREC_I8X3, _lib.PREC_I8X3_FC
S1_BAR = 1e-4  # the bar of every assertion of tests/test_gpu_stage1.py (a literal there)
PATTERNS = ("ZERO", "FF", "BIG", "INF")
SEED = 0x9E3779B97F4A7C15


def fill(ws, pattern):
    """Overwrite every byte of the uint8 tensor `ws` in place."""
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() % 4 == 0 and ws.data_ptr() % 4 == 0
    if pattern == "ZERO":
        ws.zero_()
    elif pattern == "FF":
        ws.fill_(0xFF)
    elif pattern == "BIG":
        ws.fill_(0x7F)
    elif pattern == "INF":
        ws.view(torch.float32).fill_(float("inf"))
    else:
        raise ValueError(pattern)


def fill_stage2(eng, B, T, pattern):
    eng.workspace(B, T)  # the buffer (and, from the second call of a shape on, its captured graphs) exists
    fill(eng._ws[(B, T)], pattern)
    eng.outlier_stats(B, T, reset=True)  # the one persistent region, established the documented way


def fill_satellite(eng, pattern):
    assert eng._ws is not None, "one warm-up call of the shape comes first"
    fill(eng._ws, pattern)


def finite(*tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


def every_pattern(run, same, what):
    """run(pattern) -> result under that fill; same(got, base) -> None or what differs.  ZERO first: the others are held to it."""
    base = run("ZERO")
    for pattern in PATTERNS[1:]:
        d = same(run(pattern), base)
        assert d is None, f"{what}: workspace filled with {pattern}: {d}"
    return base


def same_tensors(got, base):
    for i, (g, b) in enumerate(zip(got, base)):
        if isinstance(g, torch.Tensor):
            if not finite(g):
                return f"result {i} is not finite ({int((~torch.isfinite(g)).sum())} values)"
            if not torch.equal(g, b):
                return f"result {i} differs from the ZERO run in {int((g != b).sum())} values, max |d| = {float((g - b).abs().max()):.3e}"
        else:
            if not all(np.isfinite(v) for v in g):
                return f"result {i} is not finite: {g}"
            if g != b:
                return f"result {i}: {g} against the ZERO run's {b}"
    return None


# ------------------------------------------------------------------------------------------------ stage 2: every kernel form
FORMS = (P3, P8, P9) + tuple(FLAG_FORMS)  # precisions 3, 8, 9, 9 + FC24, 8 + FFN16
FORM_IDS = {P3: "bf16x3", P8: "i8x3", P9: "i8x3fc", FLAG_FORMS[0]: "i8x3fc_fc24", FLAG_FORMS[1]: "i8x3_ffn16"}


@functools.lru_cache(maxsize=1)
def _inputs(T):
    """256 seeded windows per T, on the GPU (no oracle: only the inputs are needed)."""
    g = torch.Generator().manual_seed(8000 + T)
    x, xc, nz = (torch.randn(256, T, 198, generator=g).cuda() for _ in range(3))
    t = torch.randint(0, 1000, (256,), generator=g).cuda()
    return x, xc, nz, t


def _sweep_engine(T, form):
    if isinstance(form, tuple):
        m, eng, _ = _form_engine(T, form)
    else:
        m, eng = _engine(T, form)
    return m, eng


@pytest.mark.parametrize("T, form", [(T, f) for T in (120, 196, 30, 150) for f in FORMS],
                         ids=[f"T{T}-{FORM_IDS[f]}" for T in (120, 196, 30, 150) for f in FORMS])
def test_stage2_every_kernel_form(T, form):
    """Every B of the dispatch sweep (the smallest set of batches that reaches every kernel form; its large values are the dispatch
    thresholds themselves): denoise — the kernel of every launch site against the dispatch table, so coverage stays tied to it —,
    one p_sample_ step with injected and one with Philox noise, and the outlier monitor after the denoise and after the two steps.
    Stale pad rows, the phantom window of an odd B at T = 120 and keys Lr..Lp-1 of 208-row windows must not count anywhere."""
    m, eng = _sweep_engine(T, form)
    x, xc, nz, t = _inputs(T)
    for B in SWEEP_B[T]:
        xb, xcb, nzb, tb = x[:B].contiguous(), xc[:B].contiguous(), nz[:B].contiguous(), t[:B].contiguous()
        want = expected_names(form, T, B)

        def run(pattern):
            fill_stage2(eng, B, T, pattern)
            y = eng.denoise(xb, xcb, tb)
            names = {s: eng.last_kernel(s) for s in SLOTS}
            assert names == want, (T, B, pattern, {s: (names[s], want[s]) for s in SLOTS if names[s] != want[s]})
            mon_y = eng.outlier_stats(B, T)
            fill_stage2(eng, B, T, pattern)
            xi = eng.p_sample_(xb.clone(), xcb, tb, noise=nzb)
            fill_stage2(eng, B, T, pattern)
            xp = eng.p_sample_(xb.clone(), xcb, tb, noise_mode=_lib.NOISE_PHILOX, seed=SEED, window_offset=1000)
            return y, mon_y, xi, xp, eng.outlier_stats(B, T)

        every_pattern(run, same_tensors, f"{FORM_IDS[form]} T={T} B={B} (denoise, its monitor, p_sample injected, p_sample Philox, monitor)")
    assert (form, T) in EXPECT


# ------------------------------------------------------------------------------------------------ stage 2: the other entry points
@functools.lru_cache(maxsize=2)
def _small_model(T, prec, graph):
    cfg = ModelConfig(max_timesteps=T + 1)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs())
    m.load_state_dict(make_weights(cfg, 0), strict=False)
    m.hip_precision = prec
    m.hip_graph = graph
    m.hip_probe_at_pack = False  # (the explicit precision as it is: no measurement, the module's own weights)
    m = m.cuda()
    eng = m.hip_engine()
    assert m.hip_precision_used == prec and m._slot.plan["flags"] == 0 and not m._slot.plan["row_shift"], m._slot.plan
    return m, eng


def _ragged_same(lens):
    """Rows below a window's length: the ZERO run's bits.  Rows past it: finite under every pattern (the engine's promise)."""
    def same(got, base):
        for i, (g, b) in enumerate(zip(got, base)):
            if not finite(g):
                return f"result {i}: {int((~torch.isfinite(g)).sum())} values are not finite (rows past a length must be finite)"
            for w, n in enumerate(lens):
                if not torch.equal(g[w, :n], b[w, :n]):
                    return f"result {i}, window {w} (length {n}): differs from the ZERO run, max |d| = {float((g[w, :n] - b[w, :n]).abs().max()):.3e}"
        return None
    return same


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
@pytest.mark.parametrize("T", [20, 65, 120, 196])
@pytest.mark.parametrize("prec", [P3, P8, P9], ids=["bf16x3", "i8x3", "i8x3fc"])
def test_stage2_ragged_masked_and_loop_entry_points(prec, T, graph):
    """B = 3 windows of lengths [T, 11, T - 7], a 10-frame prefix: denoise(lengths), denoise(row_mask) on the masked context, a
    4-step sample_loop_ and a 3-step ddim_loop_ at eta 0.5, both with Philox noise, prefix, lengths and window ids; with the step graph
    (the first step of the ZERO run on the stream, the later ones and every other run as replays) and with hip_graph = False."""
    B = 3
    m, eng = _small_model(T, prec, graph)
    eng_m = m.hip_engine(masked=True)
    lens = [T, 11, T - 7]
    ids = [7, 1000, 123456]
    g = torch.Generator().manual_seed(9000 + T)
    x, xc = (torch.randn(B, T, 198, generator=g).cuda() for _ in range(2))
    prefix = torch.randn(B, 10, 198, generator=g).cuda()
    t = torch.randint(1, 1000, (B,), generator=g).cuda()
    mask = (torch.arange(T + 1)[None, :] <= torch.tensor(lens)[:, None]).float().cuda()
    tag = f"precision {prec} T={T} {'graph' if graph else 'no graph'}"

    def ragged(pattern):
        fill_stage2(eng, B, T, pattern)
        y = eng.denoise(x, xc, t, lengths=lens)
        fill_stage2(eng, B, T, pattern)
        xs = eng.sample_loop_(x.clone(), xc, 999, 4, noise_mode=_lib.NOISE_PHILOX, seed=SEED, prefix=prefix, lengths=lens, window_ids=ids)
        fill_stage2(eng, B, T, pattern)
        xd = eng.ddim_loop_(x.clone(), xc, [900, 500, 100], eta=0.5, noise_mode=_lib.NOISE_PHILOX, seed=SEED, prefix=prefix,
                            lengths=lens, window_ids=ids)
        return y, xs, xd

    base = every_pattern(ragged, _ragged_same(lens), f"{tag}: ragged denoise / sample_loop_ / ddim_loop_")
    assert not torch.equal(base[1], x) and not torch.equal(base[2], x)  # (the loops ran)

    def masked(pattern):
        fill_stage2(eng_m, B, T, pattern)
        return (eng_m.denoise(x, xc, t, row_mask=mask),)

    every_pattern(masked, same_tensors, f"{tag}: denoise(row_mask)")


@pytest.mark.parametrize("B", [2, 25])
@pytest.mark.parametrize("T", [120, 196])
@pytest.mark.parametrize("prec", [P3, P8, P9], ids=["bf16x3", "i8x3", "i8x3fc"])
def test_stage2_debug_stops(prec, T, B):
    """egoego_debug_stage carves the SAME buffer with the tile-aligned geometry: every stop of the dispatch test, every pattern."""
    m, eng = _small_model(T, prec, True)
    x, xc, _, t = _inputs(T)
    xb, xcb, tb = x[:B].contiguous(), xc[:B].contiguous(), t[:B].contiguous()
    for li, st in STOPS:
        def run(pattern):
            fill_stage2(eng, B, T, pattern)
            return (eng.debug_stage(xb, xcb, tb, li, st),)

        every_pattern(run, same_tensors, f"precision {prec} T={T} B={B}: debug stop {li}.{st}")


# ------------------------------------------------------------------------------------------------ stage 1
S1_CONFIGS = [("headnet", 31, 1), ("gravitynet", 120, 2), ("headnet", 128, 2)]


def _s1_case(kind, window, n_layers, W=3, seed=0):
    cfg = synthetic.Stage1Config(kind, window, n_layers)
    sd = synthetic.make_stage1_weights(kind, cfg, 300 + window + n_layers)
    rng = np.random.default_rng(window * 7 + n_layers + seed)
    valid = [window, 1, window // 2] + [int(v) for v in rng.integers(1, window + 1, max(W - 3, 0))]
    valid = valid[:W]
    feats = np.zeros((W, window, cfg.d_feats), np.float32)
    for w, n in enumerate(valid):
        feats[w, :n] = rng.standard_normal((n, cfg.d_feats))
    return cfg, sd, torch.from_numpy(feats), torch.tensor(valid, dtype=torch.int32)


def _s1_engine(cfg, sd):
    eng = stage1.Stage1Engine(cfg, "cuda:0")
    eng.load(sd)
    return eng


@pytest.mark.parametrize("kind, window, n_layers", S1_CONFIGS)
def test_stage1_encode(kind, window, n_layers):
    cfg, sd, feats, valid = _s1_case(kind, window, n_layers)
    assert cfg.d_feats == (18 if kind == "gravitynet" else 512)
    eng = _s1_engine(cfg, sd)
    f, v = feats.cuda(), valid.cuda()
    eng.encode(f, v, layers=True)  # warm-up: the buffer of this shape exists

    def run(pattern):
        fill_satellite(eng, pattern)
        out, layers = eng.encode(f, v, layers=True)
        return (out,) + tuple(layers)

    every_pattern(run, same_tensors, f"stage 1 {kind} window {window} x {n_layers} layers")


# ------------------------------------------------------------------------------------------------ flow CNN
@pytest.fixture(scope="module")
def flow_model():
    return stage1.FlowFeatureExtractor(seed=4).to("cuda:0")


@pytest.fixture(scope="module")
def flow_frames():
    return torch.from_numpy(synthetic.make_flows(6, 21))


@pytest.mark.parametrize("chunk", [0, 2], ids=["chunk_default", "chunk2"])
def test_flow_cnn_features_and_stages(flow_model, flow_frames, chunk):
    """3 frames: with chunk_frames = 2 the second chunk holds one frame, in buffers the first chunk filled with two."""
    mdl = flow_model if chunk == 0 else stage1.FlowFeatureExtractor(chunk_frames=chunk, state_dict=flow_model.state_dict()).to("cuda:0")
    fl = flow_frames[:3]
    mdl.extract(fl, stages=True)  # warm-up
    eng = mdl.engine()
    assert eng.chunk_frames == chunk

    def run(pattern):
        fill_satellite(eng, pattern)
        feats, stages = mdl.extract(fl, stages=True)
        assert len(stages) == 5
        return (feats,) + tuple(stages)

    every_pattern(run, same_tensors, f"flow CNN, 3 frames, chunk_frames {chunk}")


# ------------------------------------------------------------------------------------------------ body model
BODY_V, BODY_F = 211, 33  # F = 33: the last 32-frame tile of the pose features has 31 unwritten pad rows
BODY_SEQ = np.repeat(np.arange(3), [10, 12, 11])


@pytest.fixture(scope="module")
def body_models():
    return {nw: synthetic.make_body_model(10 + nw, n_verts=BODY_V, n_faces=40, max_weights=nw) for nw in (4, 52)}


@pytest.fixture(scope="module")
def body_inputs():
    aa, trans = synthetic.make_body_poses(70, 52, seed=7)
    betas = np.random.default_rng(8).uniform(-2.5, 2.5, (3, 16)).astype(np.float32)
    return aa, trans, betas


def _body_run(bm, aa, trans, betas, seq, nj):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = bm(root_orient=t(aa[:, 0]), pose_body=t(aa[:, 1:22].reshape(len(aa), 63)),
             pose_hand=t(aa[:, 22:].reshape(len(aa), 90)) if nj == 52 else None, betas=t(betas), trans=t(trans),
             seq_index=t(seq.astype(np.int32)), return_pose_offsets=True)
    return out.v, out.Jtr, out.pose_offsets


@pytest.mark.parametrize("chunk", [0, 5], ids=["chunk_default", "chunk5"])
@pytest.mark.parametrize("nj", [22, 52])
@pytest.mark.parametrize("nw", [4, 52])
def test_body_model_forward(body_models, body_inputs, nw, nj, chunk):
    aa, trans, betas = body_inputs
    bm = body.BodyModel(model=body_models[nw], device="cuda", chunk_frames=chunk)
    args = (aa[:BODY_F], trans[:BODY_F], betas, BODY_SEQ, nj)
    _body_run(bm, *args)  # warm-up
    eng = bm.engine()

    def run(pattern):
        fill_satellite(eng, pattern)
        return _body_run(bm, *args)

    every_pattern(run, same_tensors, f"body model max_weights {nw}, {nj} joints, F = {BODY_F}, chunk_frames {chunk}")


# ------------------------------------------------------------------------------------------------ window statistics
def test_window_statistics():
    """egoego_win_stats through the library with a workspace of the test's own (motion_data allocates its own internally): N = 3
    windows of W = 40 with lengths [40, 0, 7].  Minima and maxima are exact: the anchor is torch's own over the real frames."""
    lib = _lib.load()
    N, W = 3, 40
    g = torch.Generator().manual_seed(17)
    jpos, jvel = (torch.randn(N, W, 66, generator=g).cuda() for _ in range(2))
    lens = torch.tensor([40, 0, 7], dtype=torch.int32).cuda()
    nbytes = lib.egoego_win_stats_workspace_bytes(N, W)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(pattern):
        fill(ws, pattern)
        out = torch.empty(4, 66, device="cuda")
        _lib.check_win(lib.egoego_win_stats(jpos.data_ptr(), jvel.data_ptr(), lens.data_ptr(), N, W, out.data_ptr(), ws.data_ptr(), nbytes, stream))
        return (out,)

    base = every_pattern(run, same_tensors, "egoego_win_stats")[0]
    real = torch.cat((jpos[0], jpos[2, :7])), torch.cat((jvel[0], jvel[2, :7]))
    want = torch.stack((real[0].amin(0), real[0].amax(0), real[1].amin(0), real[1].amax(0)))
    assert torch.equal(base, want)


# ------------------------------------------------------------------------------------------------ call history on the grow-only buffers
def test_a_small_call_after_a_large_one_on_the_grow_only_buffers(flow_model, flow_frames, body_models, body_inputs):
    """_engine.ContextEngine._workspace only grows: after a large call a small one works in the front of the large call's buffer,
    on whatever that left there.  It must have the bits of the same call on a fresh engine."""
    cfg, sd, feats, valid = _s1_case("headnet", 31, 1, W=40)
    used, fresh = _s1_engine(cfg, sd), _s1_engine(cfg, sd)
    used.encode(feats.cuda(), valid.cuda(), layers=True)
    n_large = used._ws.numel()
    small = (feats[:3].contiguous().cuda(), valid[:3].contiguous().cuda())
    a, b = used.encode(*small, layers=True), fresh.encode(*small, layers=True)
    assert used._ws.numel() == n_large > fresh._ws.numel()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and finite(*a), "stage 1"

    other = stage1.FlowFeatureExtractor(state_dict=flow_model.state_dict()).to("cuda:0")
    flow_model.extract(flow_frames, stages=True)
    fa, sa = flow_model.extract(flow_frames[:2], stages=True)
    fb, sb = other.extract(flow_frames[:2], stages=True)
    assert flow_model.engine()._ws.numel() > other.engine()._ws.numel()
    assert torch.equal(fa, fb) and all(torch.equal(u, v) for u, v in zip(sa, sb)) and finite(fa, *sa), "flow CNN"

    aa, trans, betas = body_inputs
    seq70 = np.repeat(np.arange(3), [10, 25, 35])
    used_b, fresh_b = (body.BodyModel(model=body_models[4], device="cuda") for _ in range(2))
    _body_run(used_b, aa, trans, betas, seq70, 52)
    ra = _body_run(used_b, aa[:5], trans[:5], betas, seq70[:5], 52)
    rb = _body_run(fresh_b, aa[:5], trans[:5], betas, seq70[:5], 52)
    assert used_b.engine()._ws.numel() > fresh_b.engine()._ws.numel()
    assert all(torch.equal(u, v) for u, v in zip(ra, rb)) and finite(*ra), "body model"


# ------------------------------------------------------------------------------------------------ one anchor per module
def test_anchor_stage2_ff_filled_against_the_oracle():
    """Precision 9, T = 120, B = 3 on an FF-filled workspace against the fp32 oracle at the project's pose bar."""
    T, B = 120, 3
    m, eng = _small_model(T, P9, True)
    g = torch.Generator().manual_seed(31)
    x, xc = torch.randn(B, T, 198, generator=g), torch.randn(B, T, 198, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    fill_stage2(eng, B, T, "FF")
    y = eng.denoise(x.cuda(), xc.cuda(), t.cuda()).cpu()
    with torch.no_grad():
        want = O.denoise(make_weights(ModelConfig(max_timesteps=T + 1), 0), torch.cat((x, xc), -1), t)
    e = float((y - want).abs().max())
    print(f"anchor stage 2 (FF): max |HIP - oracle| = {e:.3e}")
    assert e < POSE_TOL, e


def test_anchor_stage1_ff_filled_against_the_oracle():
    kind, window, n_layers = S1_CONFIGS[0]
    cfg, sd, feats, valid = _s1_case(kind, window, n_layers)
    eng = _s1_engine(cfg, sd)
    f, v = feats.cuda(), valid.cuda()
    eng.encode(f, v, layers=True)
    fill_satellite(eng, "FF")
    out, layers = eng.encode(f, v, layers=True)
    ref = S1O.decoder(sd, feats, valid, n_layers)
    for l in range(n_layers):
        e = (layers[l].cpu() - ref[l]).abs().max().item()
        assert e < S1_BAR, (l, e)
    rh = _heads_oracle(sd, kind, ref[-1], valid)
    mk = torch.arange(window)[None, :] < valid[:, None].long()
    for c in range(4):
        assert s1_rel(out.cpu()[..., c][mk], rh[..., c][mk]) < S1_BAR, c


def test_anchor_flow_cnn_ff_filled_against_the_oracle(flow_model):
    """FEAT_BAR is a ratio, max |HIP - fp64| / max |fp64| over the eight frames of test_gpu_flow_cnn._frames() (its +-40 px frame sets
    the denominator), so the anchor measures on those frames: on three plain ego-motion fields alone the same absolute error is 2.7e-5
    of their smaller maximum (measured, with bits equal to the ZERO run)."""
    fl = torch.from_numpy(flow_cnn_frames())
    flow_model.extract(fl)
    fill_satellite(flow_model.engine(), "FF")
    feats = flow_model.extract(fl)
    ref, _ = FO.forward({k: v.cpu() for k, v in flow_model.state_dict().items()}, fl.numpy(), torch.float64)
    ef = float((feats.double().cpu() - ref).abs().max() / ref.abs().max())
    e3 = float((feats[:3].double().cpu() - ref[:3]).abs().max() / ref[:3].abs().max())
    print(f"anchor flow CNN (FF): features {ef:.2e} (max |fp64| {float(ref.abs().max()):.3f}); its first three frames alone {e3:.2e} "
          f"(max |fp64| {float(ref[:3].abs().max()):.3f})")
    assert ef < FEAT_BAR, ef


def test_anchor_body_model_ff_filled_against_the_oracle(body_models, body_inputs):
    aa, trans, betas = body_inputs
    bm = body.BodyModel(model=body_models[4], device="cuda")
    args = (aa[:BODY_F], trans[:BODY_F], betas, BODY_SEQ, 52)
    _body_run(bm, *args)
    fill_satellite(bm.engine(), "FF")
    v, jtr, off = _body_run(bm, *args)
    ref = BO.forward(body_models[4], aa[:BODY_F], trans[:BODY_F], betas[BODY_SEQ])
    for k, got in (("v", v), ("Jtr", jtr), ("offsets", off)):
        e = body_rel(got, ref[k])
        assert e < body_bound(k), (k, e, body_bound(k))
