#!/usr/bin/env python3
"""Body-model timing: BodyModel (the SMPL-H forward on libegoego_hip) on 139, 8 x 139 and 64 x 139 frames of the 6890-vertex
synthetic model, with 22-joint and with 52-joint poses, against the same computation as stock fp32 torch ops on the GPU.

    python tools/body_model_bench.py [--frames 139,1112,8896] [--iters 30] [--chunk-frames N] [--out profiles/body_model_bench.json]

Times are CUDA events around one call, inputs already on the GPU, one sequence per 139 frames: after one warm-up call of the
same shape, --iters calls are timed one by one; the median is reported with the smallest and largest next to it (the spread; the
clocks are whatever the device runs at, nothing is pinned).  The torch baseline runs in chunks of 256 frames (its [frames, V, 3, 4] blend matrices would not fit otherwise) and, like
the reference, always contracts all 459 pose features; its Rodrigues clamps the angle at 1e-12 instead of switching to the series,
which is all a baseline needs.  FLOPs are algorithmic: 2 * 3 V * K for the pose blend shapes (K = 459, or
189 for a 22-joint pose) plus 2 * 12 * n_weights + 18 per vertex for the skinning.  The fraction of peak is the blend-shape
FLOPs over the time of the WHOLE call (all four kernels, launches included) against the bf16 dense peak (2.5 PFLOP/s); it is an
end-to-end figure, not the hot kernel's share: that comes from a kernel trace of this tool taken in a run of its own
(`rocprofv3 --kernel-trace -- python tools/body_model_bench.py --no-torch`, summarised in profiles/body_model_kernel_stats.csv and
profiles/body_model_dispatches.csv; DESIGN.md §5e derives the share from the kernel's own time).  Split-bf16
issues three MFMAs per product.
Prints one JSON line per size and writes everything to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import body, synthetic  # noqa: E402

BF16_PEAK = 2.5e15
T_SEQ = 139


def rodrigues(aa):
    a = aa.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    x, y, z = (aa / a).unbind(-1)
    s, c = torch.sin(a[..., 0]), torch.cos(a[..., 0])
    o = 1 - c
    return torch.stack([c + o * x * x, o * x * y - s * z, o * x * z + s * y, o * x * y + s * z, c + o * y * y, o * y * z - s * x,
                        o * x * z - s * y, o * y * z + s * x, c + o * z * z], -1).reshape(aa.shape[:-1] + (3, 3))


def torch_body(m, par, pose, trans, betas, seq, chunk=256):
    """The forward as fp32 torch ops on the GPU (pose [N, 52, 3]); the shape blend and the joint regression once per sequence."""
    vs = m["v_template"][None] + torch.einsum("vcb,sb->svc", m["shapedirs"], betas)
    Js = torch.einsum("jv,svc->sjc", m["J_regressor"], vs)
    pd = m["posedirs"].reshape(-1, 459)
    eye = torch.eye(3, device=pose.device)
    outs = []
    for i in range(0, pose.shape[0], chunk):
        R, J, v0 = rodrigues(pose[i:i + chunk]), Js[seq[i:i + chunk]], vs[seq[i:i + chunk]]
        n = R.shape[0]
        off = ((R[:, 1:] - eye).reshape(n, -1) @ pd.T).reshape(n, -1, 3)
        Gr, Gt = [R[:, 0]], [J[:, 0]]
        for j in range(1, 52):
            p = par[j]
            Gr.append(Gr[p] @ R[:, j])
            Gt.append((Gr[p] @ (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[p])
        Gr, Gt = torch.stack(Gr, 1), torch.stack(Gt, 1)
        A = torch.cat([Gr, (Gt - (Gr @ J[..., None])[..., 0])[..., None]], -1).reshape(n, 52, 12)
        T = (m["weights"] @ A).reshape(n, -1, 3, 4)
        vp = v0 + off
        outs.append((T[..., :3] @ vp[..., None])[..., 0] + T[..., 3] + trans[i:i + chunk, None])
    return torch.cat(outs)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="139,1112,8896")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--chunk-frames", type=int, default=0, help="frames per pass through the workspace (0 = the library's default)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "body_model_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    arrays = synthetic.make_body_model(0)
    bm = body.BodyModel(model=arrays, device=dev, chunk_frames=a.chunk_frames)
    e = bm.engine()
    V, nw = e.n_verts, e.n_weights
    m = {k: torch.from_numpy(arrays[k].astype(np.float32)).to(dev) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    par = [int(p) for p in synthetic.body_model_parents()]
    res = {"n_verts": V, "n_weights": nw, "bf16_peak": BF16_PEAK, "chunk_frames": e.chunk_frames or 8192,
           "flow_cnn_bf16_peak_fraction": 0.062, "iters": a.iters, "warmup_calls": 1,
           "device": torch.cuda.get_device_name(0), "sizes": []}
    for n in [int(v) for v in a.frames.split(",")]:
        S = (n + T_SEQ - 1) // T_SEQ
        aa, trans = synthetic.make_body_poses(n, 52, seed=1, amplitude=1.0)
        aa, trans = torch.from_numpy(aa).to(dev), torch.from_numpy(trans).to(dev)
        betas = torch.from_numpy(np.random.default_rng(2).uniform(-2, 2, (S, 16)).astype(np.float32)).to(dev)
        seq = torch.arange(S, dtype=torch.int32, device=dev).repeat_interleave(T_SEQ)[:n].contiguous()
        for nj in (22, 52):
            pose = aa.clone()
            if nj == 22:
                pose[:, 22:] = 0
            hand = pose[:, 22:].reshape(n, 90).contiguous() if nj == 52 else None
            ro, pb = pose[:, 0].contiguous(), pose[:, 1:22].reshape(n, 63).contiguous()
            call = lambda: bm(root_orient=ro, pose_body=pb, pose_hand=hand, betas=betas, trans=trans, seq_index=seq)  # noqa: E731
            t_hip, t_lo, t_hi = timed(call, a.iters)
            K = 459 if nj == 52 else 189
            gemm = 2.0 * 3 * V * K * n
            row = {"frames": n, "joints": nj, "hip_ms": round(t_hip, 3), "hip_ms_min": round(t_lo, 3), "hip_ms_max": round(t_hi, 3),
                   "frames_per_s": round(n / t_hip * 1e3),
                   "gemm_gflop": round(gemm / 1e9, 2), "skin_gflop": round((2.0 * 12 * nw + 18) * V * n / 1e9, 2),
                   "hip_gemm_tflops": round(gemm / t_hip / 1e9, 2), "bf16_peak_fraction": round(gemm / (t_hip * 1e-3) / BF16_PEAK, 4),
                   "output_gb_per_s": round(n * V * 12 / t_hip / 1e6, 1)}
            if not a.no_torch:
                with torch.no_grad():
                    t_t, tt_lo, tt_hi = timed(lambda: torch_body(m, par, pose, trans, betas, seq.long()), max(3, a.iters // 6))
                    k = min(n, 139)
                    d = float((torch_body(m, par, pose[:k], trans[:k], betas, seq[:k].long()) - call().v[:k]).abs().max())
                row.update(torch_fp32_ms=round(t_t, 3), torch_fp32_ms_min=round(tt_lo, 3), torch_fp32_ms_max=round(tt_hi, 3),
                           torch_iters=max(3, a.iters // 6), speedup=round(t_t / t_hip, 2), max_abs_diff_vs_torch=d)
            res["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
