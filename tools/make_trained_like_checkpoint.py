#!/usr/bin/env python3
"""A stage-2 checkpoint that is no longer the initialisation (repo code only; meant for the GPU box, works on CPU too).

The reference's pretrained weights (`pretrained_models/stage2_diffusion_4.pt`, /root/reference/README.md:51-55) are a download
this build cannot make, and every other weight in the tests is the seeded INITIALISATION distribution (LayerNorm gains 1 +- 0.1).
This script optimises the module's own training half — `CondGaussianDiffusion.forward` = the reference's
`p_losses` (l1 on pred_x0 with the head-condition mask, trainer_amass_cond_motion_diffusion.py:399-403, Adam, dropout on) —
for a few thousand steps on seeded synthetic motion windows (`synthetic.make_motion_windows`), so that the LayerNorm affines,
the projections and the FFN have moved where the data pushes them.  The result is what the trained-like parity tests
(tests/test_gpu_trained_like.py) and `bench.py --weights trained-like` sample from.

    python tools/make_trained_like_checkpoint.py --steps 2000 --out /tmp/trained_like.pt      (reference checkpoint layout)
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egoego_release_amd import ModelConfig, make_weights, head_condition_mask  # noqa: E402
from egoego_release_amd.synthetic import make_motion_windows  # noqa: E402


def train_like(steps=3000, seed=0, device=None, T=120, batch=32, lr=2e-4, log_every=0, pool=4096, hip=False, fused=False):
    """Returns (state_dict on the CPU, info).  Deterministic given (steps, seed, T, batch, lr, hip) on one device type.
    hip=True: loss and gradients come from the HIP training step (model.hip_training; needs a ROCm device) instead of autograd
    over the plain-PyTorch forward; the draws of t and of the noises are the same, the dropout masks are not.
    fused=True: the update is optim.FusedAdam with an optim.EMA written in the same call (the reference's beta 0.995, every 10
    steps), and info["ema"] is the EMA's state dict (a real EMA entry for the checkpoint); False: torch.optim.Adam, no EMA.
    lr: twice the reference's 1e-4 (trainer:39); 1e-3 collapses the post-LN stack to the mean pose within 2000 steps (measured, round 4)."""
    from egoego_release_amd.model import CondGaussianDiffusion

    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    cfg = ModelConfig(max_timesteps=T + 1)
    model = CondGaussianDiffusion(**cfg.ctor_kwargs())
    model.load_state_dict(make_weights(cfg, seed), strict=False)
    model = model.to(dev)
    model.hip_training = bool(hip)
    model.train()
    data = make_motion_windows(pool, T, seed=seed + 1, device=dev)
    mask = head_condition_mask((batch, T, cfg.d_feats), device=dev)
    ema = None
    if fused:
        from egoego_release_amd.optim import EMA, FusedAdam
        on_gpu = dev.type == "cuda"
        ema = EMA(model, beta=0.995, update_every=10, fused=on_gpu)
        opt = FusedAdam(model.parameters(), lr=lr, fused=on_gpu, modules=(model,))
    else:
        opt = torch.optim.Adam(model.parameters(), lr=lr)
    g = torch.Generator(device="cpu").manual_seed(seed + 17)
    torch.manual_seed(seed + 23)  # q_sample noise, the timestep draw and dropout use the global generator (like the reference)
    t0, first, last = time.time(), None, None
    for it in range(steps):
        idx = torch.randint(0, pool, (batch,), generator=g).to(dev)
        loss = model(data[idx], mask)
        opt.zero_grad(set_to_none=True) if ema is None else opt.zero_grad()
        loss.backward()
        opt.step() if ema is None else opt.step(ema=ema, losses=[loss.detach()])
        if it < 20:
            first = loss.item() if first is None else 0.9 * first + 0.1 * loss.item()
        if it >= steps - 50:
            last = loss.item() if last is None else 0.9 * last + 0.1 * loss.item()
        if log_every and it % log_every == 0:
            print(f"step {it:5d}  l1 {loss.item():.4f}", flush=True)
    model.invalidate_engine()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    gains = [v.abs() for k, v in sd.items() if k.endswith("layer_norm.weight")]
    info = {"steps": steps, "seed": seed, "lr": lr, "batch": batch, "T": T, "device": str(dev), "hip": bool(hip), "fused": bool(fused), "seconds": time.time() - t0,
            "loss_first": first, "loss_last": last,
            "gain_spread": max(float(a.max() / a.median()) for a in gains),
            "beta_absmax": max(float(v.abs().max()) for k, v in sd.items() if k.endswith("layer_norm.bias"))}
    if ema is not None:
        info["ema"] = {k: v.detach().cpu().clone() for k, v in ema.state_dict().items()}
    return sd, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--device", default=None)
    ap.add_argument("--out", default="trained_like.pt")
    ap.add_argument("--hip", action="store_true", help="train through the HIP training step (CondGaussianDiffusion.hip_training)")
    ap.add_argument("--fused", action="store_true", help="update through optim.FusedAdam + optim.EMA and write the EMA's own entry")
    args = ap.parse_args()
    sd, info = train_like(args.steps, args.seed, args.device, args.window, args.batch, args.lr, log_every=max(1, args.steps // 10), hip=args.hip,
                          fused=args.fused)
    ema_entry = info.pop("ema", None) or {"ema_model." + k: v for k, v in sd.items()}
    # the reference's checkpoint layout (Trainer.save, trainer_amass_cond_motion_diffusion.py:99-106; ema-pytorch prefixes)
    torch.save({"step": args.steps, "model": sd, "ema": ema_entry, "scaler": {}}, args.out)
    print(info)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
