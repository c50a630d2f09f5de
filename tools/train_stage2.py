#!/usr/bin/env python3
"""Train the stage-2 diffusion model on prebuilt motion windows (needs a ROCm GPU): the reference's
trainer_amass_cond_motion_diffusion.py run_train over egoego_release_amd.trainer.Stage2Trainer.

    python tools/build_motion_windows.py --data train.p --test_data test.p --rest_offsets rest.npy --out data/
    python tools/train_stage2.py --windows data/train_diffusion_amass_window_120.p --stats data/min_max_mean_std_data_window_120.p \
        --val_windows data/test_diffusion_amass_window_120.p --save_dir weights/ --steps 10000 --hip_loss

Writes model-<milestone>.pt with the reference's keys {'step', 'model', 'ema', 'scaler'} (harness.load_stage2_checkpoint reads it).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--windows", required=True, help="<split>_diffusion_amass_window_<W>.p of tools/build_motion_windows.py")
    p.add_argument("--stats", required=True, help="min_max_mean_std_data_window_<W>.p of the training split")
    p.add_argument("--val_windows", default=None)
    p.add_argument("--save_dir", default="./results")
    p.add_argument("--steps", type=int, default=10000, help="iterations of the loop (a skipped one counts)")
    # the reference's flags (trainer_amass_cond_motion_diffusion.py parse_opt)
    p.add_argument("--window", type=int, default=120)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--n_dec_layers", type=int, default=4)
    p.add_argument("--n_head", type=int, default=4)
    p.add_argument("--d_k", type=int, default=256)
    p.add_argument("--d_v", type=int, default=256)
    p.add_argument("--d_model", type=int, default=512)
    p.add_argument("--diffusion_timesteps", type=int, default=1000)
    p.add_argument("--diffusion_objective", default="pred_x0", choices=("pred_x0", "pred_noise"))
    p.add_argument("--diffusion_loss_type", default="l1", choices=("l1", "l2"))
    p.add_argument("--gradient_accumulate_every", type=int, default=2)
    p.add_argument("--save_and_sample_every", type=int, default=200000)
    p.add_argument("--ema_update_every", type=int, default=10)
    p.add_argument("--amp", action="store_true")
    p.add_argument("--host_check", type=int, default=50, help="read the counters back every N iterations (1: every iteration)")
    p.add_argument("--hip_loss", action="store_true", help="loss and gradients on the HIP training step (model.hip_training)")
    p.add_argument("--plain_update", action="store_true", help="torch.optim.Adam and the plain EMA instead of the fused update")
    p.add_argument("--save_optimizer", action="store_true")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--weight_path", default=None, help="continue from a checkpoint")
    return p


def main(argv=None):
    opt = parser().parse_args(argv)
    import torch
    from torch.utils.data import DataLoader

    from egoego_release_amd.model import CondGaussianDiffusion
    from egoego_release_amd.motion_data import MotionWindowDataset, MotionWindows
    from egoego_release_amd.trainer import Stage2Trainer

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from build_motion_windows import load_any

    if not torch.cuda.is_available():
        raise SystemExit("train_stage2 needs a ROCm GPU")
    dev = torch.device("cuda")
    stats = load_any(opt.stats)
    sets = [MotionWindowDataset(MotionWindows.from_window_data_dict(load_any(path), window=opt.window, device=dev), stats)
            for path in (opt.windows, opt.val_windows) if path]
    torch.manual_seed(opt.seed)
    train = DataLoader(sets[0], batch_size=opt.batch_size, shuffle=True, num_workers=0)
    val = DataLoader(sets[1], batch_size=opt.batch_size, shuffle=False, num_workers=0) if len(sets) > 1 else None
    model = CondGaussianDiffusion(d_feats=198, d_model=opt.d_model, n_head=opt.n_head, n_dec_layers=opt.n_dec_layers, d_k=opt.d_k,
                                  d_v=opt.d_v, max_timesteps=opt.window + 1, out_dim=198, timesteps=opt.diffusion_timesteps,
                                  objective=opt.diffusion_objective, loss_type=opt.diffusion_loss_type, batch_size=opt.batch_size).to(dev)
    model.hip_training = bool(opt.hip_loss)
    model.train()
    trainer = Stage2Trainer(model, train, val, train_lr=opt.learning_rate, gradient_accumulate_every=opt.gradient_accumulate_every,
                            amp=opt.amp, ema_update_every=opt.ema_update_every, save_and_sample_every=opt.save_and_sample_every,
                            results_folder=opt.save_dir, fused=not opt.plain_update, host_check=opt.host_check,
                            save_optimizer=opt.save_optimizer)
    if opt.weight_path:
        trainer.load_weight_path(opt.weight_path)
    step = trainer.train(opt.steps)
    c = trainer.optimizer.counters()
    trainer.save("final")
    print({"step": step, "applied": c["applied"], "skipped": c["skipped"], "last_grad_norm": c["total_norm"],
           "last_losses": [float(l) for l in trainer.last_losses]})
    print("wrote", trainer._path("final"))


if __name__ == "__main__":
    main()
