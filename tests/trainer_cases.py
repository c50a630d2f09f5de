"""The small Stage2Trainer that tests/test_gpu_optim.py and tests/test_gpu_trainer.py build: a one-layer denoiser at 11 frames over
two batches of 2 windows, gradient_accumulate_every = 2 — one iteration consumes the whole two-batch cycle — and what such a
trainer holds on the device, cloned, for bit comparisons."""
import torch

from egoego_release_amd import ModelConfig, make_weights


def make_trainer(fused, folder, seed=0, keep_grads=False, **kw):
    """-> (cfg, the state dict the model started from, the trainer).  keep_grads: the fused step leaves the gradients in place
    (the plain path always does), for a test that reads them after the step."""
    from egoego_release_amd.model import CondGaussianDiffusion
    from egoego_release_amd.trainer import Stage2Trainer
    cfg = ModelConfig(n_dec_layers=1, max_timesteps=12)
    m = CondGaussianDiffusion(**cfg.ctor_kwargs(), loss_type="l1")
    sd = make_weights(cfg, seed)
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    m.hip_training = True
    m.train()
    gen = torch.Generator().manual_seed(5)
    batches = [{"motion": (torch.randn(2, 11, 198, generator=gen) * 0.5).cuda(), "seq_len": torch.tensor([11, 8])} for _ in range(2)]
    kw.setdefault("ema_update_every", 1)
    tr = Stage2Trainer(m, batches, fused=fused, results_folder=str(folder), gradient_accumulate_every=2, **kw)
    if keep_grads:
        tr.optimizer.zero_grads = False
    return cfg, sd, tr


def trainable(tr):
    return [(n, p) for n, p in tr.model.named_parameters() if p.requires_grad]


def adam_step(tr):
    """The Adam step counter where the path keeps it: the device's state block (fused) or the optimizer's state (plain)."""
    return int(tr.optimizer.counters()["adam_step"])


def device_state(tr):
    """Clones of everything an iteration may write: {name: tensor} over the parameters, both moments, the EMA's tensors and its two
    counters, and the Adam step counter."""
    out = {}
    shadow = dict(tr.ema.ema_model.named_parameters())
    for n, p in trainable(tr):
        out["p." + n] = p.detach().clone()
        st = tr.optimizer.state.get(p, {})
        for k in ("exp_avg", "exp_avg_sq"):
            if k in st:
                out[k + "." + n] = st[k].detach().clone()
        out["ema." + n] = shadow[n].detach().clone()
    out["ema.step"] = tr.ema.step.detach().clone()
    out["ema.initted"] = tr.ema.initted.detach().clone()
    out["adam_step"] = torch.tensor([adam_step(tr)])
    return out


def differing(a, b):
    """The names at which two device_state() dicts differ in any bit (or in their keys)."""
    if a.keys() != b.keys():
        return sorted(set(a) ^ set(b))
    bits = lambda t: t.cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.cpu()  # noqa: E731
    return [k for k in a if a[k].shape != b[k].shape or not torch.equal(bits(a[k]), bits(b[k]))]
