"""The stage-2 training loop: the reference's Trainer.train() (trainer_amass_cond_motion_diffusion.py:124-205) without wandb and
visualisation, over the fused parameter update of optim.py.

    trainer = Stage2Trainer(model, DataLoader(MotionWindowDataset(windows, stats), batch_size=32, shuffle=True),
                            results_folder="weights", fused=True, host_check=50)
    trainer.train(10000)          # -> model-<milestone>.pt with the reference's keys {'step', 'model', 'ema', 'scaler'}
"""
import os

import torch

from . import harness
from .optim import EMA, FusedAdam, FusedAdamW
from .synthetic import head_condition_mask


def cycle(dl):
    while True:
        for data in dl:
            yield data


class Stage2Trainer:
    """Gradient accumulation, the NaN skip, Adam, the EMA and the checkpoints of the reference's Trainer.

    NaN handling is the reference's end state: an iteration with a NaN loss or a NaN gradient norm in any micro-batch changes
    nothing and does not advance `step`.  The reference checks after every backward; a NaN planted by one micro-batch survives
    accumulation, so ONE norm check on the accumulated gradients, together with the micro-batches' loss scalars, decides the same
    iterations.  The decision is taken on the device (optim.FusedAdam.step(losses=...)).

    host_check=1 reads the skip flag back every iteration: `self.step` and the save cadence are exactly the reference's.
    host_check=N reads the counters every N iterations only — no synchronisation in between — and sets `self.step` from the
    applied count then: the checkpoint of a milestone may be written up to N - 1 iterations late (with the weights of that later
    iteration), and `self.step` is only current right after a check or after train() returns.  A check writes one checkpoint, that
    of the latest milestone reached, so with fused=True save_and_sample_every must be at least host_check: a smaller value would
    let several milestones pass between two checks and lose all but the last without a word; the constructor raises ValueError.

    fused=False is the plain path (torch.optim.Adam, ema-pytorch's lerp; any device); it decides on the host every iteration
    (host_check is taken as 1)."""

    def __init__(self, model, train_batches, val_batches=None, *, ema_decay=0.995, train_lr=1e-4, gradient_accumulate_every=2,
                 amp=False, ema_update_every=10, save_and_sample_every=200000, results_folder="./results", fused=True, host_check=1,
                 save_optimizer=False, ema_kwargs=None):
        if host_check < 1:
            raise ValueError("host_check >= 1")
        if gradient_accumulate_every < 1 or gradient_accumulate_every > 8:
            raise ValueError("gradient_accumulate_every: 1 .. 8 (the update takes up to 8 loss scalars)")
        if fused and int(save_and_sample_every) < int(host_check):
            raise ValueError(f"save_and_sample_every = {save_and_sample_every} is below host_check = {host_check}: the host learns the step "
                             "count every host_check iterations and writes one checkpoint then, so the milestones in between would "
                             "never be written; check at least as often as you save")
        self.model = model
        self.fused = bool(fused)
        self.ema = EMA(model, beta=ema_decay, update_every=ema_update_every, fused=self.fused, **(ema_kwargs or {}))
        self.save_and_sample_every = int(save_and_sample_every)
        self.gradient_accumulate_every = int(gradient_accumulate_every)
        self.optimizer = FusedAdam(model.parameters(), lr=train_lr, fused=self.fused, modules=(model,), zero_grads=self.fused)
        self.step = 0
        self.amp = bool(amp)
        dev = next(model.parameters()).device
        self.scaler = torch.amp.GradScaler(dev.type, enabled=self.amp)
        self.results_folder = results_folder
        self.save_optimizer = bool(save_optimizer)
        self.host_check = 1 if not self.fused else int(host_check)
        self.window = int(model.seq_len)
        self.dl = cycle(train_batches)
        self.val_dl = None if val_batches is None else cycle(val_batches)
        self.last_losses = None
        self._saved = 0      # the last milestone written
        self._base = 0       # self.step minus the optimizer's applied count (a loaded checkpoint starts above 0)
        self.inject_loss = None  # tests: f(iteration, micro-batch, loss) -> loss

    # ------------------------------------------------------------------ checkpoints (trainer:99-122)
    def _path(self, milestone):
        return os.path.join(self.results_folder, "model-" + str(milestone) + ".pt")

    def save(self, milestone):
        data = {"step": self.step, "model": self.model.state_dict(), "ema": self.ema.state_dict(), "scaler": self.scaler.state_dict()}
        if self.save_optimizer:
            data["optimizer"] = self.optimizer.state_dict()
        os.makedirs(self.results_folder, exist_ok=True)
        torch.save(data, self._path(milestone))

    def load(self, milestone):
        self.load_weight_path(self._path(milestone))

    def load_weight_path(self, weight_path):
        data = torch.load(weight_path, map_location=next(self.model.parameters()).device)
        self.step = int(data["step"])
        self.model.load_state_dict(data["model"], strict=False)
        self.ema.load_state_dict(data["ema"], strict=False)
        self.scaler.load_state_dict(data["scaler"])
        if "optimizer" in data:
            self.optimizer.load_state_dict(data["optimizer"])
        for m in (self.model, self.ema.ema_model):
            if hasattr(m, "invalidate_engine"):
                m.invalidate_engine()
        self._base = self.step - self.optimizer.counters()["applied"]
        self._saved = self.step // self.save_and_sample_every

    # ------------------------------------------------------------------ the loop (trainer:124-205)
    def prep_padding_mask(self, data, seq_len):
        return harness.prep_padding_mask(data, torch.as_tensor(seq_len), self.window)

    def prep_head_condition_mask(self, data):
        return head_condition_mask(tuple(data.shape), device=data.device)

    def _sync_step(self):
        """host_check > 1: self.step from the device's applied count (one synchronisation)."""
        self.step = self._base + int(self.optimizer.counters()["applied"])

    def _iteration(self, idx):
        """One iteration: the micro-batches, then the update.  -> whether the host knows the step was applied (None: not read)."""
        dev = next(self.model.parameters()).device
        self.optimizer.zero_grad()
        losses = []
        for i in range(self.gradient_accumulate_every):
            batch = next(self.dl)
            data = batch["motion"].to(dev)
            padding_mask = self.prep_padding_mask(data, batch["seq_len"])
            with torch.autocast(dev.type, enabled=self.amp):
                cond_mask = self.prep_head_condition_mask(data)
                loss = self.model(data, cond_mask, padding_mask=padding_mask)
                if self.inject_loss is not None:
                    loss = self.inject_loss(idx, i, loss)
                self.scaler.scale(loss / self.gradient_accumulate_every).backward()
            losses.append(loss.detach())
        self.last_losses = losses
        # with amp on, a skipped iteration goes through GradScaler.update() like any other (found_inf halves the scale); the
        # reference leaves the scaler alone there.  amp off (the reference's default): both are no-ops.
        self.scaler.step(self.optimizer, ema=self.ema, losses=losses)
        self.scaler.update()
        if self.host_check == 1:
            return not bool(self.optimizer.last_skipped)
        return None

    def train(self, num_iterations):
        """Runs `num_iterations` iterations of the reference's loop (a skipped iteration counts as one, as there) -> self.step."""
        every = self.save_and_sample_every
        for idx in range(num_iterations):
            applied = self._iteration(idx)
            if applied:  # host_check = 1: the reference's bookkeeping, line by line (trainer:181-203)
                if self.step != 0 and self.step % every == 0:
                    self._sample_and_save(self.step // every)
                self.step += 1
            elif applied is None and (idx + 1) % self.host_check == 0:
                self._sync_step()
                if self.step // every > self._saved:
                    self._sample_and_save(self.step // every)
        if self.host_check > 1:
            self._sync_step()
        return self.step

    def _sample_and_save(self, milestone):
        self._saved = milestone
        if self.val_dl is not None:
            self.ema.ema_model.eval()
            with torch.no_grad():
                dev = next(self.model.parameters()).device
                val = next(self.val_dl)
                val_data = val["motion"].to(dev)
                cond_mask = self.prep_head_condition_mask(val_data)
                padding_mask = self.prep_padding_mask(val_data, val["seq_len"])
                self.last_sample = self.ema.ema_model.sample(val_data, cond_mask, padding_mask=padding_mask)
        self.save(milestone)


class Stage1Trainer:
    """The reference's two stage-1 loops (trainer_head_estimation.py:78-212 for HeadFormer, trainer_amass_head_gravity_normal_
    estimation.py:60-173 for HeadNormalFormer) over any iterable of reference-format batch dicts, without wandb and plots:
    per iteration forward, compute_loss, zero_grad, backward, clip_grad_norm_(1.0, error_if_nonfinite=False), AdamW step; StepLR
    (gamma 0.3; step_size 1000 for HeadNet and 2000 for GravityNet unless given) stepped per epoch; the validation loss in eval()
    mode under no_grad at the first iteration of every epoch with (epoch + 1) % validation_iter == 0 (at most val_batches_max
    batches; the HeadNet loop's 50); a checkpoint train-<epoch>.pt every save_interval epochs with the reference's keys {'epoch',
    'transformer_encoder_state_dict', 'optimizer_state_dict', 'loss'}, plus 'data_state' when train_batches has a state_dict() (a
    stage1_data.GravityBatches: its epoch count and shuffle generator, so that a resumed run draws the batches the uninterrupted
    run would have).

    The model is a stage1.HeadFormer or stage1.HeadNormalFormer with its parameters on the GPU; the trainer sets hip_training (the
    gradients come from egoego_s1_train_backward) and train() mode.  The update is clip_grad_norm_ and torch.optim.AdamW by default.
    fused_update=True makes it optim.FusedAdamW(max_grad_norm=max_grad_norm, zero_grads=True, skip_on="nonfinite"): norm, clip,
    decoupled decay, Adam and the gradients' zeros in three launches, with the same scheduler, history and checkpoint keys
    ('optimizer_state_dict' in AdamW's layout: a checkpoint of either path resumes under the other).  Two differences from the
    default path: the gradients are not rewritten with their clipped values (they are cleared), and a step whose gradient norm is
    not finite is skipped on the device (the parameters, moments and step counter stay), where the reference, like the default
    path, would multiply every gradient by NaN and fill the net with it.  Nothing is read back from the device inside an epoch;
    `history` holds one dict of epoch means (device work done once per epoch), `val_history` the validation means."""

    def __init__(self, model, train_batches, val_batches=None, *, lr=1e-4, step_size=None, gamma=0.3, validation_iter=1,
                 save_interval=50, save_dir="./results", val_batches_max=50, max_grad_norm=1.0, fused_update=False):
        self.model = model
        self.train_batches, self.val_batches = train_batches, val_batches
        self.headnet = model.cfg.kind == "headnet"
        self.keys = ("loss", "orient", "va", "dist") if self.headnet else ("loss", "normal")
        model.hip_training = True
        model.train()
        self.fused_update = bool(fused_update)
        if self.fused_update:
            self.optimizer = FusedAdamW(model.parameters(), lr=lr, max_grad_norm=max_grad_norm, modules=(model,), zero_grads=True,
                                        skip_on="nonfinite")
        else:
            self.optimizer = torch.optim.AdamW(model.parameters(), lr=lr)
        if step_size is None:
            step_size = 1000 if self.headnet else 2000
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=step_size, gamma=gamma)
        self.validation_iter, self.save_interval = int(validation_iter), int(save_interval)
        self.save_dir, self.val_batches_max, self.max_grad_norm = save_dir, int(val_batches_max), float(max_grad_norm)
        self.epoch = 0
        self.history, self.val_history = [], []
        self.last_loss = None

    def _path(self, epoch):
        return os.path.join(self.save_dir, "weights", f"train-{epoch}.pt")

    def save(self, epoch):
        os.makedirs(os.path.dirname(self._path(epoch)), exist_ok=True)
        data = {"epoch": epoch, "transformer_encoder_state_dict": self.model.state_dict(),
                "optimizer_state_dict": self.optimizer.state_dict(), "loss": self.last_loss}
        if hasattr(self.train_batches, "state_dict"):  # a batch source with epochs of its own (stage1_data.GravityBatches)
            data["data_state"] = self.train_batches.state_dict()
        torch.save(data, self._path(epoch))
        return self._path(epoch)

    def load(self, path):
        ck = torch.load(path, map_location=next(self.model.parameters()).device)
        self.model.load_state_dict(ck["transformer_encoder_state_dict"])
        self.optimizer.load_state_dict(ck["optimizer_state_dict"])
        self.epoch = int(ck["epoch"])
        self.last_loss = ck.get("loss")
        if "data_state" in ck and hasattr(self.train_batches, "load_state_dict"):
            self.train_batches.load_state_dict(ck["data_state"])

    def step(self, batch):
        """One iteration -> the loss parts (detached device scalars, in the order of self.keys)."""
        out = self.model(batch)
        parts = self.model.compute_loss(out, batch)
        self.optimizer.zero_grad()
        parts[0].backward()
        if not self.fused_update:  # (the fused step clips)
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm, error_if_nonfinite=False)
        self.optimizer.step()
        self.last_loss = parts[0].detach()
        return tuple(p.detach() for p in parts)

    def validate(self):
        """The mean loss parts over (at most val_batches_max of) the validation batches, in eval() mode under no_grad."""
        was_training = self.model.training
        self.model.eval()
        got = []
        with torch.no_grad():
            for i, batch in enumerate(self.val_batches):
                if i >= self.val_batches_max:
                    break
                got.append(torch.stack([p.detach().double() for p in self.model.compute_loss(self.model(batch), batch)]))
        self.model.train(was_training)
        if not got:
            return None
        return dict(zip(self.keys, torch.stack(got).mean(0).tolist()))

    def train(self, epochs):
        """Runs `epochs` more epochs -> self.epoch."""
        for _ in range(epochs):
            self.epoch += 1
            got = []
            for it, batch in enumerate(self.train_batches):
                got.append(torch.stack([p.double() for p in self.step(batch)]))
                if self.val_batches is not None and (self.epoch + 1) % self.validation_iter == 0 and it == 0:
                    v = self.validate()
                    if v is not None:
                        self.val_history.append(dict(v, epoch=self.epoch))
            if got:
                self.history.append(dict(zip(self.keys, torch.stack(got).mean(0).tolist()), epoch=self.epoch))
            self.scheduler.step()
            if self.epoch % self.save_interval == 0:
                self.save(self.epoch)
        return self.epoch
