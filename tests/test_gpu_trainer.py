"""Stage2Trainer on its fused path (egoego_release_amd/trainer.py over optim.FusedAdam / optim.EMA on the HIP library): a NaN
micro-batch, host_check > 1, and resuming from a checkpoint.  The trainers are tests/trainer_cases.py's: one layer, 11 frames, two
batches of 2 windows, two micro-batches per iteration.  Every run starts from torch.manual_seed(s): the draws of two runs are then
equal, the gradients of the HIP training step have the same bits from run to run, and runs compare bit for bit."""
import pytest
import torch

import optim_oracle as OO
import trainer_cases as TC

pytestmark = pytest.mark.gpu

RESUME = dict(ema_update_every=2, ema_kwargs={"update_after_step": 2})


def _planted(accumulate=2):
    """inject_loss: the loss of micro-batch 1 of the trainer's iteration 1 (counted over all train() calls) becomes NaN."""
    calls = {"n": 0}

    def inject(idx, i, loss):
        iteration = calls["n"] // accumulate
        calls["n"] += 1
        return loss * float("nan") if (iteration, i) == (1, 1) else loss
    return inject


def _grads(tr):
    return [p.grad for _, p in TC.trainable(tr)]


@pytest.mark.parametrize("fused", [True, False])
def test_a_nan_micro_batch_changes_nothing(tmp_path, fused):
    """Three iterations, the second with a NaN loss in its second micro-batch: across it every parameter, both moments, every
    EMA tensor, the EMA's two counters and the Adam step keep their bits; 2 applied, 1 skipped, step == 2 — on both paths.  The
    fused step clears the gradients of the skipped iteration itself; the plain path leaves them (NaN) to the next iteration's
    zero_grad().  train(3) in one call ends on the bits of three train(1) calls."""
    _, _, tr = TC.make_trainer(fused, tmp_path / "a")
    tr.inject_loss = _planted()
    torch.manual_seed(3)
    assert tr.train(1) == 1
    before = TC.device_state(tr)
    assert int(before["adam_step"]) == 1 and int(before["ema.step"]) == 1
    assert tr.train(1) == 1
    after = TC.device_state(tr)
    assert TC.differing(before, after) == []
    c = tr.optimizer.counters()
    assert (c["applied"], c["skipped"], c["last_skip"]) == (1, 1, 1) and tr.step == 1
    if fused:
        assert not any(bool(g.any()) for g in _grads(tr))  # (NaN != 0: a NaN left behind counts)
    else:
        assert any(bool(torch.isnan(g).any()) for g in _grads(tr))
    assert tr.train(1) == 2
    end = TC.device_state(tr)
    c = tr.optimizer.counters()
    assert (c["applied"], c["skipped"], c["last_skip"]) == (2, 1, 0) and tr.step == 2
    assert int(end["adam_step"]) == 2 and int(end["ema.step"]) == 2
    assert all(bool(torch.isfinite(g).all()) for g in _grads(tr))
    moved = TC.differing(after, end)
    names = [n for n, _ in TC.trainable(tr)]  # (a tensor whose gradient is exactly zero would stay: most is what the run shows)
    for kind in ("p.", "exp_avg.", "exp_avg_sq.", "ema."):
        assert sum(kind + n in moved for n in names) > len(names) // 2, kind
    _, _, whole = TC.make_trainer(fused, tmp_path / "b")
    whole.inject_loss = _planted()
    torch.manual_seed(3)
    assert whole.train(3) == 2
    assert TC.differing(end, TC.device_state(whole)) == []
    c = whole.optimizer.counters()
    assert (c["applied"], c["skipped"]) == (2, 1)


def _strict(fn):
    """fn under torch.cuda.set_sync_debug_mode("error"): a synchronisation inside it raises."""
    def wrapped(*args, **kwargs):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn(*args, **kwargs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return wrapped


def test_host_check_changes_only_what_the_host_knows(tmp_path):
    """host_check = 1 against host_check = 3 over 7 iterations with the same planted NaN and save_and_sample_every = 3: the device
    ends on the same bits and counters, `step` is equal, and the milestone the first run wrote exists for the second with a stored
    step of at least milestone * 3 and less than milestone * 3 + 3 (up to host_check - 1 iterations late).

    The sync debug mode is "error" around scaler.step / scaler.update of every iteration of the host_check = 3 run, the first one
    included, and not around the micro-batches: harness.prep_padding_mask builds each padding mask on the host from the batch's
    host-side `seq_len` and copies it over, which the mode counts as a synchronisation whatever the trainer does (measured: it is
    the only one the mode reports in an iteration's micro-batches)."""
    runs = {}
    for hc in (1, 3):
        _, _, tr = TC.make_trainer(True, tmp_path / f"check{hc}", host_check=hc, save_and_sample_every=3, save_optimizer=True)
        tr.inject_loss = _planted()
        if hc == 3:
            tr.scaler.step, tr.scaler.update = _strict(tr.scaler.step), _strict(tr.scaler.update)
        torch.manual_seed(4)
        assert tr.train(7) == 6
        runs[hc] = tr
    a, b = runs[1], runs[3]
    assert TC.differing(TC.device_state(a), TC.device_state(b)) == []
    ca, cb = a.optimizer.counters(), b.optimizer.counters()
    for k in ("adam_step", "applied", "skipped", "last_skip", "total_norm"):
        assert ca[k] == cb[k], k
    assert (ca["applied"], ca["skipped"]) == (6, 1) and a.step == b.step == 6
    written = sorted(p.name for p in (tmp_path / "check1").iterdir())
    assert written == ["model-1.pt"]
    for name in written:
        milestone = int(name[len("model-"):-len(".pt")])
        assert torch.load(tmp_path / "check1" / name, map_location="cpu")["step"] == milestone * 3
        late = torch.load(tmp_path / "check3" / name, map_location="cpu")
        assert milestone * 3 <= late["step"] < milestone * 3 + 3
        assert sorted(late) == ["ema", "model", "optimizer", "scaler", "step"]
        assert int(late["optimizer"]["state"][0]["step"]) == late["step"]  # no skip between: the Adam step of that later iteration
    assert sorted(p.name for p in (tmp_path / "check3").iterdir()) == written


@pytest.mark.parametrize("host_check", [1, 2])
def test_resume_equals_not_stopping(tmp_path, host_check):
    """A: train(3), train(2).  B: train(3), save with the optimizer; a fresh model (other weights) and trainer, load, train(2).
    ema_update_every = 2, update_after_step = 2: the EMA copies at counters 0 and 2, the first call past update_after_step (4)
    copies and sets `initted`, and 6 is the first lerp — so both go on for two more iterations.  Bit-identical throughout.
    host_check = 2 after the load: `step` then comes from the loaded step plus the device's applied count.  Last, the same file
    into B itself, which has stepped by then: it lands on A's bits at step 5 again."""
    _, _, a = TC.make_trainer(True, tmp_path / "a", **RESUME)
    torch.manual_seed(1)
    assert a.train(3) == 3
    torch.manual_seed(2)
    assert a.train(2) == 5
    _, _, b0 = TC.make_trainer(True, tmp_path / "b", save_optimizer=True, **RESUME)
    torch.manual_seed(1)
    assert b0.train(3) == 3
    b0.save(1)
    saved = TC.device_state(b0)
    assert int(saved["ema.step"]) == 3 and float(saved["ema.initted"]) == 0.0
    _, _, b = TC.make_trainer(True, tmp_path / "b", seed=9, host_check=host_check, **RESUME)
    assert TC.differing({k: v for k, v in saved.items() if k.startswith("p.")}, {k: v for k, v in TC.device_state(b).items() if k.startswith("p.")})
    b.load(1)
    assert b.step == 3 and int(b.ema.step) == 3
    torch.manual_seed(2)
    assert b.train(2) == 5
    sa, sb = TC.device_state(a), TC.device_state(b)
    at5 = sa
    assert TC.differing(sa, sb) == []
    assert int(sb["adam_step"]) == 5 and int(sb["ema.step"]) == 5 and float(sb["ema.initted"]) == 1.0 and a.step == b.step == 5
    assert b.optimizer.counters()["applied"] == 2
    torch.manual_seed(6)
    assert a.train(2) == 7
    torch.manual_seed(6)
    assert b.train(2) == 7
    sa, sb = TC.device_state(a), TC.device_state(b)
    assert TC.differing(sa, sb) == [] and int(sb["adam_step"]) == 7 and int(sb["ema.step"]) == 7
    n = TC.trainable(a)[0][0]
    assert not torch.equal(sa["ema." + n], sa["p." + n])  # counter 6 was a lerp: the EMA is no copy
    # the same file into the trainer that has just stepped: its engine exists, so load() itself has to take the device's Adam
    # step back to 3 and `initted` back to 0, and `step` has to allow for the 4 updates the device has already counted
    b.load(1)
    assert b.step == 3 and int(b.ema.step) == 3 and float(b.ema.initted) == 0.0
    torch.manual_seed(2)
    assert b.train(2) == 5
    assert TC.differing(at5, TC.device_state(b)) == []


def test_a_checkpoint_without_the_optimizer_loads_and_trains_on(tmp_path):
    """The reference's layout {'step', 'model', 'ema', 'scaler'}: Adam starts over (step 1, fresh moments), `step` continues."""
    _, _, a = TC.make_trainer(True, tmp_path, **RESUME)
    torch.manual_seed(1)
    assert a.train(3) == 3
    a.save(1)
    assert sorted(torch.load(tmp_path / "model-1.pt", map_location="cpu")) == ["ema", "model", "scaler", "step"]
    _, _, b = TC.make_trainer(True, tmp_path, seed=9, **RESUME)
    b.load(1)
    before = TC.device_state(b)
    assert b.step == 3 and TC.differing({k: v for k, v in before.items() if k[:2] == "p."}, {k: v for k, v in TC.device_state(a).items() if k[:2] == "p."}) == []
    torch.manual_seed(2)
    assert b.train(1) == 4
    after = TC.device_state(b)
    assert int(after["adam_step"]) == 1 and int(after["ema.step"]) == 4 and b.optimizer.counters()["applied"] == 1
    moved = TC.differing({k: v for k, v in before.items() if k[:2] == "p."}, {k: v for k, v in after.items() if k[:2] == "p."})
    assert len(moved) > len(TC.trainable(b)) // 2


@pytest.mark.parametrize("source_fused", [True, False])
def test_a_checkpoint_of_either_path_steps_on_both(tmp_path, source_fused):
    """Three iterations on one path, saved with the optimizer, loaded into a fused and into a plain trainer; one iteration each.
    Both load the same bits and see the same gradients, the Adam step goes from 3 to 4 on both, and p, exp_avg and exp_avg_sq end
    inside the bar of tests/test_gpu_optim.py against the fp64 oracle: d_hip <= 2 d_torch + 1, d_torch the plain trainer's."""
    _, _, src = TC.make_trainer(source_fused, tmp_path, save_optimizer=True, **RESUME)
    torch.manual_seed(1)
    assert src.train(3) == 3
    src.save(1)
    ends, start, grads = {}, {}, {}
    for fused in (True, False):
        _, _, tr = TC.make_trainer(fused, tmp_path, seed=9, keep_grads=True, **RESUME)
        tr.load(1)
        state = TC.device_state(tr)
        state.pop("adam_step")  # (the fused path pushes it to the device with its first step)
        start[fused] = state
        assert tr.step == 3 and int(tr.ema.step) == 3
        torch.manual_seed(2)
        assert tr.train(1) == 4
        assert TC.adam_step(tr) == 4 and int(tr.ema.step) == 4
        ends[fused], grads[fused] = TC.device_state(tr), [g.detach().clone() for g in _grads(tr)]
    assert TC.differing(start[True], start[False]) == []
    assert all(torch.equal(x, y) for x, y in zip(grads[True], grads[False]))
    names = [n for n, _ in TC.trainable(src)]
    flat = lambda state, kind: [state[kind + "." + n].reshape(-1).cpu().numpy() for n in names]  # noqa: E731
    s = start[True]
    P, M, V, _, c, info = OO.step(flat(s, "p"), [g.reshape(-1).cpu().numpy() for g in grads[False]], flat(s, "exp_avg"), flat(s, "exp_avg_sq"),
                                  flat(s, "ema"), OO.Counters(adam_step=3, ema_step=3), lr=1e-4, update_every=2, update_after_step=2)
    assert c.adam_step == 4 and info["action"] == "none" and not info["skip"]
    for kind, want in (("p", P), ("exp_avg", M), ("exp_avg_sq", V)):
        d_hip = max(OO.ulp_distance(x, w) for x, w in zip(flat(ends[True], kind), want))
        d_torch = max(OO.ulp_distance(x, w) for x, w in zip(flat(ends[False], kind), want))
        print(f"resume from fused={source_fused}: {kind}: d_hip {d_hip:.3f}  d_torch {d_torch:.3f}")
        assert d_hip <= 2 * d_torch + 1, (kind, d_hip, d_torch)
    assert TC.differing({k: v for k, v in ends[True].items() if k.startswith("ema.")}, {k: v for k, v in start[True].items() if k.startswith("ema.")}) == ["ema.step"]
