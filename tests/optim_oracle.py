"""An fp64 restatement of one step of the fused parameter update (csrc/optim_step.*): the gradient norm, the skip rule, Adam
(torch.optim.Adam, amsgrad off, L2 weight decay), ema-pytorch's schedule and lerp, and the counters.  Inputs are fp32 arrays (or
anything numpy converts); every result is fp64.  Host code only."""
import math

import numpy as np


class Counters:
    """What the device keeps between steps."""

    def __init__(self, adam_step=0, ema_step=0, initted=False, applied=0, skipped=0):
        self.adam_step, self.ema_step, self.initted, self.applied, self.skipped = adam_step, ema_step, initted, applied, skipped

    def as_tuple(self):
        return (self.adam_step, self.ema_step, int(self.initted), self.applied, self.skipped)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def total_norm(grads, inv_scale=1.0):
    """sqrt(sum (g * inv_scale)^2): the product is the fp32 one the kernel forms, the sum is fp64."""
    inv = np.float32(inv_scale)
    return math.sqrt(sum(float(np.sum(f64(np.asarray(g, dtype=np.float32) * inv) ** 2)) for g in grads))


def decay_at(step_after, beta=0.995, update_after_step=100, inv_gamma=1.0, power=2.0 / 3.0, min_value=0.0):
    e = max(step_after - update_after_step - 1, 0)
    if e <= 0:
        return 0.0
    return min(max(1.0 - (1.0 + e / inv_gamma) ** -power, min_value), beta)


def ema_action(step, initted, update_every=10, update_after_step=100):
    if step % update_every != 0:
        return "none"
    if step <= update_after_step or not initted:
        return "copy"
    return "lerp"


def step(p, g, m, v, ema, c, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, inv_scale=1.0, losses=(), found_inf=0.0,
         skip_on="nan", do_adam=True, do_ema=True, beta=0.995, update_every=10, update_after_step=100, inv_gamma=1.0, power=2.0 / 3.0,
         min_value=0.0):
    """Lists of arrays p, g, m, v, ema (ema may be None) and Counters c -> (p, m, v, ema as lists of fp64 arrays, new Counters,
    info).  A skipped step returns its inputs (as fp64) and advances `skipped` only."""
    P, M, V = [f64(x) for x in p], [f64(x) for x in m], [f64(x) for x in v]
    E = None if ema is None else [f64(x) for x in ema]
    n = Counters(*[c.adam_step, c.ema_step, c.initted, c.applied, c.skipped])
    bad = (lambda x: math.isnan(x)) if skip_on == "nan" else (lambda x: not math.isfinite(x))
    norm = total_norm(g, inv_scale) if do_adam else None
    skip = (do_adam and bad(norm)) or any(bad(float(l)) for l in losses) or float(found_inf) != 0.0
    info = {"norm": norm, "skip": bool(skip), "action": "none", "decay": None}
    if skip:
        n.skipped += 1
        return P, M, V, E, n, info
    n.applied += 1
    if do_adam:
        n.adam_step += 1
        k = n.adam_step
        b1, b2 = betas
        step_size = lr / (1.0 - b1 ** k)
        bc2_sqrt = math.sqrt(1.0 - b2 ** k)
        inv = np.float32(inv_scale)
        for i in range(len(P)):
            G = f64(np.asarray(g[i], dtype=np.float32) * inv)
            if weight_decay:
                G = G + weight_decay * P[i]
            M[i] = M[i] + (G - M[i]) * (1.0 - b1)
            V[i] = b2 * V[i] + (1.0 - b2) * G * G
            with np.errstate(all="ignore"):  # (an inf gradient under "nan": inf / inf, as on the device)
                P[i] = P[i] - step_size * M[i] / (np.sqrt(V[i]) / bc2_sqrt + eps)
    if do_ema and E is not None:
        s = n.ema_step
        n.ema_step += 1
        act = ema_action(s, n.initted, update_every, update_after_step)
        info["action"] = act
        if act == "copy":
            E = [x.copy() for x in P]
            if s > update_after_step:
                n.initted = True
        elif act == "lerp":
            d = decay_at(n.ema_step, beta, update_after_step, inv_gamma, power, min_value)
            info["decay"] = d
            E = [e - (e - x) * (1.0 - d) for e, x in zip(E, P)]
    return P, M, V, E, n, info


def ulp_distances(got, want64):
    """|got - want| element by element in units of the fp32 ulp of `want` (want: fp64; its ulp is that of its fp32 rounding; values
    below the smallest normal count in units of the smallest subnormal)."""
    w = f64(want64)
    w32 = np.abs(w.astype(np.float32))
    ulp = f64(np.spacing(np.maximum(w32, np.float32(np.finfo(np.float32).tiny))))
    return np.abs(f64(got) - w) / ulp


def ulp_distance(got, want64):
    """The largest of ulp_distances()."""
    d = ulp_distances(got, want64)
    return float(d.max()) if d.size else 0.0
