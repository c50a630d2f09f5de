"""An fp64 restatement of one step of the fused clip + AdamW update (egoego_optimw_step): the gradient norm, clip_grad_norm_'s
coefficient, torch.optim.AdamW's decoupled decay (or Adam's L2 term), Adam, the skip rule and the counters.  Like optim_oracle.step
it rounds nothing except the fp32 product g * inv_scale: the coefficient, the decay factor and every moment are fp64.  Host code
only.

Pinned on the CPU against clip_grad_norm_(foreach=False) + torch.optim.AdamW(foreach=False): exp_avg_sq agrees to 1-8 fp32 ulp on
16 k elements after one step; for a lone gradient of 1.0 at max_norm = 1 the coefficient rounds to float32(1 / 1.000001) =
0.99999899, one ulp below torch's all-fp32 0.99999905 (tests/test_adamw.py)."""
import math

import numpy as np

from optim_oracle import Counters, f64, total_norm, ulp_distance, ulp_distances  # noqa: F401  (re-exported for the tests)


def clip_coef(norm, max_norm, clip_eps=1e-6):
    """clip_grad_norm_'s clamp(max_norm / (total_norm + 1e-6), max=1) in fp64; 1 without clipping."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    c = max_norm / (norm + clip_eps)
    return c if c < 1.0 else 1.0  # (a NaN norm never gets here: the step is skipped)


def step(p, g, m, v, c, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, clip_eps=1e-6, decoupled=True,
         inv_scale=1.0, losses=(), found_inf=0.0, skip_on="nan"):
    """Lists of arrays p, g, m, v and Counters c -> (p, m, v as lists of fp64 arrays, new Counters, info).  info: 'norm' (before
    clipping: what clip_grad_norm_ returns), 'coef', 'skip'.  A skipped step returns its inputs (as fp64), coef 1, and advances
    `skipped` only."""
    P, M, V = [f64(x) for x in p], [f64(x) for x in m], [f64(x) for x in v]
    n = Counters(c.adam_step, c.ema_step, c.initted, c.applied, c.skipped)
    bad = (lambda x: math.isnan(x)) if skip_on == "nan" else (lambda x: not math.isfinite(x))
    norm = total_norm(g, inv_scale)
    skip = bad(norm) or any(bad(float(l)) for l in losses) or float(found_inf) != 0.0
    info = {"norm": norm, "skip": bool(skip), "coef": 1.0}
    if skip:
        n.skipped += 1
        return P, M, V, n, info
    n.applied += 1
    n.adam_step += 1
    k = n.adam_step
    b1, b2 = betas
    coef = info["coef"] = clip_coef(norm, max_norm, clip_eps)
    step_size = lr / (1.0 - b1 ** k)
    bc2_sqrt = math.sqrt(1.0 - b2 ** k)
    inv = np.float32(inv_scale)
    for i in range(len(P)):
        with np.errstate(all="ignore"):  # (an inf gradient under "nan": inf * 0 and inf / inf, as on the device)
            G = f64(np.asarray(g[i], dtype=np.float32) * inv) * coef
            if decoupled:
                P[i] = P[i] * (1.0 - lr * weight_decay)
            elif weight_decay:
                G = G + weight_decay * P[i]
            M[i] = M[i] + (G - M[i]) * (1.0 - b1)
            V[i] = b2 * V[i] + (1.0 - b2) * G * G
            P[i] = P[i] - step_size * M[i] / (np.sqrt(V[i]) / bc2_sqrt + eps)
    return P, M, V, n, info
