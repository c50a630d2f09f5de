#!/usr/bin/env python3
"""A/B of several builds of the library in ONE process on one device (precision 9, graph replay): each TAG is a variant built with
`python -m egoego_release_amd.build --variant --tag=TAG [-D...]` (from any source tree: a checkout of the parent commit gives the
baseline), `product` is the package's own library.  First every variant's seeded chains — 256 x T=120, 65 x T=100 (the smallest grid
of the two-workgroups-per-CU tail, padded rows), 65 x T=120 with EGOEGO_FLAG_FC24 — must equal the first variant's bit for bit; then
ROUNDS timing rounds of STEPS steps at B x T=120, the variants interleaved (order reversed every other round), median / min / max per
variant, and the tail's launch time by the library's own events.

    python tools/lib_ab.py parent product [TAG ...] [--rounds=7] [--steps=200] [--batch=256] [--nocheck] [--out=ab.json]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from egoego_release_amd import ModelConfig, make_weights, _lib  # noqa: E402
from egoego_release_amd.engine import HipEngine  # noqa: E402
from egoego_release_amd.model import CondGaussianDiffusion  # noqa: E402
from egoego_release_amd.precision import _engine_cfg  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
opt = {a.split("=")[0]: (a.split("=")[1] if "=" in a else "1") for a in sys.argv[1:] if a.startswith("--")}
ROUNDS, STEPS = int(opt.get("--rounds", 7)), int(opt.get("--steps", 200))
B, T = int(opt.get("--batch", 256)), 120
out_path = os.path.abspath(opt.get("--out", "ab.json"))


def lib_path(tag):
    return os.path.join(ROOT, "egoego_release_amd", "libegoego_hip.so") if tag == "product" else os.path.join(ROOT, "tools", "_build", f"libegoego_hip_perfdebug_{tag}.so")


models = {}


def model(Tm):
    if Tm not in models:
        cfg = ModelConfig(max_timesteps=Tm + 1)
        m = CondGaussianDiffusion(**cfg.ctor_kwargs())
        m.load_state_dict(make_weights(cfg, 0), strict=False)
        models[Tm] = m
    return models[Tm]


def engine(tag, Tm, flags=0):
    _lib._lib = None
    _lib.LIB_PATH = lib_path(tag)
    m = model(Tm)
    return HipEngine(_engine_cfg(m), m.state_dict(), torch.device("cuda"), _lib.PREC_I8X3_FC, flags)


res = {"variants": args, "device": torch.cuda.get_device_name(0), "B": B, "T": T, "steps": STEPS, "rounds": ROUNDS}
if "--nocheck" not in opt:
    ref = {}
    for tag in args:
        bad = []
        for name, (Tm, Bc, flags) in {"256x120": (120, 256, 0), "65x100": (100, 65, 0), "65x120_fc24": (120, 65, _lib.FLAG_FC24)}.items():
            e = engine(tag, Tm, flags)
            g = torch.Generator().manual_seed(3)
            x = torch.randn(Bc, Tm, 198, generator=g).cuda()
            xc = torch.randn(Bc, Tm, 198, generator=g).cuda()
            e.sample_loop_(x, xc, 999, 4, noise_mode=_lib.NOISE_PHILOX, seed=5)
            torch.cuda.synchronize()
            kn = e.last_kernel("fc_ln")
            x = x.cpu()
            if tag == args[0]:
                ref[name] = x
            elif not torch.equal(x, ref[name]):
                bad.append((name, float((x - ref[name]).abs().max())))
            e.close()
        print(f"check {tag}: {'bit-equal to ' + args[0] if not bad else 'DIFFERS ' + str(bad)} ({kn})", flush=True)
        res.setdefault("bit_equal", {})[tag] = not bad
    if not all(res["bit_equal"].values()):
        json.dump(res, open(out_path, "w"), indent=1)
        sys.exit(3)

engs = {tag: engine(tag, T) for tag in args}
x0 = torch.randn(B, T, 198, device="cuda")
xc = torch.randn(B, T, 198, device="cuda")
for tag in args:  # warm-up: packs the workspace, captures the graph
    x = x0.clone()
    engs[tag].sample_loop_(x, xc, 999, 20, noise_mode=_lib.NOISE_PHILOX, seed=1)
torch.cuda.synchronize()
times = {tag: [] for tag in args}
for r in range(ROUNDS):
    for tag in (args if r % 2 == 0 else args[::-1]):
        x = x0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engs[tag].sample_loop_(x, xc, 999, STEPS, noise_mode=_lib.NOISE_PHILOX, seed=1)
        torch.cuda.synchronize()
        times[tag].append(1e3 * (time.perf_counter() - t0) / STEPS)
res["ms_per_step"] = {}
for tag in args:
    v = times[tag]
    res["ms_per_step"][tag] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "rounds": [round(a, 5) for a in v]}
    print(f"{tag:8s} median {statistics.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}  spread {max(v) - min(v):.4f}   {[round(a, 4) for a in v]}", flush=True)
# per-launch time of the tail (the library's own event timing)
res["tail_us"] = {}
for tag in args:
    x = x0.clone()
    engs[tag].profile_begin("fc_ln")
    engs[tag].sample_loop_(x, xc, 900, 10, noise_mode=_lib.NOISE_PHILOX, seed=1)
    torch.cuda.synchronize()
    us, n = engs[tag].profile_end()
    res["tail_us"][tag] = round(us, 2) if n else None
print("tail us per launch:", res["tail_us"], flush=True)
json.dump(res, open(out_path, "w"), indent=1)
