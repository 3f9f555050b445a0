#!/usr/bin/env python3
"""What PPO2-style value-function clipping (PPO.set_value_clip, mi_ppo_train_step_vclip) costs per SGD step on ONE GPU.

    python tools/ppo_value_clip_bench.py [--rounds 3] [--steps 200] [--sizes 32,256,2048] [--modes fp32,bf16x3] [--value-clip 0.2] [--no-box]

Prints ONE JSON line:
  step      ms per SGD step on device-resident minibatch tensors (cached log pi_old) per precision mode and minibatch size M, median / min / max over --rounds
            rounds that interleave the two forms in one process so that both see the same box state:
              plain    mi_ppo_train_step (M <= 256: Adam inside the gradient kernels; above: the flat Adam launch), the yardstick
              clipped  mi_ppo_train_step_vclip on the same tensors plus old values spread +- 0.5 around the returns: the same chain, the clipped instantiation of the
                       head / loss kernel (one more 4-byte gather per sample and a few VALU operations)
            with clipped - plain and the round spread of the plain form (max - min) to judge it by
  box       the in-run calibration of this GPU (mi_device_probe, as bench.py reports it)"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

FORMS = ("plain", "clipped")


class Box:
    low, high, shape = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32), (2,)


def make_ppo(tmp, precision, tag):
    from ppo import PPO
    m = PPO(np.array([67]), Box(), learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0,
            model_dir=os.path.join(tmp, "%s_%s" % (tag, precision)), seed=0, precision=precision)
    m.set_max_grad_norm(None)                               # (whatever MI355_PPO_MAX_GRAD_NORM says: both forms run without the norm)
    m.init_session(init_logging=False)
    return m


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_legs(tmp, modes, sizes, rounds, steps, warmup, eps_v):
    from ppo import _adam_alpha
    rng = np.random.RandomState(7)
    alpha = _adam_alpha(1e-4, 0.9, 0.999)
    legs = {}
    for M in sizes:
        ret = rng.randn(M).astype(np.float32)
        data = ((0.5 * rng.standard_normal((M, 67))).astype(np.float32), np.stack([rng.uniform(-1, 1, M), rng.uniform(0, 1, M)], axis=1).astype(np.float32),
                ret, rng.randn(M).astype(np.float32), (ret + rng.uniform(-0.5, 0.5, M)).astype(np.float32))
        for mode in modes:
            for form in FORMS:                               # an engine per leg: every form trains its own parameters
                m = make_ppo(tmp, mode, "%s%d" % (form, M))
                m.dev.ensure_batch(M)
                t = [torch.from_numpy(x).to(m.dev.device) for x in data]
                lp = torch.empty(M, device=m.dev.device)
                m.dev.logp_old(t[0], t[1], M, lp)
                legs[(mode, M, form)] = (m, t, lp)

    def run(key, n):
        (mode, M, form), (m, t, lp) = key, legs[key]
        d = m.dev
        for _ in range(n):
            if form == "plain":
                d.train_step(t[0], t[1], t[2], t[3], M, 1.0 / M, 1.0, alpha, logp_old=lp)
            else:
                d.train_step_vclip(None, t[0], t[1], t[2], t[3], lp, t[4], eps_v, None, M, 1.0 / M, 1.0, alpha)

    times = {k: [] for k in legs}
    for k in legs:                                           # every leg warm before the first timed round
        run(k, warmup)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k in legs:
            run(k, warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(k, steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {}
    for mode in modes:
        out[mode] = {}
        for M in sizes:
            r = {form: summary(times[(mode, M, form)]) for form in FORMS}
            r["clipped_minus_plain_ms"] = r["clipped"]["median"] - r["plain"]["median"]
            r["plain_round_spread_ms"] = r["plain"]["max"] - r["plain"]["min"]
            r["last_value_loss"] = {form: float(legs[(mode, M, form)][0].dev.losses[1].item()) for form in FORMS}
            out[mode][str(M)] = r
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="timed SGD steps per leg and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="32,256,2048")
    ap.add_argument("--modes", default="fp32,bf16x3")
    ap.add_argument("--value-clip", type=float, default=0.2, help="eps_v of the clipped form (inf: the clipped kernel, never a clipped sample)")
    ap.add_argument("--no-box", action="store_true")
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    if not modes or any(m not in ("fp32", "bf16x3") for m in modes):
        ap.error("--modes: fp32 and / or bf16x3")
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if not args.value_clip > 0:
        ap.error("--value-clip: a positive float or inf")
    if not torch.cuda.is_available():
        raise SystemExit("ppo_value_clip_bench: no GPU visible (timings are only taken on the device)")
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp(prefix="ppo_value_clip_bench_")
    sizes = [int(x) for x in args.sizes.split(",") if x]
    res = {"tool": "ppo_value_clip_bench", "modes": modes, "rounds": args.rounds, "steps_per_round": args.steps, "value_clip": args.value_clip}
    if not args.no_box:
        from bench import box_probe
        from mi355.ppo_device import PpoDevice
        probe_dev = PpoDevice(67, 2, Box.low, Box.high, 0.2, 1.0, 0.01, max_batch=32)
        res["box"] = box_probe(probe_dev, 0)
        probe_dev.close()
    res["step"] = step_legs(tmp, modes, sizes, args.rounds, args.steps, args.warmup, args.value_clip)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
