#!/usr/bin/env python3
"""The PPO minibatch SGD step in its two precision modes on ONE GPU: exact fp32 and split-bf16 ("bf16x3", mi_ppo_set_precision), same box, same call.

    python tools/ppo_precision_bench.py [--rounds 3] [--steps 50] [--sizes 32,256,2048] [--rows 1024] [--no-replay] [--no-box] [--modes fp32,bf16x3]

(--modes fp32 / --modes bf16x3: one mode alone, e.g. under rocprofv3 --kernel-trace --stats for the per-kernel split of one mode's step.)

Prints ONE JSON line:
  step      ms per SGD step (mi_ppo_train_step: the single-rank one-call step on device-resident minibatch tensors) per mode and minibatch size M, as the
            median over --rounds rounds with the min / max; the rounds interleave the modes (fp32, bf16x3, fp32, ...) so that both see the same box state
  replay    replay.replay_update (BASELINE configs[4] on one GPU: bf16 VAE encode of an HBM-resident uint8 frame table, values, GAE, PPO SGD 4 epochs x minibatch
            2048) per mode: the "sgd" stage in seconds (median, min, max over the rounds, interleaved likewise) and the SGD steps it ran
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

MODES = ["fp32", "bf16x3"]


class Box:
    low, high, shape = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32), (2,)


def make_ppo(tmp, precision, tag):
    from ppo import PPO
    m = PPO(np.array([67]), Box(), learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0,
            model_dir=os.path.join(tmp, "%s_%s" % (tag, precision)), seed=0, precision=precision)
    m.init_session(init_logging=False)
    return m


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_legs(tmp, sizes, rounds, steps, warmup):
    from ppo import _adam_alpha
    rng = np.random.RandomState(7)
    legs = {}
    for M in sizes:
        data = ((0.5 * rng.standard_normal((M, 67))).astype(np.float32), np.stack([rng.uniform(-1, 1, M), rng.uniform(0, 1, M)], axis=1).astype(np.float32),
                rng.randn(M).astype(np.float32), rng.randn(M).astype(np.float32))
        for mode in MODES:
            m = make_ppo(tmp, mode, "step%d" % M)
            t = [torch.from_numpy(x).to(m.dev.device) for x in data]
            m.dev.ensure_batch(M)
            legs[(mode, M)] = (m, t)
    alpha = _adam_alpha(1e-4, 0.9, 0.999)
    times = {k: [] for k in legs}

    def run(m, t, M, n):
        for _ in range(n):
            m.dev.train_step(t[0], t[1], t[2], t[3], M, 1.0 / M, 1.0, alpha)

    for (mode, M), (m, t) in legs.items():                   # every leg warm before the first timed round
        run(m, t, M, warmup)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for M in sizes:
            for mode in MODES:
                m, t = legs[(mode, M)]
                run(m, t, M, warmup)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(m, t, M, steps)
                torch.cuda.synchronize()
                times[(mode, M)].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {}
    for M in sizes:
        out[str(M)] = {mode: summary(times[(mode, M)]) for mode in MODES}
        if len(MODES) == 2:
            out[str(M)]["bf16x3_over_fp32"] = out[str(M)]["bf16x3"]["median"] / out[str(M)]["fp32"]["median"]
    return out


def replay_legs(tmp, rows, rounds, T=128, batch=2048, epochs=4):
    import replay
    from vae.models import ConvVAE
    vae = ConvVAE(np.array([80, 160, 3]), z_dim=64, model_dir=os.path.join(tmp, "rvae"), precision="bf16", training=False, seed=0)
    vae.init_session(init_logging=False)
    rng = np.random.default_rng(1234)
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    table = torch.randint(0, 256, (rows, T + 1, 80, 160, 3), device="cuda", generator=g, dtype=torch.uint8)      # uint8 frame table resident in HBM
    meas = np.stack([rng.uniform(-1, 1, (rows, T + 1)), rng.uniform(0, 1, (rows, T + 1)), rng.uniform(0, 30, (rows, T + 1))], axis=-1).astype(np.float32)
    actions = np.stack([rng.uniform(-1, 1, (rows, T)), rng.uniform(0, 1, (rows, T))], axis=-1).astype(np.float32)
    rewards, dones = rng.uniform(0, 1, (rows, T)), np.zeros((rows, T))
    ppos = {mode: make_ppo(tmp, mode, "replay") for mode in MODES}
    for mode in MODES:                                       # engines sized, every stage warm
        replay.replay_update(vae, ppos[mode], table, meas, actions, rewards, dones, 0.99, 0.95, 1, batch)
    torch.cuda.synchronize()
    sgd = {mode: [] for mode in MODES}
    steps = {}
    for _ in range(rounds):
        for mode in MODES:
            st = {}
            out = replay.replay_update(vae, ppos[mode], table, meas, actions, rewards, dones, 0.99, 0.95, epochs, batch, stage_times=st)
            torch.cuda.synchronize()
            sgd[mode].append(st["sgd"])
            steps[mode] = len(out["losses"])
    res = {"rows": rows, "horizon": T, "minibatch": batch, "epochs": epochs}
    for mode in MODES:
        res[mode] = {"sgd_s": summary(sgd[mode]), "sgd_steps": steps[mode], "ms_per_sgd_step": statistics.median(sgd[mode]) * 1e3 / max(steps[mode], 1)}
    if len(MODES) == 2:
        res["bf16x3_over_fp32"] = res["bf16x3"]["sgd_s"]["median"] / res["fp32"]["sgd_s"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50, help="timed SGD steps per leg and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="32,256,2048")
    ap.add_argument("--rows", type=int, default=1024, help="trajectories of the replay leg (horizon 128)")
    ap.add_argument("--no-replay", action="store_true")
    ap.add_argument("--no-box", action="store_true")
    ap.add_argument("--modes", default="fp32,bf16x3")
    args = ap.parse_args()
    MODES[:] = [m for m in args.modes.split(",") if m]
    if not MODES or any(m not in ("fp32", "bf16x3") for m in MODES):
        ap.error("--modes: fp32 and / or bf16x3")
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("ppo_precision_bench: no GPU visible (timings are only taken on the device)")
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp(prefix="ppo_precision_bench_")
    sizes = [int(x) for x in args.sizes.split(",") if x]
    res = {"tool": "ppo_precision_bench", "modes": list(MODES), "rounds": args.rounds, "steps_per_round": args.steps}
    if not args.no_box:
        from bench import box_probe
        from mi355.ppo_device import PpoDevice
        probe_dev = PpoDevice(67, 2, Box.low, Box.high, 0.2, 1.0, 0.01, max_batch=32)
        res["box"] = box_probe(probe_dev, 0)
        probe_dev.close()
    res["step"] = step_legs(tmp, sizes, args.rounds, args.steps, args.warmup)
    if not args.no_replay:
        res["replay"] = replay_legs(tmp, args.rows, args.rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
