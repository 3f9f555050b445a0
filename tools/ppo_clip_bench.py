#!/usr/bin/env python3
"""What global-norm gradient clipping (PPO.set_max_grad_norm, mi_ppo_set_max_grad_norm) costs per SGD step and per rollout-buffer update on ONE GPU.

    python tools/ppo_clip_bench.py [--rounds 3] [--steps 200] [--sizes 32,256,2048] [--modes fp32,bf16x3] [--max-grad-norm 0.5]
                                   [--updates 64x128,1024x128] [--batch 32,2048] [--epochs 1] [--no-updates] [--no-box]

Prints ONE JSON line:
  step      ms per SGD step on device-resident minibatch tensors per precision mode and minibatch size M, median / min / max over --rounds rounds that interleave
            the three forms so that all see the same box state:
              one_call  mi_ppo_train_step with clipping off (M <= 256: Adam inside the gradient kernels; above: the flat Adam launch)
              unfused   mi_ppo_forward_backward + mi_ppo_apply_adam with clipping off: the gradients through the flat buffer, the yardstick of the clipped step
              clipped   mi_ppo_train_step with clipping on: the same chain, the sum-of-squares launch, the clipped Adam
            and the differences clipped - unfused (the price of the norm) and clipped - one_call (what giving up the in-tile Adam costs)
  update    seconds per RolloutBuffer.update of E x T recorded steps (scripted frames from a pool, full rows) at each minibatch size, clipping off against on,
            interleaved likewise, with the "sgd" stage and the SGD steps per update
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

FORMS = ("one_call", "unfused", "clipped")


class Box:
    low, high, shape = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32), (2,)


def make_ppo(tmp, precision, tag):
    from ppo import PPO
    m = PPO(np.array([67]), Box(), learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0,
            model_dir=os.path.join(tmp, "%s_%s" % (tag, precision)), seed=0, precision=precision)
    m.set_max_grad_norm(None)                               # (whatever MI355_PPO_MAX_GRAD_NORM says: the forms set it themselves)
    m.init_session(init_logging=False)
    return m


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_legs(tmp, modes, sizes, rounds, steps, warmup, max_norm):
    from ppo import _adam_alpha
    rng = np.random.RandomState(7)
    alpha = _adam_alpha(1e-4, 0.9, 0.999)
    legs = {}
    for M in sizes:
        data = ((0.5 * rng.standard_normal((M, 67))).astype(np.float32), np.stack([rng.uniform(-1, 1, M), rng.uniform(0, 1, M)], axis=1).astype(np.float32),
                rng.randn(M).astype(np.float32), rng.randn(M).astype(np.float32))
        for mode in modes:
            for form in FORMS:                               # an engine per leg: every form trains its own parameters
                m = make_ppo(tmp, mode, "%s%d" % (form, M))
                m.dev.ensure_batch(M)
                m.dev.set_max_grad_norm(max_norm if form == "clipped" else None)
                legs[(mode, M, form)] = (m, [torch.from_numpy(x).to(m.dev.device) for x in data])

    def run(key, n):
        (mode, M, form), (m, t) = key, legs[key]
        d = m.dev
        for _ in range(n):
            if form == "unfused":
                d.forward_backward(t[0], t[1], t[2], t[3], M, 1.0 / M, 1.0)
                d.apply_adam(alpha)
            else:
                d.train_step(t[0], t[1], t[2], t[3], M, 1.0 / M, 1.0, alpha)

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
            r["clipped_minus_unfused_ms"] = r["clipped"]["median"] - r["unfused"]["median"]
            r["clipped_minus_one_call_ms"] = r["clipped"]["median"] - r["one_call"]["median"]
            clip = legs[(mode, M, "clipped")][0].last_grad_norm()
            r["last_grad_norm"], r["last_clip_scale"] = clip["grad_norm"], clip["clip_scale"]
            out[mode][str(M)] = r
    return out


def update_legs(tmp, shapes, batches, epochs, rounds, max_norm, pool_size=256):
    from rollout import RolloutBuffer
    from vae.models import ConvVAE
    vae = ConvVAE(np.array([80, 160, 3]), z_dim=64, model_dir=os.path.join(tmp, "vae"), precision="bf16", training=False, seed=0)
    vae.init_session(init_logging=False)
    rng = np.random.RandomState(0)
    pool = rng.randint(0, 256, (pool_size, 80, 160, 3), dtype=np.uint8)
    out = {}
    for E, T in shapes:
        agent = make_ppo(tmp, "fp32", "update%dx%d" % (E, T))
        buf = RolloutBuffer(vae, agent, E, T)
        idx = rng.randint(0, pool_size, (E, T + 1))
        meas = np.stack([rng.uniform(-1, 1, (E, T + 1)), rng.uniform(0, 1, (E, T + 1)), rng.uniform(0, 30, (E, T + 1))], axis=-1)
        buf.reset()
        for t in range(T):
            buf.step(pool[idx[:, t]], meas[:, t])
            buf.outcome(rng.uniform(0, 1, E), np.zeros(E, bool))
        buf.bootstrap(pool[idx[:, T]], meas[:, T])

        def run(batch, clip):
            agent.set_max_grad_norm(max_norm if clip else None)
            st = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = buf.update(num_epochs=epochs, batch_size=batch, stage_times=st)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, st["sgd"], len(res["losses"]), (int((res["clip_scales"] < 1).sum()) if clip else None)
        for batch in batches:
            for clip in (False, True):
                run(batch, clip)                             # warm-up (engine growth, allocator)
            rows = {False: [], True: []}
            for _ in range(rounds):
                for clip in (False, True):
                    rows[clip].append(run(batch, clip))
            r = {"sgd_steps": rows[True][0][2], "clipped_steps_last_round": rows[True][-1][3]}
            for clip, name in ((False, "unclipped"), (True, "clipped")):
                r[name] = {"update_s": summary([x[0] for x in rows[clip]]), "sgd_s": summary([x[1] for x in rows[clip]])}
            r["clipped_minus_unclipped_ms_per_step"] = (r["clipped"]["sgd_s"]["median"] - r["unclipped"]["sgd_s"]["median"]) * 1e3 / max(r["sgd_steps"], 1)
            out["%dx%d/batch%d" % (E, T, batch)] = r
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="timed SGD steps per leg and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="32,256,2048")
    ap.add_argument("--modes", default="fp32,bf16x3")
    ap.add_argument("--max-grad-norm", type=float, default=0.5, help="the limit of the clipped forms (inf: the norm is formed, nothing is scaled down; the launches are the same)")
    ap.add_argument("--updates", default="64x128,1024x128", help="E x T of the rollout-buffer legs")
    ap.add_argument("--batch", default="32,2048")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--no-updates", action="store_true")
    ap.add_argument("--no-box", action="store_true")
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    if not modes or any(m not in ("fp32", "bf16x3") for m in modes):
        ap.error("--modes: fp32 and / or bf16x3")
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if not args.max_grad_norm > 0:
        ap.error("--max-grad-norm: a positive float or inf")
    if not torch.cuda.is_available():
        raise SystemExit("ppo_clip_bench: no GPU visible (timings are only taken on the device)")
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp(prefix="ppo_clip_bench_")
    sizes = [int(x) for x in args.sizes.split(",") if x]
    res = {"tool": "ppo_clip_bench", "modes": modes, "rounds": args.rounds, "steps_per_round": args.steps, "max_grad_norm": args.max_grad_norm}
    if not args.no_box:
        from bench import box_probe
        from mi355.ppo_device import PpoDevice
        probe_dev = PpoDevice(67, 2, Box.low, Box.high, 0.2, 1.0, 0.01, max_batch=32)
        res["box"] = box_probe(probe_dev, 0)
        probe_dev.close()
    res["step"] = step_legs(tmp, modes, sizes, args.rounds, args.steps, args.warmup, args.max_grad_norm)
    if not args.no_updates:
        shapes = [tuple(int(v) for v in x.split("x")) for x in args.updates.split(",") if x]
        res["update"] = update_legs(tmp, shapes, [int(x) for x in args.batch.split(",") if x], args.epochs, args.rounds, args.max_grad_norm)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
