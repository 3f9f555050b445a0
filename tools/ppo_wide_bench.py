#!/usr/bin/env python3
"""The PPO minibatch SGD step of a policy with more than 96 inputs on ONE GPU, in the three forms mi_ppo_set_wide_inputs offers, same box, same process:

    python tools/ppo_wide_bench.py [--rounds 3] [--steps 30] [--widths 131,259,515] [--sizes 32,256,2048] [--no-buffer] [--no-box]

  (a) per_layer   mode 0: the per-layer path (what such a policy ran before the setting existed; fp32 only -- the split mode has no per-layer form)
  (b) narrow_l1   mode 2: the fused kernels with ppo_l1_kernel (one wave walks the whole K)
  (c) wide_l1     mode 1: the fused kernels with ppo_l1_wide_kernel (four waves split K and meet in LDS)

Prints ONE JSON line:
  step      microseconds per SGD step (mi_ppo_train_step on device-resident minibatch tensors of the 500 / 300 trunk) per input width, minibatch size M, precision
            and form: the median over --rounds rounds with the min / max, timed with device events around --steps steps; the rounds interleave the forms
            (a, b, c, a, ...) so that all see the same box state
  buffer    one RolloutBuffer.update (64 environments x 128 steps, 131 inputs from an MlpVAE of 128 latents, 3 epochs) at minibatch 32 and 2048 with the setting off
            (host-side gather, the old policy evaluated in every step) and on: wall seconds, median / min / max over the rounds, interleaved likewise
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

FORMS = [("per_layer", 0), ("narrow_l1", 2), ("wide_l1", 1)]
HIDDEN = (500, 300)


class Box:
    low, high, shape = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32), (2,)


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_legs(widths, sizes, rounds, steps, warmup):
    from mi355.init import init_ppo
    from mi355.ppo_device import PpoDevice
    from ppo import _adam_alpha
    alpha = _adam_alpha(1e-4, 0.9, 0.999)
    rng = np.random.RandomState(7)
    out = {}
    for din in widths:
        d = PpoDevice(din, 2, Box.low, Box.high, 0.2, 1.0, 0.01, hidden=HIDDEN, max_batch=max(sizes))
        values = init_ppo(0, din, 2, 1.0, hidden=HIDDEN)
        d.load_params(values, {k.replace("policy/", "policy_old/", 1): v for k, v in values.items()})
        theta = d.params.clone()
        out[str(din)] = {}
        for M in sizes:
            t = [torch.from_numpy(x).to(d.device) for x in (
                (0.5 * rng.standard_normal((M, din))).astype(np.float32), np.stack([rng.uniform(-1, 1, M), rng.uniform(0, 1, M)], axis=1).astype(np.float32),
                rng.randn(M).astype(np.float32), rng.randn(M).astype(np.float32))]
            legs = [(prec, form, mode) for prec in ("fp32", "bf16x3") for form, mode in FORMS if not (prec == "bf16x3" and mode == 0)]
            times = {(prec, form): [] for prec, form, _ in legs}

            def run(n):
                for _ in range(n):
                    d.train_step(t[0], t[1], t[2], t[3], M, 1.0 / M, 1.0, alpha)

            def select(prec, mode):
                d.set_precision("fp32")
                d.set_wide_inputs(mode)
                d.set_precision(prec)
                d.params.copy_(theta); d.adam_m.zero_(); d.adam_v.zero_(); d.grads.zero_()      # every leg starts from the same state
            for r in range(rounds + 1):                      # round 0 warms every leg and is not kept
                for prec, form, mode in legs:
                    select(prec, mode)
                    run(warmup)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(steps)
                    e1.record()
                    e1.synchronize()
                    if r:
                        times[(prec, form)].append(e0.elapsed_time(e1) * 1e3 / steps)
            out[str(din)][str(M)] = {prec: {form: summary(times[(prec, form)]) for p2, form, _ in legs if p2 == prec} for prec in ("fp32", "bf16x3")}
        d.close()
    return out


def buffer_legs(tmp, rounds, E=64, T=128, z=128, batches=(32, 2048), epochs=3):
    from ppo import PPO
    from rollout import RolloutBuffer
    from vae.models import MlpVAE
    src = (4, 6, 3)
    vae = MlpVAE(np.array(src), encoder_sizes=(36,), decoder_sizes=(8,), z_dim=z, model_dir=os.path.join(tmp, "vae"), precision="fp32", training=False, seed=0)
    vae.init_session(init_logging=False)
    m = PPO(np.array([z + 3]), Box(), learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0,
            model_dir=os.path.join(tmp, "ppo"), seed=0)
    m.init_session(init_logging=False)
    buf = RolloutBuffer(vae, m, E, T, seed=3)
    rng = np.random.RandomState(11)
    buf.reset()
    for _ in range(T):
        frames = rng.randint(0, 256, (E,) + src, dtype=np.uint8)
        meas = np.stack([rng.uniform(-1, 1, E), rng.uniform(0, 1, E), rng.uniform(0, 30, E)], axis=1)
        buf.step(frames, meas)
        buf.outcome(rng.uniform(0, 1, E), np.zeros(E, bool))
    buf.bootstrap(frames, meas)
    theta = [x.clone() for x in (m.dev.params, m.dev.params_old, m.dev.adam_m, m.dev.adam_v)]
    res = {"envs": E, "horizon": T, "inputs": z + 3, "epochs": epochs}
    for batch in batches:
        times = {False: [], True: []}
        for r in range(rounds + 1):                          # round 0 warms both and is not kept
            for on in (False, True):
                m.set_wide_inputs(on)
                for dst, src_t in zip((m.dev.params, m.dev.params_old, m.dev.adam_m, m.dev.adam_v), theta):
                    dst.copy_(src_t)
                np.random.seed(5)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = buf.update(num_epochs=epochs, batch_size=batch)
                torch.cuda.synchronize()
                if r:
                    times[on].append(time.perf_counter() - t0)
        res[str(batch)] = {"mode0_s": summary(times[False]), "mode1_s": summary(times[True]), "sgd_steps": len(out["losses"]),
                           "mode1_over_mode0": statistics.median(times[True]) / statistics.median(times[False])}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30, help="timed SGD steps per leg and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--widths", default="131,259,515")
    ap.add_argument("--sizes", default="32,256,2048")
    ap.add_argument("--no-buffer", action="store_true")
    ap.add_argument("--no-box", action="store_true")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("ppo_wide_bench: no GPU visible (timings are only taken on the device)")
    torch.cuda.set_device(0)
    tmp = tempfile.mkdtemp(prefix="ppo_wide_bench_")
    widths, sizes = [int(x) for x in args.widths.split(",") if x], [int(x) for x in args.sizes.split(",") if x]
    res = {"tool": "ppo_wide_bench", "rounds": args.rounds, "steps_per_round": args.steps, "hidden": list(HIDDEN)}
    if not args.no_box:
        from bench import box_probe
        from mi355.ppo_device import PpoDevice
        probe_dev = PpoDevice(67, 2, Box.low, Box.high, 0.2, 1.0, 0.01, max_batch=32)
        res["box"] = box_probe(probe_dev, 0)
        probe_dev.close()
    res["step"] = step_legs(widths, sizes, args.rounds, args.steps, args.warmup)
    if not args.no_buffer:
        res["buffer"] = buffer_legs(tmp, args.rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
