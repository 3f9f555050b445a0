"""Microseconds per finish call of a rollout buffer: mi_rollout_finish_segments (normalize 0 and 1) against mi_rollout_finish on the same tables in the same process.

    python tools/rollout_finish_bench.py [--shapes 64x128,1024x128] [--calls 200] [--rounds 3] [--boot] [--reward-scaling] [--no-box]

Layouts of the segment descriptors: `one` = one full segment per lane (what mi_rollout_finish computes, the yardstick applies), `few` = 2-4 segments per lane at seeded
random cuts, `short` = every segment 1-4 steps (the worst case: E x T / 2.5 one-wave blocks).  The dense call is timed next to every layout on the same tables (its work
does not depend on the descriptors).  A figure is device time between two events around `--calls` back-to-back calls, divided by the calls; the variants are interleaved in
every round and every round is printed.  --boot adds mi_rollout_finish_segments_boot (the finish that takes a per-segment bootstrap source) to every layout, with all
flags 0 (the same work as mi_rollout_finish_segments: the same bits, asserted) and with the LAST segment of every lane truncated (one truncation per lane), both
normalisations.  --reward-scaling times, instead of the layouts, what RolloutBuffer.set_reward_scaling adds in front of the dense finish: device time per call of
mi_rollout_scale_rewards alone and followed by mi_rollout_finish, and the buffers' "finish" STAGE as RolloutBuffer._update runs it -- a host clock around the upload of
the fp64 rewards and dones from host arrays, the call(s) and a device synchronise -- with the setting off and on, interleaved."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np, torch
from mi355 import lib as milib

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="64x128,1024x128")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--boot", action="store_true", help="also time mi_rollout_finish_segments_boot, all flags 0 and one truncation per lane")
ap.add_argument("--reward-scaling", action="store_true", help="time mi_rollout_scale_rewards and the buffers' finish stage with and without it, instead of the layouts")
ap.add_argument("--no-box", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rollout_finish_bench: needs a GPU")
L = milib.get()
if not args.no_box:
    import tempfile
    from bench import box_probe
    from ppo import PPO

    class Box:
        low, high, shape = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32), (2,)
    agent = PPO(np.array([67]), Box(), learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0, model_dir=tempfile.mkdtemp())
    agent.init_session(init_logging=False)
    b = box_probe(agent.dev, 0)
    print("box: %.0f TFLOP/s bf16 MFMA at %.0f MHz, %.2f TB/s read" % (b["mfma_bf16_tflops"], b["sclk_mhz"], b["hbm_read_tbps"]), flush=True)


def cuts(layout, E, T, rng):
    """-> (descriptors int32 [n_seg, 2] of (table row, length), dones [E, T]): every lane full, a done at the end of every segment but a lane's last."""
    desc, dones = [], np.zeros((E, T))
    for e in range(E):
        if layout == "one":
            ends = [T]
        elif layout == "few":
            ends = sorted(set(rng.choice(np.arange(1, T), size=min(T - 1, rng.randint(1, 4)), replace=False).tolist())) + [T]
        else:
            ends, s = [], 0
            while s < T:
                s = min(T, s + rng.randint(1, 5))
                ends.append(s)
        s = 0
        for end in ends:
            desc.append((e * (T + 1) + s, end - s))
            if end < T:
                dones[e, end - 1] = 1.0
            s = end
    return np.asarray(desc, np.int32), dones


def reward_scaling_bench(E, T):
    """Device time per call and the host-clocked finish stage, reward scaling off / on, on full lanes with a done every 40 steps or so."""
    import time
    rng = np.random.RandomState(E + T)
    values = torch.from_numpy(rng.standard_normal(E * (T + 1)).astype(np.float32)).cuda()
    r_h, d_h = rng.uniform(-1, 1, (E, T)), (rng.uniform(size=(E, T)) < 0.025).astype(np.float64)
    lengths = torch.full((E,), T, dtype=torch.int32, device="cuda")
    ret32, adv32 = torch.zeros(E * (T + 1), device="cuda"), torch.zeros(E * (T + 1), device="cuda")
    f64 = torch.zeros(3, E, T, dtype=torch.float64, device="cuda")
    state, carry = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(E, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(int(L.mi_rollout_scale_rewards_scratch_doubles(E)), dtype=torch.float64, device="cuda")
    scaled = torch.zeros(2, E, T, dtype=torch.float64, device="cuda")
    r_d, d_d = torch.from_numpy(r_h).cuda(), torch.from_numpy(d_h).cuda()

    def finish(r, d):
        L.mi_rollout_finish(st, values.data_ptr(), r.data_ptr(), d.data_ptr(), lengths.data_ptr(), E, T, 0.99, 0.95, ret32.data_ptr(), adv32.data_ptr(),
                            f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())

    def scale(r, d):
        L.mi_rollout_scale_rewards(st, r.data_ptr(), d.data_ptr(), None, lengths.data_ptr(), E, T, 0.99, 1e-8, 10.0, 1, state.data_ptr(), carry.data_ptr(), scratch.data_ptr(),
                                   scaled[0].data_ptr(), scaled[1].data_ptr())

    def both(r, d):
        scale(r, d)
        finish(scaled[1], d)

    def device_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn(r_d, d_d)
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / args.calls

    def stage_us(fn):
        times = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(torch.from_numpy(r_h).cuda(), torch.from_numpy(d_h).cuda())
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return 1e6 * sorted(times)[len(times) // 2]
    variants = [("device: mi_rollout_finish", device_us, finish), ("device: mi_rollout_scale_rewards", device_us, scale), ("device: scale_rewards + finish", device_us, both),
                ("finish stage, scaling off", stage_us, finish), ("finish stage, scaling on", stage_us, both)]
    for _, _, fn in variants:
        for _ in range(20):
            fn(r_d, d_d)
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, how, fn in variants:
            res[name].append(how(fn))
    print("E x T = %d x %d, reward scaling (full lanes):" % (E, T), flush=True)
    for name, _, _ in variants:
        r = res[name]
        print("  %-40s %8.1f us per call (rounds %s)" % (name, sorted(r)[len(r) // 2], " ".join("%.1f" % x for x in r)), flush=True)


st = torch.cuda.current_stream().cuda_stream
for shape in args.shapes.split(","):
    E, T = (int(x) for x in shape.split("x"))
    if args.reward_scaling:
        reward_scaling_bench(E, T)
        continue
    rng = np.random.RandomState(E + T)
    values = torch.from_numpy(rng.standard_normal(E * (T + 1)).astype(np.float32)).cuda()
    rewards = torch.from_numpy(rng.uniform(-1, 1, (E, T))).cuda()
    lengths = torch.full((E,), T, dtype=torch.int32, device="cuda")
    ret32, adv32 = torch.zeros(E * (T + 1), device="cuda"), torch.zeros(E * (T + 1), device="cuda")
    f64 = torch.zeros(3, E, T, dtype=torch.float64, device="cuda")
    for layout in ("one", "few", "short"):
        desc, dones = cuts(layout, E, T, rng)
        n_seg = len(desc)
        d_d, row_d, len_d = torch.from_numpy(dones).cuda(), torch.from_numpy(desc[:, 0].copy()).cuda(), torch.from_numpy(desc[:, 1].copy()).cuda()
        scratch = torch.zeros(int(L.mi_rollout_finish_segments_scratch_doubles(n_seg)), dtype=torch.float64, device="cuda")

        def dense():
            L.mi_rollout_finish(st, values.data_ptr(), rewards.data_ptr(), d_d.data_ptr(), lengths.data_ptr(), E, T, 0.99, 0.95, ret32.data_ptr(), adv32.data_ptr(),
                                f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())

        def seg(normalize):
            L.mi_rollout_finish_segments(st, values.data_ptr(), rewards.data_ptr(), d_d.data_ptr(), row_d.data_ptr(), len_d.data_ptr(), n_seg, E, T, 0.99, 0.95, normalize,
                                         scratch.data_ptr(), ret32.data_ptr(), adv32.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())
        variants = [("mi_rollout_finish", dense), ("segments, normalize 0", lambda: seg(0)), ("segments, normalize 1", lambda: seg(1))]
        if args.boot:
            final = torch.from_numpy(rng.standard_normal(E * (T + 1)).astype(np.float32)).cuda()
            last = np.zeros(n_seg, np.int32)
            last[np.nonzero(desc[:, 0] + desc[:, 1] == (desc[:, 0] // (T + 1)) * (T + 1) + T)[0]] = 1      # the segment that ends at the lane's last slot
            flags = {"flags 0": torch.zeros(n_seg, dtype=torch.int32, device="cuda"), "1 truncation per lane": torch.from_numpy(last).cuda()}

            def boot(normalize, which):
                L.mi_rollout_finish_segments_boot(st, values.data_ptr(), rewards.data_ptr(), d_d.data_ptr(), row_d.data_ptr(), len_d.data_ptr(), n_seg, E, T, 0.99, 0.95, normalize,
                                                  scratch.data_ptr(), ret32.data_ptr(), adv32.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr(), final.data_ptr(),
                                                  flags[which].data_ptr())
            for normalize in (0, 1):
                seg(normalize)
                want = (ret32.clone(), adv32.clone(), f64.clone())
                boot(normalize, "flags 0")
                assert all(torch.equal(x, y) for x, y in zip(want, (ret32, adv32, f64))), "mi_rollout_finish_segments_boot with no flag set differs from mi_rollout_finish_segments"
                for which in flags:
                    variants.append(("boot, normalize %d, %s" % (normalize, which), lambda normalize=normalize, which=which: boot(normalize, which)))
        if layout == "one":                                                          # same work: same bits
            dense()
            want = (ret32.clone(), adv32.clone(), f64.clone())
            seg(0)
            assert all(torch.equal(x, y) for x, y in zip(want, (ret32, adv32, f64))), "one segment per lane differs from mi_rollout_finish"

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            return 1e3 * a.elapsed_time(b) / args.calls
        for _, fn in variants:
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                res[name].append(timed(fn))
        print("E x T = %d x %d, layout %-5s %6d segments (%.1f steps each):" % (E, T, layout, n_seg, E * T / n_seg), flush=True)
        for name, _ in variants:
            r = res[name]
            print("  %-40s %8.1f us per call (rounds %s)" % (name, sorted(r)[len(r) // 2], " ".join("%.1f" % x for x in r)), flush=True)
