"""Seconds per PPO update from a device-resident rollout buffer (rollout.RolloutBuffer.update) against replay.replay_update on the same collection, from host
uint8 frames and from a device-resident frame table, with both functions' stage times.

    python tools/rollout_buffer_bench.py [--envs 64] [--steps 128] [--batch 32,2048] [--epochs 1] [--rounds 3] [--no-host-frames] [--no-box]

The collection: E environments x T steps (full rows, no terminal), frames drawn from a pool of random camera frames; the buffer records it through its own step
(mi_rollout_step_batch_rec), replay_update is handed the frames, the measurements and the actions the buffer's steps returned.  The three paths are interleaved in
every round; a line gives the median over the rounds and the stage times of the median round's neighbours (all rounds are printed).  The SGD stage is the same code
on every path; what differs is everything in front of it: upload + encode + values + GAE + casts against finish + log pi_old.

    python tools/rollout_buffer_bench.py --continuous [--mean-episode N] [--envs 8] [--steps 128] [--batch 32] ...

drives ONE scripted set of simulators (episode lengths from a seeded geometric draw with mean N, default a third of the horizon) through rollout.RolloutBuffer (a lane is
one episode segment: a simulator that reported done waits for the update) and through rollout.ContinuousRolloutBuffer (the simulator goes on from its reset observation),
and prints for both: step calls per update, samples per update, samples per step call, seconds per collection and seconds per update with the stage times.

    python tools/rollout_buffer_bench.py --diagnostics [--envs 64] [--steps 128] [--batch 32,2048] [--epochs 3] ...

adds the same update through RolloutBuffer.update_with_diagnostics (one statistics pass per epoch, mi_ppo_update_stats_idx) to the interleaved rounds, without the
replay paths: the "stats" stage is the cost of the passes, everything else is the plain update's.  A third path runs it with PPO.set_value_clip(--value-clip) on:
its "stats" stage also holds the mi_ppo_value_clip_stats launches (the difference of the two "stats" stages per epoch is their cost) and its SGD steps are
mi_ppo_train_step_vclip calls.

    python tools/rollout_buffer_bench.py --minibatch-norm [--ddof 0] [--envs 1024] [--steps 128] [--batch 32,2048] [--epochs 3] ...

runs the same update with RolloutBuffer.set_minibatch_normalization off and on in interleaved rounds, without the replay paths: the "minibatch_norm" stage (part of
"sgd") is the cost of the one mi_ppo_minibatch_advantages call per epoch, and the line ends with the on / off ratio of the medians.

    python tools/rollout_buffer_bench.py --recompute [--envs 64] [--steps 128] [--batch 32,2048] [--epochs 3] ...

runs the same update (three epochs unless --epochs says otherwise) with RolloutBuffer.set_advantage_recomputation off and on in interleaved rounds, without the
replay paths: the "recompute" stage (part of "sgd") is the cost of the refreshes -- one mi_ppo_values_idx call and one finish call before every epoch but the first
-- printed per refresh beside the "sgd" stage per epoch.  Then the bare value pass over 1024 x 128 table rows (one mi_ppo_values_idx call) against
mi_ppo_update_stats_idx with value_out and mi_ppo_kl_stats_idx over the same rows in chunks of 4096: one process, device events, three interleaved rounds.

    python tools/rollout_buffer_bench.py --vtrace [--envs 1024] [--steps 128] [--batch 2048] [--epochs 3] ...

runs the same update with advantage recomputation alone and with RolloutBuffer.set_vtrace on top of it in interleaved rounds (the refresh of the first is the code
--recompute measures): the "recompute" stage per refresh of both, and their ratio.  Then the bare log-probability pass over 1024 x 128 table rows (one
mi_ppo_logp_idx call) against one mi_ppo_values_idx call over the same rows, and mi_rollout_finish_vtrace alone against mi_rollout_finish on the collection's E x T
steps (one segment per lane), interleaved likewise."""
import argparse, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np, torch
from vae.models import ConvVAE
from ppo import PPO
import replay
from rollout import ContinuousRolloutBuffer, RolloutBuffer

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=64)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--batch", default="32,2048")
ap.add_argument("--epochs", type=int, default=1)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--pool", type=int, default=512, help="distinct random frames the collection draws from")
ap.add_argument("--no-host-frames", action="store_true", help="skip replay_update from host frames (E x (T + 1) x 38400 bytes of host memory)")
ap.add_argument("--no-box", action="store_true")
ap.add_argument("--continuous", action="store_true", help="RolloutBuffer against ContinuousRolloutBuffer on one scripted set of simulators (no replay paths)")
ap.add_argument("--diagnostics", action="store_true", help="RolloutBuffer.update against update_with_diagnostics in interleaved rounds (no replay paths)")
ap.add_argument("--minibatch-norm", action="store_true", help="RolloutBuffer.update with per-minibatch advantage normalisation off and on in interleaved rounds (no replay paths)")
ap.add_argument("--recompute", action="store_true", help="RolloutBuffer.update with advantage recomputation off and on in interleaved rounds, then the bare value pass (no replay paths)")
ap.add_argument("--vtrace", action="store_true", help="RolloutBuffer.update with advantage recomputation alone and with V-trace on top in interleaved rounds, then the bare log-probability pass and the bare finish call (no replay paths)")
ap.add_argument("--ddof", type=int, default=0, help="ddof of the normalised path of --minibatch-norm")
ap.add_argument("--value-clip", type=float, default=0.2, help="eps_v of the value-clipped path of --diagnostics")
ap.add_argument("--mean-episode", type=float, default=None, help="mean of the geometric episode lengths of --continuous (default: steps / 3)")
args = ap.parse_args()
if (args.recompute or args.vtrace) and args.epochs == 1:
    args.epochs = 3                                                                   # (the first epoch never refreshes)


class Box:
    low, high, shape = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32), (2,)


vae = ConvVAE(np.array([80, 160, 3]), z_dim=64, model_dir=tempfile.mkdtemp(), precision="bf16", training=False, seed=0)
vae.init_session(init_logging=False)
agent = PPO(np.array([67]), Box(), learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0, model_dir=tempfile.mkdtemp())
agent.init_session(init_logging=False)
if not args.no_box:
    from bench import box_probe
    b = box_probe(agent.dev, 0)
    print("box: %.0f TFLOP/s bf16 MFMA at %.0f MHz, %.2f TB/s read" % (b["mfma_bf16_tflops"], b["sclk_mhz"], b["hbm_read_tbps"]), flush=True)

E, T = args.envs, args.steps
rng = np.random.RandomState(0)
pool = rng.randint(0, 256, (args.pool, 80, 160, 3), dtype=np.uint8)


def continuous_bench():
    """Both buffer classes on the same scripted simulators: simulator e's k-th episode lasts episodes[e][k] steps (its last step reports done)."""
    mean = args.mean_episode or T / 3.0
    erng = np.random.RandomState(1)
    episodes = erng.geometric(1.0 / mean, (E, T))                                     # at most T episodes fit into a lane
    frame_of = erng.randint(0, args.pool, (E, T + 1))
    ms = np.stack([erng.uniform(-1, 1, (E, T + 1)), erng.uniform(0, 1, (E, T + 1)), erng.uniform(0, 30, (E, T + 1))], axis=-1)
    rew = erng.uniform(0, 1, (E, T))
    bufs = {"RolloutBuffer": RolloutBuffer(vae, agent, E, T), "ContinuousRolloutBuffer": ContinuousRolloutBuffer(vae, agent, E, T)}

    def collect(name):
        b = bufs[name]
        b.reset()
        episode, left = np.zeros(E, np.int64), episodes[:, 0].copy()                  # current episode of every simulator, steps left in it
        live, calls = np.arange(E), 0
        t0 = time.perf_counter()
        while len(live):
            slot = b.lengths[live]
            b.step(pool[frame_of[live, slot]], ms[live, slot], env_ids=live)
            left[live] -= 1
            dones = left[live] == 0
            b.outcome(rew[live, slot], dones, env_ids=live)
            calls += 1
            over = live[dones]
            episode[over] += 1
            left[over] = episodes[over, np.minimum(episode[over], T - 1)]
            keep = b.lengths[live] < T
            live = live[keep] if name == "ContinuousRolloutBuffer" else live[keep & ~dones]
        need = b.rows.needs_bootstrap() if name == "ContinuousRolloutBuffer" else b.rows.stepped()
        if len(need):
            b.bootstrap(pool[frame_of[need, b.lengths[need]]], ms[need, b.lengths[need]], env_ids=need)
            calls += 1
        return calls, time.perf_counter() - t0

    print("mean episode length %.1f steps (drawn: %.1f), E x T = %d x %d" % (mean, episodes.mean(), E, T), flush=True)
    for batch in [int(x) for x in args.batch.split(",") if x]:
        res = {name: [] for name in bufs}
        for rnd in range(args.rounds + 1):                                            # round 0 warms up (engine growth, allocator)
            for name in bufs:
                calls, t_collect = collect(name)
                st = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = bufs[name].update(num_epochs=args.epochs, batch_size=batch, stage_times=st)
                torch.cuda.synchronize()
                if rnd:
                    res[name].append((time.perf_counter() - t0, st, calls, out["samples"], t_collect, len(out["segments"]) if "segments" in out else int((out["lengths"] > 0).sum())))
        print("batch_size %d, %d epoch(s):" % (batch, args.epochs), flush=True)
        for name in bufs:
            tot = sorted(r[0] for r in res[name])
            med = next(r for r in res[name] if r[0] == tot[len(tot) // 2])
            _, stages, calls, samples, t_collect, n_seg = med
            print("  %-24s %4d step calls per update (incl. the bootstrap call), %6d samples per update in %d segments, %6.1f samples per step call, %d SGD steps; "
                  "collection %.4f s; update %.4f s (rounds %.4f - %.4f) | %s" % (name, calls, samples, n_seg, samples / calls, args.epochs * -(-samples // batch), t_collect, med[0],
                                                                                  tot[0], tot[-1], "  ".join("%s %.4f" % kv for kv in stages.items())), flush=True)


if args.continuous:
    continuous_bench()
    sys.exit(0)
idx = rng.randint(0, args.pool, (E, T + 1))
meas = np.stack([rng.uniform(-1, 1, (E, T + 1)), rng.uniform(0, 1, (E, T + 1)), rng.uniform(0, 30, (E, T + 1))], axis=-1).astype(np.float32)
rewards, dones = rng.uniform(0, 1, (E, T)), np.zeros((E, T))
frames_d = None if args.diagnostics or args.minibatch_norm or args.recompute or args.vtrace else torch.from_numpy(pool).to("cuda")[torch.from_numpy(idx).to("cuda")]           # [E, T + 1, 80, 160, 3] uint8 in HBM
frames_h = None if args.no_host_frames or args.diagnostics or args.minibatch_norm or args.recompute or args.vtrace else pool[idx]

buf = RolloutBuffer(vae, agent, E, T)


def collect(buf=buf):
    buf.reset()
    acts = np.zeros((E, T, 2), np.float32)
    t0 = time.perf_counter()
    for t in range(T):
        a, _, _ = buf.step(pool[idx[:, t]], meas[:, t])
        acts[:, t] = a
        buf.outcome(rewards[:, t], dones[:, t])
    buf.bootstrap(pool[idx[:, T]], meas[:, T])
    return acts, time.perf_counter() - t0


actions, t_collect = collect()
print("collection of %d x %d steps through the recording step: %.3f s (%.1f us per call incl. the host's frame gather)" % (E, T, t_collect, 1e6 * t_collect / (T + 1)), flush=True)


buf_on = buf_vt = None
if args.vtrace:                                                                       # recomputation with V-trace on top: a third buffer, the same collection
    buf_vt = RolloutBuffer(vae, agent, E, T)
    buf_vt.set_advantage_recomputation(True)
    buf_vt.set_vtrace(1.0, 1.0)
    collect(buf_vt)
if args.recompute or args.vtrace:                                                                    # the setting is switched with no step recorded: a buffer of its own, the same collection
    buf_on = RolloutBuffer(vae, agent, E, T)
    buf_on.set_advantage_recomputation(True)
    collect(buf_on)


def value_pass_bench(rows_total=1024 * 128, rounds=3, passes=10, chunk=4096):
    """The bare value pass against the two existing forward-only passes on the same table rows, interleaved: microseconds per pass over all rows (device events)."""
    from mi355.ppo_device import N_KL_STATS, N_STATS
    d, dev = agent.dev, agent.dev.device
    g = torch.Generator(device="cpu").manual_seed(0)
    S = (0.5 * torch.randn(rows_total, 67, generator=g)).to(dev)
    Act, Ret, LP, MO = torch.zeros(rows_total, 2, device=dev), torch.zeros(rows_total, device=dev), torch.zeros(rows_total, device=dev), torch.zeros(rows_total, 2, device=dev)
    rows = torch.randperm(rows_total, generator=g).to(torch.int32).to(dev)
    V, V2 = torch.zeros(rows_total, device=dev), torch.zeros(rows_total, device=dev)
    d.ensure_batch(chunk)
    us, uscr = torch.zeros(N_STATS, dtype=torch.float64, device=dev), torch.zeros(d.stats_scratch_doubles(chunk), dtype=torch.float64, device=dev)
    ks, kscr = torch.zeros(N_KL_STATS, dtype=torch.float64, device=dev), torch.zeros(d.kl_stats_scratch_doubles(chunk), dtype=torch.float64, device=dev)

    def values():
        d.values_idx(S, rows, rows_total, V)

    def stats():
        for lo in range(0, rows_total, chunk):
            d.update_stats(S, Act, Ret, LP, rows[lo:lo + chunk], chunk, us, uscr, accumulate=lo > 0, value_out=V2)

    def kl():
        for lo in range(0, rows_total, chunk):
            d.kl_stats(S, MO, rows[lo:lo + chunk], chunk, ks, kscr, accumulate=lo > 0)
    fns = {"values_idx": values, "update_stats + value_out": stats, "kl_stats": kl}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(passes):
                f()
            b.record()
            torch.cuda.synchronize()
            res[k].append(1e3 * a.elapsed_time(b) / passes)
    assert torch.equal(V.view(torch.int32), V2.view(torch.int32))                     # the two value tables hold the same bits
    print("value pass over %d table rows (max_batch %d, %d passes per window, %d interleaved rounds), us per pass:" % (rows_total, d.max_batch, passes, rounds), flush=True)
    for k, v in res.items():
        print("  %-26s median %.1f  (rounds %s)" % (k, sorted(v)[len(v) // 2], "  ".join("%.1f" % x for x in v)), flush=True)


def timed_rounds(fns, rounds, passes):
    """-> {name: [us per pass of every round]}: the functions interleaved in every round, device events around `passes` calls."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(passes):
                f()
            b.record()
            torch.cuda.synchronize()
            res[k].append(1e3 * a.elapsed_time(b) / passes)
    return res


def vtrace_pass_bench(rows_total=1024 * 128, rounds=3, passes=10):
    """The bare log-probability pass against the bare value pass on the same table rows, then mi_rollout_finish_vtrace against mi_rollout_finish on E x T steps."""
    d, dev = agent.dev, agent.dev.device
    g = torch.Generator(device="cpu").manual_seed(0)
    S = (0.5 * torch.randn(rows_total, 67, generator=g)).to(dev)
    Act = torch.rand(rows_total, 2, generator=g).to(dev)
    rows = torch.randperm(rows_total, generator=g).to(torch.int32).to(dev)
    V, LPN = torch.zeros(rows_total, device=dev), torch.zeros(rows_total, device=dev)
    res = timed_rounds({"values_idx": lambda: d.values_idx(S, rows, rows_total, V), "logp_idx": lambda: d.logp_idx(S, Act, rows, rows_total, LPN)}, rounds, passes)
    print("log-probability pass over %d table rows (max_batch %d, %d passes per window, %d interleaved rounds), us per pass:" % (rows_total, d.max_batch, passes, rounds), flush=True)
    for k, v in res.items():
        print("  %-26s median %.1f  (rounds %s)" % (k, sorted(v)[len(v) // 2], "  ".join("%.1f" % x for x in v)), flush=True)
    L, st = buf.L, torch.cuda.current_stream(dev).cuda_stream
    n = E * (T + 1)
    vals, lpo = torch.randn(n, generator=g).to(dev), (-1.5 + torch.randn(n, generator=g)).to(dev)
    lpn = lpo + (0.2 * torch.randn(n, generator=g)).to(dev)
    r, dn = torch.rand(E, T, generator=g, dtype=torch.float64).to(dev), torch.zeros(E, T, dtype=torch.float64, device=dev)
    ln = torch.full((E,), T, dtype=torch.int32, device=dev)
    row0 = (torch.arange(E, dtype=torch.int32) * (T + 1)).to(dev)
    ret, adv = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    f64, w = torch.zeros(3, E, T, dtype=torch.float64, device=dev), torch.zeros(E, T, dtype=torch.float64, device=dev)

    def gae():
        L.mi_rollout_finish(st, vals.data_ptr(), r.data_ptr(), dn.data_ptr(), ln.data_ptr(), E, T, 0.99, 0.95, ret.data_ptr(), adv.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(),
                            f64[2].data_ptr())

    def vtrace():
        L.mi_rollout_finish_vtrace(st, vals.data_ptr(), lpn.data_ptr(), lpo.data_ptr(), r.data_ptr(), dn.data_ptr(), row0.data_ptr(), ln.data_ptr(), E, E, T, 0.99, 0.95, 1.0, 1.0, 1, 0,
                                   None, ret.data_ptr(), adv.data_ptr(), f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr(), w.data_ptr(), None, None)
    res = timed_rounds({"mi_rollout_finish": gae, "mi_rollout_finish_vtrace": vtrace}, rounds, passes)
    print("finish call on %d x %d steps, one segment per lane (%d passes per window, %d interleaved rounds), us per call:" % (E, T, passes, rounds), flush=True)
    for k, v in res.items():
        print("  %-26s median %.1f  (rounds %s)" % (k, sorted(v)[len(v) // 2], "  ".join("%.1f" % x for x in v)), flush=True)


def run(path, batch):
    st = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if path == "buffer":
        buf.update(num_epochs=args.epochs, batch_size=batch, stage_times=st)
    elif path == "buffer + diagnostics":
        buf.update_with_diagnostics(num_epochs=args.epochs, batch_size=batch, stage_times=st)
    elif path == "+ recompute":
        buf_on.update(num_epochs=args.epochs, batch_size=batch, stage_times=st)
    elif path == "+ recompute + vtrace":
        buf_vt.update(num_epochs=args.epochs, batch_size=batch, stage_times=st)
    elif path == "+ minibatch norm":
        buf.set_minibatch_normalization(args.ddof)
        try:
            buf.update(num_epochs=args.epochs, batch_size=batch, stage_times=st)
        finally:
            buf.set_minibatch_normalization(None)
    elif path == "+ value clip":
        agent.set_value_clip(args.value_clip)
        try:
            buf.update_with_diagnostics(num_epochs=args.epochs, batch_size=batch, stage_times=st)
        finally:
            agent.set_value_clip(None)
    else:
        replay.replay_update(vae, agent, frames_h if path == "replay, host frames" else frames_d, meas, actions, rewards, dones, num_epochs=args.epochs, batch_size=batch, stage_times=st)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, st


paths = ["buffer", "replay, device frames"] + ([] if frames_h is None else ["replay, host frames"])
if args.diagnostics:
    paths = ["buffer", "buffer + diagnostics", "+ value clip"]
if args.minibatch_norm:
    paths = ["buffer", "+ minibatch norm"]
if args.recompute:
    paths = ["buffer", "+ recompute"]
if args.vtrace:
    paths = ["+ recompute", "+ recompute + vtrace"]
for batch in [int(x) for x in args.batch.split(",") if x]:
    for p in paths:
        run(p, batch)                                                                     # warm-up (engine growth, allocator)
    res = {p: [] for p in paths}
    for _ in range(args.rounds):
        for p in paths:
            res[p].append(run(p, batch))
    print("E x T = %d x %d, batch_size %d, %d epoch(s), %d SGD steps:" % (E, T, batch, args.epochs, args.epochs * -(-E * T // batch)), flush=True)
    for p in paths:
        tot = sorted(r[0] for r in res[p])
        med = tot[len(tot) // 2]
        stages = next(r[1] for r in res[p] if r[0] == med)
        front = sum(v for k, v in stages.items() if k not in ("sgd", "stats", "minibatch_norm", "recompute"))
        print("  %-22s %.4f s (rounds %.4f - %.4f)  in front of the SGD loop %.4f s  | %s" % (p, med, tot[0], tot[-1], front, "  ".join("%s %.4f" % kv for kv in stages.items())), flush=True)
        if args.minibatch_norm:
            off = sorted(r[0] for r in res["buffer"])[args.rounds // 2]
            print("    every round: %s" % "  ".join("%.4f" % r[0] for r in res[p]) + ("" if "minibatch_norm" not in stages else
                  "   minibatch_norm stage %.6f s = %.1f us per epoch, %.3f %% of the update;  on / off %.4f" % (stages["minibatch_norm"], 1e6 * stages["minibatch_norm"] / max(args.epochs, 1),
                                                                                                                   100.0 * stages["minibatch_norm"] / med, med / off)), flush=True)
        if args.recompute or args.vtrace:
            off = sorted(r[0] for r in res[paths[0]])[args.rounds // 2]
            print("    every round: %s   sgd stage %.4f s per epoch" % ("  ".join("%.4f" % r[0] for r in res[p]), stages["sgd"] / max(args.epochs, 1)) + ("" if "recompute" not in stages else
                  "   recompute stage %.6f s = %.1f us per refresh (%d refreshes), %.3f %% of the update;  on / off %.4f"
                  % (stages["recompute"], 1e6 * stages["recompute"] / max(args.epochs - 1, 1), max(args.epochs - 1, 0), 100.0 * stages["recompute"] / med, med / off)), flush=True)
        if args.diagnostics:
            print("    every round: %s" % "  ".join("%.4f" % r[0] for r in res[p]) + ("" if "stats" not in stages else
                  "   stats stage %.4f s = %.4f s per epoch, %.1f %% of the update" % (stages["stats"], stages["stats"] / max(args.epochs, 1), 100.0 * stages["stats"] / med)), flush=True)
if args.recompute:
    value_pass_bench()
if args.vtrace:
    vtrace_pass_bench()
