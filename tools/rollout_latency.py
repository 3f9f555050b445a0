"""Latency of the rollout-loop inference path at batch 1 (SURVEY 8f.3 callers: vae_common.py:45-61, train.py:142, run_eval.py:54):
VAE.encode([frame]) (host frame -> device, conv stack, mean to host) followed by PPO.predict(state) (host -> device, two MLP trunks, action to host).

    python tools/rollout_latency.py --envs [1,2,4,8,16,32,64] [--rounds 3] [--calls 200] [--batched-only | --record | --value | --obs-norm] [--no-box]
    python tools/rollout_latency.py --mlp [--envs 1,8,64] [--rounds 3] [--calls 200] [--no-box]
    python tools/rollout_latency.py --stack 4 [--envs 1,8,64] [--rounds 3] [--calls 200] [--no-box]

times, for each number of environments E, one BatchedRolloutStep call against a loop of E RolloutStep calls and against the two-call path (VAE.encode of E float
frames + PPO.predict of E states) on the same engines: the three are interleaved in every round, the line gives the median of the rounds' medians, the spread of
those medians (min - max) and the p90 over all calls.  --batched-only runs the batched calls alone (the form a kernel trace is taken of).  --record times
RolloutBuffer.step (the recording step, mi_rollout_step_batch_rec: the same eight launches, the heads also store state / action / value into the device tables)
against BatchedRolloutStep, interleaved; the buffer's outcome() / reset() book-keeping runs between the timed calls.  --value times the value-only call of
ContinuousRolloutBuffer.truncate (mi_rollout_value_batch_rec: the encoder chain, the value trunk and the value head) against the GREEDY recording call (what a bootstrap
is: mi_rollout_step_batch_rec) on the same frames, both without the row book-keeping and at fixed table rows, interleaved.  --obs-norm times the recording call and
the value-only call with running observation normalisation on (mi_rollout_step_batch_norm / mi_rollout_value_batch_norm: one more launch, rollout_obs_norm_kernel)
against the same calls of a twin buffer with the setting off, without the row book-keeping and at fixed table rows, interleaved; behind the table it times the merge
(mi_rollout_obs_stats alone, device events) over 1024 rows of 128 columns.  --mlp builds an MlpVAE (38400 -> 512 -> 256 -> 64) in place of the ConvVAE and times, at
E = 1, 8, 64 in interleaved rounds, the batched step (mi_mlp_rollout_step_batch), the two-call path on the same model and the recording call at fixed table rows, next to
the floor of layer 1: the 78.6 MB of its fp32 kernel at the box's measured read rate.  --stack K times the recording call and the value-only call with latent stacking on
(stacked(.., latent_stack=K) at z_dim = 64: a policy of 64 K + 3 inputs with PPO.set_wide_inputs(); mi_rollout_step_batch_stack / mi_rollout_value_batch_stack: one more launch,
rollout_stack_kernel) against the same calls of a buffer with the setting off (the 67-input policy), without the row book-keeping and at fixed table rows, interleaved,
at E = 1, 8, 64 (or --envs)."""
import argparse, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "carla-ppo_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np, torch
from vae.models import ConvVAE, MlpVAE
from ppo import PPO

ap = argparse.ArgumentParser()
ap.add_argument("--envs", nargs="?", const="1,2,4,8,16,32,64", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=200, help="timed calls per path, E and round")
ap.add_argument("--batched-only", action="store_true")
ap.add_argument("--record", action="store_true", help="RolloutBuffer.step against BatchedRolloutStep")
ap.add_argument("--value", action="store_true", help="the value-only call (mi_rollout_value_batch_rec) against the greedy recording call")
ap.add_argument("--obs-norm", action="store_true", help="the recording and value-only calls with observation normalisation on against the setting off; the merge at 1024 x 128")
ap.add_argument("--mlp", action="store_true", help="an MlpVAE encoder: the batched step, the two-call path and the recording call at E = 1, 8, 64 (or --envs)")
ap.add_argument("--stack", type=int, default=0, metavar="K", help="the recording and value-only calls with latent_stack=K against the setting off at E = 1, 8, 64 (or --envs)")
ap.add_argument("--no-box", action="store_true")
args = ap.parse_args()

class Box:
    low, high, shape = np.array([-1.0, 0.0], np.float32), np.array([1.0, 1.0], np.float32), (2,)
vae = (MlpVAE if args.mlp else ConvVAE)(np.array([80, 160, 3]), z_dim=64, model_dir=tempfile.mkdtemp(), precision=os.environ.get("MI355_PRECISION", "bf16"), training=False)
vae.init_session(init_logging=False)
agent = PPO(np.array([67]), Box(), model_dir=tempfile.mkdtemp())
agent.init_session(init_logging=False)
rng = np.random.RandomState(0)


def timed(fn, calls, after=None):
    for i in range(10):
        fn(i)
        if after: after()
    ts = []
    for i in range(calls):
        t0 = time.perf_counter(); fn(i); ts.append(time.perf_counter() - t0)
        if after: after()
    return np.array(ts) * 1e6


def envs_table():
    from rollout import BatchedRolloutStep, RolloutStep
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if not args.no_box:
        from bench import box_probe
        b = box_probe(agent.dev, 0)
        print("box: %.0f TFLOP/s bf16 MFMA at %.0f MHz, %.2f TB/s read" % (b["mfma_bf16_tflops"], b["sclk_mhz"], b["hbm_read_tbps"]))
    u8 = rng.randint(0, 256, (128, 80, 160, 3), dtype=np.uint8)
    f32 = u8.astype(np.float32) / 255.0
    ms = rng.rand(128, 3).astype(np.float32)
    one = RolloutStep(vae, agent)
    for E in [int(x) for x in args.envs.split(",") if x]:
        many = BatchedRolloutStep(vae, agent, E)
        sl = lambda i: slice((i * E) % 64, (i * E) % 64 + E)       # noqa: E731

        def batched(i): many(u8[sl(i)], ms[sl(i)])
        def loop(i):
            for e in range(E): one(u8[(i * E) % 64 + e], ms[(i * E) % 64 + e])
        def two_call(i):
            z = vae.encode(f32[sl(i)])
            agent.predict(np.concatenate([z, ms[sl(i)]], axis=1))
        paths = [("batched", batched)] if args.batched_only else [("batched", batched), ("loop of B=1", loop), ("two-call", two_call)]
        after = {}
        if args.record:
            from rollout import RolloutBuffer
            buf = RolloutBuffer(vae, agent, E, horizon=64, io=many.io)
            zeros, no = np.zeros(E), np.zeros(E, bool)

            def recording(i): buf.step(u8[sl(i)], ms[sl(i)])
            def book():                                              # untimed: the step's outcome, and a fresh buffer when the rows are full
                buf.outcome(zeros, no)
                if buf.lengths[0] >= buf.horizon: buf.reset()
            fixed = (np.arange(E) * (buf.horizon + 1)).astype(np.int32)

            def device_only(i):                                      # the recording call without the row book-keeping: always slot 0
                buf._step.record(*buf._step.check(u8[sl(i)], ms[sl(i)], False, None), False, fixed, buf.states, buf.actions, buf.values)
            paths, after = [("batched", batched), ("recording", recording), ("recording w/o book-keeping", device_only)], {"recording": book}
        if args.value:
            from rollout import ContinuousRolloutBuffer
            cbuf = ContinuousRolloutBuffer(vae, agent, E, horizon=64, io=many.io)
            slot0 = (np.arange(E) * (cbuf.horizon + 1)).astype(np.int32)

            def greedy_recording(i):
                cbuf._step.record(*cbuf._step.check(u8[sl(i)], ms[sl(i)], True, None), True, slot0, cbuf.states, cbuf.actions, cbuf.values)
            def value_only(i):
                f, n, meas, _ = cbuf._step.check(u8[sl(i)], ms[sl(i)], True, None)
                cbuf._step.record_value(f, n, meas, slot0, cbuf.final_values)
            paths, after = [("greedy recording", greedy_recording), ("value-only", value_only)], {}
        if args.stack:
            from rollout import ContinuousRolloutBuffer
            off = ContinuousRolloutBuffer(vae, agent, E, horizon=64, io=many.io)
            on = ContinuousRolloutBuffer.stacked(vae, stacked_agent(), E, 64, args.stack, io=many.io)
            slot0, lanes = (np.arange(E) * (off.horizon + 1)).astype(np.int32), np.arange(E)

            def recording_of(b):
                kw = {"lanes": lanes} if b is on else {}
                return lambda i: b._step.record(*b._step.check(u8[sl(i)], ms[sl(i)], False, None), False, slot0, b.states, b.actions, b.values, b.raw_states, **kw)
            def value_of(b):
                def call(i):
                    f, n, meas, _ = b._step.check(u8[sl(i)], ms[sl(i)], True, None)
                    b._step.record_value_lanes(f, n, meas, slot0, b.final_values, lanes)
                return call
            paths, after = [("recording", recording_of(off)), ("recording, stack", recording_of(on)), ("value-only", value_of(off)), ("value-only, stack", value_of(on))], {}
        if args.obs_norm:
            from rollout import ContinuousRolloutBuffer
            off, on = (ContinuousRolloutBuffer(vae, agent, E, horizon=64, io=many.io) for _ in range(2))
            on.set_observation_normalization()
            slot0 = (np.arange(E) * (off.horizon + 1)).astype(np.int32)

            def recording_of(b):
                return lambda i: b._step.record(*b._step.check(u8[sl(i)], ms[sl(i)], False, None), False, slot0, b.states, b.actions, b.values, b.raw_states)
            def value_of(b):
                def call(i):
                    f, n, meas, _ = b._step.check(u8[sl(i)], ms[sl(i)], True, None)
                    b._step.record_value(f, n, meas, slot0, b.final_values)
                return call
            paths, after = [("recording", recording_of(off)), ("recording, obs-norm", recording_of(on)), ("value-only", value_of(off)), ("value-only, obs-norm", value_of(on))], {}
        ts = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                ts[name].append(timed(fn, args.calls if name != "loop of B=1" else max(20, args.calls // E), after.get(name)))
        line, med = "E = %3d (io=%s):" % (E, many.io), {}
        for name, _ in paths:
            meds = [np.median(t) for t in ts[name]]
            med[name] = np.median(meds)
            line += "  %s %.1f us (rounds %.1f - %.1f, p90 %.1f)" % (name, med[name], min(meds), max(meds), np.percentile(np.concatenate(ts[name]), 90))
        if args.record and not args.value:
            line += "  | recording - batched %+.2f us, w/o book-keeping %+.2f us" % (med["recording"] - med["batched"], med["recording w/o book-keeping"] - med["batched"])
        elif args.stack:
            line += "  | stack %d - off: recording %+.2f us, value-only %+.2f us" % (args.stack, med["recording, stack"] - med["recording"], med["value-only, stack"] - med["value-only"])
        elif args.obs_norm:
            line += "  | obs-norm - off: recording %+.2f us, value-only %+.2f us" % (med["recording, obs-norm"] - med["recording"], med["value-only, obs-norm"] - med["value-only"])
        elif args.value:
            line += "  | value-only - greedy recording %+.2f us" % (med["value-only"] - med["greedy recording"])
        elif not args.batched_only:
            line += "  | loop / batched %.2f x, two-call / batched %.2f x" % (med["loop of B=1"] / med["batched"], med["two-call"] / med["batched"])
        print(line, flush=True)


_stacked = []


def stacked_agent():
    """The policy of --stack K: 64 K + 3 inputs, on the fused kernels' wide range (one engine for every E)."""
    if not _stacked:
        a = PPO(np.array([64 * args.stack + 3]), Box(), model_dir=tempfile.mkdtemp())
        a.set_wide_inputs()
        a.init_session(init_logging=False)
        _stacked.append(a)
    return _stacked[0]


def mlp_table():
    """The MlpVAE's batched step against the two-call path on the same model and the recording call, and the floor of layer 1's weight stream."""
    from rollout import BatchedRolloutStep, RolloutBuffer
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    w1_bytes = 4 * int(np.prod(vae.dev.source_shape)) * vae.dev.enc_sizes[0]
    rate = None
    if not args.no_box:
        from bench import box_probe
        b = box_probe(agent.dev, 0)
        rate = b["hbm_read_tbps"]
        print("box: %.0f TFLOP/s bf16 MFMA at %.0f MHz, %.2f TB/s read" % (b["mfma_bf16_tflops"], b["sclk_mhz"], rate))
        print("layer 1: %.1f MB of fp32 weights, %.1f us at that read rate" % (w1_bytes / 1e6, w1_bytes / (rate * 1e12) * 1e6))
    u8 = rng.randint(0, 256, (128, 80, 160, 3), dtype=np.uint8)
    f32 = u8.astype(np.float32) / 255.0
    ms = rng.rand(128, 3).astype(np.float32)
    for E in [int(x) for x in (args.envs or "1,8,64").split(",") if x]:
        many = BatchedRolloutStep(vae, agent, E)
        buf = RolloutBuffer(vae, agent, E, horizon=64, io=many.io)
        fixed = (np.arange(E) * (buf.horizon + 1)).astype(np.int32)
        sl = lambda i: slice((i * E) % 64, (i * E) % 64 + E)       # noqa: E731

        def batched(i): many(u8[sl(i)], ms[sl(i)])
        def two_call(i):
            z = vae.encode(f32[sl(i)])
            agent.predict(np.concatenate([z, ms[sl(i)]], axis=1))
        def recording(i):                                            # the recording call without the row book-keeping: always slot 0
            buf._step.record(*buf._step.check(u8[sl(i)], ms[sl(i)], False, None), False, fixed, buf.states, buf.actions, buf.values)
        paths = [("batched", batched), ("two-call", two_call), ("recording", recording)]
        ts = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                ts[name].append(timed(fn, args.calls))
        line, med = "E = %3d (io=%s, MlpVAE %s):" % (E, many.io, vae.precision), {}
        for name, _ in paths:
            meds = [np.median(t) for t in ts[name]]
            med[name] = np.median(meds)
            line += "  %s %.1f us (rounds %.1f - %.1f, p90 %.1f)" % (name, med[name], min(meds), max(meds), np.percentile(np.concatenate(ts[name]), 90))
        line += "  | two-call / batched %.2f x, recording - batched %+.2f us" % (med["two-call"] / med["batched"], med["recording"] - med["batched"])
        if rate:
            line += ", batched / W1 floor %.2f x" % (med["batched"] / (w1_bytes / (rate * 1e12) * 1e6))
        print(line, flush=True)


def merge_time(n=1024, din=128, calls=50):
    """mi_rollout_obs_stats alone over n rows of din columns (every row of the table, in order): device events around each call."""
    from mi355 import lib as milib
    L = milib.get()
    tab = torch.randn(n, din, device="cuda")
    rows = torch.arange(n, dtype=torch.int32, device="cuda")
    state = torch.zeros(1 + 2 * din, dtype=torch.float64, device="cuda")
    m32, i32 = torch.zeros(din, device="cuda"), torch.ones(din, device="cuda")
    scratch = torch.empty(int(L.mi_rollout_obs_stats_scratch_doubles(n, din)), dtype=torch.float64, device="cuda")
    batch = torch.zeros(3, din, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream()
    ts = []
    for i in range(calls + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        L.mi_rollout_obs_stats(st.cuda_stream, tab.data_ptr(), n, rows.data_ptr(), n, din, 0, 1, 1e-8, 10.0, state.data_ptr(), m32.data_ptr(), i32.data_ptr(), scratch.data_ptr(),
                               batch.data_ptr())
        b.record(st)
        b.synchronize()
        if i >= 5: ts.append(a.elapsed_time(b) * 1e3)
    print("mi_rollout_obs_stats, %d x %d (three launches, device events): median %.1f us, min %.1f us, p90 %.1f us" % (n, din, np.median(ts), min(ts), np.percentile(ts, 90)), flush=True)


if args.mlp:
    mlp_table()
    sys.exit(0)
if args.stack and args.envs is None:
    args.envs = "1,8,64"
if args.envs is not None:
    envs_table()
    if args.obs_norm:
        merge_time()
    sys.exit(0)
frames = rng.randint(0, 256, (64, 80, 160, 3)).astype(np.float32) / 255.0
meas = rng.rand(64, 3).astype(np.float32)
def one(i):
    z = vae.encode([frames[i % 64]])[0]
    return agent.predict(np.concatenate([z, meas[i % 64]]), greedy=True)
for i in range(20): one(i)
torch.cuda.synchronize()
ts = []
for i in range(200):
    t0 = time.perf_counter(); one(i); ts.append(time.perf_counter() - t0)
ts = np.array(ts) * 1e6
t_enc = []
for i in range(200):
    t0 = time.perf_counter(); vae.encode([frames[i % 64]]); t_enc.append(time.perf_counter() - t0)
print("encode + predict at batch 1: median %.0f us, p90 %.0f us (encode alone: median %.0f us)" % (np.median(ts), np.percentile(ts, 90), np.median(np.array(t_enc) * 1e6)))
# the one-call form: raw uint8 frame + measurements -> action, value, state
from rollout import RolloutStep
step = RolloutStep(vae, agent)
u8 = rng.randint(0, 256, (64, 80, 160, 3), dtype=np.uint8)
for i in range(20): step(u8[i % 64], meas[i % 64])
ts = []
for i in range(500):
    t0 = time.perf_counter(); step(u8[i % 64], meas[i % 64]); ts.append(time.perf_counter() - t0)
ts = np.array(ts) * 1e6
print("RolloutStep (one call, uint8 frame in, action / value / state out; io=%s): median %.1f us, p90 %.1f us, min %.1f us" % (step.io, np.median(ts), np.percentile(ts, 90), ts.min()))
