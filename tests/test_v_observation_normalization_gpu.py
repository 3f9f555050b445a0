"""Running observation normalisation on the GPU (mi_rollout_obs_stats, mi_rollout_step_batch_norm, mi_rollout_value_batch_norm,
RolloutBuffer.set_observation_normalization).

The moments kernel alone (torch tensors and the C ABI only): (n, din) = (1, 67), (5, 67), (257, 67) -- nine blocks of 32 list entries, the last with one --, (1000, 5)
and (300, 100), and (40, 200), where a thread of the 128 owns two columns; the index list has holes, one negative row and one row behind the table, and every table row it does not name holds NaN.  The reference is
tests/test_observation_normalization_host.py's numpy float64 one.  Bounds: the count exact; mean within 1e-12 max|x| of the column and M2 / count within 1e-9 relative
(at most 1000 fp64 terms: n 2^-53 ~ 1e-13), in one merge and across three chained ones; a constant column's M2 exactly 0.0; the fp32 pair within 1 fp32 ulp of the
reference formula applied to the DEVICE's fp64 state.

The step entries at n = 1, 3, 33 (33 crosses the 32-row MFMA tile) with 2 and 3 actions, on a synthetic, well-conditioned state (column means N(0, 0.1), variances in
[0.25, 4], the speed column mean 15 / var 75): tolerances of rollout_gpu_common against the oracle fed normalize_observations() of the device's returned states, 1e-5
between device paths.

The buffers at (E, T) = (3, 5) and (5, 20), both classes, one truncation in the continuous one.  Their statistics are those of the collection itself: frames of varied
brightness, so that the latent columns really vary, and epsilon = 1e-2, which bounds inv_std by 10 -- a latent column of near-zero variance would otherwise be scaled
by up to 1e4 and carry the last bit of the encoder's fp32 atomics into the actions, above the 1e-5 asked between two device paths."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rollout_gpu_common import A, K, SENTINEL, Z, bitwise, close, flat_state, inputs, make_pair, make_world, same_update  # noqa: E402
from test_observation_normalization_host import check_moments, columns, derive, reference  # noqa: E402

DIN = Z + K
INF = float("inf")
SHAPES = [(1, 67), (5, 67), (257, 67), (1000, 5), (300, 100)]
WIDE = [(40, 200)]                                                                   # more columns than the 128 threads of a block: a thread's second column


def ulp_close(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Stats:
    """mi_rollout_obs_stats on numpy inputs."""

    def __init__(self):
        import torch
        from mi355 import lib as milib
        self.torch, self.L, self.device = torch, milib.get(), torch.device("cuda:0")

    def run(self, table, idx, state, pair=None, merge=1, clip=10.0, epsilon=1e-8, first_col=0):
        """-> (state', mean32, inv32, batch [3, din]); pair: the fp32 (mean32, inv32) on entry (None: 0 / 1)."""
        torch = self.torch
        n_rows, din = table.shape
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.device)      # noqa: E731
        tab, rows, st = up(table.astype(np.float32)), up(np.asarray(idx, np.int32)), up(np.asarray(state, np.float64))
        m32 = up(np.zeros(din, np.float32) if pair is None else pair[0])
        i32 = up(np.ones(din, np.float32) if pair is None else pair[1])
        n = len(idx)
        scratch = torch.full((int(self.L.mi_rollout_obs_stats_scratch_doubles(n, din)),), -1.0, dtype=torch.float64, device=self.device)
        batch = torch.full((3, din), float("nan"), dtype=torch.float64, device=self.device)
        self.L.mi_rollout_obs_stats(torch.cuda.current_stream(self.device).cuda_stream, tab.data_ptr(), n_rows, rows.data_ptr(), n, din, first_col, merge, epsilon, clip,
                                    st.data_ptr(), m32.data_ptr(), i32.data_ptr(), scratch.data_ptr(), batch.data_ptr())
        torch.cuda.synchronize(self.device)
        assert same_bits(tab.cpu().numpy(), table.astype(np.float32))                 # the table is read, never written
        return st.cpu().numpy(), m32.cpu().numpy(), i32.cpu().numpy(), batch.cpu().numpy()


@pytest.fixture(scope="module")
def stats():
    return Stats()


def make_list(rng, n, din):
    """-> (table [n_rows, din] with NaN in every row the list does not name, list of n + 2 entries: n distinct table rows in random order with holes between them, one
    negative entry and one behind the table, x [n, din]: the named rows in list order)."""
    n_rows = 2 * n + 3
    x = columns(rng, n, din)
    named = rng.permutation(n_rows)[:n]
    table = np.full((n_rows, din), np.nan, np.float32)
    table[named] = x
    idx = named.astype(np.int64).tolist()
    idx.insert(n // 2, -1)
    idx.insert(len(idx) - (1 if n > 1 else 0), n_rows)
    return table, np.asarray(idx, np.int32), x


@pytest.mark.parametrize("n,din", SHAPES + WIDE)
def test_moments_against_the_reference(stats, n, din):
    rng = np.random.RandomState(7 * n + din)
    state0 = np.zeros(1 + 2 * din)
    state0[0], state0[1:1 + din], state0[1 + din:] = 40.0, 0.1 * rng.standard_normal(din), 40.0 * rng.uniform(0.25, 4.0, din)      # statistics of 40 earlier rows
    table, idx, x = make_list(rng, n, din)
    want, _, _, m_b, m2_b = reference(x, state0, 1)
    got, m32, i32, batch = stats.run(table, idx, state0)
    assert got[0] == want[0] == 40.0 + n                                             # the count is exact: the two entries outside the table do not count
    scale = np.abs(x.astype(np.float64)).max(0)
    errs = dict(mean=np.abs(got[1:1 + din] - want[1:1 + din]).max(), batch_mean=np.abs(batch[0] - m_b).max())
    assert np.all(np.abs(got[1:1 + din] - want[1:1 + din]) <= 1e-12 * scale), errs
    assert np.all(np.abs(batch[0] - m_b) <= 1e-12 * scale), errs
    var_g, var_w = got[1 + din:] / got[0], want[1 + din:] / want[0]
    assert np.all(np.abs(var_g - var_w) <= 1e-9 * var_w), np.abs(var_g / var_w - 1).max()
    assert np.all(np.abs(batch[1] - m2_b) <= 1e-9 * m2_b)
    if din > 1:
        assert batch[1][1] == 0.0 and batch[0][1] == np.float64(np.float32(0.375))   # the constant column: its fp64 sums are exact
    # the fp32 pair from the device's own fp64 state
    w_mean, w_inv = derive(got, din, 1e-8, 0)
    bitwise = same_bits(m32, w_mean) and same_bits(i32, w_inv)
    print("\n(n, din) = (%d, %d): mean err %.3g, var rel err %.3g; fp32 pair bitwise the reference formula on the device state: %s"
          % (n, din, errs["mean"], np.abs(var_g / np.maximum(var_w, 1e-300) - 1).max(), bitwise))
    assert ulp_close(m32, w_mean) and ulp_close(i32, w_inv)
    # the clamped counts: the normalise expression under the pair ON ENTRY (0 / 1), clip 10: the raw entries of magnitude >= 10
    assert np.array_equal(batch[2], (np.abs(x) >= 10.0).sum(0).astype(np.float64))
    if n >= 257:
        assert batch[2][-1] > 0                                                      # the speed column (mean 15) has some
    # NaN in the rows the list does not name changes nothing; two runs are bitwise equal
    table0 = np.where(np.isnan(table), np.float32(0.0), table)
    for other in (stats.run(table0, idx, state0), stats.run(table, idx, state0)):
        assert all(same_bits(p, q) for p, q in zip(other, (got, m32, i32, batch)))
    # merge = 0 leaves the state bitwise and derives from it; first_col: mean 0 / inv 1 below it
    first = min(din, 64)
    fz, fm, fi, fb = stats.run(table, idx, state0, merge=0, first_col=first)
    assert same_bits(fz, state0) and same_bits(fb, batch)
    z_mean, z_inv = derive(state0, din, 1e-8, first)
    assert ulp_close(fm, z_mean) and ulp_close(fi, z_inv) and np.all(fm[:first] == 0.0) and np.all(fi[:first] == 1.0)
    # from the zero state the first merge is the batch's own moments; a fresh state derives mean 0 / inv exactly 1.0
    z, zm, zi, _ = stats.run(table, idx, np.zeros(1 + 2 * din))
    check_moments(z, x, (n, din, "zero state"))
    f, fm, fi, _ = stats.run(table, idx, np.zeros(1 + 2 * din), merge=0)
    assert not f.any() and not fm.any() and np.all(fi == 1.0)


@pytest.mark.parametrize("n,din", SHAPES + WIDE)
def test_three_chained_merges(stats, n, din):
    rng = np.random.RandomState(n + din)
    state, want, seen, pair = np.zeros(1 + 2 * din), np.zeros(1 + 2 * din), [], None
    for k, nk in enumerate((n, 1, max(n // 3, 1))):
        table, idx, x = make_list(rng, nk, din)
        want = reference(x, want, 1)[0]
        state, m32, i32, batch = stats.run(table, idx, state, pair)
        seen.append(x)
        check_moments(state, np.concatenate(seen), (n, din, k))
        assert state[0] == want[0] and np.all(np.abs(state[1:1 + din] - want[1:1 + din]) <= 1e-12 * np.abs(np.concatenate(seen)).max(0))
        assert np.all(np.abs(state[1 + din:] - want[1 + din:]) <= 1e-9 * want[1 + din:])
        if din > 1:
            assert state[1 + din + 1] == 0.0                                         # the constant column stays exact across merges
        if pair is not None:                                                         # the clamped counts follow the pair on entry
            normed = np.minimum(np.maximum((x - pair[0]) * pair[1], np.float32(-10.0)), np.float32(10.0))
            assert normed.dtype == np.float32 and np.array_equal(batch[2], (np.abs(normed) == 10.0).sum(0))
        pair = (m32, i32)


@pytest.mark.parametrize("bad", [float("nan"), INF, -INF])
def test_a_batch_that_is_not_finite_is_not_merged(stats, bad):
    """One entry that is not finite, in the last of three blocks: no column is merged, the state stays bitwise, the pair is derived from it, and the batch mean of that
    column alone shows it.  (One NaN merged would stay in mean / M2 for good.)"""
    n, din, col = 70, 67, 5
    rng = np.random.RandomState(70)
    state0 = np.zeros(1 + 2 * din)
    state0[0], state0[1:1 + din], state0[1 + din:] = 40.0, 0.1 * rng.standard_normal(din), 40.0 * rng.uniform(0.25, 4.0, din)
    table, idx, x = make_list(rng, n, din)
    good = stats.run(table, idx, state0)
    assert good[0][0] == 40.0 + n and np.isfinite(good[3]).all()
    table[idx[-1], col] = bad                                                        # (the list's last entry is a table row: the one behind the table sits before it)
    assert 0 <= idx[-1] < len(table)
    got, m32, i32, batch = stats.run(table, idx, state0)
    assert same_bits(got, state0)
    other = np.arange(din) != col
    assert not np.isfinite(batch[0][col]) and same_bits(batch[0][other], good[3][0][other]) and same_bits(batch[1][other], good[3][1][other])
    w_mean, w_inv = derive(state0, din, 1e-8, 0)
    assert ulp_close(m32, w_mean) and ulp_close(i32, w_inv)
    frozen = stats.run(table, idx, state0, merge=0)
    assert all(same_bits(p, q) for p, q in zip(frozen, (got, m32, i32, batch)))


def test_an_empty_list_derives_only(stats):
    import torch
    din = 5
    state = np.array([10.0] + [1.0, -2.0, 0.0, 0.5, 15.0] + [2.5, 40.0, 0.0, 10.0, 750.0])
    st, m32, i32 = (torch.from_numpy(x).cuda() for x in (state, np.full(din, 9.0, np.float32), np.full(din, 9.0, np.float32)))
    batch = torch.full((3, din), float("nan"), dtype=torch.float64, device="cuda")
    for merge in (0, 1):
        stats.L.mi_rollout_obs_stats(torch.cuda.current_stream().cuda_stream, None, 0, None, 0, din, 2, merge, 1e-8, 10.0, st.data_ptr(), m32.data_ptr(), i32.data_ptr(), None,
                                     batch.data_ptr())
        torch.cuda.synchronize()
        assert same_bits(st.cpu().numpy(), state) and not batch.cpu().numpy().any()
        w_mean, w_inv = derive(state, din, 1e-8, 2)
        assert ulp_close(m32.cpu().numpy(), w_mean) and ulp_close(i32.cpu().numpy(), w_inv)
        assert m32.cpu().numpy().tolist() == [0.0, 0.0, 0.0, 0.5, 15.0] and i32.cpu().numpy()[:2].tolist() == [1.0, 1.0]


# ---- the step entries ----
def synthetic_state(seed=5, count=1000.0, **settings):
    rng = np.random.RandomState(seed)
    mean, var = 0.1 * rng.standard_normal(DIN), rng.uniform(0.25, 4.0, DIN)
    mean[-1], var[-1] = 15.0, 75.0
    d = dict(count=count, mean=mean, m2=var * count, z_dim=Z, clip=10.0, epsilon=1e-8, frozen=False, normalize_latents=True)
    d.update(settings)
    return d


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = make_world(tmp_path_factory, "observation_normalization")
    w["pairs"] = {A: (w["o"], w["m"])}
    return w


def pair_of(world, n_act):
    """The oracle / device policy pair with n_act actions (2: the world's; 3: bounds and logstd of tests/ppo_shape_cases.py, N(0, 0.05) biases)."""
    if n_act not in world["pairs"]:
        import ppo_shape_cases as pc
        from oracle import ppo_oracle as po
        from ppo import PPO
        hp = dict(learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0)
        space = po.ActionSpace(*pc.bounds(n_act))
        o = po.OraclePPO([DIN], space, seed=4, **hp)
        rng = np.random.RandomState(41 + n_act)
        for k in o.params:
            if k.endswith("bias"):
                o.params[k] = (0.05 * rng.standard_normal(o.params[k].shape)).astype(np.float32)
        o.params["policy/action_logstd"] = pc.logstd_of(n_act)
        m = PPO(np.array([DIN]), space, model_dir=str(world["tmp"] / ("ppo_%d" % n_act)), seed=4, **hp)
        m.set_weights(o.params)
        m.init_session(init_logging=False)
        world["pairs"][n_act] = (o, m)
    return world["pairs"][n_act]


def all_tables(buf):
    return [t.cpu().numpy() for t in (buf.states, buf.raw_states, buf.actions, buf.values)]


@pytest.mark.parametrize("n_act", [2, 3])
@pytest.mark.parametrize("n", [1, 3, 33])
def test_step_entries(world, n, n_act):
    import torch
    from mi355 import lib as milib
    from rollout import BatchedRolloutStep, ContinuousRolloutBuffer, normalize_observations
    o, m = pair_of(world, n_act)
    rng = np.random.RandomState(100 * n + n_act)
    frames, meas, noise = inputs(rng, n, n_act)
    T = 2
    state = synthetic_state()
    buf = ContinuousRolloutBuffer(world["vae"], m, n, T)
    buf.load_observation_normalization_state(state)
    for t in (buf.states, buf.raw_states, buf.actions, buf.values, buf.final_values):
        t.fill_(SENTINEL)
    perm = rng.permutation(n)
    rows = perm * (T + 1)
    for greedy in (False, True):
        buf.reset()
        actions, values, states = buf.step(frames, meas, env_ids=perm, greedy=greedy, noise=noise)
        ts, tr, ta, tv = all_tables(buf)
        # the raw table holds, bitwise, the returned raw state; the normalised table the formula of it
        assert states.dtype == np.float64 and same_bits(tr[rows], states.astype(np.float32)) and np.array_equal(states[:, Z:], meas)
        want = normalize_observations(tr[rows], state)
        print("\nn = %d, A = %d, greedy %s: tab_states bitwise normalize_observations(tab_raw_states): %s" % (n, n_act, greedy, same_bits(ts[rows], want)))
        assert ulp_close(ts[rows], want)
        assert np.abs(ts[rows][:, -1]).max() <= 3.0                                   # the speed column (0..30) is on the others' scale now
        assert same_bits(ta[rows], actions) and same_bits(tv[rows], values)
        other = np.ones(len(tv), bool)
        other[rows] = False
        assert all(np.all(t[other] == SENTINEL) for t in (ts, tr, ta, tv))           # untouched rows keep their sentinel
        # against the oracle fed the normalised device states
        a_o, v_o = o.predict(normalize_observations(states, state), greedy=greedy, noise=None if greedy else noise)
        a_o, v_o = np.asarray(a_o).reshape(n, n_act), np.asarray(v_o).reshape(n)
        for e in range(n):
            assert np.allclose(actions[e], a_o[e], rtol=1e-4, atol=1e-5), (n, n_act, greedy, e, actions[e], a_o[e])
            assert float(values[e]) == pytest.approx(float(v_o[e]), rel=1e-4, abs=1e-5), (n, n_act, greedy, e)
        # the value-only entry: within 1e-5 of the value of the full normalised step (same frames)
        buf.outcome(np.zeros(n), np.zeros(n, bool), env_ids=perm)
        v_only = buf.truncate(frames, meas, env_ids=perm)
        assert np.allclose(v_only, values, rtol=1e-5, atol=1e-5), np.abs(v_only - values).max()
        assert same_bits(buf.final_values.cpu().numpy()[rows], v_only) and bool((buf.final_values.cpu()[torch.from_numpy(other)] == SENTINEL).all())
        # table_rows = NULL records nothing, whatever tables are passed; the evaluation step gives the step's greedy actions
        if greedy:
            s, L = buf._step, milib.get()
            before = all_tables(buf)
            base = s.h_in.data_ptr()
            fptr = base + s._f_off
            on = buf._obs_norm
            f, nn, mm, _ = s.check(frames, meas, True, None)
            s._in_np[:nn * s.frame_bytes] = f.reshape(-1)
            s._f_np[:nn * K] = mm.reshape(-1)
            rc = L.cdll.mi_rollout_step_batch_norm(world["vae"].dev.handle, m.dev.handle, torch.cuda.current_stream().cuda_stream, base, fptr, K, None, 1, n,
                                                   s.scratch.data_ptr(), s.scratch_bytes, s.h_out.data_ptr(), on["mean32"].data_ptr(), on["inv32"].data_ptr(), 10.0,
                                                   on["nstate"].data_ptr(), None, buf.n_table_rows, buf.states.data_ptr(), buf.raw_states.data_ptr(),
                                                   buf.actions.data_ptr(), buf.values.data_ptr())
            torch.cuda.synchronize()
            assert rc == 0 and all(same_bits(p, q) for p, q in zip(all_tables(buf), before))
            assert np.allclose(s._out_np[:n, :n_act], actions, rtol=1e-5, atol=1e-5)
            ev = BatchedRolloutStep(world["vae"], m, n)
            ev.set_observation_normalization(buf.observation_normalization_state())
            got = ev(frames, meas, greedy=True)
            assert close(got[:2], (actions, values)) and same_bits(got[2][:, Z:], meas)
            ev.set_observation_normalization(None)
            assert not close(ev(frames, meas, greedy=True)[:2], (actions, values))    # (the statistics matter)
    # fresh statistics and clip = inf: the identity -- the normalised table is the raw one, actions / values those of the unnormalised recording step
    fresh = ContinuousRolloutBuffer(world["vae"], m, n, T)
    fresh.set_observation_normalization(clip=INF)
    plain = ContinuousRolloutBuffer(world["vae"], m, n, T)
    got = fresh.step(frames, meas, env_ids=perm, noise=noise)
    ref = plain.step(frames, meas, env_ids=perm, noise=noise)
    assert same_bits(fresh.states.cpu().numpy(), fresh.raw_states.cpu().numpy()) and bool(fresh.states[torch.from_numpy(rows)].ne(0).any())
    assert close(got, ref)
    assert np.allclose(fresh.states.cpu().numpy(), plain.states.cpu().numpy(), rtol=1e-5, atol=1e-5)


# ---- the buffers ----
BATCH, EPOCHS, SEED, EPS = 8, 2, 3, 1e-2
ON_KEYS = {"observation_rms", "observation_clip_fraction"}


def varied(rng, n):
    """inputs() with every frame at a brightness of its own (5% .. 100%)."""
    f, ms, nz = inputs(rng, n)
    return (f * rng.uniform(0.05, 1.0, (n, 1, 1, 1))).astype(np.uint8), ms, nz


def fill(buf, continuous, seed=571):
    """One collection through the buffer's own step.  RolloutBuffer: the last lane reports done at its step 4 and stops.  ContinuousRolloutBuffer: lane 1 reports done at
    its step 3 and goes on, lane 0 is truncated at its step 4."""
    E, T = buf.num_envs, buf.horizon
    rng = np.random.RandomState(seed)
    buf.reset()
    live = np.arange(E)
    for t in range(1, T + 1):
        f, ms, nz = varied(rng, E)
        buf.step(f[live], ms[live], env_ids=live, noise=nz[live])
        rewards = rng.standard_normal(E)
        dones = np.array([(continuous and e == 1 and t == 3) or (not continuous and e == E - 1 and t == 4) for e in range(E)])
        buf.outcome(rewards[live], dones[live], env_ids=live)
        if continuous and t == 4:
            buf.truncate(f[:1], ms[:1], env_ids=np.array([0]))
        if not continuous:
            live = live[~dones[live]]
    f, ms, _ = varied(rng, E)
    if continuous:
        need = buf.rows.needs_bootstrap()
        buf.bootstrap(f[need], ms[need], env_ids=need)
    else:
        buf.bootstrap(f, ms)
    return f, ms


def new_buffer(world, tmp, continuous, E, T, ppo=None):
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    m = make_pair(tmp)[1] if ppo is None else ppo
    return m, (ContinuousRolloutBuffer if continuous else RolloutBuffer)(world["vae"], m, E, T)


def run_update(buf, **kw):
    np.random.seed(SEED)
    return buf.update(num_epochs=EPOCHS, batch_size=BATCH, **kw)


def as_state(d):
    return np.concatenate([[d["count"]], d["mean"], d["m2"]])


@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("E,T", [(3, 5), (5, 20)])
def test_buffers(world, tmp_path, E, T, continuous):
    import torch
    from rollout import BatchedRolloutStep, normalize_observations
    m1, b1 = new_buffer(world, tmp_path / "w1", continuous, E, T)
    b1.set_observation_normalization(epsilon=EPS)
    s0 = b1.observation_normalization_state()
    assert s0["count"] == 0.0 and not s0["mean"].any() and not s0["m2"].any() and s0["z_dim"] == Z
    assert {k: s0[k] for k in ("clip", "epsilon", "frozen", "normalize_latents")} == dict(clip=10.0, epsilon=EPS, frozen=False, normalize_latents=True)
    fill(b1, continuous)
    valid = b1.rows.valid_rows()
    raw, normed = b1.raw_states.clone(), b1.states.cpu().numpy()
    # the first collection runs on fresh statistics: mean 0 and inv_std = float32(1 / sqrt(1 + epsilon)) for every column, and the clamp
    assert ulp_close(normed[valid], normalize_observations(raw.cpu().numpy()[valid], s0))
    assert np.all(np.abs(normed[valid]) <= np.abs(raw.cpu().numpy()[valid])) and np.abs(normed[valid][:, -1]).max() == 10.0
    times = {}
    out1 = run_update(b1, stage_times=times)
    assert set(times) == {"finish", "logp_old", "sgd", "observation_stats"} and times["observation_stats"] > 0
    # the twin: the setting off, the tables and rewards of the first buffer
    m2, b2 = new_buffer(world, tmp_path / "w2", continuous, E, T)
    fill(b2, continuous)
    for mine, theirs in zip([b2.states, b2.actions, b2.values] + ([b2.final_values] if continuous else []),
                            [b1.states, b1.actions, b1.values] + ([b1.final_values] if continuous else [])):
        mine.copy_(theirs)
    b2.rows.rewards[:] = b1.rows.rewards
    out2 = run_update(b2)
    assert set(out1) == set(out2) | ON_KEYS and b2.raw_states is None
    assert same_update(out1, out2) and bitwise(flat_state(m1), flat_state(m2))
    assert bitwise([b1.returns, b1.advantages, b1.logp_old], [b2.returns, b2.advantages, b2.logp_old])
    # the merge: numpy over raw_states[valid]; the raw table itself is untouched by the update
    assert torch.equal(raw, b1.raw_states)
    x = raw.cpu().numpy()[valid]
    s1 = b1.observation_normalization_state()
    check_moments(as_state(s1), x, (E, T, continuous))
    rms = out1["observation_rms"]
    assert rms["count"] == len(valid) == s1["count"] and same_bits(rms["mean"], s1["mean"]) and same_bits(rms["var"], s1["m2"] / s1["count"])
    frac = out1["observation_clip_fraction"]
    assert frac.shape == (DIN,) and same_bits(frac, (np.abs(normed[valid]) == np.float32(10.0)).sum(0) / len(valid))      # counted on the table the normalise kernel wrote
    assert 0 < frac[-1] < 1                                                          # the raw speed (0..30) on fresh statistics
    # the next step normalises with the new statistics
    b1.reset()
    rng = np.random.RandomState(9)
    f, ms, nz = varied(rng, E)
    a_new, v_new, st_new = b1.step(f, ms, greedy=True)
    rows = np.arange(E) * (T + 1)
    got, raw_rows = b1.states.cpu().numpy()[rows], b1.raw_states.cpu().numpy()[rows]
    assert same_bits(raw_rows, st_new.astype(np.float32)) and ulp_close(got, normalize_observations(raw_rows, s1)) and np.abs(got[:, -1]).max() < 10.0
    # an evaluation step loaded with the checkpointed state reproduces the buffer's greedy actions
    ev = BatchedRolloutStep(world["vae"], m1, E)
    ev.set_observation_normalization(s1)
    assert close(ev(f, ms, greedy=True)[:2], (a_new, v_new))
    # merge_observation_statistics() + reset() on the same rows = the update's merge; the state round trip is bitwise
    _, b3 = new_buffer(world, None, continuous, E, T, ppo=m1)
    b3.set_observation_normalization(epsilon=EPS)
    fill(b3, continuous)
    b3.raw_states.copy_(raw)
    rms3 = b3.merge_observation_statistics()
    b3.reset()
    s3 = b3.observation_normalization_state()
    assert same_bits(as_state(s3), as_state(s1)) and same_bits(rms3["mean"], rms["mean"]) and same_bits(rms3["var"], rms["var"]) and rms3["count"] == rms["count"]
    assert bitwise([b3._obs_norm["mean32"], b3._obs_norm["inv32"]], [ev._obs_norm["mean32"], ev._obs_norm["inv32"]])
    _, b4 = new_buffer(world, None, continuous, E, T, ppo=m1)
    b4.load_observation_normalization_state(s1)
    s4 = b4.observation_normalization_state()
    assert same_bits(as_state(s4), as_state(s1)) and all(s4[k] == s1[k] for k in ("z_dim", "clip", "epsilon", "frozen", "normalize_latents"))
    # frozen: the state stays bitwise, the keys are still there
    b4.set_observation_normalization(epsilon=EPS, frozen=True)
    fill(b4, continuous)
    out4 = b4.update(num_epochs=0, batch_size=BATCH)
    assert same_bits(as_state(b4.observation_normalization_state()), as_state(s1)) and out4["observation_rms"]["count"] == s1["count"]
    with pytest.raises(ValueError, match="frozen"):
        b4.merge_observation_statistics()
    # normalize_latents = False: mean 0 / inv 1 for the latent columns
    b4.reset()
    b4.set_observation_normalization(epsilon=EPS, normalize_latents=False)
    assert not b4._obs_norm["mean32"][:Z].any() and bool((b4._obs_norm["inv32"][:Z] == 1.0).all()) and bool((b4._obs_norm["inv32"][Z:] != 1.0).all())
    b4.step(f, ms, greedy=True)
    got4 = b4.states.cpu().numpy()[rows]
    raw4 = b4.raw_states.cpu().numpy()[rows]
    assert same_bits(got4[:, :Z], raw4[:, :Z]) and ulp_close(got4, normalize_observations(raw4, dict(s1, normalize_latents=False)))
    # a second collection, normalised with the merged statistics and a clip it does reach: the clamped counts of the moments pass are those of the table the normalise
    # kernel wrote, under a pair that is neither 0 / 1 nor the same for every column
    b1.reset()
    b1.set_observation_normalization(clip=1.0, epsilon=EPS)
    assert same_bits(as_state(b1.observation_normalization_state()), as_state(s1))    # (new settings keep the statistics)
    fill(b1, continuous, seed=572)
    valid2, normed2 = b1.rows.valid_rows(), b1.states.cpu().numpy()
    assert ulp_close(normed2[valid2], normalize_observations(b1.raw_states.cpu().numpy()[valid2], b1.observation_normalization_state()))
    out6 = b1.update(num_epochs=0, batch_size=BATCH)
    hits = (np.abs(normed2[valid2]) == np.float32(1.0)).sum(0)
    assert same_bits(out6["observation_clip_fraction"], hits / len(valid2)) and hits[Z:].sum() > 0  # (uniform measurements: 42% beyond one sigma)
    assert out6["observation_rms"]["count"] == s1["count"] + len(valid2)
    # off again: the new keys are gone, the table is dropped, the update is the one that never had the setting
    b1.reset()
    b1.set_observation_normalization(None)
    assert b1.raw_states is None and b1._step._obs_norm is None
    fill(b1, continuous)
    times = {}
    out5 = run_update(b1, stage_times=times)
    assert not ON_KEYS & set(out5) and set(out5) == set(out2) and sorted(times) == ["finish", "logp_old", "sgd"]


def test_buffers_refuse_an_observation_that_is_not_finite(world, tmp_path):
    """The merge kernels leave the statistics as they were, and merge_observation_statistics() / update() say so."""
    m, b = new_buffer(world, tmp_path / "w", False, 3, 5)
    b.set_observation_normalization(epsilon=EPS)
    fill(b, False)
    b.merge_observation_statistics()
    before = as_state(b.observation_normalization_state())
    pair = [b._obs_norm["mean32"].clone(), b._obs_norm["inv32"].clone()]
    valid = b.rows.valid_rows()
    kept = b.raw_states[int(valid[2]), DIN - 1].item()
    b.raw_states[int(valid[2]), DIN - 1] = float("nan")
    with pytest.raises(ValueError, match=r"RolloutBuffer\.merge_observation_statistics: a recorded observation is not finite \(column %d of raw_states\)" % (DIN - 1)):
        b.merge_observation_statistics()
    assert same_bits(as_state(b.observation_normalization_state()), before) and bitwise([b._obs_norm["mean32"], b._obs_norm["inv32"]], pair)
    with pytest.raises(ValueError, match=r"RolloutBuffer\.update: a recorded observation is not finite"):
        b.update(num_epochs=0, batch_size=BATCH)
    assert same_bits(as_state(b.observation_normalization_state()), before) and bitwise([b._obs_norm["mean32"], b._obs_norm["inv32"]], pair)
    b.raw_states[int(valid[2]), DIN - 1] = kept                                      # finite again: the same collection merges
    assert b.update(num_epochs=0, batch_size=BATCH)["observation_rms"]["count"] == before[0] + len(valid)
