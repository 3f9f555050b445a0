"""Per-minibatch advantage normalisation on the GPU (mi_ppo_minibatch_advantages, RolloutBuffer.set_minibatch_normalization).

Kernel level (torch tensors and the C ABI only): advantages 0.3 + 2 N(0, 1), a shuffled permutation of the table rows of ragged lanes, (E, T, batch) = (1, 1, 1);
(3, 5, 4) with lengths 5 / 2 / 0 -- the last minibatch is partial --; (3, 5, 64) -- one partial minibatch larger than n --; (5, 70, 64) and (5, 70, 65) -- a minibatch of
one wave, and of one wave and one entry --; (5, 70, 256) and (5, 70, 257) -- n = 350: the thread stride of the block wraps at 257, the partial minibatch holds 94 / 93
--; (70, 3, 32); both ddof.  The reference is tests/test_minibatch_adv_host.py's numpy float64 loop.  Bounds: count exact; mean and std within 1e-12 max|a| (a bound,
not a measurement: at most 512 terms at 2^-53 each leave about 2e-13 relative to the largest term); every table entry within 1 fp32 ulp of
float32((a - mean_dev) / (std_dev + 1e-8)) formed in numpy from the DEVICE's statistics (fp64 subtraction and division are correctly rounded on both sides, as is the
conversion; the ulp allows for a division sequence that is not); the achieved figures are printed before they are asserted.

Buffer level: 3 x 5 and 5 x 12 through the buffers' own recording step, both classes, minibatches of 4 and 7, 2 epochs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rollout_gpu_common import SENTINEL, bitwise, flat_state, inputs, make_pair, make_world  # noqa: E402
from test_minibatch_adv_host import CASES, case_lengths, make_case, reference  # noqa: E402

PAD = 8                                                     # sentinel entries behind the table: a row outside the table that was stored after all would land here


class Device:
    """The device call on numpy inputs.  The table starts as SENTINEL everywhere, the statistics as -1."""

    def __init__(self):
        import torch
        from mi355 import lib as milib
        self.torch, self.L = torch, milib.get()
        self.device = torch.device("cuda:0")

    def run(self, a, perm, batch, E, T, ddof, unnamed=np.nan):
        """-> (table float32 [E (T + 1) + PAD], stats float64 [n_mb, 3]).  unnamed: what every adv_raw entry holds that perm does not name."""
        torch = self.torch
        perm = np.ascontiguousarray(perm, np.int32)
        n = int(perm.shape[0])
        named = np.zeros(E * T, bool)
        ok = perm[(perm >= 0) & (perm < E * (T + 1))]
        ok = ok[ok % (T + 1) != T]
        named[ok // (T + 1) * T + ok % (T + 1)] = True
        a_in = np.where(named, np.asarray(a, np.float64).reshape(-1), unnamed)
        assert np.isfinite(a_in[named]).all()
        a_d = torch.from_numpy(a_in).to(self.device)
        p_d = torch.from_numpy(perm).to(self.device)
        n_stats = int(self.L.mi_ppo_minibatch_advantages_stats_doubles(n, batch))
        assert n_stats == 3 * -(-n // batch)
        table = torch.full((E * (T + 1) + PAD,), SENTINEL, dtype=torch.float32, device=self.device)
        stats = torch.full((n_stats // 3, 3), -1.0, dtype=torch.float64, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.L.mi_ppo_minibatch_advantages(stream, a_d.data_ptr(), p_d.data_ptr(), n, batch, E, T, ddof, table.data_ptr(), stats.data_ptr())
        torch.cuda.synchronize(self.device)
        assert np.array_equal(a_d.cpu().numpy(), a_in, equal_nan=True) and np.array_equal(p_d.cpu().numpy(), perm)      # the inputs are read, never written
        return table.cpu().numpy(), stats.cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    return Device()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def gathered(a, rows, T):
    return np.asarray(a, np.float64)[rows // (T + 1), rows % (T + 1)]


def check_table(a, perm, batch, E, T, table, stats):
    """Every entry a counted row names, against the device's own statistics; every other entry is the sentinel.  -> is the table bitwise the numpy value?"""
    perm = np.asarray(perm, np.int64)
    written = np.zeros(E * (T + 1) + PAD, bool)
    bitwise = True
    for b in range(stats.shape[0]):
        rows = perm[b * batch:(b + 1) * batch]
        rows = rows[(rows >= 0) & (rows < E * (T + 1)) & (rows % (T + 1) != T)]
        want = ((gathered(a, rows, T) - stats[b, 1]) / (stats[b, 2] + 1e-8)).astype(np.float32)
        got = table[rows]
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)), (b, got, want)
        bitwise = bitwise and same_bits(got, want)
        written[rows] = True
    assert np.all(table[~written] == np.float32(SENTINEL))                           # rows that perm does not name, bootstrap slots and the padding survive
    return bitwise


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("E,T,batch,lens", CASES)
def test_against_the_reference(dev, E, T, batch, lens, ddof):
    lens = case_lengths(E, T, lens, 50 + E)
    a, perm = make_case(E, T, lens, 7 * E + T)
    n = perm.shape[0]
    assert n == sum(lens) and ((E, T) != (5, 70) or n == 350)
    want_table, want_stats = reference(a, perm, batch, E, T, ddof)
    table, stats = dev.run(a, perm, batch, E, T, ddof)
    scale = np.abs(a[~np.isnan(a)]).max()
    errs = dict(mean=np.abs(stats[:, 1] - want_stats[:, 1]).max() / scale, std=np.abs(stats[:, 2] - want_stats[:, 2]).max() / scale)
    assert np.array_equal(stats[:, 0], want_stats[:, 0]) and stats[:, 0].sum() == n  # the counts, exact
    assert stats[:, 0].tolist() == [min(batch, n - lo) for lo in range(0, n, batch)]
    bitwise = check_table(a, perm, batch, E, T, table, stats)
    print("\n(E, T, batch) = (%d, %d, %d) ddof %d: |error| / max|a| %s (bound 1e-12); table bitwise float32((a - mean_dev) / (std_dev + 1e-8)): %s"
          % (E, T, batch, ddof, errs, bitwise))
    assert all(v <= 1e-12 for v in errs.values()), errs
    # against the reference's own table: 1 fp32 ulp and the statistics' 1e-12 through the division
    named = ~np.isnan(want_table)
    assert np.allclose(table[:-PAD][named], want_table[named], rtol=2e-7, atol=1e-7)
    # a one-sample minibatch: std 0 with either ddof, the entry exactly 0.0
    for b in np.nonzero(stats[:, 0] == 1)[0]:
        assert stats[b, 2] == 0.0 and table[perm[b * batch]] == 0.0 and stats[b, 1] == gathered(a, perm[b * batch:b * batch + 1].astype(np.int64), T)[0]
    # NaN against finite values in every adv_raw entry that perm does not name: nothing changes, bitwise; and two runs are bitwise equal
    table2, stats2 = dev.run(a, perm, batch, E, T, ddof, unnamed=5.0)
    assert same_bits(table2, table) and same_bits(stats2, stats)
    table3, stats3 = dev.run(a, perm, batch, E, T, ddof)
    assert same_bits(table3, table) and same_bits(stats3, stats)


@pytest.mark.parametrize("ddof", [0, 1])
def test_one_sample_and_equal_minibatches(dev, ddof):
    E, T = 3, 5
    a, perm = make_case(E, T, [5, 2, 0], 11)
    # batch 3 over 7 entries: 3, 3, 1
    table, stats = dev.run(a, perm, 3, E, T, ddof)
    assert stats[:, 0].tolist() == [3.0, 3.0, 1.0] and stats[2, 2] == 0.0 and stats[2, 1] == gathered(a, perm[6:].astype(np.int64), T)[0]
    assert table[perm[6]] == 0.0 and not np.signbit(table[perm[6]]) and np.all(table[perm[:6]] != 0.0)
    # equal advantages whose sums are exact (-2.75 c is a double for every c here, so mean == a): exactly 0.0 everywhere, std exactly 0
    flat = np.where(np.isnan(a), np.nan, -2.75)
    for batch in (3, 4, 64):
        table, stats = dev.run(flat, perm, batch, E, T, ddof)
        assert np.all(stats[:, 1] == -2.75) and np.all(stats[:, 2] == 0.0) and stats[:, 0].sum() == 7
        assert np.all(table[perm] == 0.0) and check_table(flat, perm, batch, E, T, table, stats)
    # a drawn value: minibatches of 4 = a power of two add it pairwise without rounding, the partial one of 3 need not (its mean is whatever 3 a / 3 rounds to)
    drawn = np.where(np.isnan(a), np.nan, a[0, 0])
    table, stats = dev.run(drawn, perm, 4, E, T, ddof)
    assert stats[0, 1] == a[0, 0] and stats[0, 2] == 0.0 and np.all(table[perm[:4]] == 0.0)
    check_table(drawn, perm, 4, E, T, table, stats)
    # one minibatch equal, the others not: only its entries are 0.0
    mixed = a.copy()
    rows = perm[4:].astype(np.int64)
    mixed[rows // (T + 1), rows % (T + 1)] = 1.5
    table, stats = dev.run(mixed, perm, 4, E, T, ddof)
    assert stats[1].tolist() == [3.0, 1.5, 0.0] and np.all(table[perm[4:]] == 0.0) and np.all(table[perm[:4]] != 0.0) and stats[0, 2] > 0.0


@pytest.mark.parametrize("E,T,batch,lens", [(3, 5, 4, [5, 2, 0]), (5, 70, 64, [70] * 5)])
def test_entries_that_name_no_step_slot(dev, E, T, batch, lens):
    """One planted bootstrap slot (slot T) and one row outside the table lower their minibatches' counts and write nothing; a negative row likewise."""
    a, perm = make_case(E, T, lens, 23)
    n = perm.shape[0]
    planted = perm.copy()
    boot, outside = 0 * (T + 1) + T, E * (T + 1) + 2                                 # lane 0's bootstrap slot; a row in the sentinel padding behind the table
    planted[1], planted[batch + 1] = boot, outside                                   # the first and the second minibatch
    table, stats = dev.run(a, planted, batch, E, T, 0)
    full = [min(batch, n - lo) for lo in range(0, n, batch)]
    assert stats[:, 0].tolist() == [full[0] - 1, full[1] - 1] + full[2:]
    check_table(a, planted, batch, E, T, table, stats)                               # (the sentinel at `boot`, at `outside` and at the two displaced rows survives)
    assert table[boot] == table[outside] == table[perm[1]] == table[perm[batch + 1]] == np.float32(SENTINEL)
    want_table, want_stats = reference(a, planted, batch, E, T, 0)
    assert np.array_equal(stats[:, 0], want_stats[:, 0]) and np.abs(stats[:, 1:] - want_stats[:, 1:]).max() <= 1e-12 * np.abs(a[~np.isnan(a)]).max()
    # the later minibatches do not depend on the planted entries
    clean = dev.run(a, perm, batch, E, T, 0)
    assert same_bits(stats[2:], clean[1][2:])
    negative = perm.copy()
    negative[0] = -1
    t3, s3 = dev.run(a, negative, batch, E, T, 0)
    assert s3[0, 0] == full[0] - 1 and t3[perm[0]] == np.float32(SENTINEL)
    check_table(a, negative, batch, E, T, t3, s3)
    # a minibatch without a counted entry: {0, 0, 0}, nothing stored
    none = np.array([boot, outside, -1, boot], np.int32)
    t4, s4 = dev.run(a, none, 4, E, T, 1)
    assert np.array_equal(s4, np.zeros((1, 3))) and np.all(t4 == np.float32(SENTINEL))


# ---- the buffers ----
EPOCHS, SEED = 2, 3
MB_KEYS = {"minibatch_adv_stats", "minibatch_advantages"}
SHAPES = [(3, 5, 4), (5, 12, 7)]                            # (environments, horizon, minibatch)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "minibatch_adv", policy=False)


def fill(buf, continuous, source, seed=571):
    """One collection through the buffer's own step.  RolloutBuffer: lane 2 reports done at its step 4 and stops (length 4).  ContinuousRolloutBuffer: lane 1 reports
    done at its step 3 and goes on, lane 0 is truncated at its step 4.  The device tables are those of the first collection with this key (the recording step's
    split-K layers end in fp32 atomics, so two collections of the same frames can differ in the last bit)."""
    E, T = buf.num_envs, buf.horizon
    rng = np.random.RandomState(seed)
    buf.reset()
    live = np.arange(E)
    for t in range(1, T + 1):
        f, ms, nz = inputs(rng, E)
        buf.step(f[live], ms[live], env_ids=live, noise=nz[live])
        rewards = 1.0 + 2.0 * rng.standard_normal(E)
        dones = np.array([(continuous and e == 1 and t == 3) or (not continuous and e == 2 and t == 4) for e in range(E)])
        buf.outcome(rewards[live], dones[live], env_ids=live)
        if continuous and t == 4:
            buf.truncate(f[:1], ms[:1], env_ids=np.array([0]))
        if not continuous:
            live = live[~dones[live]]
    f, ms, _ = inputs(rng, E)
    if continuous:
        need = buf.rows.needs_bootstrap()
        buf.bootstrap(f[need], ms[need], env_ids=need)
    else:
        buf.bootstrap(f, ms)
    mine = [buf.states, buf.actions, buf.values] + ([buf.final_values] if continuous else [])
    key = (continuous, E, T, seed)
    if key not in source:
        source[key] = [x.clone() for x in mine]
    for x, y in zip(mine, source[key]):
        x.copy_(y)


def new_buffer(world, tmp, continuous, E, T, ppo=None):
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    m = make_pair(tmp)[1] if ppo is None else ppo
    return m, (ContinuousRolloutBuffer if continuous else RolloutBuffer)(world["vae"], m, E, T)


def run_update(buf, batch, diagnostics=False, epochs=EPOCHS, **kw):
    np.random.seed(SEED)
    return (buf.update_with_diagnostics if diagnostics else buf.update)(num_epochs=epochs, batch_size=batch, **kw)


FINISH_KEYS = ("returns", "raw_advantages", "advantages", "values", "bootstrap_values", "lengths")


def same_finish(a, b):
    return a["samples"] == b["samples"] and all(np.array_equal(a[k], b[k], equal_nan=True) for k in FINISH_KEYS)


@pytest.mark.parametrize("E,T,batch", SHAPES)
@pytest.mark.parametrize("continuous", [False, True])
def test_update_is_a_host_loop_on_a_twin(world, tmp_path, continuous, E, T, batch):
    import torch
    source = {}
    m1, b1 = new_buffer(world, tmp_path / "w1", continuous, E, T)
    b1.set_minibatch_normalization()
    fill(b1, continuous, source)
    times = {}
    out1 = run_update(b1, batch, stage_times=times)
    assert set(times) == {"finish", "logp_old", "sgd", "minibatch_norm"} and 0 < times["minibatch_norm"] < times["sgd"]
    # the twin: the same finish (an update of no epochs with the setting off), then per epoch one device pass over the same permutation and PPO._step_rows per minibatch
    m2, b2 = new_buffer(world, tmp_path / "w2", continuous, E, T)
    fill(b2, continuous, source)
    out0 = run_update(b2, batch, epochs=0)
    assert not MB_KEYS & set(out0) and set(out1) == set(out0) | MB_KEYS
    assert same_finish(out1, out0)                                                   # returns, raw_advantages, advantages, values: those of the setting off
    assert bitwise([b1.returns, b1.advantages], [b2.returns, b2.advantages])
    L, device = b2.L, b2.device
    raw = torch.from_numpy(out0["raw_advantages"]).to(device)
    valid = b2.rows.valid_rows()
    n = int(valid.shape[0])
    n_mb = -(-n // batch)
    assert n == out0["samples"] and n % batch != 0 and n_mb > 1                      # more than one minibatch, the last one partial
    table = torch.full((b2.n_table_rows,), SENTINEL, dtype=torch.float32, device=device)
    stats = torch.zeros(EPOCHS, n_mb, 3, dtype=torch.float64, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    records = []
    np.random.seed(SEED)
    for epoch in range(EPOCHS):
        indices = np.arange(n)
        np.random.shuffle(indices)
        perm = torch.from_numpy(valid[indices]).to(device)
        L.mi_ppo_minibatch_advantages(stream, raw.data_ptr(), perm.data_ptr(), n, batch, E, T, 0, table.data_ptr(), stats[epoch].data_ptr())
        for i in range(0, n, batch):
            mb = perm[i:i + batch]
            k = int(mb.numel())
            m2._step_rows(b2.states, b2.actions, b2.returns, table, b2.logp_old, mb, k, k)
            m2.train_step_counter += 1
            records.append(m2.dev.losses.clone())
    assert bitwise(flat_state(m1), flat_state(m2))                                   # parameters, Adam slots, theta_old
    losses = torch.stack(records).cpu().numpy()
    keys = ("policy_loss", "value_loss", "entropy_loss", "loss", "prob_ratio")
    assert out1["losses"] == [dict(zip(keys, (float(x) for x in row))) for row in losses] and len(out1["losses"]) == EPOCHS * n_mb
    got = out1["minibatch_adv_stats"]
    assert got.dtype == np.float64 and got.shape == (EPOCHS * n_mb, 3) and same_bits(got, stats.cpu().numpy().reshape(-1, 3))
    assert got[:, 0].tolist() == ([float(batch)] * (n_mb - 1) + [float(n - batch * (n_mb - 1))]) * EPOCHS
    # ... and against the numpy reference on the raw advantages the update returned (the second epoch's permutation)
    want_table, want_stats = reference(out0["raw_advantages"], perm.cpu().numpy(), batch, E, T, 0)
    scale = np.nanmax(np.abs(out0["raw_advantages"]))
    assert np.abs(got[n_mb:, 1:] - want_stats[:, 1:]).max() <= 1e-12 * scale
    # the table of the last epoch, as the result shows it
    mba = out1["minibatch_advantages"]
    recorded = np.arange(T)[None, :] < out1["lengths"][:, None]
    assert mba.dtype == np.float32 and mba.shape == (E, T) and np.all(np.isnan(mba[~recorded]))
    tab = table.view(E, T + 1)[:, :T].cpu().numpy()
    assert same_bits(mba[recorded], tab[recorded]) and np.all(tab[recorded] != np.float32(SENTINEL))
    assert np.allclose(mba[recorded], want_table.reshape(E, T + 1)[:, :T][recorded], rtol=2e-7, atol=1e-7)
    assert not np.array_equal(mba[recorded], out1["advantages"][recorded].astype(np.float32))      # `advantages` is the finish call's: the steps did not read it
    # no epoch: no pass, all NaN, no statistics
    m3, b3 = new_buffer(world, None, continuous, E, T, ppo=m2)
    b3.set_minibatch_normalization(1)
    fill(b3, continuous, source)
    out3 = run_update(b3, batch, epochs=0)
    assert out3["minibatch_adv_stats"].shape == (0, 3) and np.all(np.isnan(out3["minibatch_advantages"])) and out3["minibatch_advantages"].shape == (E, T)


@pytest.mark.parametrize("continuous", [False, True])
def test_setting_off_again_is_the_buffer_that_never_had_it(world, tmp_path, continuous):
    E, T, batch = SHAPES[0]
    source = {}
    m0, b0 = new_buffer(world, tmp_path / "w0", continuous, E, T)
    fill(b0, continuous, source)
    times0 = {}
    out0 = run_update(b0, batch, stage_times=times0)
    m1, b1 = new_buffer(world, tmp_path / "w1", continuous, E, T)
    b1.set_minibatch_normalization(1)
    fill(b1, continuous, source)
    on = run_update(b1, batch, epochs=1)                                             # the table exists ...
    assert MB_KEYS <= set(on) and b1._minibatch_advantages is not None
    b1.set_minibatch_normalization(None)
    assert b1._minibatch_norm is None and b1._minibatch_advantages is None           # ... and is dropped
    m2, b2 = new_buffer(world, tmp_path / "w2", continuous, E, T)
    b2.set_minibatch_normalization()
    b2.set_minibatch_normalization(None)
    fill(b2, continuous, source)
    times2 = {}
    out2 = run_update(b2, batch, stage_times=times2)
    assert set(out2) == set(out0) and not MB_KEYS & set(out2) and sorted(times2) == sorted(times0) == ["finish", "logp_old", "sgd"]
    assert out2["losses"] == out0["losses"] and same_finish(out2, out0) and bitwise(flat_state(m2), flat_state(m0))
    # the setting changes the steps: the policy that trained on per-minibatch advantages is another one
    m3, b3 = new_buffer(world, tmp_path / "w3", continuous, E, T)
    b3.set_minibatch_normalization()
    fill(b3, continuous, source)
    out3 = run_update(b3, batch)
    assert same_finish(out3, out0) and out3["losses"] != out0["losses"] and not bitwise(flat_state(m3), flat_state(m0))


@pytest.mark.parametrize("continuous", [False, True])
def test_together_with_the_other_settings(world, tmp_path, continuous):
    """Value clipping, gradient clipping and reward scaling on as well: it runs, the other settings' keys are there, and two such runs are bitwise equal."""
    E, T, batch = SHAPES[1]
    source = {}
    runs = []
    for k in range(2):
        m, b = new_buffer(world, tmp_path / ("w%d" % k), continuous, E, T)
        m.set_value_clip(0.2)
        m.set_max_grad_norm(0.5)
        b.set_reward_scaling()
        b.set_minibatch_normalization(1)
        fill(b, continuous, source)
        runs.append((m, run_update(b, batch, diagnostics=True)))
    (m1, out1), (m2, out2) = runs
    n_steps = EPOCHS * -(-out1["samples"] // batch)
    assert out1["minibatch_adv_stats"].shape == (n_steps, 3) and out1["grad_norms"].shape == (n_steps,) and len(out1["losses"]) == n_steps
    assert "return_rms" in out1 and len(out1["epochs"]) == EPOCHS and "value_clip_fraction" in out1["epochs"][0]
    assert all(np.isfinite(x["loss"]) for x in out1["losses"]) and np.isfinite(out1["minibatch_adv_stats"]).all()
    assert bitwise(flat_state(m1), flat_state(m2)) and out1["losses"] == out2["losses"] and out1["epochs"] == out2["epochs"]
    for key in ("minibatch_adv_stats", "minibatch_advantages", "grad_norms", "clip_scales", "scaled_rewards"):
        assert same_bits(out1[key], out2[key]), key
    # the statistics are those of the raw advantages of the SCALED rewards
    recorded = ~np.isnan(out1["raw_advantages"])
    assert np.abs(out1["minibatch_adv_stats"][:, 1]).max() <= np.abs(out1["raw_advantages"][recorded]).max()


@pytest.mark.parametrize("continuous", [False, True])
def test_kl_stop_and_ddof(world, tmp_path, continuous):
    E, T, batch = SHAPES[1]
    source = {}
    m, b = new_buffer(world, tmp_path / "w", continuous, E, T)
    b.set_minibatch_normalization()
    fill(b, continuous, source)
    out = run_update(b, batch, diagnostics=True, epochs=3, target_kl=1e-12)          # any SGD step moves the policy further than that
    n_mb = -(-out["samples"] // batch)
    assert out["stopped_early"] and out["epochs_run"] == 1 and out["epochs"][0]["approx_kl"] > 1e-12
    assert out["minibatch_adv_stats"].shape == (n_mb, 3) and len(out["losses"]) == n_mb          # exactly one epoch's rows
    assert not np.all(np.isnan(out["minibatch_advantages"]))
    # ddof = 1 on the same collection and permutation (the statistics depend on the recorded values, not on the policy's parameters): the same counts and means,
    # std_1 = std_0 sqrt(c / (c - 1))
    _, b1 = new_buffer(world, None, continuous, E, T, ppo=m)
    b1.set_minibatch_normalization(ddof=1)
    fill(b1, continuous, source)
    out1 = run_update(b1, batch, epochs=1)
    s0, s1 = out["minibatch_adv_stats"], out1["minibatch_adv_stats"]
    assert same_bits(s0[:, :2], s1[:, :2]) and np.all(s0[:, 0] > 1)
    want = s0[:, 2] * np.sqrt(s0[:, 0] / (s0[:, 0] - 1))
    rel = np.abs(s1[:, 2] - want) / want
    print("\nddof 1 against ddof 0 x sqrt(c / (c - 1)): relative difference at most %.3g" % rel.max())
    assert np.all(rel <= 1e-12)
