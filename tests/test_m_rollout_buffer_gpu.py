"""The device-resident rollout buffer (rollout.RolloutBuffer: mi_rollout_step_batch_rec records state / action / value of every environment into the tables
mi_ppo_train_step_idx gathers from, mi_rollout_finish turns the ragged rows into returns and normalised advantages, update() trains from the tables) against
what the same call returned to the host (bitwise), the dense GAE / normalisation kernels on each row alone (bitwise), the trainer's loop built from existing pieces
and the oracle.  Set-up restated from test_l_rollout_batch_gpu.py (make_pair, vae_params, make_vae, inputs, the per-row oracle); tolerances are that file's for
the step (1e-5 between device paths, check_against_oracle against the oracle) and test_e_c5_replay_gpu.py's for the update's losses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ppo_oracle as po  # noqa: E402
from rollout_gpu_common import (SENTINEL, Oracle, check_against_oracle, check_losses, check_recorded, close, fill_tables, inputs, make_pair, make_world,  # noqa: E402
                                rel_err, tables)

K, A = 3, 2


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "rollout_buffer")


def test_recording_is_exact_and_confined(world):
    """E in {1, 5, 33, 64} x io pinned / device x sampled / greedy with permuted env_ids, and at the C level table rows of -1 and far outside the tables."""
    from rollout import BatchedRolloutStep, RolloutBuffer
    rng = np.random.RandomState(51)
    frames, meas, noise = inputs(rng, 64)
    z_all = world["orc"].latents(frames)
    T = 3
    for io in ("pinned", "device"):
        for E in (1, 5, 33, 64):
            buf = RolloutBuffer(world["vae"], world["m"], E, T, io=io)
            plain = BatchedRolloutStep(world["vae"], world["m"], E, io=io)
            buf.reset()
            fill_tables(buf)
            lo = 64 - E if io == "device" else 0
            f, ms, nz, z_o = frames[lo:lo + E], meas[lo:lo + E], noise[lo:lo + E], z_all[lo:lo + E]
            for slot, greedy in enumerate((False, True)):
                perm = rng.permutation(E)
                before = tables(buf)
                got = buf.step(f, ms, env_ids=perm, greedy=greedy, noise=nz)
                rows = perm * (T + 1) + slot
                check_recorded(tables(buf), before, rows, got, ms, (io, E, greedy))
                assert close(got, plain(f, ms, greedy=greedy, noise=nz)), (io, E, greedy)
                a_o, v_o, _ = world["orc"].predict(z_o, ms, nz, greedy)
                check_against_oracle(got, z_o, a_o, v_o, ms, (io, E, greedy))
                buf.outcome(np.zeros(E), np.zeros(E, bool), env_ids=perm)
            assert buf.lengths.tolist() == [2] * E
            # the C level: -1 and rows far outside the tables are skipped, whatever their value; the others are recorded; the host output is complete either way
            n_rows = buf.n_table_rows
            trows = (rng.permutation(E) * (T + 1) + 2).astype(np.int32)
            skip = np.zeros(E, bool)
            skip[::3] = True
            trows[skip] = np.resize(np.array([-1, n_rows, 2 ** 31 - 1, -2 ** 31, -5, n_rows + 7], np.int64), int(skip.sum())).astype(np.int32)
            before = tables(buf)
            st = buf._step
            ff, n, mm, nn = st.check(f, ms, False, nz)
            got = st.record(ff, n, mm, nn, False, trows, buf.states, buf.actions, buf.values)
            keep = ~skip
            check_recorded(tables(buf), before, trows[keep], tuple(x[keep] for x in got), ms[keep], (io, E, "C level"))
            assert close(got, plain(f, ms, noise=nz)), (io, E, "C level")
            # the tables that no recording call writes
            assert bool((buf.returns == SENTINEL).all()) and bool((buf.advantages == SENTINEL).all()) and bool((buf.logp_old == SENTINEL).all())


def test_missing_tables_and_bad_calls_are_refused(world):
    import torch
    from mi355 import lib as milib
    from rollout import RolloutBuffer
    rng = np.random.RandomState(52)
    frames, meas, noise = inputs(rng, 5)
    buf = RolloutBuffer(world["vae"], world["m"], 4, 2)
    fill_tables(buf)
    buf._step.h_out.fill_(SENTINEL)
    for bad in (lambda: buf.step(frames, meas),                                       # n > num_envs
                lambda: buf.step(frames[:4].astype(np.float32), meas[:4]),             # float frames
                lambda: buf.step(frames[:4], meas[:4, :2]),                            # wrong measurement shape
                lambda: buf.step(frames[:4], meas[:4], noise=noise[:4, :1]),           # wrong noise shape
                lambda: buf.step(frames[:2], meas[:2], env_ids=[1, 1]),                # duplicate
                lambda: buf.step(frames[:2], meas[:2], env_ids=[1, 4]),                # out of range
                lambda: buf.outcome([0.0], [False], env_ids=[0]),                      # no recorded step
                lambda: buf.bootstrap(frames[:1], meas[:1], env_ids=[0]),              # empty row
                lambda: buf.update()):                                                 # no samples
        with pytest.raises(ValueError):
            bad()
    assert not buf.rows.awaiting.any()                                                # a refused call leaves the book-keeping alone
    L, st = milib.get(), torch.cuda.current_stream().cuda_stream
    s = buf._step
    base = s.h_in.data_ptr()
    fptr = base + s._f_off

    def raw(n=4, rows=fptr + 4 * 4 * (K + A), n_rows=buf.n_table_rows, states=buf.states.data_ptr(), actions=buf.actions.data_ptr(), values=buf.values.data_ptr()):
        return L.cdll.mi_rollout_step_batch_rec(world["vae"].dev.handle, world["m"].dev.handle, st, base, fptr, K, None, 1, n, s.scratch.data_ptr(), s.scratch_bytes,
                                                s.h_out.data_ptr(), rows, n_rows, states, actions, values)
    for kw in (dict(rows=None), dict(states=None), dict(actions=None), dict(values=None), dict(n_rows=0)):
        assert raw(**kw) == -1 and b"missing tables" in L.cdll.mi_last_error(), kw
    assert raw(n=0) == -1 and raw(n=1025) == -1
    torch.cuda.synchronize()
    assert np.all(s.h_out.numpy() == SENTINEL) and bool((buf.states == SENTINEL).all())  # nothing was launched by any of the refused calls
    with pytest.raises(ValueError):
        RolloutBuffer(world["vae"], world["m"], 0, 4)
    with pytest.raises(ValueError):
        RolloutBuffer(world["vae"], world["m"], 4, 0)


@pytest.mark.parametrize("T", [4, 128, 1024])
def test_finish_kernel_matches_the_dense_kernels_row_by_row(T):
    """Every row of a ragged buffer comes out of mi_rollout_finish bit for bit as mi_gae_scan + mi_adv_normalize give it on that row alone."""
    import torch
    import utils
    from mi355 import lib as milib
    L = milib.get()
    gamma, lam = 0.99, 0.95
    rng = np.random.RandomState(60 + T)
    lengths = np.array([x for x in (1, 2, 63, 64, 65, T, 0, T - 1, 3, 0, T, 1) if x <= T], np.int32)
    E = len(lengths)
    values = rng.standard_normal((E, T + 1)).astype(np.float32)
    rewards = rng.uniform(-1, 1, (E, T))
    dones = np.zeros((E, T))
    for e in range(0, E, 2):                                                         # one terminal at the end of every other row
        if lengths[e] > 0:
            dones[e, lengths[e] - 1] = 1.0
    dev = "cuda"
    v_d, r_d, d_d, l_d = (torch.from_numpy(x).to(dev) for x in (values.reshape(-1), rewards, dones, lengths))
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(2):
        ret32, adv32 = torch.full((E * (T + 1),), SENTINEL, device=dev), torch.full((E * (T + 1),), SENTINEL, device=dev)
        f64 = torch.full((3, E, T), SENTINEL, dtype=torch.float64, device=dev)
        L.mi_rollout_finish(st, v_d.data_ptr(), r_d.data_ptr(), d_d.data_ptr(), l_d.data_ptr(), E, T, gamma, lam, ret32.data_ptr(), adv32.data_ptr(),
                            f64[0].data_ptr(), f64[1].data_ptr(), f64[2].data_ptr())
        runs.append((ret32.cpu().numpy().reshape(E, T + 1), adv32.cpu().numpy().reshape(E, T + 1), f64.cpu().numpy()))
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(x, y)                                                  # two runs are bitwise equal
    ret32, adv32, (raw, ret, advn) = runs[0]
    for e in range(E):
        n = int(lengths[e])
        for arr in (raw[e], ret[e], advn[e], ret32[e], adv32[e]):
            assert np.all(arr[n:] == SENTINEL), (T, e, n)                            # slots beyond the row, and empty rows, are not written
        if n == 0:
            continue
        want_raw, want_ret, want_adv = utils.compute_gae_batched(rewards[e, :n][None], values[e, :n + 1][None], dones[e, :n][None], gamma, lam, normalize=True)
        assert np.array_equal(raw[e, :n], want_raw[0]), (T, e, n)
        assert np.array_equal(ret[e, :n], want_ret[0]), (T, e, n)
        assert np.array_equal(advn[e, :n], want_adv[0]), (T, e, n)
        assert np.array_equal(ret32[e, :n], want_ret[0].astype(np.float32)) and np.array_equal(adv32[e, :n], want_adv[0].astype(np.float32)), (T, e, n)
        if n == 1:
            assert advn[e, 0] == 0.0                                                 # std 0: (A - mean) / (0 + 1e-8) = 0
    # without the optional fp64 outputs the tables come out the same
    ret_b, adv_b = torch.full((E * (T + 1),), SENTINEL, device=dev), torch.full((E * (T + 1),), SENTINEL, device=dev)
    L.mi_rollout_finish(st, v_d.data_ptr(), r_d.data_ptr(), d_d.data_ptr(), l_d.data_ptr(), E, T, gamma, lam, ret_b.data_ptr(), adv_b.data_ptr(), None, None, None)
    assert np.array_equal(ret_b.cpu().numpy().reshape(E, T + 1), ret32) and np.array_equal(adv_b.cpu().numpy().reshape(E, T + 1), adv32)


def collect(buf, rng, done_at, noise_rng=None, frames_per_step=None):
    """A ragged collection: environment e reports done at its step done_at[e] (1-based), the others run to the horizon.  Returns the valid-row list."""
    E, T = buf.num_envs, buf.horizon
    buf.reset()
    live = np.arange(E)
    t = 0
    while len(live):
        f, ms, nz = inputs(rng, len(live))
        buf.step(f, ms, env_ids=live, noise=nz)
        dones = np.array([done_at.get(int(e)) == t + 1 for e in live])
        buf.outcome(rng.uniform(0, 1, len(live)), dones, env_ids=live)
        t += 1
        live = live[~dones & (buf.lengths[live] < T)]
    f, ms, _ = inputs(rng, E)
    buf.bootstrap(f, ms)
    return buf.rows.valid_rows()


def host_samples(buf, valid, gamma, lam):
    """The trainer's own statements on the tables read back: per row compute_gae + normalize_advantages, samples concatenated in the valid-row order."""
    import utils
    E, T = buf.num_envs, buf.horizon
    s, a, v = tables(buf)
    v = v.reshape(E, T + 1)
    rets, advs = [], []
    for e in range(E):
        n = int(buf.lengths[e])
        if n == 0:
            continue
        adv = utils.compute_gae(buf.rows.rewards[e, :n], v[e, :n], v[e, n], buf.rows.dones[e, :n], gamma, lam)
        ret, advn = utils.normalize_advantages(adv, v[e, :n])
        rets.append(ret)
        advs.append(advn)
    return s[valid], a[valid], np.concatenate(rets), np.concatenate(advs)


# Parameters after the update, route A (the buffer: cached log pi_old, gather inside the kernels) against route B (PPO.train_step per minibatch: in-step old-policy
# forward, rows gathered on the host), largest |difference| of a tensor relative to the tensor's max.  MEASURED on one MI355X: 5.223e-07 (policy/dense/bias; the
# value net's tensors came out bitwise equal: log pi_old does not enter their gradients); asserted with a factor of 4 as the margin for other boxes and library
# builds.  Both routes read the same tables, so the collection's fp32 atomics do not enter.
PARAM_REL_MEASURED = 5.223e-07


def test_update_matches_the_trainers_loop_and_the_oracle(world, tmp_path):
    from rollout import RolloutBuffer
    gamma, lam, seed, epochs, batch = 0.99, 0.95, 5, 3, 32
    E, T = 8, 16
    o, m_a = make_pair(tmp_path / "a")
    _, m_b = make_pair(tmp_path / "b")
    buf = RolloutBuffer(world["vae"], m_a, E, T)
    valid = collect(buf, np.random.RandomState(71), {2: 5, 6: 11})
    assert buf.lengths.tolist() == [16, 16, 5, 16, 16, 16, 11, 16] and len(valid) == 112
    s, a, ret, adv = host_samples(buf, valid, gamma, lam)
    # route A
    np.random.seed(seed)
    times = {}
    out = buf.update(gamma, lam, num_epochs=epochs, batch_size=batch, stage_times=times)
    n_steps = epochs * -(-len(valid) // batch)
    assert len(out["losses"]) == n_steps and out["samples"] == len(valid) and out["lengths"].tolist() == buf.lengths.tolist()
    assert sorted(times) == ["finish", "logp_old", "sgd"]
    # its returns / advantages are the host statements', bit for bit (same kernels' operation sequences), NaN beyond a row
    k = 0
    for e in range(E):
        n = int(buf.lengths[e])
        assert np.array_equal(out["returns"][e, :n], ret[k:k + n]) and np.array_equal(out["advantages"][e, :n], adv[k:k + n]), e
        assert np.isnan(out["returns"][e, n:]).all() and np.isnan(out["advantages"][e, n:]).all() and np.isnan(out["values"][e, n:]).all(), e
        assert out["values"].dtype == np.float32 and not np.isnan(out["values"][e, :n]).any()
        k += n
    assert np.array_equal(buf.returns.cpu().numpy()[valid], ret.astype(np.float32)) and np.array_equal(buf.advantages.cpu().numpy()[valid], adv.astype(np.float32))
    # route B: the loop of train.py:193-207 on a second model with the same weights
    m_b.update_old_policy()
    np.random.seed(seed)
    logs_b = [m_b.train_step(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    # route O: the oracle fed the same
    o.update_old_policy()
    np.random.seed(seed)
    logs_o = [o.train(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    check_losses(out["losses"], logs_o, "A against O")
    check_losses(out["losses"], logs_b, "A against B")
    assert out["losses"][0]["prob_ratio"] == pytest.approx(1.0, abs=1e-5)             # theta_old == theta at the first step
    assert m_a.get_train_step_idx() == m_b.get_train_step_idx() == n_steps
    pa, pb = m_a.dev.export_params(), m_b.dev.export_params()
    worst = max(rel_err(pa[name], pb[name]) for name in pa)
    print("\nparameters after the update, buffer against PPO.train_step loop: max |diff| / tensor max = %.3e" % worst)
    for name in pa:
        print("  %-34s %.3e" % (name, rel_err(pa[name], pb[name])))
    assert worst <= 4 * PARAM_REL_MEASURED, worst


def test_second_collection_after_reset_matches_a_fresh_buffer(world, tmp_path):
    """No state leaks from one collect -> update cycle into the next: the same second cycle on a fresh buffer gives the same losses.  (The two models reach the
    second cycle through their own first cycles, whose collections end in fp32 atomics: the comparison is at the update tolerances, not bitwise.)"""
    from rollout import RolloutBuffer
    E, T = 6, 8
    _, m1 = make_pair(tmp_path / "m1", learning_rate=1e-3)
    _, m2 = make_pair(tmp_path / "m2", learning_rate=1e-3)
    used, first = RolloutBuffer(world["vae"], m1, E, T, seed=3), RolloutBuffer(world["vae"], m2, E, T, seed=3)
    outs = []
    for buf, m in ((used, m1), (first, m2)):
        collect(buf, np.random.RandomState(81), {})                                   # cycle 1: every row full
        np.random.seed(9)
        buf.update(num_epochs=1, batch_size=16)
        if buf is first:
            buf = RolloutBuffer(world["vae"], m, E, T, seed=3)                        # cycle 2 on a buffer that has seen nothing
        valid = collect(buf, np.random.RandomState(82), {0: 2, 3: 5, 4: 1})           # shorter rows: stale slots of cycle 1 lie behind them
        assert buf.lengths.tolist() == [2, 8, 8, 5, 1, 8]
        np.random.seed(10)
        outs.append((buf.update(num_epochs=2, batch_size=16), valid))
    (a, va), (b, vb) = outs
    assert np.array_equal(va, vb) and a["lengths"].tolist() == b["lengths"].tolist() and a["samples"] == b["samples"] == 32
    check_losses(a["losses"], b["losses"], "reused against fresh")
    assert np.array_equal(np.isnan(a["returns"]), np.isnan(b["returns"]))
    assert np.allclose(np.nan_to_num(a["returns"]), np.nan_to_num(b["returns"]), rtol=1e-4, atol=1e-4)


def test_other_steps_are_undisturbed_and_the_engine_may_grow(world, tmp_path):
    from rollout import BatchedRolloutStep, RolloutBuffer, RolloutStep
    rng = np.random.RandomState(91)
    o, m = make_pair(tmp_path / "grow", learning_rate=1e-2)
    orc = Oracle(world["vparams"], o)
    E, T = 20, 16
    frames, meas, noise = inputs(rng, E)
    one, many = RolloutStep(world["vae"], m), BatchedRolloutStep(world["vae"], m, E)
    buf = RolloutBuffer(world["vae"], m, E, T)
    before_many, before_one = many(frames, meas, noise=noise), one(frames[3], meas[3], noise=noise[3])
    buf.reset()
    got = buf.step(frames, meas, noise=noise)
    assert close(got, before_many)
    assert close(many(frames, meas, noise=noise), before_many) and close(one(frames[3], meas[3], noise=noise[3]), before_one)
    buf.outcome(np.ones(E), np.zeros(E, bool))
    assert close(many(frames, meas, noise=noise), before_many)
    # a full collection and an update whose minibatch is larger than the engine's max_batch: the engine is recreated inside the update
    assert m.dev.max_batch == 256
    collect(buf, np.random.RandomState(92), {1: 3})
    np.random.seed(4)
    out = buf.update(num_epochs=1, batch_size=300)
    assert m.dev.max_batch >= 300 and len(out["losses"]) == 2 and out["samples"] == 19 * 16 + 3
    for k, val in m.dev.export_params().items():
        o.params[k] = np.array(val, np.float32)
    buf.reset()
    z_o = orc.latents(frames)
    a_o, v_o, _ = orc.predict(z_o, meas, noise, False)
    got = buf.step(frames, meas, noise=noise)                                         # the step reads the new engine's handle
    check_against_oracle(got, z_o, a_o, v_o, meas, "after growth")
    assert np.abs(got[0] - before_many[0]).max() > 1e-4                               # the update moved the policy
    s, a, v = tables(buf)
    check_recorded((s, a, v), (s, a, v), np.arange(E) * (T + 1), got, meas, "after growth")


def test_bf16x3_update_matches_the_oracle(world, tmp_path):
    from rollout import RolloutBuffer
    gamma, lam, seed, epochs, batch = 0.99, 0.95, 6, 3, 32
    o, m = make_pair(tmp_path / "x3", precision="bf16x3")
    assert m.precision == "bf16x3"
    buf = RolloutBuffer(world["vae"], m, 8, 16)
    valid = collect(buf, np.random.RandomState(72), {0: 7, 5: 2})
    s, a, ret, adv = host_samples(buf, valid, gamma, lam)
    np.random.seed(seed)
    out = buf.update(gamma, lam, num_epochs=epochs, batch_size=batch)
    o.update_old_policy()
    np.random.seed(seed)
    logs_o = [o.train(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    check_losses(out["losses"], logs_o, "bf16x3 against O")
    assert out["losses"][0]["prob_ratio"] == pytest.approx(1.0, abs=1e-5)
