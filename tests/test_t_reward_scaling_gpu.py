"""Running-return reward scaling on the GPU (mi_rollout_scale_rewards, RolloutBuffer.set_reward_scaling).

Kernel level (torch tensors and the C ABI only): (E, T) = (1, 1), (3, 5), (5, 70) -- the lane stride of the sums wraps past 64 -- and (70, 3) -- the one-wave reduction
over the lanes wraps --, ragged lengths that include 0 and T, terminals in the middle of a lane and at a last step, truncs NULL and given (one truncated last step), a
non-zero starting carry and non-zero starting statistics, gamma = 0.99.  The reference is tests/test_reward_scaling_host.py's numpy float64 loop.  Bounds: the
recurrence and the carries bitwise (one multiply and one add per step, no contraction); count exact; mean, M2 / count and den 1e-9 relative, the project's bound on an
ordered fp64 sum against numpy's pairwise one (tests/test_s_value_clip_gpu.py); rewards_out within 1 ulp of np.clip(r / den, -clip, clip) formed from the DEVICE's den
(fp64 division is correctly rounded on both sides; the ulp allows for a division sequence that is not), clamped entries exactly +-clip.  Every case asserts on the
reference itself that var >= 1e-2 mean^2 (no cancellation) and that with clip = 1.5 at least one reward is clamped and one is not; the single reward of (1, 1) can only
be one of the two: it is planned to be clamped, and its clip = inf run is the other side.

Buffer level: 3 environments x 6 steps through the buffers' own recording step, both classes; the continuous one has a done in the middle of lane 1 and one truncate()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rollout_gpu_common import bitwise, flat_state, inputs, make_pair, make_world, same_update  # noqa: E402
from test_reward_scaling_host import reference, rel  # noqa: E402

GAMMA, EPSILON, CLIP = 0.99, 1e-8, 1.5
INF = float("inf")
STATE0 = np.array([40.0, 1.5, 300.0, 0.0])                  # statistics of 40 earlier returns: mean 1.5, variance 7.5
SHAPES = [(1, 1), (3, 5), (5, 70), (70, 3)]


def make_case(E, T, seed, with_truncs):
    """-> (rewards, terminals, truncs or None, len, carry): lane 0 is full, lane 1 (if any) unused, the others ragged; the last recorded step of the last lane is
    terminal, with truncs the last recorded step of lane 0 is truncated; terminals elsewhere with probability 0.15."""
    rng = np.random.RandomState(seed)
    r = 2.0 + 3.0 * rng.standard_normal((E, T))
    r[rng.uniform(size=(E, T)) < 0.1] -= 25.0                                        # a collision penalty an order of magnitude above the other terms
    d = (rng.uniform(size=(E, T)) < 0.15).astype(np.float64)
    lens = rng.randint(1, T + 1, E).astype(np.int32)
    lens[0] = T
    if E > 1:
        lens[1] = 0
    if E > 2:
        lens[2] = min(T, 3)
        d[2, 0], d[2, 1:] = 1.0, 0.0                                                 # a terminal in the middle of a lane for certain
    d[E - 1, max(lens[E - 1], 1) - 1] = 1.0                                          # ... and at a last step
    tr = None
    if with_truncs:
        tr = (rng.uniform(size=(E, T)) < 0.1) & (d == 0)
        if E > 1:
            d[0, T - 1] = 0.0
            tr[0, T - 1] = True                                                      # a truncated last step
    carry = 1.0 + rng.standard_normal(E)
    if (E, T) == (1, 1):
        r[0, 0] = 9.0                                                                # 9 / sqrt(7.5 ..) > 1.5: clamped
    return r, d, tr, lens, carry


class Device:
    """The device call on numpy inputs.  Entries of the inputs at t >= len are NaN (truncs: 1), the outputs start as NaN."""

    def __init__(self):
        import torch
        from mi355 import lib as milib
        self.torch, self.L = torch, milib.get()
        self.device = torch.device("cuda:0")

    def up(self, x, dtype=None):
        t = self.torch.from_numpy(np.ascontiguousarray(x))
        return (t if dtype is None else t.to(dtype)).to(self.device)

    def run(self, r, d, tr, lens, carry, state, clip=CLIP, merge=1, gamma=GAMMA, epsilon=EPSILON, plant=True):
        torch = self.torch
        E, T = r.shape
        beyond = np.arange(T)[None, :] >= np.minimum(lens, T)[:, None]
        r_in, d_in = r.copy(), d.copy()
        tr_in = None if tr is None else tr.astype(np.uint8)
        if plant:
            r_in[beyond], d_in[beyond] = np.nan, np.nan
            if tr_in is not None:
                tr_in[beyond] = 1
        r_d, d_d, ln = self.up(r_in), self.up(d_in), self.up(lens.astype(np.int32))
        tr_d = None if tr_in is None else self.up(tr_in)
        st, ca = self.up(np.asarray(state, np.float64)), self.up(np.asarray(carry, np.float64))
        n_scratch = int(self.L.mi_rollout_scale_rewards_scratch_doubles(E))
        assert n_scratch == 2 * E + 2
        scratch = torch.full((n_scratch,), -1.0, dtype=torch.float64, device=self.device)
        out = torch.full((2, E, T), float("nan"), dtype=torch.float64, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.L.mi_rollout_scale_rewards(stream, r_d.data_ptr(), d_d.data_ptr(), None if tr_d is None else tr_d.data_ptr(), ln.data_ptr(), E, T, gamma, epsilon, clip,
                                        merge, st.data_ptr(), ca.data_ptr(), scratch.data_ptr(), out[0].data_ptr(), out[1].data_ptr())
        torch.cuda.synchronize(self.device)
        assert torch.equal(r_d.isnan(), self.up(beyond)) if plant else True           # the inputs are read, never written
        o = out.cpu().numpy()
        return o[0], o[1], st.cpu().numpy(), ca.cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    return Device()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_planned(r, lens, want_out, want_state):
    """The case's own conditions, on the reference: no cancellation, and the clamp both bites and does not."""
    T = r.shape[1]
    rec = np.arange(T)[None, :] < np.minimum(lens, T)[:, None]
    count, mean, m2, den = want_state
    assert m2 / count >= 1e-2 * mean * mean, want_state
    clamped = np.abs(want_out[rec]) == CLIP
    if rec.sum() > 1:
        assert clamped.any() and (~clamped).any(), clamped
    else:
        assert clamped.all()
    return rec


@pytest.mark.parametrize("with_truncs", [False, True])
@pytest.mark.parametrize("E,T", SHAPES)
def test_against_the_reference(dev, E, T, with_truncs):
    r, d, tr, lens, carry = make_case(E, T, 100 * E + T, with_truncs)
    G, out, state, c = reference(r, d, tr, lens, GAMMA, EPSILON, CLIP, 1, STATE0, carry)
    rec = check_planned(r, lens, out, state)
    g_dev, out_dev, st_dev, c_dev = dev.run(r, d, tr, lens, carry, STATE0)
    # the recurrence and the carries bit for bit; slots >= len keep the NaN they started with (same_bits compares those too)
    assert same_bits(g_dev, G), np.abs(g_dev - G)[rec].max()
    assert same_bits(c_dev, c)
    assert c_dev[E - 1] == 0.0 and not np.signbit(c_dev[E - 1])                     # behind a terminal last step: exactly 0.0
    if with_truncs and E > 1:
        assert c_dev[0] == 0.0 and not np.signbit(c_dev[0])                          # behind a truncated last step
    elif E > 1 and d[0, T - 1] == 0:
        assert c_dev[0] == G[0, T - 1] != 0.0
    if E > 1:
        assert same_bits(c_dev[1], carry[1]) and carry[1] != 0.0                     # an unused lane keeps its carry
    # the moments
    assert st_dev[0] == state[0] == STATE0[0] + rec.sum()
    errs = dict(mean=rel(st_dev[1], state[1]), var=rel(st_dev[2] / st_dev[0], state[2] / state[0]), den=rel(st_dev[3], state[3]))
    # the scaled rewards, from the device's own den
    want = np.clip(r[rec] / st_dev[3], -CLIP, CLIP)
    got = out_dev[rec]
    bitwise = same_bits(got, want)
    print("\n(E, T) = (%d, %d) truncs %s: relative errors %s; rewards_out bitwise np.clip(r / den_device): %s" % (E, T, with_truncs, errs, bitwise))
    assert all(v <= 1e-9 for v in errs.values()), errs
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))), np.abs(got - want).max()
    clamped = np.abs(want) == CLIP
    assert np.array_equal(got[clamped], want[clamped]) and np.all(np.abs(got[clamped]) == CLIP)
    assert np.all(np.isnan(out_dev[~rec])) and np.all(np.isnan(g_dev[~rec]))
    # NaNs planted in the inputs at t >= len change nothing
    again = dev.run(r, d, tr, lens, carry, STATE0, plant=False)
    assert all(same_bits(x, y) for x, y in zip(again, (g_dev, out_dev, st_dev, c_dev)))
    # clip = inf clamps nothing
    g_inf, out_inf, st_inf, c_inf = dev.run(r, d, tr, lens, carry, STATE0, clip=INF)
    assert same_bits(g_inf, g_dev) and same_bits(st_inf, st_dev) and same_bits(c_inf, c_dev)
    want_inf = r[rec] / st_dev[3]
    assert np.all(np.abs(out_inf[rec] - want_inf) <= np.spacing(np.abs(want_inf))) and np.abs(out_inf[rec]).max() > CLIP


def test_three_chained_collections(dev):
    E, T = 5, 70
    state, carry = np.zeros(4), np.zeros(E)                                          # from the zero state: the first call's statistics are the batch's own
    st_dev, c_dev, all_g = state, carry, []
    for k in range(3):
        r, d, tr, lens, _ = make_case(E, T, 900 + k, k != 1)                         # the middle collection has no truncs
        G, _, state, carry = reference(r, d, tr, lens, GAMMA, EPSILON, CLIP, 1, state, carry)
        g_dev, _, st_dev, c_dev = dev.run(r, d, tr, lens, c_dev, st_dev)
        assert same_bits(g_dev, G) and same_bits(c_dev, carry), k
        all_g.append(g_dev[~np.isnan(g_dev)])
        cat = np.concatenate(all_g)
        errs = dict(mean=rel(st_dev[1], state[1]), var=rel(st_dev[2] / st_dev[0], state[2] / state[0]), den=rel(st_dev[3], state[3]),
                    mean_np=rel(st_dev[1], np.mean(cat)), var_np=rel(st_dev[2] / st_dev[0], np.var(cat)))
        print("\ncollection %d: relative errors %s" % (k, errs))
        assert st_dev[0] == state[0] == cat.size
        assert all(v <= 1e-9 for v in errs.values()), (k, errs)


def test_frozen_statistics(dev):
    E, T = 3, 5
    r, d, tr, lens, carry = make_case(E, T, 77, True)
    G, out, state, c = reference(r, d, tr, lens, GAMMA, EPSILON, CLIP, 0, STATE0, carry)
    g_dev, out_dev, st_dev, c_dev = dev.run(r, d, tr, lens, carry, STATE0, merge=0)
    assert same_bits(st_dev[:3], STATE0[:3])                                         # count, mean, M2 as they were
    assert same_bits(g_dev, G) and same_bits(c_dev, c) and not same_bits(c_dev, carry)       # the carry still advances
    assert rel(st_dev[3], np.sqrt(7.5 + EPSILON)) <= 1e-9
    rec = ~np.isnan(G)
    want = np.clip(r[rec] / st_dev[3], -CLIP, CLIP)
    assert np.all(np.abs(out_dev[rec] - want) <= np.spacing(np.abs(want)))
    # from the zero state: var = 1
    _, out0, st0, _ = dev.run(r, d, tr, lens, carry, np.zeros(4), merge=0, clip=INF)
    assert st0[3] == np.sqrt(1.0 + EPSILON) and same_bits(st0[:3], np.zeros(3))
    want0 = r[rec] / st0[3]
    assert np.all(np.abs(out0[rec] - want0) <= np.spacing(np.abs(want0)))


@pytest.mark.parametrize("E,T", [(5, 70), (70, 3)])
def test_two_runs_are_bitwise_equal(dev, E, T):
    r, d, tr, lens, carry = make_case(E, T, 5 * E + T, True)
    first = dev.run(r, d, tr, lens, carry, STATE0)
    again = dev.run(r, d, tr, lens, carry, STATE0)
    assert all(same_bits(x, y) for x, y in zip(first, again))


def test_a_length_beyond_the_horizon_is_clamped(dev):
    E, T = 3, 5
    r, d, tr, lens, carry = make_case(E, T, 31, False)
    full = lens.copy()
    full[0] = T
    over = full.copy()
    over[0] = T + 9
    assert all(same_bits(x, y) for x, y in zip(dev.run(r, d, tr, over, carry, STATE0), dev.run(r, d, tr, full, carry, STATE0)))


# ---- the buffers: 3 environments x 6 steps, scripted frames ----
E, T, BATCH, EPOCHS, SEED = 3, 6, 8, 2, 3
RS_KEYS = {"return_rms", "reward_scale_den", "scaled_rewards", "discounted_returns", "reward_clip_fraction", "return_carry"}
BCLIP = 0.5                                                 # a clamp that bites on 18 rewards of spread 8 divided by their returns' deviation


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "reward_scaling", policy=False)


def fill(buf, continuous, source, seed=571):
    """One collection through the buffer's own step.  RolloutBuffer: lane 2 reports done at its step 4 and stops (length 4).  ContinuousRolloutBuffer: lane 1 reports
    done at its step 3 and goes on, lane 0 is truncated at its step 4.  The device tables are those of the first collection with this seed (the recording step's
    split-K layers end in fp32 atomics, so two collections of the same frames can differ in the last bit)."""
    rng = np.random.RandomState(seed)
    buf.reset()
    live = np.arange(E)
    for t in range(1, T + 1):
        f, ms, nz = inputs(rng, E)
        buf.step(f[live], ms[live], env_ids=live, noise=nz[live])
        rewards = 3.0 + 8.0 * rng.standard_normal(E)
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
    key = (continuous, seed)
    if key not in source:
        source[key] = [x.clone() for x in mine]
    for x, y in zip(mine, source[key]):
        x.copy_(y)


def new_buffer(world, tmp, continuous, ppo=None):
    from rollout import ContinuousRolloutBuffer, RolloutBuffer
    m = make_pair(tmp)[1] if ppo is None else ppo
    return m, (ContinuousRolloutBuffer if continuous else RolloutBuffer)(world["vae"], m, E, T)


def run_update(buf, diagnostics=False, **kw):
    np.random.seed(SEED)
    return (buf.update_with_diagnostics if diagnostics else buf.update)(num_epochs=EPOCHS, batch_size=BATCH, **kw)


def host_truncs(buf):
    return getattr(buf.rows, "truncs", None)


@pytest.mark.parametrize("continuous", [False, True])
def test_setting_off_is_the_buffer_that_never_had_it(world, tmp_path, continuous):
    source = {}
    m0, b0 = new_buffer(world, tmp_path / "w0", continuous)
    fill(b0, continuous, source)
    times0 = {}
    out0 = run_update(b0, stage_times=times0)
    m1, b1 = new_buffer(world, tmp_path / "w1", continuous)
    b1.set_reward_scaling()
    b1.set_reward_scaling(None)
    assert b1._reward_scaling is None
    fill(b1, continuous, source)
    times1 = {}
    out1 = run_update(b1, stage_times=times1)
    assert set(out1) == set(out0) and not RS_KEYS & set(out1) and sorted(times1) == sorted(times0) == ["finish", "logp_old", "sgd"]
    assert same_update(out1, out0) and bitwise(flat_state(m1), flat_state(m0))
    for fn in (b1.reward_scaling_state, b1.zero_return_carry):
        with pytest.raises(ValueError, match="reward scaling is off"):
            fn()


@pytest.mark.parametrize("continuous", [False, True])
def test_setting_on_is_an_unscaled_twin_fed_the_scaled_rewards(world, tmp_path, continuous):
    """... and a second collection continues the carries and the statistics; state round trip; zero_return_carry."""
    source = {}
    m1, b1 = new_buffer(world, tmp_path / "w1", continuous)
    b1.set_reward_scaling(clip=BCLIP)
    st = b1.reward_scaling_state()
    assert (st["count"], st["mean"], st["m2"]) == (0.0, 0.0, 0.0) and st["carry"].tolist() == [0.0] * E and (st["clip"], st["epsilon"], st["frozen"]) == (BCLIP, 1e-8, False)
    fill(b1, continuous, source)
    r1, d1, l1, tr1 = b1.rows.rewards.copy(), b1.rows.dones.copy(), b1.rows.lengths.copy(), host_truncs(b1)
    tr1 = None if tr1 is None else tr1.copy()
    times = {}
    out1 = run_update(b1, stage_times=times)
    assert set(times) == {"finish", "logp_old", "sgd", "reward_scaling"} and 0 < times["reward_scaling"] < times["finish"]
    # against the reference: G and carries bitwise, the moments to 1e-9, the scaled rewards from the device's own den within 1 ulp
    G, _, state, carry = reference(r1, d1, tr1, l1, 0.99, 1e-8, BCLIP, 1, np.zeros(4), np.zeros(E))
    rec = ~np.isnan(G)
    assert same_bits(out1["discounted_returns"], G) and same_bits(out1["return_carry"], carry)
    rms, den = out1["return_rms"], out1["reward_scale_den"]
    assert rms["count"] == state[0] == rec.sum() and all(type(v) is float for v in rms.values()) and type(den) is float
    assert rel(rms["mean"], state[1]) <= 1e-9 and rel(rms["var"], state[2] / state[0]) <= 1e-9 and rel(den, state[3]) <= 1e-9
    want = np.clip(r1[rec] / den, -BCLIP, BCLIP)
    scaled = out1["scaled_rewards"]
    assert np.all(np.isnan(scaled[~rec])) and np.all(np.abs(scaled[rec] - want) <= np.spacing(np.abs(want)))
    assert out1["reward_clip_fraction"] == (np.abs(want) == BCLIP).mean() and 0.0 < out1["reward_clip_fraction"] < 1.0
    assert den > 2.0                                                                 # the rewards really are on another scale
    # the twin: no scaling, host rewards = the first buffer's scaled rewards
    m2, b2 = new_buffer(world, tmp_path / "w2", continuous)
    fill(b2, continuous, source)
    b2.rows.rewards[:] = np.where(rec, scaled, 0.0)
    out2 = run_update(b2)
    assert set(out1) == set(out2) | RS_KEYS
    assert same_update(out1, out2) and bitwise(flat_state(m1), flat_state(m2))
    assert bitwise([b1.returns, b1.advantages, b1.logp_old], [b2.returns, b2.advantages, b2.logp_old])
    # ---- a second collection on the same buffer
    s1 = b1.reward_scaling_state()
    assert s1["count"] == rms["count"] and s1["mean"] == rms["mean"] and same_bits(s1["carry"], carry)
    fill(b1, continuous, source, seed=572)                                           # (reset() inside)
    after_reset = b1.reward_scaling_state()
    assert all(same_bits(after_reset[k], s1[k]) for k in ("count", "mean", "m2", "carry"))
    r2, d2, l2, tr2 = b1.rows.rewards.copy(), b1.rows.dones.copy(), b1.rows.lengths.copy(), host_truncs(b1)
    out3 = run_update(b1)
    dev_state = np.array([s1["count"], s1["mean"], s1["m2"], 0.0])
    G2, _, state2, carry2 = reference(r2, d2, tr2, l2, 0.99, 1e-8, BCLIP, 1, dev_state, s1["carry"])
    assert same_bits(out3["discounted_returns"], G2) and same_bits(out3["return_carry"], carry2)
    assert not same_bits(G2, reference(r2, d2, tr2, l2, 0.99, 1e-8, BCLIP, 1, dev_state, np.zeros(E))[0])      # the carry matters
    both = np.concatenate([G[rec], G2[~np.isnan(G2)]])
    rms2 = out3["return_rms"]
    assert rms2["count"] == both.size
    assert rel(rms2["mean"], np.mean(both)) <= 1e-9 and rel(rms2["var"], np.var(both)) <= 1e-9 and rel(out3["reward_scale_den"], state2[3]) <= 1e-9
    # the reference over both from the zero state (its own chained statistics)
    _, _, ref2, _ = reference(r2, d2, tr2, l2, 0.99, 1e-8, BCLIP, 1, state, carry)
    assert rel(rms2["mean"], ref2[1]) <= 1e-9 and rel(rms2["var"], ref2[2] / ref2[0]) <= 1e-9
    # ---- the round trip: a policy that made the same first update, a FRESH buffer that loads the first buffer's state
    m4, b4 = new_buffer(world, tmp_path / "w4", continuous)
    b4.set_reward_scaling(clip=BCLIP)
    fill(b4, continuous, source)
    run_update(b4)
    _, b5 = new_buffer(world, None, continuous, ppo=m4)
    b5.load_reward_scaling_state(s1)
    got = b5.reward_scaling_state()
    assert all(same_bits(got[k], s1[k]) for k in ("count", "mean", "m2", "carry")) and all(got[k] == s1[k] for k in ("clip", "epsilon", "frozen"))
    fill(b5, continuous, source, seed=572)
    out5 = run_update(b5)
    assert same_update(out5, out3) and bitwise(flat_state(m4), flat_state(m1))
    for k in ("discounted_returns", "scaled_rewards", "return_carry"):
        assert same_bits(out5[k], out3[k]), k
    assert out5["return_rms"] == out3["return_rms"] and out5["reward_scale_den"] == out3["reward_scale_den"]
    # ---- zero_return_carry([1]) changes lane 1's G alone (no epoch runs: the returns do not depend on the policy)
    _, b6 = new_buffer(world, None, continuous, ppo=m4)
    b6.load_reward_scaling_state(s1)
    b6.zero_return_carry([1])
    assert b6.reward_scaling_state()["carry"].tolist() == [s1["carry"][0], 0.0, s1["carry"][2]] and s1["carry"][1] != 0.0
    fill(b6, continuous, source, seed=572)
    np.random.seed(SEED)
    out6 = b6.update(num_epochs=0, batch_size=BATCH)
    g6 = out6["discounted_returns"]
    assert same_bits(g6[[0, 2]], G2[[0, 2]]) and not same_bits(g6[1], G2[1])
    zeroed = s1["carry"].copy()
    zeroed[1] = 0.0
    assert same_bits(g6, reference(r2, d2, tr2, l2, 0.99, 1e-8, BCLIP, 1, dev_state, zeroed)[0])
    b6.zero_return_carry()
    assert b6.reward_scaling_state()["carry"].tolist() == [0.0] * E
    with pytest.raises(ValueError):
        b6.zero_return_carry([E])
    # frozen: the statistics stay, the carries advance
    before = b6.reward_scaling_state()
    b6.set_reward_scaling(clip=BCLIP, frozen=True)
    fill(b6, continuous, source, seed=572)
    out7 = b6.update(num_epochs=0, batch_size=BATCH)
    after = b6.reward_scaling_state()
    assert all(same_bits(after[k], before[k]) for k in ("count", "mean", "m2")) and after["frozen"] is True
    assert same_bits(out7["return_carry"], after["carry"]) and np.any(after["carry"] != 0.0)
    assert out7["return_rms"]["count"] == before["count"]


@pytest.mark.parametrize("continuous", [False, True])
def test_a_reward_that_is_not_finite(world, tmp_path, continuous):
    import torch
    source = {}
    m, b = new_buffer(world, tmp_path / "w", continuous)
    b.set_reward_scaling()
    fill(b, continuous, source)
    run_update(b)                                                                    # statistics and carries that are not zero
    fill(b, continuous, source, seed=572)
    keep = b.rows.rewards[0, 2]
    state, carry = b._reward_scaling["state"].clone(), b._reward_scaling["carry"].clone()
    params, tables = flat_state(m), [b.returns.clone(), b.advantages.clone()]
    rng_state = np.random.get_state()[1].copy()
    for bad in (float("nan"), float("inf")):
        b.rows.rewards[0, 2] = bad
        for fn in (b.update, b.update_with_diagnostics):
            with pytest.raises(ValueError, match="a recorded reward is not finite"):
                fn(num_epochs=EPOCHS, batch_size=BATCH)
    assert bitwise([b._reward_scaling["state"], b._reward_scaling["carry"]], [state, carry]) and float(state[0]) > 0 and bool(carry.ne(0).any())
    assert bitwise(flat_state(m), params) and torch.equal(b.returns, tables[0]) and torch.equal(b.advantages, tables[1])
    assert np.array_equal(np.random.get_state()[1], rng_state)
    b.rows.rewards[0, 2] = keep
    if not continuous:                                                               # lane 2 holds 4 steps: a NaN behind them is not looked at
        assert b.rows.lengths[2] == 4
        b.rows.rewards[2, 5] = np.nan
    out = run_update(b)
    assert np.isfinite(out["reward_scale_den"]) and np.isfinite(out["return_carry"]).all() and all(np.isfinite(x["loss"]) for x in out["losses"])
    # with the setting off the host array is not looked at (the parent's behaviour)
    b.set_reward_scaling(None)
    assert not RS_KEYS & set(run_update(b))


@pytest.mark.parametrize("continuous", [False, True])
def test_value_clipping_together_with_scaling(world, tmp_path, continuous):
    source = {}
    m1, b1 = new_buffer(world, tmp_path / "w1", continuous)
    m1.set_value_clip(0.2)
    b1.set_reward_scaling(clip=BCLIP)
    fill(b1, continuous, source)
    out1 = run_update(b1, diagnostics=True)
    m2, b2 = new_buffer(world, tmp_path / "w2", continuous)
    m2.set_value_clip(0.2)
    fill(b2, continuous, source)
    b2.rows.rewards[:] = np.nan_to_num(out1["scaled_rewards"], nan=0.0)
    out2 = run_update(b2, diagnostics=True)
    assert len(out1["epochs"]) == EPOCHS and set(out1) == set(out2) | RS_KEYS
    for e1, e2 in zip(out1["epochs"], out2["epochs"]):
        assert "value_clip_fraction" in e1 and e1["value_clip_fraction"] == e2["value_clip_fraction"]
        assert e1 == e2
    assert same_update(out1, out2) and bitwise(flat_state(m1), flat_state(m2))
