"""The batched rollout step, the recording step, the value-only call and both rollout buffers on an MlpVAE encoder (mi_mlp_rollout_step_batch /
mi_mlp_rollout_value_batch; csrc/rollout_mlp.hip for layer 1, the flat layers and the trunks of csrc/rollout.hip behind it).

Reference: oracle.vae_oracle.mlp_vae_forward(params, frames / 255, sample=False)["mean"] in float64, np.append, OraclePPO.predict.  Parameters: init_mlp_vae_params
with N(0, 0.05) biases; the policy: rollout_gpu_common.make_pair(input_dim = z + 3).  Tolerances are the project's for this step (rollout_gpu_common): latents 1e-4 of the
row's max, actions rtol 1e-4 / atol 1e-5, values rel 1e-4 / abs 1e-5, and 1e-5 between two device paths (both end in fp32 atomics).  A CPU emulation of fp32 64-wide
K-slab sums in random order lies 2.3e-7 to 5.3e-7 from float64 on models A, B and C, so the 1e-4 bound leaves the reference room.

Shapes (source_shape, encoder_sizes, z_dim):
  A  (80, 160, 3), (512, 256), 64       the reference's model: 600 K-slabs of 64 (n = 1, 5), 150 of 256 and four 128-column passes (n = 33)
  B  (4, 6, 3) = 72 bytes, (36,), 8     K below two slabs (n <= 32) and below one (n >= 33); a 4-column tail behind a 32-column tile; one hidden layer
  C  (8, 11, 3) = 264 bytes, (132, 20, 12, 8), 8      256 + 8 bytes; four hidden layers
  D  layer 1's own tile edges.  rollout_mlp_layer1_kernel<KS>'s grid is ceil(S / KS) blocks of 4 waves and nothing else: block b owns bytes [KS b, KS b + KS) of every
     environment (staged once in LDS, KS bytes per environment rounded up to 32 environments) and every column; a wave holds the weights of CT = 256 / KS 32-column
     tiles (w, w + 4, ..) of a pass of 4 CT tiles and walks the row tiles (32 environments each) with them; N1 past a pass takes another.  The launcher picks
     KS = 64 for n <= 32, else the widest of 256 / 128 / 64 whose LDS stage fits 64 KB: 256 for n <= 256, 128 for n <= 512, 64 above.  So, per kernel:
       KS = 64   S = 64 / 68 (one slab, + 4), N1 = 32 / 36 (a column tile, + 4) and 512 / 516 (a pass, + 4), n = 31, 32 -- and 33, the first call of KS = 256
       KS = 256  S = 256 / 260, N1 = 128 / 132 (its pass, + 4), n = 33 (above the row tile), 64, 256 (its last n: the 64 KB stage)
       KS = 128  S = 128 / 132, N1 = 256 / 260 (its pass, + 4), n = 257 (its first n), 512 (its last: 64 KB)
       KS = 64 again at n = 513 (its first n above) and 1024 (the largest call: 64 KB, 32 row tiles per weight fragment)

The first thing the module does is to look for the new symbol: on a tree without the feature every test fails there, before any device call -- an MlpVAE handle must
never reach the ConvVAE's entries.
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "carla-ppo_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import ppo_oracle as po  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402
from rollout_gpu_common import SENTINEL, check_losses, make_pair, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

K, A = 3, 2
SHAPES = {
    "A": ((80, 160, 3), (512, 256), 64),
    "B": ((4, 6, 3), (36,), 8),
    "C": ((8, 11, 3), (132, 20, 12, 8), 8),
    "D64x32": ((4, 4, 4), (32,), 8),
    "D68x36": ((4, 17, 1), (36,), 8),
    "D64x512": ((4, 4, 4), (512,), 8),
    "D68x516": ((4, 17, 1), (516,), 8),
    "D256x128": ((8, 8, 4), (128,), 8),
    "D260x132": ((4, 65, 1), (132,), 8),
    "D128x256": ((4, 8, 4), (256,), 8),
    "D132x260": ((4, 11, 3), (260,), 8),
}
GAMMA, LAM = 0.99, 0.95


def mlp_params(name):
    src, enc, z = SHAPES[name]
    rng = np.random.RandomState(21)
    p = vo.init_mlp_vae_params(3, z_dim=z, source_shape=src, target_shape=src, encoder_sizes=enc, decoder_sizes=(8,))
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    return p


def oracle_latents(params, frames):
    """float64: mlp_vae_forward(params, frames / 255, sample=False)["mean"]"""
    import torch
    p64 = OrderedDict((k, torch.from_numpy(np.asarray(v, np.float64))) for k, v in params.items())
    return vo.mlp_vae_forward(p64, np.asarray(frames).reshape(len(frames), -1) / 255, sample=False, dtype=torch.float64)["mean"].numpy()


def oracle_predict(o, z, meas, noise, greedy):
    states = np.stack([np.append(z[e], meas[e]) for e in range(len(z))])
    a, v = o.predict(states, greedy=greedy, noise=None if greedy else noise)
    return np.asarray(a).reshape(len(z), o.num_actions), np.asarray(v).reshape(len(z))


def inputs(rng, name, n):
    frames = rng.randint(0, 256, (n,) + SHAPES[name][0], dtype=np.uint8)
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 30, n)], axis=1)
    noise = rng.standard_normal((n, A)).astype(np.float32)
    return frames, meas, noise


class World:
    """VAEs, policies and steps, made on first use and shared by the module's tests."""

    def __init__(self, tmp):
        self.tmp, self.vaes, self.pairs, self.steps, self.params = tmp, {}, {}, {}, {}

    def vparams(self, name):
        if name not in self.params:
            self.params[name] = mlp_params(name)
        return self.params[name]

    def vae(self, name, precision="fp32"):
        from vae.models import MlpVAE
        key = (name, precision)
        if key not in self.vaes:
            src, enc, z = SHAPES[name]
            v = MlpVAE(np.array(src), encoder_sizes=enc, decoder_sizes=(8,), z_dim=z, model_dir=str(self.tmp / ("vae_%s_%s" % key)), precision=precision, training=False)
            v.set_weights(self.vparams(name))
            v.init_session(init_logging=False)
            self.vaes[key] = v
        return self.vaes[key]

    def pair(self, z):
        if z not in self.pairs:
            self.pairs[z] = make_pair(self.tmp / ("ppo_%d" % z), input_dim=z + K)
        return self.pairs[z]

    def step(self, name, num_envs, precision="fp32", io="pinned"):
        from rollout import BatchedRolloutStep
        key = (name, num_envs, precision, io)
        if key not in self.steps:
            self.steps[key] = BatchedRolloutStep(self.vae(name, precision), self.pair(SHAPES[name][2])[1], num_envs, seed=3, io=io)
        return self.steps[key]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from mi355 import lib as milib
    assert hasattr(milib.get().cdll, "mi_mlp_rollout_step_batch"), "the library has no rollout step for the MlpVAE: nothing here may hand its handle to mi_rollout_*"
    return World(tmp_path_factory.mktemp("mlp_rollout"))


def call(step, frames, meas, noise, greedy):
    """One call with the scratch full of NaN and the output buffers at the sentinel -> (actions, values, states), and the rows >= n of the output buffers."""
    import torch
    step.scratch.view(torch.float32).fill_(float("nan"))
    step.h_out.fill_(SENTINEL)
    if step.d_out is not None:
        step.d_out.fill_(SENTINEL)
    torch.cuda.synchronize()
    got = step(frames, meas, greedy=greedy, noise=noise)
    n = len(frames)
    rest = [step._out_np[n:].copy()] + ([] if step.d_out is None else [step.d_out.cpu().numpy().reshape(step.num_envs, step.row)[n:]])
    assert all((r == np.float32(SENTINEL)).all() for r in rest), "output rows >= n were written"
    return got


def check(got, z_o, a_o, v_o, meas, z, tag, worst=None):
    a, v, states = got
    n = len(z_o)
    assert a.shape == (n, A) and a.dtype == np.float32 and v.shape == (n,) and v.dtype == np.float32, tag
    assert states.shape == (n, z + K) and states.dtype == np.float64, tag
    assert np.array_equal(states[:, z:], np.asarray(meas, np.float64)), tag
    errs = [rel_err(states[e, :z], z_o[e]) for e in range(n)]
    if worst is not None:
        worst.append(max(errs))
    print("%s: latents max rel %.3e, actions max abs %.3e, values max abs %.3e" % (tag, max(errs), np.abs(a - a_o).max(), np.abs(v - v_o).max()))
    for e in range(n):
        assert errs[e] < 1e-4, (tag, e, errs[e])
        assert np.allclose(a[e], a_o[e], rtol=1e-4, atol=1e-5), (tag, e, a[e], a_o[e])
        assert float(v[e]) == pytest.approx(float(v_o[e]), rel=1e-4, abs=1e-5), (tag, e)


def run_and_check(world, name, ns, num_envs, precision="fp32", io="pinned", seed=5):
    z = SHAPES[name][2]
    o, _ = world.pair(z)
    step = world.step(name, num_envs, precision, io)
    rng = np.random.RandomState(seed)
    frames, meas, noise = inputs(rng, name, max(ns))
    z_o = oracle_latents(world.vparams(name), frames)                                 # once for the largest n: a shorter call takes the first rows
    for n in ns:
        for greedy in (False, True):
            a_o, v_o = oracle_predict(o, z_o[:n], meas[:n], noise[:n], greedy)
            got = call(step, frames[:n], meas[:n], noise[:n], greedy)
            check(got, z_o[:n], a_o, v_o, meas[:n], z, "%s %s %s n=%d %s" % (name, precision, io, n, "greedy" if greedy else "sampled"))


@pytest.mark.parametrize("io", ["pinned", "device"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_shape_a_matches_the_oracle(world, precision, io):
    """The reference's model at n = 1, 5, 33, sampled and greedy.  bf16 storage gives the same answers: the step reads the fp32 master weights."""
    run_and_check(world, "A", (1, 5, 33), 33, precision, io)


def test_shape_b_matches_the_oracle(world):
    run_and_check(world, "B", (1, 2, 31, 32, 33, 64, 65), 65)


def test_shape_c_matches_the_oracle(world):
    run_and_check(world, "C", (1, 33), 33)


@pytest.mark.parametrize("name,ns", [("D64x32", (31, 32, 33)), ("D68x36", (31, 32, 33)), ("D64x512", (31, 32, 33)), ("D68x516", (31, 32, 33)),
                                     ("D256x128", (33, 64, 256)), ("D260x132", (33, 64, 256)), ("D128x256", (257, 512)), ("D132x260", (257, 512))])
def test_shape_d_layer1_tile_edges(world, name, ns):
    """Kernel D's grids (see the module docstring): for each of the three K-slabs one slab and a slab + 4, a column tile / a pass and + 4, and the n at which the
    launcher changes the slab."""
    run_and_check(world, name, ns, max(ns))


def test_the_largest_calls_513_and_1024_environments(world):
    """n = 513 (the first call back on the 64-byte slab) and n = MI_ROLLOUT_MAX_ENVS on the smallest model: the 64 KB LDS stage, 32 row tiles per weight fragment."""
    run_and_check(world, "D68x36", (513, 1024), 1024)


@pytest.mark.parametrize("name", ["A", "B"])
def test_repeated_permuted_and_shorter_calls(world, name):
    """Calls of n = 8, 8, 3, 8 each match their own oracle (the scratch is NaN before every call: nothing is carried over); a permutation of the environments
    permutes the rows; a shorter call gives the first rows; the sampled action is not the greedy one."""
    z = SHAPES[name][2]
    o, _ = world.pair(z)
    step = world.step(name, 8)
    rng = np.random.RandomState(17)
    for i, n in enumerate((8, 8, 3, 8)):
        frames, meas, noise = inputs(rng, name, n)
        z_o = oracle_latents(world.vparams(name), frames)
        a_o, v_o = oracle_predict(o, z_o, meas, noise, False)
        got = call(step, frames, meas, noise, False)
        check(got, z_o, a_o, v_o, meas, z, "%s call %d n=%d" % (name, i, n))
    perm = np.random.RandomState(3).permutation(8)
    got_p = call(step, frames[perm], meas[perm], noise[perm], False)
    for x, y in zip(got, got_p):
        assert np.allclose(x[perm], y, rtol=1e-5, atol=1e-5)
    got_s = call(step, frames[:3], meas[:3], noise[:3], False)
    for x, y in zip(got, got_s):
        assert np.allclose(x[:3], y, rtol=1e-5, atol=1e-5)
    greedy = call(step, frames, meas, None, True)
    assert np.abs(greedy[0] - got[0]).max() > 1e-3                                   # sampled != greedy ...
    assert np.allclose(greedy[1], got[1], rtol=1e-5, atol=1e-5) and np.allclose(greedy[2], got[2], rtol=1e-5, atol=1e-5)   # ... value and state do not depend on it


def tables(buf):
    return buf.states.cpu().numpy(), buf.actions.cpu().numpy(), buf.values.cpu().numpy()


def fill_tables(buf):
    for t in (buf.states, buf.actions, buf.values, buf.returns, buf.advantages, buf.logp_old):
        t.fill_(SENTINEL)


def test_recording_is_exact_and_confined(world, tmp_path):
    """Shape B, n = 5 through RolloutBuffer.step: the table rows hold bitwise what the call returned, every other row keeps its sentinel, table_rows = -1 records nothing."""
    from rollout import RolloutBuffer
    z = SHAPES["B"][2]
    o, _ = world.pair(z)
    _, m = make_pair(tmp_path / "m", input_dim=z + K)
    E, T = 6, 4
    buf = RolloutBuffer(world.vae("B"), m, E, T, seed=3)
    buf.reset()
    fill_tables(buf)
    rng = np.random.RandomState(31)
    ids = np.array([4, 0, 5, 2, 1])
    frames, meas, noise = inputs(rng, "B", 5)
    before = tables(buf)
    got = buf.step(frames, meas, env_ids=ids, noise=noise)
    z_o = oracle_latents(world.vparams("B"), frames)
    a_o, v_o = oracle_predict(o, z_o, meas, noise, False)
    check(got, z_o, a_o, v_o, meas, z, "recording step")
    rows = ids * (T + 1)
    s, a, v = tables(buf)
    actions, values, states = got
    assert np.array_equal(s[rows, :z], states[:, :z].astype(np.float32)) and np.array_equal(s[rows, z:], meas.astype(np.float32))
    assert np.array_equal(a[rows], actions) and np.array_equal(v[rows], values)
    other = np.ones(len(v), bool)
    other[rows] = False
    for now, was in zip((s, a, v), before):
        assert np.array_equal(now[other], was[other]) and (now[other] == np.float32(SENTINEL)).all()
    # table_rows = -1 (and a row behind the table): the call returns its rows and records nothing
    st = buf._step
    now = tables(buf)
    got2 = st.record(frames[:3], 3, meas[:3], noise[:3], False, np.array([-1, E * (T + 1), -1], np.int32), buf.states, buf.actions, buf.values)
    for x, y in zip(got, got2):
        assert np.allclose(x[:3], y, rtol=1e-5, atol=1e-5)
    for x, y in zip(tables(buf), now):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("io", ["pinned", "device"])
def test_value_only_call(world, tmp_path, io):
    """truncate() on shape B: within 1e-5 of the greedy step's value; final_values[row] is written, bitwise what came back, every other row untouched; a NULL
    table_rows (the raw entry) writes nothing at all."""
    from rollout import ContinuousRolloutBuffer
    z = SHAPES["B"][2]
    _, m = make_pair(tmp_path / "m", input_dim=z + K)
    E, T = 4, 4
    buf = ContinuousRolloutBuffer(world.vae("B"), m, E, T, io=io, seed=3)
    from rollout import BatchedRolloutStep
    step = BatchedRolloutStep(world.vae("B"), m, E, io=io, seed=3)                    # the greedy step on the same policy engine
    rng = np.random.RandomState(41)
    buf.reset()
    f, ms, nz = inputs(rng, "B", E)
    buf.step(f, ms, noise=nz)
    buf.outcome(rng.uniform(0, 1, E), np.zeros(E, bool))
    ids = np.array([3, 0, 1])
    f, ms, _ = inputs(rng, "B", 3)
    before = tables(buf)
    got = buf.truncate(f, ms, env_ids=ids)
    assert got.shape == (3,) and got.dtype == np.float32
    _, v_step, _ = step(f, ms, greedy=True)
    print("io=%s: value-only call against the greedy step: max |diff| = %.3e" % (io, np.abs(got - v_step).max()))
    assert np.allclose(got, v_step, rtol=1e-5, atol=1e-5)
    want = np.zeros(E * (T + 1), np.float32)
    want[ids * (T + 1)] = got
    assert np.array_equal(buf.final_values.cpu().numpy(), want)
    for now, was in zip(tables(buf), before):
        assert np.array_equal(now, was)
    # the raw entry with table_rows = NULL: the values come back, no table is touched
    L, s = buf.L, buf._step
    base = (s.h_in if s.d_in is None else s.d_in).data_ptr()
    s.h_out.fill_(SENTINEL)
    if s.d_out is not None:
        s.d_out.fill_(SENTINEL)
    out = (s.h_out if s.d_out is None else s.d_out)
    import torch
    s.scratch.view(torch.float32).fill_(float("nan"))
    torch.cuda.synchronize()
    L.mi_mlp_rollout_value_batch(buf.vae.dev.handle, m.dev.handle, torch.cuda.current_stream().cuda_stream, base, base + s._f_off, s.n_meas, 3, s.scratch.data_ptr(),
                                 s.scratch_bytes, out.data_ptr(), None, None, 0.0, None, None, 0, None)
    torch.cuda.synchronize()
    o_np = out.cpu().numpy()
    assert np.allclose(o_np[:3], got, rtol=1e-5, atol=1e-5) and (o_np[3:] == np.float32(SENTINEL)).all()
    assert np.array_equal(buf.final_values.cpu().numpy(), want)


def test_observation_normalisation(world, tmp_path):
    """set_observation_normalization on synthetic statistics: `states` within 1 fp32 ulp of normalize_observations(raw_states), raw_states bitwise the returned state;
    fresh statistics with clip = inf give states == raw_states."""
    from rollout import RolloutBuffer, normalize_observations
    z = SHAPES["B"][2]
    din = z + K
    _, m = make_pair(tmp_path / "m", input_dim=din)
    E, T = 5, 3
    rng = np.random.RandomState(51)
    buf = RolloutBuffer(world.vae("B"), m, E, T, seed=3)
    buf.set_observation_normalization(clip=2.5, epsilon=1e-8)
    sd = buf.observation_normalization_state()
    sd = dict(sd, count=100.0, mean=rng.uniform(-0.5, 0.5, din), m2=100.0 * rng.uniform(0.2, 4.0, din))
    buf.load_observation_normalization_state(sd)
    buf.reset()
    frames, meas, noise = inputs(rng, "B", E)
    _, _, states = buf.step(frames, meas, noise=noise)
    rows = np.arange(E) * (T + 1)
    raw, nrm = buf.raw_states.cpu().numpy()[rows], buf.states.cpu().numpy()[rows]
    assert np.array_equal(raw, states.astype(np.float32))
    want = normalize_observations(raw, buf.observation_normalization_state())
    ulp = np.spacing(np.abs(want).astype(np.float32))
    assert (np.abs(nrm.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert np.abs(nrm).max() <= np.float32(2.5)                                      # (the clamp holds)
    # fresh statistics (count 0: mean 0, inv_std exactly 1) and clip = inf: the identity
    buf2 = RolloutBuffer(world.vae("B"), m, E, T, seed=3)
    buf2.set_observation_normalization(clip=float("inf"))
    buf2.reset()
    _, _, states2 = buf2.step(frames, meas, noise=noise)
    assert np.array_equal(buf2.states.cpu().numpy()[rows], buf2.raw_states.cpu().numpy()[rows])
    assert np.array_equal(buf2.raw_states.cpu().numpy()[rows], states2.astype(np.float32))


def scripted(E, T):
    rng = np.random.RandomState(61)
    return rng.uniform(0, 1, (T, E))


def test_rollout_buffer_collection_and_update(world, tmp_path):
    """(E, T) = (3, 5) on shape B, scripted rewards and dones (environment 1 is done at its step 3): returns and raw advantages against compute_gae on the recorded
    values (test_m_rollout_buffer_gpu.py: the host statements, bit for bit), the losses against the oracle fed the same samples (check_losses)."""
    import utils
    from rollout import RolloutBuffer
    z = SHAPES["B"][2]
    o, m = make_pair(tmp_path / "a", input_dim=z + K)
    E, T, epochs, batch, seed = 3, 5, 2, 4, 5
    buf = RolloutBuffer(world.vae("B"), m, E, T, seed=3)
    rng = np.random.RandomState(71)
    rewards, done_at = scripted(E, T), {1: 3}
    buf.reset()
    live, t = np.arange(E), 0
    while len(live):
        f, ms, nz = inputs(rng, "B", len(live))
        buf.step(f, ms, env_ids=live, noise=nz)
        dones = np.array([done_at.get(int(e)) == t + 1 for e in live])
        buf.outcome(rewards[t, live], dones, env_ids=live)
        t += 1
        live = live[~dones & (buf.lengths[live] < T)]
    f, ms, _ = inputs(rng, "B", E)
    buf.bootstrap(f, ms)
    valid = buf.rows.valid_rows()
    assert buf.lengths.tolist() == [5, 3, 5] and len(valid) == 13
    s_tab, a_tab, v_tab = tables(buf)
    v_tab = v_tab.reshape(E, T + 1)
    np.random.seed(seed)
    out = buf.update(GAMMA, LAM, num_epochs=epochs, batch_size=batch)
    rets, advs = [], []
    for e in range(E):
        n = int(buf.lengths[e])
        raw_o = po.compute_gae(buf.rows.rewards[e, :n], v_tab[e, :n].astype(np.float64), float(v_tab[e, n]), buf.rows.dones[e, :n], GAMMA, LAM)
        ret_o, _ = po.returns_and_normalized_advantages(raw_o, v_tab[e, :n].astype(np.float64))
        assert np.array_equal(out["raw_advantages"][e, :n], raw_o) and np.array_equal(out["returns"][e, :n], ret_o), e
        adv = utils.compute_gae(buf.rows.rewards[e, :n], v_tab[e, :n], v_tab[e, n], buf.rows.dones[e, :n], GAMMA, LAM)
        ret, advn = utils.normalize_advantages(adv, v_tab[e, :n])
        assert np.array_equal(out["returns"][e, :n], ret) and np.array_equal(out["advantages"][e, :n], advn), e
        rets.append(ret)
        advs.append(advn)
    ret, adv = np.concatenate(rets), np.concatenate(advs)
    s, a = s_tab[valid], a_tab[valid]
    o.update_old_policy()
    np.random.seed(seed)
    logs_o = [o.train(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    check_losses(out["losses"], logs_o, "MlpVAE RolloutBuffer against the oracle")


def test_continuous_buffer_collection_with_a_truncation_and_update(world, tmp_path):
    """(E, T) = (3, 5) on shape B: lane 0 is truncated behind its step 2, lane 1 reports done at its step 3, lane 2 runs through.  Per segment, returns and raw
    advantages against oracle compute_gae on the returned values / final_values / bootstrap_values (test_o_rollout_truncation_gpu.py: bitwise), losses by check_losses."""
    import utils
    from rollout import ContinuousRolloutBuffer
    z = SHAPES["B"][2]
    o, m = make_pair(tmp_path / "a", input_dim=z + K)
    E, T, epochs, batch, seed = 3, 5, 2, 5, 5
    buf = ContinuousRolloutBuffer(world.vae("B"), m, E, T, seed=3)
    rng = np.random.RandomState(81)
    rewards = scripted(E, T)
    buf.reset()
    returned = None
    for t in range(1, T + 1):
        f, ms, nz = inputs(rng, "B", E)
        buf.step(f, ms, noise=nz)
        buf.outcome(rewards[t - 1], np.array([e == 1 and t == 3 for e in range(E)]))
        if t == 2:
            f, ms, _ = inputs(rng, "B", 1)
            returned = buf.truncate(f, ms, env_ids=np.array([0]))
    need = buf.rows.needs_bootstrap()
    assert need.tolist() == [0, 1, 2]
    f, ms, _ = inputs(rng, "B", E)
    buf.bootstrap(f[need], ms[need], env_ids=need)
    valid = buf.rows.valid_rows()
    segs = buf.rows.segments()
    assert segs.tolist() == [[0, 0, 2], [0, 2, 3], [1, 0, 3], [1, 3, 2], [2, 0, 5]]
    s_tab, a_tab, _ = tables(buf)
    np.random.seed(seed)
    out = buf.update(GAMMA, LAM, num_epochs=epochs, batch_size=batch)
    assert out["samples"] == E * T and out["segment_truncated"].tolist() == [1, 0, 0, 0, 0]
    fv = out["final_values"]
    assert fv[0, 1] == returned[0]
    rets, advs = [], []
    for (e, first, n), tr in zip(segs, out["segment_truncated"]):
        last = first + n - 1
        done = buf.rows.dones[e, last] != 0
        boot = float(fv[e, last]) if tr else 0.0 if done else float(out["bootstrap_values"][e])
        sl = slice(first, first + n)
        raw_o = po.compute_gae(buf.rows.rewards[e, sl], out["values"][e, sl].astype(np.float64), boot, buf.rows.dones[e, sl], GAMMA, LAM)
        ret_o, _ = po.returns_and_normalized_advantages(raw_o, out["values"][e, sl].astype(np.float64))
        assert np.array_equal(out["raw_advantages"][e, sl], raw_o) and np.array_equal(out["returns"][e, sl], ret_o), (e, first, n)
        adv = utils.compute_gae(buf.rows.rewards[e, sl], out["values"][e, sl], boot, buf.rows.dones[e, sl], GAMMA, LAM)
        ret, advn = utils.normalize_advantages(adv, out["values"][e, sl])
        rets.append(ret)
        advs.append(advn)
    ret, adv = np.concatenate(rets), np.concatenate(advs)
    s, a = s_tab[valid], a_tab[valid]
    o.update_old_policy()
    np.random.seed(seed)
    logs_o = [o.train(s[mb], a[mb], ret[mb], adv[mb]) for mb in po.minibatch_schedule(len(valid), batch, epochs)]
    check_losses(out["losses"], logs_o, "MlpVAE ContinuousRolloutBuffer against the oracle")


def test_the_step_follows_an_adam_step_of_the_vae(tmp_path, world):
    """The step reads the master weights: after one MlpVAE Adam step its latents match the oracle on the exported parameters, and differ from those before."""
    from rollout import BatchedRolloutStep
    from vae.models import MlpVAE
    src, enc, z = SHAPES["C"]
    _, m = world.pair(z)
    vae = MlpVAE(np.array(src), encoder_sizes=enc, decoder_sizes=(8,), z_dim=z, model_dir=str(tmp_path / "v"), precision="fp32", learning_rate=1e-3)
    vae.set_weights(world.vparams("C"))
    vae.init_session(init_logging=False)
    step = BatchedRolloutStep(vae, m, 4, seed=3)
    rng = np.random.RandomState(91)
    frames, meas, noise = inputs(rng, "C", 4)
    before = call(step, frames, meas, noise, True)[2][:, :z]
    assert max(rel_err(before[e], oracle_latents(world.vparams("C"), frames)[e]) for e in range(4)) < 1e-4
    x = frames.astype(np.float32) / 255.0
    vae.train_step(x, x, eps=rng.standard_normal((4, z)).astype(np.float32))
    after = call(step, frames, meas, noise, True)[2][:, :z]
    z_o = oracle_latents(vae.dev.export_params(), frames)
    for e in range(4):
        assert rel_err(after[e], z_o[e]) < 1e-4, e
    assert np.abs(after - before).max() > 1e-4 * np.abs(before).max()


def test_misuse_is_refused(world, tmp_path):
    """Wrong frame size, wrong measurement shape and RolloutStep(MlpVAE) raise ValueError; the raw C call refuses a scratch one byte short, n = 0 and 1025,
    n_meas = 2 (-2) and n above the policy's max_batch, the output buffer still at its sentinel."""
    import torch
    from rollout import BatchedRolloutStep, RolloutStep
    z = SHAPES["B"][2]
    _, m = make_pair(tmp_path / "m", input_dim=z + K)
    vae = world.vae("B")
    step = BatchedRolloutStep(vae, m, 4, seed=3)
    rng = np.random.RandomState(95)
    frames, meas, noise = inputs(rng, "B", 4)
    with pytest.raises(ValueError, match="uint8 frames"):
        step(frames[:, :3], meas)
    with pytest.raises(ValueError, match="measurements"):
        step(frames, meas[:, :2])
    with pytest.raises(ValueError, match=r"BatchedRolloutStep\(vae, ppo, num_envs=1\)"):
        RolloutStep(vae, m)
    L = step.L
    step(frames, meas, noise=noise)                                                   # fills the input buffer
    step.h_out.fill_(SENTINEL)
    base = step.h_in.data_ptr()
    good = dict(mlp_h=vae.dev.handle, ppo_h=m.dev.handle, stream=torch.cuda.current_stream().cuda_stream, frames_u8=base, measurements=base + step._f_off, n_meas=K,
                noise=None, greedy=1, n=4, scratch=step.scratch.data_ptr(), scratch_bytes=step.scratch_bytes, out=step.h_out.data_ptr(), obs_mean=None, obs_inv_std=None,
                obs_clip=0.0, nstate=None, table_rows=None, n_table_rows=0, tab_states=None, tab_raw_states=None, tab_actions=None, tab_values=None)
    names = [a[1] for a in L.protos["mi_mlp_rollout_step_batch"][1]]
    raw = lambda **kw: L.cdll.mi_mlp_rollout_step_batch(*[dict(good, **kw)[k] for k in names])      # noqa: E731
    err = L.cdll.mi_last_error
    me = b"mi_mlp_rollout_step_batch: "
    assert step.scratch_bytes == 4 * 4 * (36 + 8)
    assert raw(scratch_bytes=step.scratch_bytes - 1) == -1 and err().startswith(me + b"scratch too small")
    for bad in (0, 1025):
        assert raw(n=bad) == -1 and err().startswith(me + b"1 <= n <= MI_ROLLOUT_MAX_ENVS"), bad
    assert raw(n_meas=2) == -2 and err().startswith(me + b"z_dim + measurements")
    big = m.dev.max_batch + 1
    assert big <= 1024
    assert raw(n=big, scratch_bytes=1 << 40) == -1 and err().startswith(me + b"n exceeds the PPO engine's max_batch")
    torch.cuda.synchronize()
    assert (step.h_out.numpy() == np.float32(SENTINEL)).all()
    assert raw() == 0                                                                 # and the good call goes through
    torch.cuda.synchronize()
    assert (step.h_out.numpy()[:4 * step.row] != np.float32(SENTINEL)).all()
