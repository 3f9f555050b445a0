"""The batched rollout step (rollout.BatchedRolloutStep / mi_rollout_step_batch: n environments' camera bytes + measurements -> actions, values, latents in
one call) against the oracle's encode -> np.append -> predict per row, against the B = 1 path (RolloutStep), and its row independence, reuse, interplay
with training and misuse.  Set-up restated from test_c_c3_ppo_gpu.py::test_rollout_step_one_call_matches_encode_then_predict (oracle VAE with N(0, 0.05) biases,
the make_pair policy, random camera bytes); tolerances are that test's: latents 1e-4 relative, actions rtol 1e-4 / atol 1e-5, value rel 1e-4 / abs 1e-5
against the oracle, 1e-5 between the device paths (both end in fp32 atomics, so bit equality is not asked)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rollout_gpu_common import A, K, Z, Oracle, check_against_oracle, close, inputs, make_pair, make_vae, make_world  # noqa: E402


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return make_world(tmp_path_factory, "rollout_batch")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_every_row_matches_the_oracle(world, precision):
    """E in {1, 2, 5, 32, 33, 64} x sampled / greedy x io pinned / device x VAE storage fp32 / bf16 (the step computes in exact fp32 on the master weights)."""
    from rollout import BatchedRolloutStep
    vae = world["vae"] if precision == "fp32" else make_vae(world["tmp"] / "vae_bf16", world["vparams"], "bf16")
    rng = np.random.RandomState(33)
    frames, meas, noise = inputs(rng, 64)
    z_all = world["orc"].latents(frames)
    for io in ("pinned", "device"):
        for E in (1, 2, 5, 32, 33, 64):
            step = BatchedRolloutStep(vae, world["m"], E, io=io)
            lo = 64 - E if io == "device" else 0                       # the two io modes see different frames of the set
            f, ms, nz, z_o = frames[lo:lo + E], meas[lo:lo + E], noise[lo:lo + E], z_all[lo:lo + E]
            for greedy in (False, True):
                a_o, v_o, _ = world["orc"].predict(z_o, ms, nz, greedy)
                check_against_oracle(step(f, ms, greedy=greedy, noise=nz), z_o, a_o, v_o, ms, (precision, io, E, greedy))


def test_rows_match_the_oracle_at_one_and_three_actions(world, tmp_path):
    """The rollout heads at action counts other than the reference's 2 (rollout_head_kernel<2> with A = 1, the <8> forms with A = 3): a policy on action spaces of
    1 and of 3 actions (bounds and logstd per action: tests/ppo_shape_cases.py; N(0, 0.05) biases), the batched step at E in {1, 9}, sampled and greedy, and one
    single-frame RolloutStep call, against OraclePPO.predict per row with the tolerances of the test above."""
    import ppo_shape_cases as pc
    from oracle import ppo_oracle as po
    from ppo import PPO
    from rollout import BatchedRolloutStep, RolloutStep
    hp = dict(learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0)
    for n_act in (1, 3):
        space = po.ActionSpace(*pc.bounds(n_act))
        o = po.OraclePPO([Z + K], space, seed=4, **hp)
        rng = np.random.RandomState(41 + n_act)
        for k in o.params:
            if k.endswith("bias"):
                o.params[k] = (0.05 * rng.standard_normal(o.params[k].shape)).astype(np.float32)
        o.params["policy/action_logstd"] = pc.logstd_of(n_act)
        m = PPO(np.array([Z + K]), space, model_dir=str(tmp_path / ("ppo_%d" % n_act)), seed=4, **hp)
        m.set_weights(o.params)
        m.init_session(init_logging=False)
        assert m.num_actions == n_act and m.dev.fused_ok()
        orc = Oracle(world["vparams"], o)
        frames, meas, noise = inputs(rng, 9, n_act)
        noise *= 2.0                                                   # some samples leave the bounds on each side
        z_all = orc.latents(frames)
        clamped = np.zeros(2, bool)
        for E in (1, 9):
            step = BatchedRolloutStep(world["vae"], m, E)
            for greedy in (False, True):
                a_o, v_o, _ = orc.predict(z_all[:E], meas[:E], noise[:E], greedy)
                check_against_oracle(step(frames[:E], meas[:E], greedy=greedy, noise=noise[:E]), z_all[:E], a_o, v_o, meas[:E], (n_act, E, greedy), n_act)
                if not greedy:
                    clamped |= [(a_o == space.low).any(), (a_o == space.high).any()]
        assert clamped.all(), (n_act, clamped)
        one = RolloutStep(world["vae"], m)
        for greedy in (False, True):
            a_o, v_o, _ = orc.predict(z_all[3:4], meas[3:4], noise[3:4], greedy)
            a, v, state = one(frames[3], meas[3], greedy=greedy, noise=noise[3])
            check_against_oracle((a[None], np.float32([v]), state[None]), z_all[3:4], a_o, v_o, meas[3:4], (n_act, "single", greedy), n_act)


def test_rows_match_the_single_frame_path(world):
    from rollout import BatchedRolloutStep, RolloutStep
    rng = np.random.RandomState(34)
    frames, meas, noise = inputs(rng, 33)
    one, many = RolloutStep(world["vae"], world["m"]), BatchedRolloutStep(world["vae"], world["m"], 33)
    for greedy in (False, True):
        a, v, s = many(frames, meas, greedy=greedy, noise=noise)
        for e in range(33):
            a1, v1, s1 = one(frames[e], meas[e], greedy=greedy, noise=noise[e])
            assert np.allclose(a[e], a1, rtol=1e-5, atol=1e-5) and float(v[e]) == pytest.approx(v1, rel=1e-5, abs=1e-5), (greedy, e)
            assert np.allclose(s[e], s1, rtol=1e-5, atol=1e-5) and np.array_equal(s[e, Z:], s1[Z:]), (greedy, e)


def test_rows_are_independent(world):
    """A permutation of the environments permutes the rows; a shorter call gives the first rows of the full call; rows >= n of the output buffer are not written."""
    from rollout import BatchedRolloutStep
    rng = np.random.RandomState(35)
    frames, meas, noise = inputs(rng, 40)
    for io in ("pinned", "device"):
        step = BatchedRolloutStep(world["vae"], world["m"], 40, io=io)
        full = step(frames, meas, noise=noise)
        perm = rng.permutation(40)
        got = step(frames[perm], meas[perm], noise=noise[perm])
        assert close(got, [x[perm] for x in full]), io
        for n in (1, 7, 32, 39):
            step.h_out.fill_(-777.0)
            if step.d_out is not None:
                step.d_out.fill_(-777.0)
            part = step(frames[:n], meas[:n], noise=noise[:n])
            assert close(part, [x[:n] for x in full]), (io, n)
            assert np.all(step.h_out.numpy()[n * step.row:] == -777.0), (io, n)
            if step.d_out is not None:
                assert bool((step.d_out[n * step.row:] == -777.0).all()), (io, n)
            assert not np.any(step.h_out.numpy()[:n * step.row] == -777.0), (io, n)


def test_repeated_calls_give_each_call_its_own_answer(world):
    """The raw sums of the split-K layers are cleared by every call: a stale sum of the call before would show in the second and third answers."""
    from rollout import BatchedRolloutStep
    rng = np.random.RandomState(36)
    step = BatchedRolloutStep(world["vae"], world["m"], 8)
    for call, n in enumerate((8, 8, 3, 8)):
        frames, meas, noise = inputs(rng, n)
        z_o = world["orc"].latents(frames)
        a_o, v_o, _ = world["orc"].predict(z_o, meas, noise, False)
        check_against_oracle(step(frames, meas, noise=noise), z_o, a_o, v_o, meas, ("call", call))


def test_between_training_steps(world, tmp_path):
    """The step shares the PPO engine's f_h1 / f_h2 regions with training: one SGD step between two calls changes the actions, and the second call matches the
    oracle evaluated with the parameters the device holds after that step."""
    from rollout import BatchedRolloutStep
    o, m = make_pair(tmp_path / "ppo_train", learning_rate=1e-2)
    orc = Oracle(world["vparams"], o)
    rng = np.random.RandomState(37)
    frames, meas, noise = inputs(rng, 6)
    z_o = orc.latents(frames)
    step = BatchedRolloutStep(world["vae"], m, 6)
    a_o, v_o, states = orc.predict(z_o, meas, noise, True)
    first = step(frames, meas, greedy=True)
    check_against_oracle(first, z_o, a_o, v_o, meas, "before")
    m.update_old_policy()
    m.train(states.astype(np.float32), rng.uniform(-1, 1, (6, A)).astype(np.float32), rng.randn(6).astype(np.float32), rng.randn(6).astype(np.float32))
    for k, val in m.dev.export_params().items():
        o.params[k] = np.array(val, np.float32)
    a_o2, v_o2, _ = orc.predict(z_o, meas, noise, True)
    assert np.abs(a_o2 - a_o).max() > 1e-3                              # the step moved the policy
    second = step(frames, meas, greedy=True)
    check_against_oracle(second, z_o, a_o2, v_o2, meas, "after")
    assert np.abs(second[0] - first[0]).max() > 1e-3


def test_after_the_engine_grows_and_above_the_maximum(world, tmp_path):
    """num_envs above the PPO engine's default max_batch of 256: ensure_batch has recreated the engine by the first call, which must use the new handle."""
    import rollout
    o, m = make_pair(tmp_path / "ppo_grow")
    assert m.dev.max_batch == 256
    old = m.dev.handle
    step = rollout.BatchedRolloutStep(world["vae"], m, 300)
    assert m.dev.max_batch >= 300 and m.dev.handle is not None
    rng = np.random.RandomState(38)
    frames, meas, noise = inputs(rng, 300)
    a, v, s = step(frames, meas, noise=noise)
    orc = Oracle(world["vparams"], o)
    rows = np.array([0, 31, 32, 255, 256, 257, 299])                    # both sides of the old engine's capacity
    z_o = orc.latents(frames[rows])
    a_o, v_o, _ = orc.predict(z_o, meas[rows], noise[rows], False)
    check_against_oracle((a[rows], v[rows], s[rows]), z_o, a_o, v_o, meas[rows], "grown")
    del old
    with pytest.raises(ValueError):
        rollout.BatchedRolloutStep(world["vae"], m, rollout.MAX_ENVS + 1)
    with pytest.raises(ValueError):
        rollout.BatchedRolloutStep(world["vae"], m, 0)


def test_misuse_is_refused_on_the_host(world, tmp_path):
    import torch
    from mi355 import lib as milib
    from rollout import BatchedRolloutStep
    rng = np.random.RandomState(39)
    frames, meas, noise = inputs(rng, 5)
    step = BatchedRolloutStep(world["vae"], world["m"], 4)
    step.h_out.fill_(-777.0)
    for bad in (lambda: step(frames[:0], meas[:0]),                                  # n = 0
                lambda: step(frames, meas),                                          # n > num_envs
                lambda: step(frames[:4].astype(np.float32) / 255.0, meas[:4]),       # float frames
                lambda: step(frames[:4, :40], meas[:4]),                             # wrong frame size
                lambda: step(frames[:4], meas[:4, :2]),                              # wrong measurement shape
                lambda: step(frames[:4], meas[:3]),
                lambda: step(frames[:4], meas[:4], noise=noise[:4, :1])):            # wrong noise shape
        with pytest.raises(ValueError):
            bad()
    # the raw C call: a short scratch buffer, n outside the range, n above the PPO engine's max_batch, a measurement count that does not fit the policy
    L, vae, m = milib.get(), world["vae"], world["m"]
    st = torch.cuda.current_stream().cuda_stream
    base = step.h_in.data_ptr()
    fptr = base + step._f_off

    def raw(n_meas=K, n=4, scratch_bytes=step.scratch_bytes, ppo=m):
        return L.cdll.mi_rollout_step_batch(vae.dev.handle, ppo.dev.handle, st, base, fptr, n_meas, None, 1, n, step.scratch.data_ptr(), scratch_bytes, step.h_out.data_ptr())

    need = L.mi_rollout_batch_workspace_bytes(vae.dev.handle, m.dev.handle, 4)
    assert need == step.scratch_bytes == 4 * 4 * (39 * 79 * 32 + 18 * 38 * 64 + 8 * 18 * 128 + 3 * 8 * 256 + Z)
    assert raw(scratch_bytes=need - 1) == -1 and b"scratch" in L.cdll.mi_last_error()
    assert raw(n=0) == -1 and raw(n=-3) == -1 and raw(n=1025) == -1
    assert raw(n_meas=2) == -2 and b"input size" in L.cdll.mi_last_error()
    assert L.cdll.mi_rollout_batch_workspace_bytes(vae.dev.handle, m.dev.handle, 0) == -1
    o2, small = make_pair(tmp_path / "ppo_small")
    assert small.dev.max_batch == 256
    big = torch.empty(int(L.mi_rollout_batch_workspace_bytes(vae.dev.handle, small.dev.handle, 257)), dtype=torch.uint8, device="cuda")
    rc = L.cdll.mi_rollout_step_batch(vae.dev.handle, small.dev.handle, st, base, fptr, K, None, 1, 257, big.data_ptr(), big.numel(), step.h_out.data_ptr())
    assert rc == -1 and b"max_batch" in L.cdll.mi_last_error()
    o3, other = make_pair(tmp_path / "ppo_68", input_dim=68)                          # z_dim + k != input_dim through the class: k = 4 measurements are expected ...
    step4 = BatchedRolloutStep(vae, other, 2)
    assert step4.n_meas == 4
    with pytest.raises(ValueError):
        step4(frames[:2], meas[:2])                                                  # ... so [2, 3] is refused
    torch.cuda.synchronize()
    assert np.all(step.h_out.numpy() == -777.0)                                      # nothing was launched by any of the refused calls


def test_noise_stream_is_that_of_the_single_frame_path(world):
    from rollout import BatchedRolloutStep, RolloutStep
    rng = np.random.RandomState(40)
    frames, meas, _ = inputs(rng, 3)
    one, many = RolloutStep(world["vae"], world["m"], seed=11), BatchedRolloutStep(world["vae"], world["m"], 1, seed=11)
    for e in range(3):
        a1, v1, s1 = one(frames[e], meas[e])
        a, v, s = many(frames[e:e + 1], meas[e:e + 1])
        assert np.allclose(a[0], a1, rtol=1e-5, atol=1e-5) and float(v[0]) == pytest.approx(v1, rel=1e-5, abs=1e-5), e
    greedy = many(frames[:1], meas[:1], greedy=True)[0]
    assert np.abs(a - greedy).max() > 1e-4                               # the sampled action is not the mean
