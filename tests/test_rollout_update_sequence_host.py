"""CPU-only characterisation of RolloutBuffer.update / update_with_diagnostics: WHICH entries an update calls and in what order, for every setting alone and for all
of them together.  _update runs end to end on CPU tensors: the buffer is built without __init__, the library is a stub that records (entry name, number of arguments)
and returns 0, and the policy is a stub whose _step_rows / update_old_policy / logp_old / update_stats / value_clip_stats record what they were handed.  Pinned per
case: the ordered call log, the result keys, the keys of every dict of `epochs`, the stage_times keys, train_step_counter, where the legacy numpy stream is left, and
that an update without stage_times never calls torch.cuda.synchronize."""
import types

import numpy as np
import pytest

E, T, EPOCHS, BATCH = 3, 4, 2, 5                                                     # 12 samples: minibatches of 5, 5 and 2
N, N_ROWS = E * T, E * (T + 1)
KL = 0.1                                                                             # the approx_kl the stub statistics pass reports for every epoch


class StubLib:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        if not name.startswith("mi_"):
            raise AttributeError(name)

        def entry(*args):
            self.log.append((name, len(args)))
            return 0
        return entry


class StubDev:
    def __init__(self, log):
        import torch
        self.log = log
        self.losses, self.grad_clip = torch.arange(5, dtype=torch.float32), torch.tensor([2.0, 0.25, 0.5, 0.0])

    def fused_ok(self):
        return True

    def logp_old(self, states, actions, M, out):
        self.log.append(("logp_old", M))

    def stats_scratch_doubles(self, M):
        return 1

    def value_clip_scratch_doubles(self, M):
        return 1

    def _sums(self, stats, sums, accumulate):
        import torch
        sums = torch.tensor(sums, dtype=torch.float64)
        stats.copy_(stats + sums if accumulate else sums)

    def update_stats(self, states, actions, returns, logp_old, row_idx, M, stats, scratch, accumulate=False, logp_new_out=None, value_out=None):
        self.log.append(("update_stats", M, accumulate, value_out is not None))
        self._sums(stats, [M, 0.0, KL * M, 0.0, M, 0.0, M, 0.0, 0.5 * M], accumulate)      # M samples: update_stats_summary raises on a count of 0

    def value_clip_stats(self, values_new, old_values, returns, row_idx, M, clip_range_vf, stats, scratch, accumulate=False):
        self.log.append(("value_clip_stats", M, accumulate))
        self._sums(stats, [M, 0.0, 0.5 * M, 0.0], accumulate)


class StubPpo:
    def __init__(self, log, max_grad_norm, value_clip):
        self.log, self.dev, self.buf = log, StubDev(log), None
        self.max_grad_norm, self.value_clip, self.train_step_counter = max_grad_norm, value_clip, 0

    def _need_dev(self):
        return self.dev

    def update_old_policy(self):
        self.log.append(("update_old_policy",))

    def _step_rows(self, states, actions, returns, advantages, logp_old, rows, m, m_all, **kw):
        self.log.append(("_step_rows", m, tuple(sorted(kw)), advantages is self.buf.advantages))


def make(monkeypatch, continuous, grad_clip=False, value_clip=False, reward_scaling=False, minibatch_norm=False, obs_norm=False):
    """-> (buffer, log, syncs): a full collection is booked, the settings are on, and the log starts empty."""
    import torch
    import rollout
    syncs = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0, synchronize=lambda: None))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: syncs.append(1))
    cls = rollout.ContinuousRolloutBuffer if continuous else rollout.RolloutBuffer
    log = []
    b = object.__new__(cls)
    b.rows, b.L, b.device, b.num_envs, b.horizon, b.n_table_rows = cls._rows_class(E, T), StubLib(log), "cpu", E, T, N_ROWS
    b.states, b.actions = torch.zeros(N_ROWS, 7), torch.zeros(N_ROWS, 2)
    b.values, b.returns, b.advantages, b.logp_old, b.final_values = (torch.zeros(N_ROWS) for _ in range(5))
    b._reward_scaling = b._obs_norm = b.raw_states = None
    b._step = types.SimpleNamespace(z_dim=4, _obs_norm=None)
    b.ppo = StubPpo(log, 0.5 if grad_clip else None, 0.2 if value_clip else None)
    b.ppo.buf = b
    if reward_scaling:
        b.set_reward_scaling()
    if minibatch_norm:
        b.set_minibatch_normalization()
    if obs_norm:
        b.set_observation_normalization()                                            # (only with no step recorded)
    rng = np.random.RandomState(5)
    for _ in range(T):
        b.rows.step_rows(None, E)
        b.rows.outcome(rng.uniform(0, 1, E), np.zeros(E, bool))
    if continuous:                                                                   # lane 0's last step is truncated, lanes 1 and 2 are bootstrapped
        b.rows.truncate_rows([0], 1)
        b.rows.bootstrap_rows([1, 2], 2)
    else:
        b.rows.bootstrap_rows(None, E)
    del log[:]
    return b, log, syncs


BASE_KEYS = ["advantages", "bootstrap_values", "lengths", "losses", "raw_advantages", "returns", "samples", "values"]
CONTINUOUS_KEYS = ["final_values", "segment_truncated", "segments"]
DIAG_KEYS = ["epochs", "epochs_run", "stopped_early"]
SETTING_KEYS = dict(grad_clip=["clip_scales", "grad_norms"], value_clip=[],
                    reward_scaling=["discounted_returns", "return_carry", "return_rms", "reward_clip_fraction", "reward_scale_den", "scaled_rewards"],
                    minibatch_norm=["minibatch_adv_stats", "minibatch_advantages"], obs_norm=["observation_clip_fraction", "observation_rms"])
EPOCH_KEYS = ["approx_kl", "approx_kl_k1", "clip_fraction", "explained_variance", "ratio_mean", "samples", "value_mse"]
EPOCH_SETTING_KEYS = dict(grad_clip=["clipped_steps", "grad_norm_max"], value_clip=["value_clip_fraction", "value_grad_zero_fraction", "value_loss_clipped"])
SETTING_STAGES = dict(reward_scaling="reward_scaling", minibatch_norm="minibatch_norm", obs_norm="observation_stats")


def expected_log(continuous, on, diag, epochs_run):
    """The sequence as it was observed on the tree this test was written against, spelled out from its parts."""
    finish = ("mi_rollout_finish_segments_boot", 20) if continuous else ("mi_rollout_finish", 14)
    log = [("mi_rollout_scale_rewards", 16)] if "reward_scaling" in on else []
    log += [finish, ("update_old_policy",), ("logp_old", N_ROWS)]
    kw = ("old_values_all",) if "value_clip" in on else ()
    for _ in range(epochs_run):
        if "minibatch_norm" in on:
            log.append(("mi_ppo_minibatch_advantages", 10))
        log += [("_step_rows", m, kw, "minibatch_norm" not in on) for m in (5, 5, 2)]
        if diag:
            log.append(("update_stats", N, False, "value_clip" in on))
            if "value_clip" in on:
                log.append(("value_clip_stats", N, False))
    if "obs_norm" in on:
        log += [("mi_rollout_obs_stats_scratch_doubles", 2), ("mi_rollout_obs_stats", 15)]
    return log


def numpy_stream_after(shuffles):
    np.random.seed(0)
    for _ in range(shuffles):
        np.random.shuffle(np.arange(N))
    return np.random.get_state()


def same_stream(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


ALL = ("grad_clip", "value_clip", "reward_scaling", "minibatch_norm", "obs_norm")
CASES = [((), None)] + [((s,), None) for s in ALL] + [(ALL, 0.5), ((), 0.5 * KL)]      # (settings on, target_kl: None = update());  the last one stops behind epoch 1


@pytest.mark.parametrize("on,target_kl", CASES, ids=["off"] + list(ALL) + ["all_with_diagnostics", "kl_stop"])
@pytest.mark.parametrize("continuous", [False, True], ids=["RolloutBuffer", "ContinuousRolloutBuffer"])
def test_the_calls_of_an_update_in_order(monkeypatch, continuous, on, target_kl):
    diag = target_kl is not None
    epochs_run = 1 if diag and target_kl < KL else EPOCHS
    want_log = expected_log(continuous, on, diag, epochs_run)
    want_keys = sorted(BASE_KEYS + (CONTINUOUS_KEYS if continuous else []) + (DIAG_KEYS if diag else []) + sum((SETTING_KEYS[s] for s in on), []))
    want_stages = {"finish", "logp_old", "sgd"} | ({"stats"} if diag else set()) | {SETTING_STAGES[s] for s in on if s in SETTING_STAGES}
    for timed in (False, True):
        b, log, syncs = make(monkeypatch, continuous, **{s: True for s in on})
        stage_times = {} if timed else None
        np.random.seed(0)
        if diag:
            out = b.update_with_diagnostics(num_epochs=EPOCHS, batch_size=BATCH, stage_times=stage_times, target_kl=target_kl)
        else:
            out = b.update(num_epochs=EPOCHS, batch_size=BATCH, stage_times=stage_times)
        assert log == want_log, timed
        assert sorted(out) == want_keys, timed
        assert b.ppo.train_step_counter == 3 * epochs_run and len(out["losses"]) == 3 * epochs_run and out["samples"] == N
        assert same_stream(np.random.get_state(), numpy_stream_after(epochs_run))   # one shuffle of arange(12) per epoch that ran, nothing else
        if diag:
            assert out["epochs_run"] == epochs_run and out["stopped_early"] == (epochs_run < EPOCHS) and len(out["epochs"]) == epochs_run
            for e in out["epochs"]:
                assert sorted(e) == sorted(EPOCH_KEYS + sum((EPOCH_SETTING_KEYS.get(s, []) for s in on), [])), e
                assert e["samples"] == N and e["approx_kl"] == pytest.approx(KL)
        if "grad_clip" in on:
            assert out["grad_norms"].tolist() == [2.0] * (3 * epochs_run) and out["clip_scales"].tolist() == [0.25] * (3 * epochs_run)
        if "minibatch_norm" in on:
            assert out["minibatch_adv_stats"].shape == (3 * epochs_run, 3) and out["minibatch_advantages"].shape == (E, T)
        if timed:
            assert set(stage_times) == want_stages and all(v >= 0 for v in stage_times.values()) and syncs
            order = [k for k in ("reward_scaling", "finish", "logp_old", "minibatch_norm", "sgd", "stats", "observation_stats") if k in want_stages]
            assert list(stage_times) == order                                        # the tools print the stages in the order they were first marked
        else:
            assert not syncs                                                         # without stage_times the update never waits for the device
