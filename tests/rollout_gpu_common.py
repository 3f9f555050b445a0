"""Shared helpers of the GPU rollout tests (test_l_rollout_batch_gpu.py, test_m_rollout_buffer_gpu.py, test_n_rollout_segments_gpu.py): the set-up of
test_c_c3_ppo_gpu.py::test_rollout_step_one_call_matches_encode_then_predict (oracle VAE with N(0, 0.05) biases, an oracle / device policy pair with the same weights,
random camera bytes), the per-row oracle, and the comparisons.  Tolerances: against the oracle latents 1e-4 relative, actions rtol 1e-4 / atol 1e-5, value rel 1e-4 /
abs 1e-5; 1e-5 between the device paths (both end in fp32 atomics, so bit equality is not asked); the update's losses at test_e_c5_replay_gpu.py's.  Also the
comparisons of the twin tests (test_p .. test_v): bitwise tensors, a policy's flat state, two updates' results."""
import numpy as np
import pytest

from oracle import ppo_oracle as po
from oracle import vae_oracle as vo
from ppo import PPO

Z, K, A = 64, 3, 2
SENTINEL = -777.0


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def make_pair(tmp_path, seed=2, input_dim=67, precision=None, **kw):
    space = po.ActionSpace()
    hp = dict(learning_rate=1e-4, lr_decay=1.0, epsilon=0.2, value_scale=1.0, entropy_scale=0.01, initial_std=1.0)
    hp.update(kw)
    o = po.OraclePPO([input_dim], space, seed=seed, **hp)
    extra = {} if precision is None else dict(precision=precision)
    m = PPO(np.array([input_dim]), space, model_dir=str(tmp_path), seed=seed, **extra, **hp)
    m.set_weights(o.params)
    m.init_session(init_logging=False)
    return o, m


def vae_params():
    rng = np.random.RandomState(21)
    vparams = vo.init_vae_params(3)
    for k in vparams:
        if k.endswith("bias"):
            vparams[k] = (0.05 * rng.standard_normal(vparams[k].shape)).astype(np.float32)
    return vparams


def make_vae(tmp_path, vparams, precision="fp32"):
    from vae.models import ConvVAE
    vae = ConvVAE(np.array([80, 160, 3]), z_dim=Z, model_dir=str(tmp_path), precision=precision, training=False)
    vae.set_weights(vparams)
    vae.init_session(init_logging=False)
    return vae


def inputs(rng, n, n_act=A):
    frames = rng.randint(0, 256, (n, 80, 160, 3), dtype=np.uint8)
    meas = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 30, n)], axis=1)
    noise = rng.standard_normal((n, n_act)).astype(np.float32)
    return frames, meas, noise


class Oracle:
    """encode -> np.append -> predict of every row; the latents of a frame set are computed once."""

    def __init__(self, vparams, o):
        self.ovae, self.o = vo.OracleVAE(params=vparams, training=False), o

    def latents(self, frames):
        return np.concatenate([self.ovae.encode(frames[i:i + 16].astype(np.float32) / 255.0) for i in range(0, len(frames), 16)])

    def predict(self, z, meas, noise, greedy):
        states = np.stack([np.append(z[e], meas[e]) for e in range(len(z))])
        a, v = self.o.predict(states, greedy=greedy, noise=None if greedy else noise)
        return np.asarray(a).reshape(len(z), self.o.num_actions), np.asarray(v).reshape(len(z)), states


def make_world(tmp_path_factory, name, policy=True):
    """What a test module's `world` fixture holds: the fp32 VAE and its parameters, and with `policy` the oracle / device policy pair and the per-row oracle."""
    tmp = tmp_path_factory.mktemp(name)
    vparams = vae_params()
    w = dict(tmp=tmp, vparams=vparams)
    if policy:
        w["o"], w["m"] = make_pair(tmp / "ppo")
    w["vae"] = make_vae(tmp / "vae_fp32", vparams)
    if policy:
        w["orc"] = Oracle(vparams, w["o"])
    return w


def check_against_oracle(got, z_o, a_o, v_o, meas, tag, n_act=A):
    a, v, states = got
    n = len(z_o)
    assert a.shape == (n, n_act) and a.dtype == np.float32 and v.shape == (n,) and v.dtype == np.float32, tag
    assert states.shape == (n, Z + K) and states.dtype == np.float64, tag
    assert np.array_equal(states[:, Z:], np.asarray(meas, np.float64)), tag
    for e in range(n):
        err = rel_err(states[e, :Z], z_o[e])
        assert err < 1e-4, (tag, e, err)
        assert np.allclose(a[e], a_o[e], rtol=1e-4, atol=1e-5), (tag, e, a[e], a_o[e])
        assert float(v[e]) == pytest.approx(float(v_o[e]), rel=1e-4, abs=1e-5), (tag, e)


def close(x, y, tol=1e-5):
    return all(np.allclose(p, q, rtol=tol, atol=tol) for p, q in zip(x, y))


def fill_tables(buf, value=SENTINEL):
    for t in (buf.states, buf.actions, buf.values, buf.returns, buf.advantages, buf.logp_old):
        t.fill_(value)


def tables(buf):
    return buf.states.cpu().numpy(), buf.actions.cpu().numpy(), buf.values.cpu().numpy()


def check_recorded(tabs, before, rows, got, meas, tag):
    """Table rows `rows` hold, bitwise, what the call returned; every other row is what it was before the call."""
    s, a, v = tabs
    actions, values, states = got
    assert np.array_equal(s[rows, :Z], states[:, :Z].astype(np.float32)), tag        # the returned float64 latents are exact widenings of the fp32 the kernel stored
    assert np.array_equal(s[rows, Z:], np.asarray(meas, np.float32)), tag
    assert np.array_equal(a[rows], actions) and np.array_equal(v[rows], values), tag
    other = np.ones(len(v), bool)
    other[rows] = False
    for now, was in zip(tabs, before):
        assert np.array_equal(now[other], was[other]), tag


def check_losses(got, want, tag):
    """test_e_c5_replay_gpu.py's tolerances; `want` has the oracle's keys or the device's."""
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["loss"] == pytest.approx(w["loss"], rel=1e-4, abs=1e-4), (tag, i, g, w)
        assert g["value_loss"] == pytest.approx(w["value_loss"], rel=1e-4), (tag, i, g, w)
        assert g["policy_loss"] == pytest.approx(w["policy_loss"], abs=1e-4), (tag, i, g, w)
        assert g["prob_ratio"] == pytest.approx(w["ratio_mean"] if "ratio_mean" in w else w["prob_ratio"], rel=1e-4), (tag, i, g, w)


def bitwise(x, y):
    """Two tensors, or two lists of tensors, hold the same bits."""
    import torch
    x, y = (x, y) if isinstance(x, (list, tuple)) else ([x], [y])
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x, y))


def flat_state(m):
    return [m.dev.params.clone(), m.dev.adam_m.clone(), m.dev.adam_v.clone(), m.dev.params_old.clone()]


def same_update(a, b, keys=("returns", "advantages", "raw_advantages", "values", "bootstrap_values", "lengths")):
    return a["losses"] == b["losses"] and a["samples"] == b["samples"] and all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)
