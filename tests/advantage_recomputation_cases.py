"""Cases and references of the advantage-recomputation tests (test infrastructure; used by test_advantage_recomputation_host.py and
test_zzzzzzzzzzzzz_advantage_recomputation_gpu.py).  Nothing here calls rollout.py, ppo.py or the library.

1. The value pass (mi_ppo_values_idx).  POLICIES names the three policies of the GPU check -- 2 actions on the reference trunk (67 -> 500 / 300), 3 actions on
   5 -> 36 / 20 (H2 = 20 is no multiple of the head kernels' 8 parts), and 131 inputs on the reference trunk (the wide layer-1 form) -- and ROW_COUNTS its row counts.
   value64() is this module's own float64 value net (numpy; test_advantage_recomputation_host.py holds it to oracle.ppo_oracle.policy_forward at 1e-12), value32() its
   fp32 twin (every product and sum rounded to fp32 by numpy).  BOUND: rel 1e-4 / abs 1e-5, the project's bound for values everywhere else; distance() is a value's
   error in units of it.  The host test asserts that the twin stays inside it at every case, so a device value outside it says something about the device.

2. The update with a refresh.  update_reference() is a float64 PPO update from state tables -- the first finish from the RECORDED values, log pi_old once, epochs of
   shuffled minibatches (oracle.ppo_oracle.ppo_losses, autograd, tf.train.AdamOptimizer's arithmetic), and before every epoch but the first a refresh: the value net
   under the current parameters over the recorded rows and the bootstrap slots, then the finish again.  Its case (refresh_case) records values that are NOT the value
   net's own (V(s) + 0.05 N(0, 1), as a collection whose policy has moved since): only then does it matter which table epoch 1 reads.  MUTANTS are three wrong updates
   -- a refresh before epoch 1 as well, no refresh at all, bootstrap slots left at their recorded values -- and mutant_distance() is the largest distance, in units of
   BOUND, between a mutant's and the reference's `returns` (the first finish), `refreshed_values` and `refreshed_returns`: the host test asserts >= 10 for each."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import ppo_oracle as po

REL, ABS = 1e-4, 1e-5
POLICIES = OrderedDict([("ref2", (67, 2, (500, 300), 0)), ("small3", (5, 3, (36, 20), 0)), ("wide2", (131, 2, (500, 300), 1))])      # input_dim, actions, hidden, wide_inputs mode
ROW_COUNTS = (1, 5, 32, 33, 257)
EPS, VALUE_SCALE, ENTROPY_SCALE = 0.2, 1.0, 0.01
MUTANTS = ("refresh_before_epoch_1", "no_refresh", "stale_bootstrap_slots")
VALUE_NET = ("policy/dense_2/kernel", "policy/dense_2/bias", "policy/dense_3/kernel", "policy/dense_3/bias", "policy/value/kernel", "policy/value/bias")


def bounds(A):
    a = np.arange(A)
    return (-1.0 - 0.25 * a).astype(np.float32), (0.5 + 0.5 * (a % 3)).astype(np.float32)


def parameters(input_dim, A, hidden, seed=3):
    """mi355.init.init_ppo with N(0, 0.05) biases (the value bias among them) and every action its own log-std."""
    from mi355.init import init_ppo
    rng = np.random.RandomState(100 + seed)
    p = init_ppo(seed, input_dim, A, 1.0, hidden=hidden)
    for k in p:
        if k.endswith("bias"):
            p[k] = (0.05 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p["policy/action_logstd"] = (-0.5 + 0.07 * np.arange(A)).astype(np.float32)
    return p


_POLICY = {}


def policy(name):
    """-> dict(input_dim, A, hidden, wide, low, high, theta) of POLICIES[name], built once and not to be modified."""
    if name not in _POLICY:
        din, A, hidden, wide = POLICIES[name]
        low, high = bounds(A)
        _POLICY[name] = dict(input_dim=din, A=A, hidden=hidden, wide=wide, low=low, high=high, theta=parameters(din, A, hidden))
    return _POLICY[name]


def states(name, n, seed=0):
    """0.5 x N(0, 1) state rows, float32 [n, input_dim]."""
    return (0.5 * np.random.RandomState(7000 + 13 * n + seed).standard_normal((n, POLICIES[name][0]))).astype(np.float32)


def value64(theta, s):
    """V(s) in float64 from float32 parameters and states: relu(relu(s W1 + b1) W2 + b2) Wv + bv."""
    f = lambda k: np.asarray(theta[k], np.float32).astype(np.float64)      # noqa: E731
    h = np.maximum(np.asarray(s, np.float32).astype(np.float64) @ f(VALUE_NET[0]) + f(VALUE_NET[1]), 0.0)
    h = np.maximum(h @ f(VALUE_NET[2]) + f(VALUE_NET[3]), 0.0)
    return (h @ f(VALUE_NET[4]) + f(VALUE_NET[5])).reshape(-1)


def value32(theta, s):
    """The same net with every operation in float32."""
    f = lambda k: np.asarray(theta[k], np.float32)      # noqa: E731
    h = np.maximum(np.asarray(s, np.float32) @ f(VALUE_NET[0]) + f(VALUE_NET[1]), np.float32(0))
    h = np.maximum(h @ f(VALUE_NET[2]) + f(VALUE_NET[3]), np.float32(0))
    out = (h @ f(VALUE_NET[4]) + f(VALUE_NET[5])).reshape(-1)
    assert out.dtype == np.float32
    return out


def distance(got, ref):
    """max |got - ref| / (ABS + REL |ref|): <= 1 is inside BOUND.  NaN in the same places counts as equal; elsewhere it is infinitely far."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    return float((np.abs(got - ref)[ok] / (ABS + REL * np.abs(ref[ok]))).max()) if ok.any() else 0.0


# ---- the update with a refresh, float64 ----
def refresh_case(E=3, T=5, seed=4):
    """A RolloutBuffer-shaped collection on policy "small3": ragged lanes (lane 0 full, lane 1 ends in a done at T - 2, lane 2 stops at T - 1 without one), states
    [E, T + 1, din] whose slot lengths[e] is the bootstrap state, the policy's own sampled actions, rewards, and RECORDED values V(s) + 0.05 N(0, 1)."""
    pol = policy("small3")
    rng = np.random.RandomState(seed)
    lengths = np.array([T, T - 2, T - 1] + [T] * (E - 3), np.int64)[:E]
    dones = np.zeros((E, T))
    dones[1, T - 3] = 1.0
    s = (0.5 * rng.standard_normal((E, T + 1, pol["input_dim"]))).astype(np.float32)
    th = {k: torch.from_numpy(v.astype(np.float64)) for k, v in pol["theta"].items()}
    with torch.no_grad():
        mean, ls, _ = po.policy_forward(th, torch.from_numpy(s.reshape(-1, pol["input_dim"]).astype(np.float64)), pol["low"], pol["high"])
    act = mean.numpy() + np.exp(ls.numpy()) * rng.standard_normal(mean.shape)
    a = np.clip(act, pol["low"], pol["high"]).astype(np.float32).reshape(E, T + 1, pol["A"])
    values = (value64(pol["theta"], s.reshape(-1, pol["input_dim"])).reshape(E, T + 1) + 0.05 * rng.standard_normal((E, T + 1))).astype(np.float32)
    return dict(policy=pol, E=E, T=T, lengths=lengths, dones=dones, rewards=rng.uniform(0, 1, (E, T)), states=s, actions=a, values=values)


def finish64(case, values, gamma, lam):
    """Per lane compute_gae + returns + normalised advantages from a values table [E, T + 1] -> (raw, returns, advantages), float64 [E, T], NaN beyond a lane."""
    E, T = case["E"], case["T"]
    raw, ret, adv = (np.full((E, T), np.nan) for _ in range(3))
    for e in range(E):
        n = int(case["lengths"][e])
        if n:
            v = np.asarray(values[e], np.float64)
            raw[e, :n] = po.compute_gae(case["rewards"][e, :n], v[:n], v[n], case["dones"][e, :n], gamma, lam)
            ret[e, :n], adv[e, :n] = po.returns_and_normalized_advantages(raw[e, :n], v[:n])
    return raw, ret, adv


def update_reference(case, num_epochs=3, batch_size=4, gamma=0.99, lam=0.95, lr=1e-3, seed=5, mutant=None):
    """The float64 update with a refresh (module docstring) -> dict(returns, advantages: the first finish; refreshed_values, refreshed_returns, refreshed_advantages:
    the last refresh; recomputed_epochs; params).  mutant: None or one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    pol, E, T = case["policy"], case["E"], case["T"]
    din, A = pol["input_dim"], pol["A"]
    rec = np.arange(T)[None, :] < case["lengths"][:, None]
    t64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))      # noqa: E731
    p = OrderedDict((k, t64(v.astype(np.float64)).requires_grad_(True)) for k, v in pol["theta"].items())
    p_old = {k.replace("policy/", "policy_old/", 1): v.detach().clone() for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    s_all, a_all = case["states"][:, :T][rec].astype(np.float64), case["actions"][:, :T][rec].astype(np.float64)
    values_now = case["values"].astype(np.float64).copy()
    raw, ret, adv = finish64(case, values_now, gamma, lam)
    out = dict(returns=ret, advantages=adv, recomputed_epochs=0)
    b1p, b2p = 0.9, 0.999
    rng = np.random.RandomState(seed)
    for epoch in range(num_epochs):
        if mutant != "no_refresh" and (epoch > 0 or mutant == "refresh_before_epoch_1"):
            now = value64({k: v.detach().numpy() for k, v in p.items()}, case["states"].reshape(-1, din)).reshape(E, T + 1)
            slots = np.arange(T + 1)[None, :] <= case["lengths"][:, None]              # the recorded rows and the bootstrap slot
            if mutant == "stale_bootstrap_slots":
                slots = np.arange(T + 1)[None, :] < case["lengths"][:, None]
            values_now = np.where(slots, now, values_now)
            raw, ret, adv = finish64(case, values_now, gamma, lam)
            if epoch == 0:
                out["returns"], out["advantages"] = ret, adv
            out.update(refreshed_values=np.where(rec, values_now[:, :T], np.nan), refreshed_returns=ret, refreshed_advantages=adv, refreshed_raw_advantages=raw)
            out["recomputed_epochs"] += 1
        R, Ad = ret[rec], adv[rec]
        idx = np.arange(len(R))
        rng.shuffle(idx)
        for i in range(0, len(idx), batch_size):
            mb = idx[i:i + batch_size]
            for q in p.values():
                q.grad = None
            L = po.ppo_losses(p, p_old, t64(s_all[mb]), t64(a_all[mb]), t64(R[mb]), t64(Ad[mb]), pol["low"], pol["high"], EPS, VALUE_SCALE, ENTROPY_SCALE)
            L["loss"].backward()
            alpha = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
            with torch.no_grad():
                for k, q in p.items():
                    g = q.grad if q.grad is not None else torch.zeros_like(q)
                    m[k] += (g - m[k]) * 0.1
                    v2[k] += (g * g - v2[k]) * 0.001
                    q -= alpha * m[k] / (torch.sqrt(v2[k]) + 1e-8)
            b1p, b2p = b1p * 0.9, b2p * 0.999
    out["params"] = OrderedDict((k, v.detach().numpy().copy()) for k, v in p.items())
    return out


def mutant_distance(ref, mut):
    """The largest distance, in units of BOUND, over the quantities the value bound is asked of: the first finish's returns, and the last refresh's values and
    returns.  A quantity the mutant does not have at all (no refresh ran) is infinitely far."""
    return max(distance(mut.get(k, np.zeros(0)), ref[k]) for k in ("returns", "refreshed_values", "refreshed_returns"))
