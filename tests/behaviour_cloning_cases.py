"""Problems and the float64 reference of behaviour cloning (test infrastructure; used by test_behaviour_cloning_host.py and
test_zzzzzzzzzz_behaviour_cloning_gpu.py).  numpy alone: nothing of ppo.py, rollout.py or mi355/ is imported, so the reference shares no code with what it checks.

The loss, as include/mi355_carla.h defines it.  Per sample m and action a, t = tanh(u), mean = lo + (t + 1) / 2 (hi - lo), sigma = exp(logstd[a]),
z = (a_E - mean) / sigma:
  "nll"  l[m] = sum_a (z^2 / 2 + logstd[a] + log(2 pi) / 2)         "mse"  l[m] = sum_a (mean - a_E)^2
  clone_loss = mean_m l[m] ;  with returns value_loss = value_scale mean_m (V - R)^2 ;  loss = clone_loss + value_loss ;  mean_sq_error = mean_m sum_a (mean - a_E)^2
forward() / loss_and_grads() run in the dtype they are given: float64 is the reference, float32 its twin (the distance between the two is what fp32 arithmetic of
this problem costs; the split-bf16 bound and the trajectory bound are stated in units of it).  The gradients are analytic (backprop by hand) and are checked against
central differences by test_behaviour_cloning_host.py.

Shapes and sizes are those of tests/kl_penalty_cases.py: "A2" is 67 -> 500 / 300 with 2 actions (the <2> instantiation of the head kernel), "A3" is 5 -> 36 / 20
with 3 actions (the <8> instantiation), "W" is the wide case, 131 -> 500 / 300 with 2 actions; M = 5 (one partial loss block), 33 (a second block that holds one
sample) and 257 (the chunked weight-gradient route).  A problem: parameters N(0, 1 / fan_in) kernels, N(0, 0.05) biases, action_logstd = -0.5 + 0.07 a - 0.02 a^2;
bounds low[a] = -1 - 0.25 a, high[a] = 0.5 + 0.5 (a mod 3); states 0.5 N(0, 1), the first M of 4 M draws that are not next to a ReLU kink of either trunk (a
pre-activation within 1e-4 of its layer's largest: across a kink a sample's share of a gradient column switches on or off, which is no arithmetic); the expert is a
TEACHER -- a second parameter set -- whose mean plus 0.3 sigma N(0, 1) is clamped into the bounds; returns are the student's value + N(0, 1).

Bounds (the issue's; the project's existing ones): clone_loss within 1e-4 of mean_m sum_a (z^2 / 2 + |logstd| + log(2 pi) / 2) for "nll" (relative to the absolute
terms: the signed sum may cancel), 1e-4 relative for "mse"; value_loss 1e-4 relative; gradients 2e-4 of each tensor's maximum; parameters after Adam within 2e-6 of
TF-Adam on the device's gradients where |g| > 1e-3 of the tensor's maximum."""
from collections import OrderedDict

import numpy as np

NAMES = ("policy/dense/kernel", "policy/dense/bias", "policy/dense_1/kernel", "policy/dense_1/bias", "policy/action_mean/kernel", "policy/action_mean/bias",
         "policy/action_logstd",
         "policy/dense_2/kernel", "policy/dense_2/bias", "policy/dense_3/kernel", "policy/dense_3/bias", "policy/value/kernel", "policy/value/bias")
POLICY_NET, VALUE_NET = NAMES[:7], NAMES[7:]
KINDS = ("nll", "mse")
SHAPES = OrderedDict([("A2", (67, 2, (500, 300), 3)), ("A3", (5, 3, (36, 20), 11)), ("W", (131, 2, (500, 300), 5))])
MS = (5, 33, 257)
VALUE_SCALE = 0.5
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
LOSS_REL, GRAD_REL, ADAM_ABS, ADAM_GMIN = 1e-4, 2e-4, 2e-6, 1e-3
KINK_TAU = 1e-4
LR, B1, B2, EPS_ADAM = 1e-3, 0.9, 0.999, 1e-8


def bounds(A):
    a = np.arange(A)
    return (-1.0 - 0.25 * a).astype(np.float32), (0.5 + 0.5 * (a % 3)).astype(np.float32)


def init_theta(rng, din, A, hidden):
    h1, h2 = hidden
    a = np.arange(A, dtype=np.float64)
    shapes = ((din, h1), (h1,), (h1, h2), (h2,), (h2, A), (A,), (A,), (din, h1), (h1,), (h1, h2), (h2,), (h2, 1), (1,))
    th = OrderedDict()
    for name, sh in zip(NAMES, shapes):
        if name.endswith("kernel"):
            th[name] = (rng.standard_normal(sh) / np.sqrt(sh[0])).astype(np.float32)
        elif name.endswith("logstd"):
            th[name] = (-0.5 + 0.07 * a - 0.02 * a * a).astype(np.float32)
        else:
            th[name] = (0.05 * rng.standard_normal(sh)).astype(np.float32)
    return th


def forward(theta, s, low, high, dtype=np.float64, value=True):
    """-> dict of the activations in `dtype` (z1 / h1 / z2 / h2 / u / t / mean of the policy, y1 / g1 / y2 / g2 / V of the value net)."""
    th = {k: np.asarray(v, dtype) for k, v in theta.items()}
    lo, hi = np.asarray(low, dtype), np.asarray(high, dtype)
    f = {"s": np.asarray(s, dtype)}
    f["z1"] = f["s"] @ th[NAMES[0]] + th[NAMES[1]]
    f["h1"] = np.maximum(f["z1"], 0)
    f["z2"] = f["h1"] @ th[NAMES[2]] + th[NAMES[3]]
    f["h2"] = np.maximum(f["z2"], 0)
    f["u"] = f["h2"] @ th[NAMES[4]] + th[NAMES[5]]
    f["t"] = np.tanh(f["u"])
    f["mean"] = lo + (f["t"] + 1) / 2 * (hi - lo)
    if value:
        f["y1"] = f["s"] @ th[NAMES[7]] + th[NAMES[8]]
        f["g1"] = np.maximum(f["y1"], 0)
        f["y2"] = f["g1"] @ th[NAMES[9]] + th[NAMES[10]]
        f["g2"] = np.maximum(f["y2"], 0)
        f["V"] = (f["g2"] @ th[NAMES[11]] + th[NAMES[12]]).reshape(-1)
    return f


def loss_and_grads(theta, s, a_e, R, kind, low, high, value_scale=VALUE_SCALE, dtype=np.float64):
    """R None: policy only (the value net's gradients are zeros).  -> (scal: clone_loss, value_loss, loss, mean_sq_error, abs_terms; grads: 13 arrays; mean; V)."""
    assert kind in KINDS
    th = {k: np.asarray(v, dtype) for k, v in theta.items()}
    lo, hi = np.asarray(low, dtype), np.asarray(high, dtype)
    f = forward(theta, s, low, high, dtype, value=R is not None)
    a_e = np.asarray(a_e, dtype)
    M = a_e.shape[0]
    ls = th[NAMES[6]]
    sigma = np.exp(ls)
    diff = f["mean"] - a_e
    z = -diff / sigma
    slope = (hi - lo) / 2 * (1 - f["t"] ** 2)
    if kind == "nll":
        l = (z * z / 2 + ls + dtype(HALF_LOG_2PI)).sum(1)
        du = -(z / sigma) * slope / M
        dls = (1 - z * z).sum(0) / M
    else:
        l = (diff * diff).sum(1)
        du = 2 * diff * slope / M
        dls = np.zeros_like(ls)
    scal = {"clone_loss": float(l.mean()), "value_loss": 0.0, "mean_sq_error": float((diff * diff).sum(1).mean()),
            "abs_terms": float((z * z / 2 + np.abs(ls) + HALF_LOG_2PI).sum(1).mean())}
    g = OrderedDict((k, np.zeros_like(th[k])) for k in NAMES)
    g[NAMES[4]], g[NAMES[5]], g[NAMES[6]] = f["h2"].T @ du, du.sum(0), dls
    dz2 = (du @ th[NAMES[4]].T) * (f["z2"] > 0)
    g[NAMES[2]], g[NAMES[3]] = f["h1"].T @ dz2, dz2.sum(0)
    dz1 = (dz2 @ th[NAMES[2]].T) * (f["z1"] > 0)
    g[NAMES[0]], g[NAMES[1]] = f["s"].T @ dz1, dz1.sum(0)
    if R is not None:
        e = f["V"] - np.asarray(R, dtype)
        scal["value_loss"] = float(value_scale * (e * e).mean())
        dv = (2 * value_scale * e / M).reshape(-1, 1)
        g[NAMES[11]], g[NAMES[12]] = f["g2"].T @ dv, dv.sum(0)
        dy2 = (dv @ th[NAMES[11]].T) * (f["y2"] > 0)
        g[NAMES[9]], g[NAMES[10]] = f["g1"].T @ dy2, dy2.sum(0)
        dy1 = (dy2 @ th[NAMES[9]].T) * (f["y1"] > 0)
        g[NAMES[7]], g[NAMES[8]] = f["s"].T @ dy1, dy1.sum(0)
    scal["loss"] = scal["clone_loss"] + scal["value_loss"]
    return scal, g, f["mean"], f.get("V")


def adam_alpha(lr, step, dtype=np.float64):
    """alpha of tf.train.AdamOptimizer at 1-based step `step`: lr sqrt(1 - b2^t) / (1 - b1^t)."""
    return dtype(lr) * np.sqrt(dtype(1) - dtype(B2) ** step) / (dtype(1) - dtype(B1) ** step)


def adam_tf(p, m, v, g, alpha, dtype=np.float64):
    """TF ApplyAdam on one tensor: m += (g - m)(1 - b1) ; v += (g^2 - v)(1 - b2) ; p -= alpha m / (sqrt(v) + eps).  -> (p, m, v) in `dtype`."""
    p, m, v, g = (np.asarray(x, dtype) for x in (p, m, v, g))
    m = m + (g - m) * dtype(1 - dtype(B1))
    v = v + (g * g - v) * dtype(1 - dtype(B2))
    return p - (m * dtype(alpha)) / (np.sqrt(v) + dtype(EPS_ADAM)), m, v


def near_relu_kink(theta, s, low, high, tau=KINK_TAU):
    f = forward(theta, s, low, high)
    bad = np.zeros(len(s), bool)
    for k in ("z1", "z2", "y1", "y2"):
        bad |= (np.abs(f[k]) < tau * np.abs(f[k]).max()).any(1)
    return bad


class Case:
    pass


def build(shape, M):
    din, A, hidden, seed = SHAPES[shape]
    c = Case()
    c.shape, c.input_dim, c.A, c.hidden, c.M = shape, din, A, tuple(hidden), M
    c.low, c.high = bounds(A)
    rng = np.random.RandomState(1000 * seed + M)
    c.theta = init_theta(rng, din, A, hidden)
    c.teacher = init_theta(rng, din, A, hidden)
    cand = (0.5 * rng.standard_normal((4 * M, din))).astype(np.float32)
    keep = np.flatnonzero(~near_relu_kink(c.theta, cand, c.low, c.high))[:M]
    assert len(keep) == M, (len(keep), M)
    c.s = cand[keep]
    ft = forward(c.teacher, c.s, c.low, c.high, value=False)
    act = ft["mean"] + 0.3 * np.exp(c.teacher[NAMES[6]].astype(np.float64)) * rng.standard_normal((M, A))
    c.a = np.minimum(np.maximum(np.clip(act, c.low, c.high).astype(np.float32), c.low), c.high)
    c.R = (forward(c.theta, c.s, c.low, c.high)["V"] + rng.standard_normal(M)).astype(np.float32)
    return c


_BUILT, _REFS = {}, {}


def case(shape, M):
    """The problem, built once per process and not to be modified."""
    if (shape, M) not in _BUILT:
        _BUILT[(shape, M)] = build(shape, M)
    return _BUILT[(shape, M)]


def reference(shape, M, kind, with_returns, dtype=np.float64):
    """loss_and_grads of case(shape, M), computed once per process and not to be modified."""
    key = (shape, M, kind, bool(with_returns), np.dtype(dtype).name)
    if key not in _REFS:
        c = case(shape, M)
        _REFS[key] = loss_and_grads(c.theta, c.s, c.a, c.R if with_returns else None, kind, c.low, c.high, dtype=dtype)
    return _REFS[key]


def tensor_distance(got, want):
    """max |got - want| / max |want| per tensor -> {name: float} (a tensor whose reference is all zeros: max |got|)."""
    out = {}
    for k in want:
        w, g = np.asarray(want[k], np.float64), np.asarray(got[k], np.float64)
        scale = np.abs(w).max()
        out[k] = float(np.abs(g - w).max() / scale) if scale > 0 else float(np.abs(g).max())
    return out


def trajectory(c, kind, with_returns, steps, dtype=np.float64, lr=LR):
    """`steps` chained clone steps with TF-Adam from zero slots in `dtype` -> (theta after the last step, the first step's update per tensor)."""
    th = OrderedDict((k, np.asarray(v, dtype)) for k, v in c.theta.items())
    m = OrderedDict((k, np.zeros_like(v)) for k, v in th.items())
    v = OrderedDict((k, np.zeros_like(x)) for k, x in th.items())
    names = NAMES if with_returns else POLICY_NET
    for t in range(1, steps + 1):
        _, g, _, _ = loss_and_grads(th, c.s, c.a, c.R if with_returns else None, kind, c.low, c.high, dtype=dtype)
        alpha = adam_alpha(lr, t, dtype)
        for k in names:
            th[k], m[k], v[k] = adam_tf(th[k], m[k], v[k], g[k], alpha, dtype)
    return th
